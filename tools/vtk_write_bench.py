#!/usr/bin/env python3
"""Time of Solver.write_vtk on a d3q27 channel (default 256^3 fp64, every quantity and flag
group): after a warm-up plane write, one whole-lattice write and one one-plane write, each
between torch.cuda.synchronize() calls; then the file write alone, the whole file's size
written from a constant host buffer.  Prints one JSON line; run one process per sample and
alternate the arms (profiles/README.md, "Device VTK encoding").

    python tools/vtk_write_bench.py --tag device --encode device [--chunk BYTES]
    python tools/vtk_write_bench.py --tag parent          # a tree without the encode switch
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time
import xml.etree.ElementTree as ET

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASE = """<CLBConfig version="2.0" output="{out}/" permissive="true">
 <Geometry nx="{n}" ny="{n}" nz="{n}">
  <MRT><Box/></MRT>
  <WVelocity name="Inlet"><Inlet/></WVelocity>
  <EPressure name="Outlet"><Outlet/></EPressure>
  <Wall mask="ALL"><Channel/></Wall>
 </Geometry>
 <Model><Param name="Velocity" value="0.02"/><Param name="nu" value="0.05"/></Model>
 <Solve Iterations="4"/>
</CLBConfig>"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", required=True)
    ap.add_argument("--encode", default=None, help="host / device / auto; omit on a tree without the switch")
    ap.add_argument("--chunk", type=int, default=None)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--precision", default="double")
    ap.add_argument("--device", default="cuda", help="cpu: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    import torch
    from tclb_amd import handlers  # noqa: F401
    from tclb_amd.solver import Solver
    out = tempfile.mkdtemp(prefix="vtkbench_")
    s = Solver("d3q27", ET.fromstring(CASE.format(out=out, n=a.size)), conffile=os.path.join(out, "case.xml"),
               device=a.device, precision=a.precision)
    s.run()
    kw = {} if a.encode is None else {"encode": a.encode, "chunk": a.chunk}
    sync = torch.cuda.synchronize if a.device == "cuda" else (lambda: None)
    plane = (0, 0, a.size // 2, a.size, a.size, 1)

    def timed(name, region):
        sync()
        t0 = time.perf_counter()
        s.write_vtk(name, ["all"], region, **kw)
        sync()
        dt = time.perf_counter() - t0
        fn = s.out_iter_file(name, ".vti")
        size = os.path.getsize(fn)
        os.remove(fn)
        return dt, size

    timed("warm", plane)
    whole_s, whole_bytes = timed("whole", None)
    plane_s, plane_bytes = timed("plane", plane)
    # the file write alone: the same number of bytes from a constant buffer, in 64 MiB pieces
    buf = memoryview(bytes(64 << 20))
    fn = os.path.join(out, "constant.vti")
    t0 = time.perf_counter()
    with open(fn, "wb") as f:
        for o in range(0, whole_bytes, len(buf)):
            f.write(buf[:min(len(buf), whole_bytes - o)])
    file_s = time.perf_counter() - t0
    print(json.dumps({"tree": a.tag, "encode": a.encode, "chunk": a.chunk or os.environ.get("TCLB_VTK_CHUNK"),
                      "model": "d3q27", "shape": [a.size] * 3, "precision": a.precision,
                      "whole_s": round(whole_s, 4), "plane_s": round(plane_s, 5), "file_write_s": round(file_s, 4),
                      "whole_bytes": whole_bytes, "plane_bytes": plane_bytes}), flush=True)
    shutil.rmtree(out, ignore_errors=True)


if __name__ == "__main__":
    main()
