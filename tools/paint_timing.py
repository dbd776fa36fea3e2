#!/usr/bin/env python3
"""Host against device geometry painting (TCLB_GEOMETRY=host | device): Geometry.load of a
channel case (whole-domain collision box, walls, inlet, outlet, an OffgridSphere, an XPipe),
alone and with a <Sweep> of some hundred spheres, in a cubic d3q27 box.  Host clock around a
synchronised load, same process, the two paths alternating after one warm-up round of which
the flag arrays are compared.  One JSON line per case."""
import argparse
import json
import os
import statistics
import sys
import time
import xml.etree.ElementTree as ET

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tclb_amd.geometry.geometry import Geometry  # noqa: E402
from tclb_amd.lattice import Lattice  # noqa: E402
from tclb_amd.models import registry  # noqa: E402

CASE = """<Geometry nx="{n}" ny="{n}" nz="{n}">
  <MRT><Box/></MRT>
  <Wall mask="ALL"><Channel/></Wall>
  <WVelocity name="Inlet"><Inlet/></WVelocity>
  <EPressure name="Outlet"><Outlet/></EPressure>
  <Wall mask="ALL">
    <OffgridSphere x="{q}.3" y="{h}.2" z="{h}.4" R="{e}.6"/>
    <XPipe y="{h}.1" z="{h}.3" R="{s}.4" dx="{h}" nx="{q}"/>
  </Wall>{extra}
</Geometry>"""
SWEEP = """
  <Solid><Sweep r="{t}.3" step="1e-3"><Point x="{q}" y="{q}" z="{q}"/><Point x="{u}" y="{h}" z="{u}"/></Sweep></Solid>"""


def load(xml, n, where, lat):
    os.environ["TCLB_GEOMETRY"] = where
    g = Geometry(registry.get("d3q27"), (n, n, n), 0, n, 2, 0)
    g.lattice = lat          # used for its device only
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    g.load(ET.fromstring(xml))
    torch.cuda.synchronize()
    return time.perf_counter() - t0, g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    lat = Lattice("d3q27", (8, 8, 8), device=torch.device("cuda"))
    for n in a.sizes:
        f = dict(n=n, h=n // 2, q=n // 4, e=n // 8, s=n // 16, t=n // 32, u=3 * n // 4)
        for name, extra in (("channel", ""), ("channel + sweep", SWEEP.format(**f))):
            xml = CASE.format(extra=extra, **f)
            times = {"host": [], "device": []}
            for rep in range(a.reps + 1):              # the first round warms up
                got = {}
                for where in times:
                    dt, got[where] = load(xml, n, where, lat)
                    if rep:
                        times[where].append(dt)
                if rep == 0:
                    equal = bool(np.array_equal(got["host"].flags, got["device"].flags))
                launches = got["device"].device_paints
                del got
            row = {"n": n, "case": name, "equal": equal, "launches": launches}
            for where, t in times.items():
                row[where] = {"median_ms": round(1e3 * statistics.median(t), 2), "min_ms": round(1e3 * min(t), 2),
                              "max_ms": round(1e3 * max(t), 2)}
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
