"""Device geometry painter (csrc/device/paint.hip k_paint behind Geometry, TCLB_GEOMETRY): the
flag array of a Geometry painted on the GPU against the host painter (NumPy fp64) on the same
XML, exact equality of the whole (NZ, NY, gnx) array, ghost rows included."""
import struct
import xml.etree.ElementTree as ET

import numpy as np
import pytest
import torch

from tclb_amd import handlers  # noqa: F401
from tclb_amd.geometry.geometry import Geometry
from tclb_amd.lattice import Lattice
from tclb_amd.models import registry
from tclb_amd.solver import Solver

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]

# 131 = two full 64-lane segments and a 3-lane tail; 10 and 9 are multiples of no tile dimension
SHAPE = (131, 10, 9)
# (slab_lo, slab_n, axis, ghost, yz): the whole box; z planes 5 6 7 8 0 1 2; a Y x Z block with
# rows 6 7 8 9 0 and planes 7 8 0 1 2 3 4 5
DECOMPOSITIONS = [(0, 9, 2, 0, None), (6, 5, 2, 1, None), (0, 0, 3, 0, (7, 3, 1, 0, 4, 2))]

PRIMITIVES = {
    "Box": '<Box dx="3" nx="120" dy="1" ny="7" dz="2" nz="5"/>',
    "Sphere": '<Sphere dx="10" nx="100" dy="0" ny="10" dz="0" nz="9"/>',
    "HalfSphere": '<HalfSphere dx="10" nx="115" dy="1" ny="8" dz="0" nz="9"/>',
    "OffgridSphere": '<OffgridSphere x="70.3" y="4.6" z="4.2" Rx="65.5" Ry="4.3" Rz="3.7"/>',
    "OffgridPipe": '<OffgridPipe x="66.1" y="5.2" z="0" Rx="60.4" Ry="3.9" dz="1" nz="7"/>',
    "XPipe": '<XPipe y="5.1" z="4.3" R="3.6" dx="1" nx="129"/>',
    "YPipe": '<YPipe x="0" y="64.3" z="4.4" Rx="40.5" Rz="3.3"/>',
    "ZPipe": '<ZPipe x="0" y="5.3" z="0" Rx="3.4" Ry="4.2" dz="2" nz="6"/>',
    "XAnnulus": '<XAnnulus x="0" y="5.2" z="4.4" Ro="4.1" Ri="2.2"/>',
    "Pipe": '<Pipe dx="5" nx="120" dy="1" ny="8" dz="1" nz="7"/>',
    "PipeY": '<PipeY dx="3" nx="125" dy="0" ny="10" dz="1" nz="7"/>',
    "PipeZ": '<PipeZ dx="3" nx="125" dy="1" ny="8"/>',
    "Cylinder": '<Cylinder dx="2" nx="127" dy="1" ny="8"/>',
    "Wedge-LowerRight": '<Wedge dx="20" nx="100" dy="1" ny="8" direction="LowerRight"/>',
    "Wedge-UpperLeftXZ": '<Wedge dx="1" nx="129" dz="1" nz="7" direction="UpperLeftXZ"/>',
    "Wedge-unknown": '<Wedge dx="25" nx="10" dy="5" ny="3" direction="Sideways"/>',
}

LAYERED = """<Geometry nx="131" ny="10" nz="9">
  <MRT><Box/></MRT>
  <Wall mask="ALL"><Box dx="30" nx="70"/><Box dx="4" nx="2"/></Wall>
  <WVelocity mask="BOUNDARY" name="zoneA" mode="{mode}">{primitive}</WVelocity>
</Geometry>"""

SWEEP = """<Geometry nx="131" ny="10" nz="9">
  <MRT><Box/></MRT>
  <Wall mask="ALL"><Box dx="50" nx="30" dy="3" ny="4"/></Wall>
  <Solid mode="fill"><Sweep r="2.5" step="1e-3"><Point x="10" y="3" z="3"/><Point x="110" y="7" z="6"/></Sweep></Solid>
  <WPressure mode="fill"><Sweep r="1.7" step="1e-3"><Point x="120" y="2" z="6"/><Point x="20" y="8" z="2" r="3.1"/></Sweep></WPressure>
</Geometry>"""


@pytest.fixture(scope="module")
def gpu_lattice():
    return Lattice("d3q27", (8, 8, 8), device=torch.device("cuda"))


def painted(xml, where, decomposition, monkeypatch, lattice, batch=None):
    lo, n, axis, ghost, yz = decomposition
    monkeypatch.setenv("TCLB_GEOMETRY", where)
    g = Geometry(registry.get("d3q27"), SHAPE, lo, n, axis, ghost, yz=yz)
    g.lattice = lattice
    if batch:
        g.paint_batch = batch
    return g.load(ET.fromstring(xml))


@pytest.mark.parametrize("mode", ["overwrite", "fill", "change"])
@pytest.mark.parametrize("name", PRIMITIVES)
def test_primitive_equals_host(name, mode, monkeypatch, gpu_lattice):
    xml = LAYERED.format(mode=mode, primitive=PRIMITIVES[name])
    for d in DECOMPOSITIONS:
        host = painted(xml, "host", d, monkeypatch, gpu_lattice)
        dev = painted(xml, "device", d, monkeypatch, gpu_lattice)
        zone = (host.flags >> host.model.zone_shift) == host.zones["zoneA"]
        print(name, mode, d, "painted", int(zone.sum()), "of", zone.size)
        assert host.device_paints == 0 and dev.device_paints == 1
        assert 0 < zone.sum() < zone.size
        assert dev.flags.dtype == np.uint32 and np.array_equal(dev.flags, host.flags), d


@pytest.mark.parametrize("batch", [4096, 64])
def test_sweep_order_across_rounds_and_launches(batch, monkeypatch, gpu_lattice):
    """two crossing sweeps of some hundred spheres in fill mode: with the default batch one
    launch culls them in several rounds, with 64 they spread over many launches"""
    d = DECOMPOSITIONS[1]
    host = painted(SWEEP, "host", d, monkeypatch, gpu_lattice)
    dev = painted(SWEEP, "device", d, monkeypatch, gpu_lattice, batch)
    B = host.model.group_masks["BOUNDARY"]
    counts = [int(((host.flags & B) == host.model.node_type(t).value).sum()) for t in ("Solid", "WPressure")]
    print("batch", batch, "launches", dev.device_paints, "Solid, WPressure nodes", counts)
    assert min(counts) > 100
    assert dev.device_paints == 1 if batch == 4096 else dev.device_paints > 1
    assert np.array_equal(dev.flags, host.flags)


MODEL = "d3q27_cumulant_qibb_small"
CASE = """<?xml version="1.0"?>
<CLBConfig version="2.0" output="{out}/" permissive="true">
  <Geometry nx="70" ny="34" nz="30">
    <MRT><Box/></MRT>
    <Wall mask="ALL">
      <Sphere dx="2" nx="10" dy="3" ny="9" dz="4" nz="8"/>
      <STL file="{stl}" side="in" scale="14.3" x="20.4" y="9.2" z="8.7"/>
      <Box dx="60" nx="4" dy="1" ny="5"/>
    </Wall>
    <Solid mode="fill" mask="BOUNDARY">
      <STL file="{stl}" side="out" ray_axis="x" scale="27.1" x="30.3" y="3.9" z="2.6"/>
    </Solid>
    <QIBB><STL file="{stl}" side="surface" scale="11.1" x="44.3" y="12.9" z="9.6"/></QIBB>
    <WVelocity name="In">
      <Text file="{txt}" dx="5" nx="6" dy="20" ny="4" dz="5" nz="3"/>
      <OffgridSphere x="50.2" y="25.3" z="20.1" R="4.4"/>
    </WVelocity>
  </Geometry>
</CLBConfig>"""
TETRAHEDRON = np.array([[0, 0, 0, 0, 1, 0, 1, 0, 0], [0, 0, 0, 1, 0, 0, 0, 0, 1],
                        [0, 0, 0, 0, 0, 1, 0, 1, 0], [1, 0, 0, 0, 1, 0, 0, 0, 1]], dtype="<f4")


def test_geometry_handler_host_device_auto(tmp_path, monkeypatch):
    """primitives interleaved with STL bodies, an STL surface and a host-painted Text"""
    stl, txt = tmp_path / "tetrahedron.stl", tmp_path / "text.txt"
    rec = np.zeros(4, dtype=[("n", "<f4", 3), ("p", "<f4", 9), ("attr", "<u2")])
    rec["p"] = TETRAHEDRON
    stl.write_bytes(bytes(80) + struct.pack("<i", 4) + rec.tobytes())
    txt.write_text(" ".join(str((i * 7) % 3 % 2) for i in range(6 * 4 * 3)))
    got = {}
    for where in ("host", "device", "auto"):
        monkeypatch.setenv("TCLB_GEOMETRY", where)
        out = tmp_path / where
        out.mkdir()
        s = Solver(MODEL, ET.fromstring(CASE.format(out=out, stl=stl, txt=txt)), conffile=str(out / "case.xml"),
                   device="cuda")
        s.run()
        assert (s.geometry.device_paints == 0) == (where == "host"), where
        got[where] = (s.lattice.flags.cpu().numpy(), s.lattice.cuts.cpu().numpy(), s.geometry.flags)
    m = s.lattice.model
    types = {t: int(((got["host"][2] & m.node_type(t).mask) == m.node_type(t).value).sum())
             for t in ("Wall", "Solid", "QIBB", "WVelocity")}
    print(types, "cuts", int((got["host"][1] != -1).sum()))
    assert min(types.values()) > 20 and (got["host"][1] != -1).any()
    for where in ("device", "auto"):
        for a, b in zip(got[where], got["host"]):
            assert a.dtype == b.dtype and np.array_equal(a, b), where
