"""Device STL ray fill (csrc/device/voxel.hip k_stl_hits, k_ray_rows, k_ray_x): ops.device.stl_fill
against the host voxeliser ops.host.stl_fill, exact equality of the whole level byte, and
<STL side="in" | "out"> through the Geometry handler with TCLB_STL_VOXELISE=host | device | auto."""
import struct
import xml.etree.ElementTree as ET

import numpy as np
import pytest
import torch

from tclb_amd import handlers  # noqa: F401
from tclb_amd.geometry.stl import transform
from tclb_amd.ops import device as D
from tclb_amd.ops import host as H
from tclb_amd.solver import Solver

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]


def sphere(nu, nv, R=1.0, c=(0, 0, 0)):
    """UV sphere of nu x nv segments, 2 nu (nv - 1) triangles, as (n, 9)"""
    th, ph = np.pi * np.arange(nv + 1) / nv, 2 * np.pi * np.arange(nu + 1) / nu
    V = np.stack([np.sin(th)[:, None] * np.cos(ph), np.sin(th)[:, None] * np.sin(ph),
                  np.cos(th)[:, None] * np.ones_like(ph)], -1) * R + np.asarray(c)
    T = []
    for j in range(nv):
        for i in range(nu):
            if j > 0:
                T.append([V[j, i], V[j, i + 1], V[j + 1, i + 1]])
            if j < nv - 1:
                T.append([V[j, i], V[j + 1, i + 1], V[j + 1, i]])
    return np.array(T).reshape(-1, 9)


def placed(*a):
    """the rounding and offset of transform(): no barycentric coordinate on a boundary"""
    return transform(sphere(*a), ET.Element("STL"), None)


C1, C3 = (12.37, 11.79, 12.11), (35.37, 34.79, 35.11)
RAW = np.array([[4, 4, 4, 9.3, 4.2, 5.1, 5.2, 8.7, 6.4],          # a vertex on a lattice node
                [3, 3, 3, 5, 5, 5, 7, 7, 7]], dtype=np.float64)    # zero area
ONE = np.array([[2.3, 3.1, 4.2, 9.4, 3.7, 5.1, 4.2, 9.8, 6.3]])
# name: (triangles, region, odd nodes of the host result for (axis, inside_out) =
# (0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1))
CASES = {
    "coarse": (lambda: placed(6, 4, 8.3, C1), (0, 0, 0, 24, 24, 24), (1679, 12145, 1679, 12145, 1679, 12145)),
    "nested": (lambda: np.concatenate([placed(6, 4, 8.3, C1), placed(6, 4, 4.1, C1)]), (0, 0, 0, 24, 24, 24),
               (1481, 12343, 1481, 12343, 1481, 12343)),
    "clipped": (lambda: placed(12, 8, 30.2, C3), (5, 9, 13, 67, 30, 21), (26786, 15424, 26786, 15424, 26786, 15424)),
    # along x more than 64 levels with counters and more than 64 below them: several trips of k_ray_x
    "long": (lambda: placed(12, 8, 40.2, (115.37, 44.79, 45.11)), (0, 30, 35, 170, 13, 11),
             (10593, 13717, 10593, 13717, 10593, 13717)),
    "unreached": (lambda: placed(6, 4, 8.3, C1), (30, 2, 2, 9, 9, 9), (0, 729, 0, 729, 0, 729)),
    "ties": (lambda: RAW, (0, 0, 0, 12, 12, 12), (7, 1721, 38, 1690, 52, 1676)),
    "stack": (lambda: np.repeat(transform(ONE, ET.Element("STL"), None), 300, 0), (0, 0, 0, 12, 12, 12),
              (0, 1728, 0, 1728, 0, 1728)),
}


@pytest.mark.parametrize("inside_out", [0, 1])
@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("name", CASES)
def test_stl_fill_equals_host(name, axis, inside_out):
    mk, region, odd = CASES[name]
    tri = mk()
    lev_host = H.stl_fill(tri, region, axis, inside_out)
    lev, (x0, y0, z0, wx, wy, wz) = D.stl_fill(tri, region, axis, inside_out)
    print(name, axis, inside_out, "window", (x0, y0, z0, wx, wy, wz), "odd", int((lev_host & 1).sum()),
          "levels", np.unique(lev_host).tolist())
    assert int((lev_host & 1).sum()) == odd[2 * axis + inside_out]
    # 300 hits on one cell wrap the byte to 44
    assert name != "stack" or (lev_host == inside_out + 44).any()
    assert lev.dtype == torch.uint8 and tuple(lev.shape) == (wz, wy, wx)
    full = np.full_like(lev_host, inside_out)
    if wx * wy * wz:
        X, Y, Z = x0 - region[0], y0 - region[1], z0 - region[2]
        assert X >= 0 and Y >= 0 and Z >= 0
        assert X + wx <= region[3] and Y + wy <= region[4] and Z + wz <= region[5]
        full[Z:Z + wz, Y:Y + wy, X:X + wx] = lev.cpu().numpy()
    else:
        assert name == "unreached"
    assert np.array_equal(full, lev_host)


CASE = """<?xml version="1.0"?>
<CLBConfig version="2.0" output="{out}/" permissive="true">
  <Geometry nx="40" ny="34" nz="30">
    <MRT><Box/></MRT>
    <Wall mask="ALL">
      <STL file="{stl}" side="in" scale="9.3" x="15.4" y="16.2" z="14.7"/>
      <STL file="{stl}" side="out" ray_axis="x" scale="17.1" x="20.3" y="17.9" z="15.6"/>
    </Wall>
  </Geometry>
</CLBConfig>"""


def test_geometry_handler_host_and_device(tmp_path, monkeypatch):
    stl = tmp_path / "sphere.stl"
    tri = sphere(16, 10).astype("<f4")
    rec = np.zeros(len(tri), dtype=[("n", "<f4", 3), ("p", "<f4", 9), ("attr", "<u2")])
    rec["p"] = tri
    stl.write_bytes(bytes(80) + struct.pack("<i", len(tri)) + rec.tobytes())
    flags = {}
    for mode in ("host", "device", "auto"):
        monkeypatch.setenv("TCLB_STL_VOXELISE", mode)
        out = tmp_path / mode
        out.mkdir()
        s = Solver("d3q27", ET.fromstring(CASE.format(out=out, stl=stl)), conffile=str(out / "case.xml"),
                   device="cuda")
        s.run()
        assert s.lattice.stl_fills == (0 if mode == "host" else 2), mode
        assert s.lattice.cut_merges == 0 and s.lattice.cuts is None
        flags[mode] = s.lattice.flags.cpu().numpy()
    wall, boundary = s.lattice.model.node_type("Wall").value, s.lattice.model.group_masks["BOUNDARY"]
    painted = int(((flags["host"] & boundary) == wall).sum())
    print("wall nodes", painted, "of", 40 * 34 * 30)
    assert 1000 < painted < 40 * 34 * 30 - 1000
    for mode in ("device", "auto"):
        assert np.array_equal(flags[mode], flags["host"]), mode
