"""Device STL surface voxeliser (csrc/device/voxel.hip): ops.device.stl_cuts and cuts_merge
against the host voxeliser ops.host.stl_cuts, exact equality of the uint16 cuts and of the mask,
and <STL side="surface"> through the Geometry handler with TCLB_STL_VOXELISE=host | device."""
import struct
import xml.etree.ElementTree as ET

import numpy as np
import pytest
import torch

from tclb_amd import handlers  # noqa: F401
from tclb_amd.geometry.geometry import Geometry, Region
from tclb_amd.geometry.stl import D3Q27_DIRS, transform
from tclb_amd.models import registry
from tclb_amd.ops import device as D
from tclb_amd.ops import host as H
from tclb_amd.solver import Solver

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]

MODEL = "d3q27_cumulant_qibb_small"


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
# a triangle in the lattice plane x = 6: row 0 of every node's system there is all zero
PLANE = np.array([[6, 2, 2, 6, 9, 2.5, 6, 3, 9]], dtype=np.float64)
# name: (triangles, region, mask nodes and cuts of the host result)
CASES = {
    "coarse": (lambda: placed(6, 4, 8.3, C1), (0, 0, 0, 24, 24, 24), 2120, 13258),
    "fine": (lambda: placed(24, 12, 8.3, C1), (0, 0, 0, 24, 24, 24), 2549, 15652),
    "clipped": (lambda: placed(12, 8, 30.2, C3), (5, 9, 13, 67, 30, 21), 5678, None),
    "unreached": (lambda: placed(6, 4, 8.3, C1), (30, 2, 2, 9, 9, 9), 0, 0),
    "degenerate": (lambda: RAW, (0, 0, 0, 12, 12, 12), None, None),
    "in-plane": (lambda: PLANE, (0, 0, 0, 12, 12, 12), None, None),
}
_results = {}


def voxelised(name):
    """(host cuts, host mask, device cuts on the host, device mask on the host, window, device cuts)"""
    if name not in _results:
        mk, region = CASES[name][:2]
        tri = mk()
        hc, hm = H.stl_cuts(tri, region, D3Q27_DIRS)
        dc, dm, win = D.stl_cuts(tri, region, D3Q27_DIRS)
        _results[name] = (hc, hm, dc.cpu().numpy().view(np.uint16), dm.cpu().numpy(), win, dc)
    return _results[name]


@pytest.mark.parametrize("name", CASES)
def test_stl_cuts_equal_host(name):
    region, nmask, ncuts = CASES[name][1:]
    hc, hm, dc, dm, (x0, y0, z0, wx, wy, wz), _ = voxelised(name)
    print(name, "window", (x0, y0, z0, wx, wy, wz), "mask", int(hm.sum()), "cuts", int((hc != 65535).sum()))
    assert nmask is None or int(hm.sum()) == nmask
    assert ncuts is None or int((hc != 65535).sum()) == ncuts
    assert name == "unreached" or hm.any()
    full_c = np.full_like(hc, 65535)
    full_m = np.zeros_like(hm)
    if wx * wy * wz:
        assert x0 >= region[0] and y0 >= region[1] and z0 >= region[2]
        X, Y, Z = x0 - region[0], y0 - region[1], z0 - region[2]
        full_c[:, Z:Z + wz, Y:Y + wy, X:X + wx] = dc
        full_m[Z:Z + wz, Y:Y + wy, X:X + wx] = dm
    else:
        assert name == "unreached" and dc.size == 0 and dm.size == 0
    assert np.array_equal(full_m, hm)
    assert np.array_equal(full_c, hc)


@pytest.mark.parametrize("names", [("clipped",), ("coarse", "fine", "degenerate")])
def test_cuts_merge_wrapped_rows(names):
    """the merge into a lattice-shaped array against Geometry.record_cuts: a z slab with ghost
    planes that wrap periodically, px wider than nx, several windows into one array"""
    gshape = (72, 40, 36)
    g = Geometry(registry.get(MODEL), gshape, 30, 12, 2, 3)      # planes 27..44 -> 27..35, 0..8
    assert len(set(g.zs.tolist())) == len(g.zs) and g.zs.min() == 0 and g.zs.max() == 35
    px = 80
    dst = torch.full((26, len(g.zs), len(g.ys), px), -1, dtype=torch.int16, device="cuda")
    ys, zs = (torch.from_numpy(a.astype(np.int32)).cuda() for a in (g.ys, g.zs))
    for name in names:
        hc, _, _, _, win, dc = voxelised(name)
        g.record_cuts(Region(*CASES[name][1]), hc)
        D.cuts_merge(dst, dc, win, ys, zs)
    got = dst.cpu().numpy().view(np.uint16)
    assert (g.cuts != 65535).any()
    assert np.array_equal(got[..., :72], g.cuts) and (got[..., 72:] == 65535).all()


CASE = """<?xml version="1.0"?>
<CLBConfig version="2.0" output="{out}/" permissive="true">
  <Geometry nx="40" ny="34" nz="30">
    <MRT><Box/></MRT>
    <QIBB>
      <STL file="{stl}" side="surface" scale="9.3" x="15.4" y="16.2" z="14.7"/>
      <STL file="{stl}" side="surface" scale="7.1" x="24.3" y="17.9" z="15.6"/>
    </QIBB>
  </Geometry>
</CLBConfig>"""


def test_geometry_handler_host_and_device(tmp_path, monkeypatch):
    stl = tmp_path / "sphere.stl"
    tri = sphere(16, 10).astype("<f4")
    rec = np.zeros(len(tri), dtype=[("n", "<f4", 3), ("p", "<f4", 9), ("attr", "<u2")])
    rec["p"] = tri
    stl.write_bytes(bytes(80) + struct.pack("<i", len(tri)) + rec.tobytes())
    lats = {}
    for mode in ("host", "device", "auto"):
        monkeypatch.setenv("TCLB_STL_VOXELISE", mode)
        out = tmp_path / mode
        out.mkdir()
        s = Solver(MODEL, ET.fromstring(CASE.format(out=out, stl=stl)), conffile=str(out / "case.xml"),
                   device="cuda")
        s.run()
        lats[mode] = s.lattice
        assert s.lattice.cut_merges == (0 if mode == "host" else 2), mode
    ref_c, ref_f = lats["host"].cuts.cpu().numpy(), lats["host"].flags.cpu().numpy()
    qibb = lats["host"].model.node_type("QIBB").value
    assert (ref_c != -1).sum() > 10000 and ((ref_f & qibb) != 0).sum() > 2000
    for mode in ("device", "auto"):
        assert lats[mode].cuts.dtype == torch.int16 and lats[mode].cuts.shape == lats["host"].cuts.shape
        assert np.array_equal(lats[mode].cuts.cpu().numpy(), ref_c), mode
        assert np.array_equal(lats[mode].flags.cpu().numpy(), ref_f), mode
