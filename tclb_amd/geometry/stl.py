"""STL primitive (reference Geometry::loadSTL / transformSTL, src/Geometry.cpp.Rt:397-688).
Binary STL only; transforms Xrot/Yrot/Zrot, scale, x/y/z; sides in/out (ray parity) and
surface (sub-voxel cuts for interpolated bounce-back), both by the native host library or,
for a lattice on a GPU, by the device kernels of csrc/device/voxel.hip; same bits.  Where the
geometry is painted on the device too (Geometry.on_device), the mask or level bytes stay
there and enter the display list as a MASK record."""
from __future__ import annotations

import math
import os
import struct

import numpy as np

from ..ops import host


def read_stl(path: str) -> np.ndarray:
    with open(path, "rb") as f:
        header = f.read(80)
        if header[:5] == b"solid":
            raise ValueError(f"'STL' element {path} is not in binary format!")
        (ntri,) = struct.unpack("<i", f.read(4))
        rec = np.dtype([("n", "<f4", 3), ("p", "<f4", (3, 3)), ("attr", "<u2")])
        data = np.frombuffer(f.read(ntri * 50), dtype=rec, count=ntri)
    return data["p"].astype(np.float64).reshape(ntri, 9)


def transform(tri: np.ndarray, node, units) -> np.ndarray:
    P = tri.reshape(-1, 3, 3).copy()
    for d, (a1, a2) in enumerate([(1, 2), (2, 0), (0, 1)]):
        a = node.get("XYZ"[d] + "rot")
        if a is not None:
            v = units.alt(a)
            y = P[:, :, a1].copy()
            z = P[:, :, a2].copy()
            P[:, :, a1] = math.cos(v) * y - math.sin(v) * z
            P[:, :, a2] = math.sin(v) * y + math.cos(v) * z
    if node.get("scale") is not None:
        P *= units.alt(node.get("scale"))
    for d, a in enumerate("xyz"):
        if node.get(a) is not None:
            P[:, :, d] += units.alt(node.get(a))
    sm = np.array([0.1403e-4, 0.1687e-4, 0.1987e-4])
    P = np.round(P * 1e5) * 1e-5 + sm - 0.5
    return P.reshape(-1, 9)


D3Q27_DIRS = np.array([[x, y, z] for z in (0, 1, -1) for y in (0, 1, -1) for x in (0, 1, -1)])[1:]


def _on_device(geom) -> bool:
    """where the STL elements of `geom` are voxelised: TCLB_STL_VOXELISE = auto | host |
    device, auto being the device when the geometry is drawn for a lattice on a GPU
    (Geometry.lattice) and the host otherwise.  Decided at the geometry's first STL."""
    if geom.stl_device is None:
        mode = os.environ.get("TCLB_STL_VOXELISE") or "auto"
        if mode not in ("auto", "host", "device"):
            raise ValueError(f"TCLB_STL_VOXELISE '{mode}' is none of auto, host, device")
        lat = geom.lattice
        gpu = lat is not None and lat.is_gpu
        if mode == "device" and not gpu:
            raise ValueError("TCLB_STL_VOXELISE 'device' needs a lattice on a GPU")
        geom.stl_device = gpu and mode != "host"
    return geom.stl_device


def _surface_on_device(geom) -> bool:
    """_on_device for a surface: on the device the cuts go into lattice.cuts, and the
    geometry's first surface replaces those of an earlier geometry as set_cuts does on the
    host path.  A fill never touches them."""
    if not _on_device(geom):
        return False
    if geom.stl_surfaces == 0:
        geom.lattice.cuts = None
    geom.stl_surfaces += 1
    return True


def draw_stl(geom, reg, node):
    fn = node.get("file")
    if fn is None:
        raise ValueError("No 'file' attribute in 'STL' element")
    side = node.get("side", "in")
    inside_out = {"in": 0, "out": 1, "surface": 2}[side]
    axis = {"x": 0, "y": 1, "z": 2}[node.get("ray_axis", "y")]
    tri = transform(read_stl(fn), node, geom.units)
    r = reg.intersect(geom.total)
    if r.size() == 0:
        return
    box = (r.dx, r.dy, r.dz, r.nx, r.ny, r.nz)
    if inside_out == 2 and _surface_on_device(geom):
        import torch
        from ..ops import device
        from .geometry import K_MASK, Region
        lat = geom.lattice
        with torch.cuda.device(lat.device):
            cuts, mask, win = device.stl_cuts(tri, box, D3Q27_DIRS, lat._stream())
            lat.merge_cuts(cuts, win, geom.ys, geom.zs)
            r = Region(*win)
            if r.size() == 0:
                return
            if geom.on_device():                        # the mask stays on the device
                geom.paint(r, (K_MASK, 0, (mask, win, 0xFF, 0)))
                return
            sel = mask.cpu().numpy().astype(bool)       # the window's mask only
    elif inside_out == 2:
        cuts, mask = host.stl_cuts(tri, box, D3Q27_DIRS)
        geom.record_cuts(r, cuts)
        sel = mask.astype(bool)
    elif _on_device(geom):
        import torch
        from ..ops import device
        from .geometry import K_MASK, Region
        lat = geom.lattice
        with torch.cuda.device(lat.device):
            lev, win = device.stl_fill(tri, box, axis, inside_out, lat._stream())
            lat.stl_fills += 1
            w = Region(*win)
            if geom.on_device():                           # the levels stay on the device, bit 0 selects
                if inside_out == 0 and w.size() == 0:
                    return
                # side="out": off the window every node of the region is selected
                geom.paint(w if inside_out == 0 else r, (K_MASK, 0, (lev, win, 1, inside_out)))
                return
            odd = (lev.cpu().numpy() & 1).astype(bool)     # the window's levels only
        if inside_out == 0:
            # outside the window nothing is selected: paint the window alone
            r, sel = w, odd
            if r.size() == 0:
                return
        else:
            sel = np.ones((r.nz, r.ny, r.nx), dtype=bool)
            X, Y, Z = w.dx - r.dx, w.dy - r.dy, w.dz - r.dz
            sel[Z:Z + w.nz, Y:Y + w.ny, X:X + w.nx] = odd
    else:
        lev = host.stl_fill(tri, box, axis, inside_out)
        sel = (lev % 2) == 1

    def pred(X, Y, Z):
        xi = (X - r.dx).astype(int)
        yi = (Y - r.dy).astype(int)
        zi = (Z - r.dz).astype(int)
        return sel[zi, yi, xi]
    geom.paint(r, pred)
