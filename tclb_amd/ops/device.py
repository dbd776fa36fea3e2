"""ctypes binding of the model-independent HIP runtime kernels (csrc/device/*.hip,
libtclb_device.so): the per-step particle kernels, the snapshot allocator, the output
encoders (base64, flag groups, PNG frames), the STL voxelisers (surface cuts, ray fill) and the geometry
painter (display list of primitives -> flag array).  On a GPU the library must be there
(built by ``tclb_amd.build``); a missing or stale one is an error, not a silent switch to
tensor ops."""
from __future__ import annotations

import ctypes
import os
import threading

_lib = None
_lock = threading.Lock()


class DeviceRuntimeError(RuntimeError):
    pass


def lib():
    global _lib
    with _lock:
        if _lib is None:
            from .. import build as B
            path = os.path.join(B.LIB, "libtclb_device.so")
            stale = B.device_runtime_stale()
            if stale is not None:
                if os.path.exists(B.HIPCC) and not os.environ.get("TCLB_NO_BUILD"):
                    B.build_device_runtime()
                else:
                    raise DeviceRuntimeError(f"device runtime library not usable ({stale}): {path}")
            L = ctypes.CDLL(path)
            P, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
            L.tclb_part_nan_to_zero.argtypes = [P, i, P]
            L.tclb_part_nan_to_zero.restype = i
            L.tclb_part_acc_slots.argtypes = [P, i, i, P]
            L.tclb_part_acc_slots.restype = i
            L.tclb_part_rigid_step.argtypes = [P, P, P, P, i, d, d, d, i, d, d, d, P]
            L.tclb_part_rigid_step.restype = i
            L.tclb_part_build_grid.argtypes = [P, i, P, i, i, i, i, i, P, ctypes.c_longlong, P]
            L.tclb_part_build_grid.restype = i
            L.tclb_part_build_tree.argtypes = [P, i, P, i, d, P, ctypes.c_longlong, P]
            L.tclb_part_build_tree.restype = i
            L.tclb_snap_probe.argtypes = [P, P, ctypes.c_longlong, ctypes.c_longlong, i, i, i, P]
            L.tclb_snap_probe.restype = i
            L.tclb_snap_alloc.argtypes = [ctypes.POINTER(P), ctypes.c_size_t, i, i]
            L.tclb_snap_alloc.restype = i
            L.tclb_snap_free.argtypes = [P, i]
            L.tclb_snap_free.restype = i
            L.tclb_enc_b64.argtypes = [P, P, ctypes.c_longlong, P]
            L.tclb_enc_b64.restype = i
            L.tclb_enc_flag_groups.argtypes = [P, i, ctypes.c_longlong, ctypes.c_longlong, i, i, i, i,
                                               ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_uint),
                                               ctypes.POINTER(P), P]
            L.tclb_enc_flag_groups.restype = i
            LL = ctypes.c_longlong
            L.tclb_enc_png_bytes.argtypes = [i, i, ctypes.POINTER(LL), ctypes.POINTER(LL)]
            L.tclb_enc_png_bytes.restype = i
            L.tclb_enc_png.argtypes = [P, i, i, i, P, LL, P, LL, P, P, P]
            L.tclb_enc_png.restype = i
            L.tclb_stl_tmp_bytes.argtypes = [i]
            L.tclb_stl_tmp_bytes.restype = LL
            L.tclb_stl_prep.argtypes = [P, i, i, i, i, i, i, i, P, LL, ctypes.POINTER(LL), P]
            L.tclb_stl_prep.restype = i
            L.tclb_stl_cuts.argtypes = [P, i, i, i, i, i, i, i, P, P, LL, LL, P, LL, P, P]
            L.tclb_stl_cuts.restype = i
            L.tclb_stl_prep_rays.argtypes = [P, i, i, i, i, i, i, i, i, P, LL, ctypes.POINTER(LL), P]
            L.tclb_stl_prep_rays.restype = i
            L.tclb_stl_ray_fill.argtypes = [P, i, i, i, i, i, i, i, i, i, i, P, LL, LL, P, LL, P, P]
            L.tclb_stl_ray_fill.restype = i
            L.tclb_cuts_merge.argtypes = [P, i, i, i, LL, P, LL, i, i, i, i, i, i, P, P, P]
            L.tclb_cuts_merge.restype = i
            L.tclb_paint.argtypes = [P, i, i, i, P, P, P, i, i, i, i, i, i, i, i, P]
            L.tclb_paint.restype = i
            _lib = L
    return _lib


def _check(r: int, what: str):
    if r != 0:
        raise DeviceRuntimeError(f"{what} failed: HIP error {r}")


def nan_to_zero(t, stream: int):
    """t (contiguous fp64 device tensor): NaN -> 0 in place"""
    _check(lib().tclb_part_nan_to_zero(t.data_ptr(), t.numel(), stream), "particle NaN guard")


def acc_slots(acc, n6: int, nslots: int, stream: int):
    """the accumulator copies of a particle stage summed into the first (core.hpp particle_acc)"""
    _check(lib().tclb_part_acc_slots(acc.data_ptr(), int(n6), int(nslots), stream), "particle accumulator copies")


def rigid_step(P, acc, m, free, n: int, a, periodic: int, period, stream: int):
    _check(lib().tclb_part_rigid_step(P.data_ptr(), acc.data_ptr(), m.data_ptr(), free.data_ptr(), n,
                                      float(a[0]), float(a[1]), float(a[2]), periodic,
                                      float(period[0]), float(period[1]), float(period[2]), stream),
           "particle integration")


def b64encode(src, out=None, stream=None):
    """base64 (RFC 4648, '=' padding) of the bytes of the contiguous device tensor `src` (any
    dtype; its first byte 4-byte aligned) as a uint8 device tensor of 4 * ceil(n / 3)
    characters: a new one, or the front of `out` (uint8, contiguous, 4-byte aligned, long
    enough), of which the rest stays untouched (csrc/device/encode.hip k_b64).  stream: a
    raw HIP stream, default the current one of src's device."""
    import torch
    if not src.is_cuda or not src.is_contiguous():
        raise ValueError("b64encode: src must be a contiguous device tensor")
    n = src.numel() * src.element_size()
    m = 4 * ((n + 2) // 3)
    if out is None:
        out = torch.empty(m, dtype=torch.uint8, device=src.device)
    elif out.dtype != torch.uint8 or out.device != src.device or not out.is_contiguous() or out.numel() < m:
        raise ValueError(f"b64encode: out must be a contiguous uint8 tensor of at least {m} bytes on {src.device}")
    if stream is None:
        stream = torch.cuda.current_stream(src.device).cuda_stream
    with torch.cuda.device(src.device):
        _check(lib().tclb_enc_b64(src.data_ptr(), out.data_ptr(), n, stream), "base64 encoding")
    return out[:m]


FLAG_GROUPS_MAX = 16


def flag_groups(flags, pairs, stream=None):
    """[((flags & mask) >> shift) as uint8 for (mask, shift) in pairs] of the 3-D device
    tensor `flags` (int16 or int32 read as unsigned; any strides with x contiguous, e.g. a
    window of Lattice.flags): contiguous arrays of flags' shape, all views of one
    allocation, from one pass over the window per FLAG_GROUPS_MAX pairs
    (csrc/device/encode.hip k_flag_groups)"""
    import torch
    if not flags.is_cuda or flags.dim() != 3 or flags.dtype not in (torch.int16, torch.int32):
        raise ValueError("flag_groups: flags must be a 3-D int16 or int32 device tensor")
    wz, wy, wx = flags.shape
    if wx > 1 and flags.stride(2) != 1:
        raise ValueError("flag_groups: the x axis of flags must be contiguous")
    pairs = [(int(m) & 0xFFFFFFFF, int(s)) for m, s in pairs]
    total = wz * wy * wx
    pitch = (total + 3) // 4 * 4                       # every array starts 4-byte aligned
    buf = torch.empty((len(pairs), pitch), dtype=torch.uint8, device=flags.device)
    if stream is None:
        stream = torch.cuda.current_stream(flags.device).cuda_stream
    UA, PA = ctypes.c_uint * FLAG_GROUPS_MAX, ctypes.c_void_p * FLAG_GROUPS_MAX
    with torch.cuda.device(flags.device):
        for k in range(0, len(pairs) if total else 0, FLAG_GROUPS_MAX):
            part = pairs[k:k + FLAG_GROUPS_MAX]
            masks, shifts = UA(*[m for m, _ in part]), UA(*[s for _, s in part])
            outs = PA(*[buf[k + j].data_ptr() for j in range(len(part))])
            _check(lib().tclb_enc_flag_groups(flags.data_ptr(), 16 if flags.dtype == torch.int16 else 32,
                                              flags.stride(1), flags.stride(0), wx, wy, wz, len(part), masks,
                                              shifts, outs, stream), "flag group extraction")
    return [buf[j, :total].view(wz, wy, wx) for j in range(len(pairs))]


def png_encode(lw, stream=None, pixels=None):
    """the colour frame of the (2, ny, nx) colour pair `lw` (l plane, w plane: a contiguous
    fp32 or fp64 device tensor, as Lattice.color lays it out) as a complete PNG file in one
    uint8 device tensor: RGBA, 8 bits, image row r = lattice row ny-1-r, the pixels of
    render.colormap bit for bit (csrc/device/encode.hip k_frame_rows, k_png_pack,
    k_png_finish).  pixels: an (ny, nx, 4) contiguous uint8 tensor on lw's device that
    receives the image as well.  stream: a raw HIP stream, default the current one of lw's
    device; the call waits for it, since the file's length is a result."""
    import torch
    if not lw.is_cuda or not lw.is_contiguous() or lw.dim() != 3 or lw.shape[0] != 2 or \
            lw.dtype not in (torch.float32, torch.float64):
        raise ValueError("png_encode: lw must be a contiguous (2, ny, nx) fp32 or fp64 device tensor")
    _, ny, nx = lw.shape
    if nx <= 0 or ny <= 0 or nx * ny * 4 + ny >= 2 ** 31:
        raise ValueError(f"png_encode: a frame of {nx} x {ny} is empty or beyond 2^31 bytes")
    if pixels is not None and (pixels.dtype != torch.uint8 or pixels.device != lw.device or
                               tuple(pixels.shape) != (ny, nx, 4) or not pixels.is_contiguous()):
        raise ValueError(f"png_encode: pixels must be a contiguous ({ny}, {nx}, 4) uint8 tensor on {lw.device}")
    L = lib()
    nout, ntmp = ctypes.c_longlong(0), ctypes.c_longlong(0)
    _check(L.tclb_enc_png_bytes(nx, ny, ctypes.byref(nout), ctypes.byref(ntmp)), "PNG frame sizes")
    out = torch.empty(nout.value, dtype=torch.uint8, device=lw.device)
    tmp = torch.empty(ntmp.value, dtype=torch.uint8, device=lw.device)
    count = torch.empty(1, dtype=torch.int64, device=lw.device)
    if stream is None:
        stream = torch.cuda.current_stream(lw.device).cuda_stream
    with torch.cuda.device(lw.device):
        _check(L.tclb_enc_png(lw.data_ptr(), lw.element_size(), nx, ny, out.data_ptr(), out.numel(), tmp.data_ptr(),
                              tmp.numel(), 0 if pixels is None else pixels.data_ptr(), count.data_ptr(), stream),
               "PNG frame encoding")
        if stream != torch.cuda.current_stream(lw.device).cuda_stream:
            torch.cuda.ExternalStream(stream, device=lw.device).synchronize()
    n = int(count.item())
    if n < 0:
        raise DeviceRuntimeError(f"png_encode: a frame of {nx} x {ny} does not fit one IDAT chunk")
    return out[:n]


def _stl_box(tri, region, what: str):
    """(tri as a contiguous (n, 9) float64 array, origin and size of `region`, the mesh's integer
    bounding box (ceil(min) - 1, floor(max) + 1) or None without triangles or nodes)"""
    import numpy as np
    tri = np.ascontiguousarray(tri, dtype=np.float64).reshape(-1, 9)
    r0 = np.array([int(v) for v in region[:3]], dtype=np.int64)
    rn = np.array([int(v) for v in region[3:]], dtype=np.int64)
    if not len(tri) or rn.min() <= 0:
        return tri, r0, rn, None
    # per-axis extrema over contiguous rows (a reduction over the 3-wide axis is ten times slower);
    # NaN propagates through min and max, so the six numbers also carry the finiteness check
    xyz = np.ascontiguousarray(tri.reshape(-1, 3).T)
    mn, mx = xyz.min(1), xyz.max(1)
    if not (np.isfinite(mn).all() and np.isfinite(mx).all()) or max(-mn.min(), mx.max()) >= 2 ** 30:
        raise ValueError(f"{what}: triangle coordinates must be finite and below 2^30")
    return tri, r0, rn, (np.ceil(mn).astype(np.int64) - 1, np.floor(mx).astype(np.int64) + 1)


def stl_fill(tri, region, axis: int, inside_out: int, stream=None):
    """ray-parity levels of the solid body bounded by the triangles `tri` ((n, 9) float64 host
    array, lattice coordinates) over the global box `region` (x0, y0, z0, nx, ny, nz) on the
    current device, rays along `axis` (0, 1, 2), bit for bit what ops.host.stl_fill computes
    (csrc/device/voxel.hip k_tri_prep, k_stl_hits, k_ray_rows / k_ray_x).  Returns (lev, window):
    lev (wz, wy, wx) uint8 device tensor, inside_out (0, 1) + the number of surface crossings
    at or above the node, mod 256 (odd: inside); window = (x0, y0, z0, wx, wy, wz), the region
    cut down to the mesh's integer bounding box across the rays and to region bottom ...
    min(mesh top, region top) along them, outside of which every node of the region has
    lev = inside_out.  An empty window launches nothing."""
    import numpy as np
    import torch
    axis, inside_out = int(axis), int(inside_out)
    if axis not in (0, 1, 2) or inside_out not in (0, 1):
        raise ValueError("stl_fill: axis must be 0, 1 or 2 and inside_out 0 or 1")
    tri, r0, rn, box = _stl_box(tri, region, "stl_fill")
    lo, n, cb = r0, np.zeros(3, dtype=np.int64), 0
    if box is not None:
        lo = np.maximum(box[0], r0)
        hi = np.minimum(box[1], r0 + rn - 1)
        lo[axis] = r0[axis]
        if (hi >= lo).all():
            n = hi - lo + 1
            # counters from the mesh's lowest box cell up; a mesh wholly above the window
            # counts at its top
            cb = int(min(max(box[0][axis], r0[axis]), hi[axis]))
        else:
            lo = r0
    x0, y0, z0, wx, wy, wz = window = tuple(int(v) for v in (*lo, *n))
    dev = torch.device("cuda", torch.cuda.current_device())
    lev = torch.empty((wz, wy, wx), dtype=torch.uint8, device=dev)
    nodes = wx * wy * wz
    if nodes == 0:
        return lev, window
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    L = lib()
    nray = window[3 + axis]
    cells = nodes // nray * (window[axis] + nray - cb)
    tri_d = torch.from_numpy(tri).to(dev)
    tmp = torch.empty(L.tclb_stl_tmp_bytes(len(tri)), dtype=torch.uint8, device=dev)
    cnt = torch.empty(cells, dtype=torch.int32, device=dev)
    nchunks = ctypes.c_longlong(0)
    with torch.cuda.device(dev):
        _check(L.tclb_stl_prep_rays(tri_d.data_ptr(), len(tri), x0, y0, z0, wx, wy, wz, axis, tmp.data_ptr(),
                                    tmp.numel(), ctypes.byref(nchunks), stream), "STL ray columns")
        _check(L.tclb_stl_ray_fill(tri_d.data_ptr(), len(tri), x0, y0, z0, wx, wy, wz, axis, inside_out, cb,
                                   tmp.data_ptr(), tmp.numel(), nchunks.value, cnt.data_ptr(), 4 * cells,
                                   lev.data_ptr(), stream), "STL ray fill")
    return lev, window


def stl_cuts(tri, region, dirs, stream=None):
    """surface voxelisation of the triangles `tri` ((n, 9) float64 host array, lattice
    coordinates) over the global box `region` (x0, y0, z0, nx, ny, nz) on the current device,
    bit for bit what ops.host.stl_cuts computes (csrc/device/voxel.hip k_tri_prep, k_stl_cuts).
    Returns (cuts, mask, window): window = region cut down to the mesh's integer bounding box,
    as (x0, y0, z0, wx, wy, wz), outside of which no node has a cut; cuts (26, wz, wy, wx) int16
    holding the uint16 cut of every direction of `dirs` ((26, 3) ints; 65535: none) and mask
    (wz, wy, wx) uint8, device tensors over the window.  An empty window launches nothing."""
    import numpy as np
    import torch
    dirs = np.ascontiguousarray(dirs, dtype=np.int32)
    if dirs.shape != (26, 3):
        raise ValueError("stl_cuts: dirs must be 26 x 3")
    tri, r0, rn, box = _stl_box(tri, region, "stl_cuts")
    lo, n = r0, np.zeros(3, dtype=np.int64)
    if box is not None:
        lo = np.maximum(box[0], r0)
        hi = np.minimum(box[1], r0 + rn - 1)
        n = hi - lo + 1 if (hi >= lo).all() else n
    x0, y0, z0, wx, wy, wz = window = tuple(int(v) for v in (*lo, *n))
    dev = torch.device("cuda", torch.cuda.current_device())
    nodes = wx * wy * wz
    plane = nodes + (nodes & 1)                     # every direction starts on a dword
    buf = torch.empty((26, plane), dtype=torch.int16, device=dev)
    cuts = buf[:, :nodes].view(26, wz, wy, wx)
    mask = torch.empty((wz, wy, wx), dtype=torch.uint8, device=dev)
    if nodes == 0:
        return cuts, mask, window
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    L = lib()
    tri_d, dirs_d = torch.from_numpy(tri).to(dev), torch.from_numpy(dirs).to(dev)
    tmp = torch.empty(L.tclb_stl_tmp_bytes(len(tri)), dtype=torch.uint8, device=dev)
    nchunks = ctypes.c_longlong(0)
    with torch.cuda.device(dev):
        _check(L.tclb_stl_prep(tri_d.data_ptr(), len(tri), x0, y0, z0, wx, wy, wz, tmp.data_ptr(), tmp.numel(),
                               ctypes.byref(nchunks), stream), "STL triangle boxes")
        _check(L.tclb_stl_cuts(tri_d.data_ptr(), len(tri), x0, y0, z0, wx, wy, wz, dirs_d.data_ptr(),
                               tmp.data_ptr(), tmp.numel(), nchunks.value, buf.data_ptr(), plane, mask.data_ptr(),
                               stream), "STL cut distances")
    return cuts, mask, window


def cuts_merge(dst, win, window, ys, zs, stream=None):
    """dst = min(dst, win), unsigned, where they overlap: dst (26, NZ, NY, px) int16 is a
    lattice's cut array, whose local row (k, j) lies at global (ys[j], zs[k]) (int32 device
    tensors; ghost and periodic-wrap rows repeat coordinates); win (26, wz, wy, wx) the cuts
    of `window` (x0, y0, z0, wx, wy, wz) as stl_cuts returns them
    (csrc/device/voxel.hip k_cuts_merge)"""
    import torch
    x0, y0, z0, wx, wy, wz = (int(v) for v in window)
    if not dst.is_cuda or dst.dtype != torch.int16 or dst.dim() != 4 or dst.shape[0] != 26 or \
            not dst.is_contiguous():
        raise ValueError("cuts_merge: dst must be a contiguous (26, NZ, NY, px) int16 device tensor")
    if win.device != dst.device or win.dtype != torch.int16 or tuple(win.shape) != (26, wz, wy, wx):
        raise ValueError(f"cuts_merge: win must be a (26, {wz}, {wy}, {wx}) int16 tensor on {dst.device}")
    if wx * wy * wz == 0:
        return
    if win.stride()[1:] != (wy * wx, wx, 1):
        raise ValueError("cuts_merge: the planes of win must be contiguous")
    _, NZ, NY, px = dst.shape
    for t, n in ((ys, NY), (zs, NZ)):
        if t.device != dst.device or t.dtype != torch.int32 or t.shape != (n,) or not t.is_contiguous():
            raise ValueError("cuts_merge: ys / zs must be int32 device tensors of NY / NZ entries")
    if stream is None:
        stream = torch.cuda.current_stream(dst.device).cuda_stream
    with torch.cuda.device(dst.device):
        _check(lib().tclb_cuts_merge(dst.data_ptr(), NZ, NY, px, dst.stride(0), win.data_ptr(), win.stride(0),
                                     x0, y0, z0, wx, wy, wz, ys.data_ptr(), zs.data_ptr(), stream),
               "STL cut merge")


# one record of a paint display list (csrc/device/paint.hip PaintRec)
PAINT_BOX, PAINT_SPHERE, PAINT_ELLIPSE, PAINT_WEDGE, PAINT_MASK = range(5)
PAINT_CHUNK = 4096                  # records of one k_paint launch
PAINT_REC = None


def paint_rec():
    """numpy dtype of a paint record: kind, mode (0 overwrite, 1 fill, 2 change), box (x0, x1,
    y0, y1, z0, z1: global, half open, inside the lattice), fg, mask, opt (flags of the kind),
    for PAINT_MASK bit, outside, win (x0, y0, z0, nx, ny, nz), ptr, sy, sz of the byte window,
    and the kind's doubles p[10]"""
    global PAINT_REC
    if PAINT_REC is None:
        import numpy as np
        PAINT_REC = np.dtype([("kind", "<i4"), ("mode", "<i4"), ("box", "<i4", 6), ("fg", "<u4"), ("mask", "<u4"),
                              ("opt", "<i4"), ("bit", "<i4"), ("outside", "<i4"), ("win", "<i4", 6), ("pad", "<i4"),
                              ("ptr", "<u8"), ("sy", "<i8"), ("sz", "<i8"), ("p", "<f8", 10)])
        assert PAINT_REC.itemsize == 184
    return PAINT_REC


def paint(flags, ys, zs, records, stream=None) -> int:
    """paint the display list `records` (host array of paint_rec(), drawing order) into
    `flags`, the (NZ, NY, gnx) uint32 (or int32, same bits) device flag array of a Geometry
    whose local row (k, j) lies at global (ys[j], zs[k]) (int32 device tensors; ghost and
    periodic-wrap rows repeat coordinates): per node and record in order, inside the box and
    the predicate and passing the mode, v = (v & ~mask) | fg, bit for bit the NumPy painter
    (csrc/device/paint.hip k_paint).  The list is uploaded here; a launch takes PAINT_CHUNK
    records and covers the local rows and x range of their bounding box.  Returns the number
    of launches: an empty list launches nothing."""
    import numpy as np
    import torch
    if not flags.is_cuda or flags.dim() != 3 or not flags.is_contiguous() or \
            flags.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)):
        raise ValueError("paint: flags must be a contiguous (NZ, NY, gnx) uint32 device tensor")
    NZ, NY, gnx = flags.shape
    for t, n in ((ys, NY), (zs, NZ)):
        if t.device != flags.device or t.dtype != torch.int32 or t.shape != (n,) or not t.is_contiguous():
            raise ValueError("paint: ys / zs must be int32 device tensors of NY / NZ entries")
    if not isinstance(records, np.ndarray) or records.dtype != paint_rec() or records.ndim != 1:
        raise ValueError("paint: records must be a 1-D host array of paint_rec()")
    if len(records) == 0 or flags.numel() == 0:
        return 0
    records = np.ascontiguousarray(records)
    box, kind = records["box"], records["kind"]
    if (box[:, 0] < 0).any() or (box[:, 1] > gnx).any() or (kind < 0).any() or (kind > PAINT_MASK).any() or \
            ((kind == PAINT_MASK) & (records["ptr"] == 0) & (records["win"][:, 3:].min(1) > 0)).any():
        raise ValueError("paint: a record has a box off the x range, an unknown kind or a mask without data")
    if stream is None:
        stream = torch.cuda.current_stream(flags.device).cuda_stream
    ys_h, zs_h = ys.cpu().numpy(), zs.cpu().numpy()
    rec_d = torch.from_numpy(records.view(np.uint8)).to(flags.device)
    launches = 0
    with torch.cuda.device(flags.device):
        for c in range(0, len(records), PAINT_CHUNK):
            b = box[c:c + PAINT_CHUNK]
            b = b[(b[:, 1::2] > b[:, 0::2]).all(1)]
            if not len(b):
                continue
            lo, hi = b[:, 0::2].min(0), b[:, 1::2].max(0)
            jj = np.nonzero((ys_h >= lo[1]) & (ys_h < hi[1]))[0]
            kk = np.nonzero((zs_h >= lo[2]) & (zs_h < hi[2]))[0]
            if not len(jj) or not len(kk):
                continue
            n = min(PAINT_CHUNK, len(records) - c)
            _check(lib().tclb_paint(flags.data_ptr(), NZ, NY, gnx, ys.data_ptr(), zs.data_ptr(),
                                    rec_d.data_ptr() + c * PAINT_REC.itemsize, n, PAINT_REC.itemsize,
                                    int(lo[0]), int(hi[0]), int(jj[0]), int(jj[-1]) + 1, int(kk[0]), int(kk[-1]) + 1,
                                    stream), "geometry paint")
            launches += 1
    return launches


SNAP_ALLOC_MODES = {"torch": -1, "hip": 0, "contiguous": 1, "vmm": 2}


class _SnapBlock:
    """owner of one tclb_snap_alloc range, exposed through __cuda_array_interface__ (the
    torch tensor made from it keeps this object alive; the range is freed with it)"""

    def __init__(self, nbytes: int, mode: int, device: int):
        p = ctypes.c_void_p()
        _check(lib().tclb_snap_alloc(ctypes.byref(p), nbytes, mode, device), f"snapshot allocation (mode {mode})")
        self.ptr, self.nbytes, self.mode = p.value, nbytes, mode
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (self.ptr, False),
                                         "version": 2, "strides": None}

    def __del__(self):
        if self.ptr and _lib is not None:
            _lib.tclb_snap_free(ctypes.c_void_p(self.ptr), self.mode)
            self.ptr = None


def snap_buffer(nbytes: int, mode: str, device):
    """a uint8 device tensor of nbytes from the native snapshot allocator
    (csrc/device/snapalloc.hip): mode "hip" (hipMalloc), "contiguous" (one physically
    contiguous range) or "vmm" (hipMemCreate + a 1 GiB-aligned reservation)"""
    import torch
    m = SNAP_ALLOC_MODES[mode]
    dev = torch.device(device)
    blk = _SnapBlock(int(nbytes), m, dev.index or 0)
    t = torch.as_tensor(blk, device=dev)
    assert t.data_ptr() == blk.ptr and t.numel() == nbytes
    return t


def snap_probe_ms(buf, nf: int, fs: int, reps: int = 2):
    """(read ms, write ms) of the nf field planes (fs elements apart) of snapshot candidate
    `buf` (a device tensor): best of `reps` streaming passes (csrc/device/snapalloc.hip
    tclb_snap_probe); the write pass leaves the planes zero"""
    import torch
    dev = buf.device
    stream = torch.cuda.current_stream(dev).cuda_stream
    sink = torch.zeros(4, dtype=buf.dtype, device=dev)
    es = buf.element_size()
    out = []
    for op in (1, 2):
        best = float("inf")
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _check(lib().tclb_snap_probe(buf.data_ptr(), sink.data_ptr(), fs, fs, nf, es, op, stream),
                   "snapshot probe")
            e1.record()
            e1.synchronize()
            best = min(best, e0.elapsed_time(e1))
        out.append(best)
    return out[0], out[1]
