#!/usr/bin/env python3
"""Host against device colour frames (render.write_png encode="host" | "device"): a periodic
d2q9 box of n x n with a solid cylinder, driven by a body force, 300 steps, then frames of it.
Host clock around synchronised calls, one process, the two paths alternating, the first
round dropped.  Besides the two whole calls the parts are timed on their own: frame() and
png_write of the host path; encode (Lattice.color and png_encode), copy-back and file write
of the device path.  The two images are compared and the device file is decoded.
Usage: png_frame_timing.py OUTDIR [n ...]"""
import os
import struct
import sys
import time
import zlib

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tclb_amd.io import render  # noqa: E402
from tclb_amd.lattice import Lattice  # noqa: E402
from tclb_amd.ops import device as D  # noqa: E402
from tclb_amd.ops.host import png_write  # noqa: E402

REPS = 5
out = sys.argv[1]
SIZES = [int(a) for a in sys.argv[2:]] or [1024, 2048, 4096]
os.makedirs(out, exist_ok=True)


def now():
    torch.cuda.synchronize()
    return time.perf_counter()


def decode(b):
    p, idat = 8, b""
    while p < len(b):
        n = struct.unpack(">I", b[p:p + 4])[0]
        t, d = b[p + 4:p + 8], b[p + 8:p + 8 + n]
        assert zlib.crc32(t + d) == struct.unpack(">I", b[p + 8 + n:p + 12 + n])[0], t
        if t == b"IHDR":
            w, h = struct.unpack(">II", d[:8])
        if t == b"IDAT":
            idat += d
        p += 12 + n
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 4 * w)
    px = rows[:, 1:].reshape(h, w, 4).copy()
    sub = rows[:, 0] == 1
    px[sub] = np.cumsum(px[sub], axis=1, dtype=np.uint8)
    return px


for n in SIZES:
    lat = Lattice("d2q9", (n, n, 1), device=torch.device("cuda"))
    m = lat.model
    fl = np.full((lat.NZ, lat.NY, n), m.node_type("MRT").value, dtype=np.uint32)
    lat.set_flags(fl)
    solid = m.node_type("Solid")
    yy, xx = np.mgrid[0:lat.NY, 0:n]
    cyl = (xx - n // 4) ** 2 + (yy - lat.NY // 2 - n // 50) ** 2 < (n // 16) ** 2
    fl[:, cyl] = (fl[:, cyl] & ~np.uint32(solid.mask)) | np.uint32(solid.value)
    lat.set_flags(fl)
    lat.set_setting("Viscosity", 0.02)
    lat.set_setting("GravitationX", 1e-4)
    lat.init()
    lat.iterate(300)
    ph, pd = os.path.join(out, f"h{n}.png"), os.path.join(out, f"d{n}.png")
    T = {k: [] for k in ("host", "host_frame", "host_write", "device", "dev_encode", "dev_copy", "dev_write")}
    for rep in range(REPS + 1):                      # the first repetition warms up and is dropped
        t0 = now()
        ih = render.write_png(lat, ph, encode="host")
        t1 = now()
        idv = render.write_png(lat, pd, encode="device")
        t2 = now()
        img = render.frame(lat)
        t3 = now()
        png_write(ph, img)
        t4 = now()
        lw = lat.color().permute(2, 0, 1).contiguous()
        pix = torch.empty((n, n, 4), dtype=torch.uint8, device="cuda")
        data = D.png_encode(lw, pixels=pix)
        t5 = now()
        dh, _ = data.cpu().numpy(), pix.cpu().numpy()
        t6 = now()
        with open(pd, "wb") as f:
            f.write(dh.data)
        t7 = now()
        if rep:
            for k, v in zip(T, (t1 - t0, t3 - t2, t4 - t3, t2 - t1, t5 - t4, t6 - t5, t7 - t6)):
                T[k].append(v * 1e3)
    assert np.array_equal(ih, idv), "host and device images differ"
    assert np.array_equal(decode(open(pd, "rb").read()), ih), "device file does not decode to the host image"
    sizes = os.path.getsize(ph), os.path.getsize(pd)
    print(f"n={n} bytes host={sizes[0]} device={sizes[1]} raw={n * (4 * n + 1)}", flush=True)
    for k, v in T.items():
        print(f"n={n} {k:11s} ms: median {np.median(v):9.2f}  min {min(v):9.2f}  max {max(v):9.2f}  all "
              + " ".join(f"{x:.2f}" for x in v), flush=True)
    os.remove(ph)
    os.remove(pd)
    del lat
    torch.cuda.empty_cache()
