#!/usr/bin/env python3
"""Host against device STL fill (<STL side="in">): the work of draw_stl up to the painting, i.e.
ops.host.stl_fill over the region against ops.device.stl_fill and the copy of its window to the
host, for a UV sphere of 200 x 100 segments (39 600 triangles) filling a cubic box.  Both
results are compared over the whole region before anything is timed.  One JSON line per case."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tclb_amd.ops import device as D  # noqa: E402
from tclb_amd.ops import host as H  # noqa: E402


def sphere(nu, nv, R, c):
    th, ph = np.pi * np.arange(nv + 1) / nv, 2 * np.pi * np.arange(nu + 1) / nu
    V = np.stack([np.sin(th)[:, None] * np.cos(ph), np.sin(th)[:, None] * np.sin(ph),
                  np.cos(th)[:, None] * np.ones_like(ph)], -1) * R + c
    T = []
    for j in range(nv):
        for i in range(nu):
            if j > 0:
                T.append([V[j, i], V[j, i + 1], V[j + 1, i + 1]])
            if j < nv - 1:
                T.append([V[j, i], V[j + 1, i + 1], V[j + 1, i]])
    return np.array(T).reshape(-1, 9)


def timed(f, warm, reps):
    ts = []
    for k in range(warm + reps):
        t = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t)
    ts = sorted(ts[warm:])
    return {"median_ms": round(ts[len(ts) // 2] * 1e3, 3), "min_ms": round(ts[0] * 1e3, 3),
            "max_ms": round(ts[-1] * 1e3, 3), "runs": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boxes", default="128,256")
    ap.add_argument("--axes", default="1,0")
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("stl_fill_timing: no GPU")
    for n in (int(v) for v in a.boxes.split(",")):
        # the sphere of "Device STL cuts" (radius 50.3 in 128^3), scaled with the box
        tri = sphere(200, 100, 50.3 * n / 128, np.array([0.5 * n + 0.37, 0.5 * n - 0.21, 0.5 * n + 0.11]))
        tri = np.round(tri * 1e5) * 1e-5 + np.array([0.1403e-4, 0.1687e-4, 0.1987e-4] * 3)
        region = (0, 0, 0, n, n, n)
        for axis in (int(v) for v in a.axes.split(",")):
            def device():
                lev, win = D.stl_fill(tri, region, axis, 0)
                return lev.cpu().numpy(), win              # the copy synchronises

            ref = H.stl_fill(tri, region, axis, 0)
            lev, (x0, y0, z0, wx, wy, wz) = device()
            full = np.zeros_like(ref)
            full[z0:z0 + wz, y0:y0 + wy, x0:x0 + wx] = lev
            print(json.dumps({"box": n, "ray_axis": "xyz"[axis], "triangles": len(tri), "window": [wx, wy, wz],
                              "inside": int((ref & 1).sum()), "equal": bool(np.array_equal(full, ref)),
                              "host": timed(lambda: H.stl_fill(tri, region, axis, 0), 0, a.host_reps),
                              "device": timed(device, 2, a.reps)}), flush=True)


if __name__ == "__main__":
    main()
