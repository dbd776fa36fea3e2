"""Multi-process (gloo) decomposition tests: N ranks must reproduce 1 rank bit-for-bit
(halo exchange, border/interior overlap, periodic wrap, global all-reduce)."""
import json
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

import dist_worker
from tclb_amd.parallel.comm import LoopbackComm


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("native", ["1", "0"])
@pytest.mark.parametrize("model,shape,world,overlap", [
    ("d3q27", (16, 8, 12), 2, True),
    ("d3q27", (16, 8, 10), 3, False),
    ("d3q27", (16, 8, 16), 4, True),
    ("d2q9", (24, 18, 1), 2, True),
])
def test_ranks_match_single(tmp_path, model, shape, world, overlap, native):
    """N ranks = 1 rank bit for bit, through the native multi-rank loop (native=1: C++
    loop, halo plan executed by gloo through the loop's callback transport) and through
    the Python step path (native=0)"""
    steps = 5
    ref = dist_worker.run_case(model, shape, steps, LoopbackComm())
    out = str(tmp_path / "full.npy")
    mp.start_processes(dist_worker.worker, args=(world, _port(), model, shape, steps, out, overlap, None, native),
                       nprocs=world, start_method="spawn", join=True)
    full = np.load(out)
    r = ref.fields_interior().numpy()
    assert full.shape == r.shape
    assert np.array_equal(full, r)
    g = json.load(open(out + ".json"))
    assert g.pop("_native") == ("callback" if native == "1" else None)
    for k, v in ref.globals.items():
        assert abs(g[k] - v) <= 1e-11 * (1 + abs(v)), k


@pytest.mark.parametrize("model,shape,world", [
    ("d3q27", (16, 8, 12), 2),          # prev == next: both directions to one peer
    ("d3q27", (16, 8, 10), 3),
    ("d3q27_pf_velocity_thermo", (16, 8, 12), 2),   # multi-stage, stencil-2 fields
])
def test_native_plan_pairs_by_issue_order(tmp_path, monkeypatch, model, shape, world):
    """the native loop's halo plan (parallel/native.py phase_a) with sends and receives
    paired by issue order per peer, tags ignored — the semantics of RCCL's grouped
    ncclSend/ncclRecv — still equals one rank bit for bit (2 ranks: the two directions go to
    the same peer, so only the plan order keeps them apart)"""
    monkeypatch.setenv("TCLB_DIST_ORDER_MATCH", "1")
    steps = 4
    out = str(tmp_path / "full.npy")
    if model == "d3q27":
        ref = dist_worker.run_case(model, shape, steps, LoopbackComm())
        fn, args = dist_worker.worker, (world, _port(), model, shape, steps, out, True, None, "1")
    else:
        import sys
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        from model_cases import run
        ref = run(model, "cpu", steps=steps)
        fn, args = dist_worker.worker_catalog, (world, _port(), model, steps, out, True)
    mp.start_processes(fn, args=args, nprocs=world, start_method="spawn", join=True)
    assert np.array_equal(np.load(out), ref.fields_interior().numpy())


# multi-stage, stencil and multi-population models (verdict r02: the overlapped
# halo-mirror step diverged for these before the per-side mirror buffers)
CATALOG_CASES = ["d3q27_pf_velocity_thermo", "d3q19_kuper", "d2q9_csf", "d3q27_PSM_NEBB",
                 "d3q27_tePSM_per_NEBB"]


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("model", CATALOG_CASES)
def test_catalog_ranks_match_single(tmp_path, model, world):
    """N gloo ranks (overlapped step, border kernels packing the halo) reproduce one
    rank bit for bit; globals to 1e-11"""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from model_cases import run
    steps = 3
    ref = run(model, "cpu", steps=steps)
    out = str(tmp_path / "full.npy")
    mp.start_processes(dist_worker.worker_catalog, args=(world, _port(), model, steps, out, True),
                       nprocs=world, start_method="spawn", join=True)
    full = np.load(out)
    r = ref.fields_interior().numpy()
    assert full.shape == r.shape
    assert np.array_equal(full, r), np.abs(full - r).max()
    g = json.load(open(out + ".json"))
    for k, v in ref.globals.items():
        assert abs(g[k] - v) <= 1e-11 * (1 + abs(v)), k


@pytest.mark.parametrize("shape,world,grid", [
    ((16, 8, 12), 4, (2, 2)),      # explicit Y x Z grid
    ((12, 9, 8), 6, (3, 2)),
    ((8, 6, 3), 4, None),          # z too thin for 4 slabs: automatic Y x Z fallback
])
def test_yz_grid_matches_single(tmp_path, shape, world, grid):
    """reference MPIDivision (src/Solver.cpp.Rt:288-370): a Y x Z process grid with
    two-phase halos (z planes, then y rows incl. the z ghosts = edge ghosts) reproduces
    one rank bit-for-bit, corners included (d3q27 reads all 26 neighbours)"""
    steps = 4
    ref = dist_worker.run_case("d3q27", shape, steps, LoopbackComm())
    out = str(tmp_path / "full.npy")
    mp.start_processes(dist_worker.worker, args=(world, _port(), "d3q27", shape, steps, out, None, grid),
                       nprocs=world, start_method="spawn", join=True)
    assert open(out + ".axis").read() == "3"
    full = np.load(out)
    assert np.array_equal(full, ref.fields_interior().numpy())
    g = json.load(open(out + ".json"))
    for k, v in ref.globals.items():
        assert abs(g[k] - v) <= 1e-11 * (1 + abs(v)), k


@pytest.mark.parametrize("shape,world,grid", [
    ((16, 8, 12), 4, (2, 2)),
    ((12, 9, 8), 6, (3, 2)),
])
def test_yz_grid_pairs_by_issue_order(tmp_path, monkeypatch, shape, world, grid):
    """the Y x Z grid's native plan (packed z phase, staged y rows) with sends and receives
    paired by issue order per peer, tags ignored (RCCL's grouped send/receive semantics),
    equals one rank bit for bit"""
    monkeypatch.setenv("TCLB_DIST_ORDER_MATCH", "1")
    steps = 3
    ref = dist_worker.run_case("d3q27", shape, steps, LoopbackComm())
    out = str(tmp_path / "full.npy")
    mp.start_processes(dist_worker.worker, args=(world, _port(), "d3q27", shape, steps, out, None, grid, "1"),
                       nprocs=world, start_method="spawn", join=True)
    assert open(out + ".axis").read() == "3"
    assert np.array_equal(np.load(out), ref.fields_interior().numpy())
    assert json.load(open(out + ".json"))["_native"] == "callback"


def test_grid_alternating_actions(tmp_path, monkeypatch):
    """a multi-stage model on a 2 x 2 grid alternating two actions whose native plans
    have different staging sizes (Iteration / TempToSteadyState) equals one rank"""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from model_cases import make_case, perturb
    model = "d3q27_pf_velocity_thermo"
    ref = make_case(model, "cpu")
    ref.init()
    perturb(ref)
    dist_worker.alternate_actions(ref, 2)
    monkeypatch.setenv("TCLB_GRID", "2,2")
    monkeypatch.setenv("TCLB_DIST_ORDER_MATCH", "1")
    out = str(tmp_path / "full.npy")
    mp.start_processes(dist_worker.worker_catalog, args=(4, _port(), model, 2, out, True, "1", True),
                       nprocs=4, start_method="spawn", join=True)
    assert np.array_equal(np.load(out), ref.fields_interior().numpy())


def test_native_particles_four_ranks_issue_order(tmp_path, monkeypatch):
    """config 5's model on 4 z-slab ranks through the native loop (particle stages in the
    loop, forces all-reduced), sends and receives paired by issue order as RCCL pairs them:
    three spheres straddle / wrap / move across the rank cuts.  Equals one rank to
    rounding (the force sum's order differs), every rank runs the loop path"""
    monkeypatch.setenv("TCLB_DIST_ORDER_MATCH", "1")
    shape, steps = (16, 16, 24), 8
    ref = dist_worker.particle_case(shape, steps, LoopbackComm())
    out = str(tmp_path / "full.npy")
    mp.start_processes(dist_worker.worker_particles, args=(4, _port(), shape, steps, out),
                       nprocs=4, start_method="spawn", join=True)
    meta = json.load(open(out + ".json"))
    assert meta["path"] == ["loop"] * 4 and meta["transport"] == ["callback"] * 4
    full = np.load(out)
    r = ref.fields_interior().numpy()
    assert np.allclose(full, r, rtol=0, atol=1e-12), np.abs(full - r).max()
    p = np.load(out + ".part.npz")
    px = np.asarray(ref.particles.x, dtype=float)
    assert abs(px[2, 2] - (shape[2] / 4 - 1.2)) > 2.0          # the z mover changed rank
    for k, want in (("x", px), ("v", np.asarray(ref.particles.v, dtype=float)),
                    ("force", np.asarray(ref.particles.force, dtype=float))):
        for rk in range(4):
            assert np.allclose(p[k][rk], want, rtol=1e-9, atol=1e-12), (k, rk)


def test_choose_grid_minimises_cut():
    from tclb_amd.parallel.decomp import choose_grid, decompose
    assert choose_grid(512, 512, 512, 8) in ((2, 4), (4, 2))
    assert choose_grid(1280, 130, 130, 16) == (4, 4)
    s = decompose(64, 32, 32, 5, 64)         # 32 z planes cannot hold 64 slabs
    assert s.axis == 3 and (s.py, s.pz) == (8, 8) and (s.ry, s.rz) == (5, 0)
