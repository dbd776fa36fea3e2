"""The halo geometry of the two step paths (tclb_amd/parallel/halo.py): the native action
loop's plan equals, byte for byte, the plan recorded before the geometry moved into one
module (tests/data/halo_plans.json: the LoopPlan with its pointers zeroed, its HaloOp,
PackOp, SegOp and MirrorSpec arrays, the run table and the staging byte count), and the
mirror the Python step path writes into Launch for its border launches equals the plan's
MirrorSpecs field for field."""
import json
import os

import numpy as np
import pytest

from tclb_amd.lattice import Lattice
from tclb_amd.parallel.comm import LoopbackComm
from tclb_amd.parallel.native import LoopPlan, MirrorSpec, NativeLoop

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "halo_plans.json")
POINTERS = ("ops", "packs", "runs", "segs", "dsegs", "mirrors", "scratch", "staging", "series", "svals", "sslopes",
            "zonal", "samplers", "part")

# name: (model, shape, action, exchange-only field tuple or None)
CASES = {
    "z_slab": ("d3q27", (16, 8, 12), "Iteration", None),
    "y_slab": ("d2q9", (16, 24, 1), "Iteration", None),
    "multi_stage": ("d3q27_pf_velocity", (8, 8, 12), "Iteration", None),     # split stage, pack segments, stencil 2
    "csf_iteration": ("d2q9_csf", (32, 24, 1), "Iteration", None),           # the shape of tests/csf_case.py
    "csf_init": ("d2q9_csf", (32, 24, 1), "Init", None),                     # fixed-point stage, runs, scratch
    "exchange_only": ("d3q27", (16, 8, 12), "Iteration", (0, 1, 2)),
}


def _lattice(model, shape):
    return Lattice(model, shape, comm=LoopbackComm(exercise_dist_path=True), overlap=True)


def dump_plan(lat, action, fields):
    P, keep = NativeLoop(lat).plan(action, fields)
    ops, packs, runs, segs, mirrors = keep[:5]
    flat = LoopPlan.from_buffer_copy(bytes(P))
    for name in POINTERS:
        setattr(flat, name, None)
    for i in range(4):
        flat.peer_stg[i] = None
    staging = sum(t.numel() for t in keep[5:] if hasattr(t, "numel"))
    return {"plan": bytes(flat).hex(), "ops": bytes(ops).hex(), "packs": bytes(packs).hex(),
            "runs": bytes(runs).hex(), "segs": bytes(segs).hex(), "mirrors": bytes(mirrors).hex(),
            "staging_bytes": staging}


@pytest.mark.parametrize("case", list(CASES))
def test_native_plan_equals_recorded(case):
    model, shape, action, fields = CASES[case]
    got = dump_plan(_lattice(model, shape), action, fields)
    want = json.load(open(FIXTURE))[case]
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k] == want[k], k


@pytest.mark.parametrize("case", ["z_slab", "y_slab", "multi_stage"])
def test_python_path_mirror_equals_plan(case, monkeypatch):
    """one step of the Python path: every border launch's (mfs, msy, msz, moy, moz, mslot)
    is the MirrorSpec the native plan gives that stage's low / high border, and a stage
    the plan does not mirror launches no mirrored border"""
    model, shape, action, _ = CASES[case]
    monkeypatch.setenv("TCLB_DIST_NATIVE", "0")
    lat = _lattice(model, shape)
    assert lat._dist is None and lat.halo_mirror
    m = lat.model
    coll = next(t for t in m.node_types if t.group == "COLLISION")
    lat.set_flags(np.full((lat.NZ, lat.NY, shape[0]), coll.value, dtype=np.uint16 if m.flag_bits == 16 else np.uint32))
    lat.init()
    axis = lat.slab.axis
    seen = {}
    run = lat.lib.run

    def spy(L, prec):
        if L.mbase:
            lo = (L.zlo if axis == 2 else L.ylo) == 0
            seen[(L.stage, "mir_lo" if lo else "mir_hi")] = (L.mfs, L.msy, L.msz, L.moy, L.moz, bytes(L.mslot))
        return run(L, prec)
    monkeypatch.setattr(lat.lib, "run", spy)
    lat.run_action(action)

    P, keep = NativeLoop(lat).plan(action)
    mirrors = keep[4]
    want = {}
    for k in range(P.nstages):
        S = P.st[k]
        for side in ("mir_lo", "mir_hi"):
            i = getattr(S, side)
            if i >= 0:
                M: MirrorSpec = mirrors[i]
                want[(S.stage, side)] = (M.mfs, M.msy, M.msz, M.moy, M.moz, bytes(M.slot))
    assert want and seen == want
