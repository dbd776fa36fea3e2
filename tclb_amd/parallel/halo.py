"""Halo geometry of a lattice: which fields travel in which direction, the ghost depth and
extent of a split axis, the mirror of a border launch, the kind of a stage.  The one copy
read by both step paths: the Python step path (tclb_amd/lattice.py run_action) and the
plan of the native action loop (parallel/native.py, tclb_rt/dist_loop.hpp)."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

from ..ops.abi import MIRROR_FIELDS

FIXED_POINT_SWEEPS = 100   # reference: for (int fix=0; fix<100; fix++), src/Lattice.cu.Rt:484


def runs(idx: Sequence[int]) -> List[Tuple[int, int]]:
    """contiguous runs [a, b) of an index list"""
    out: List[Tuple[int, int]] = []
    for i in sorted(idx):
        if out and out[-1][1] == i:
            out[-1] = (out[-1][0], i + 1)
        else:
            out.append((i, i + 1))
    return out


def side_fields(lat, axis: int, fields: Optional[Sequence[int]] = None) -> Tuple[List[int], List[int]]:
    """(lo, hi) of the exchanged `fields` (None: all) along `axis`, in field order.
    lo: read from below, so my top planes go up and fill the next rank's lower ghost;
    hi: read from above, so my bottom planes go down into the previous rank's upper ghost.
    lat.halo_sets is read at every call (handlers/embed.py swaps it around an exchange)."""
    lo, hi = lat.halo_sets[axis]
    if fields is None:
        return lo, hi
    fs = set(fields)
    return [i for i in lo if i in fs], [i for i in hi if i in fs]


def axis_extent(lat, axis: int) -> Tuple[int, int]:
    """(ghost depth, interior extent) of a split axis: 1 = y rows, 2 = z planes"""
    return (lat.gz, lat.shape[2]) if axis == 2 else (lat.gy, lat.shape[1])


def mirror_spec(lat, axis: int, fields: Sequence[int], r0: int):
    """the halo mirror of a border launch starting at plane / row r0 (Launch.mfs, msy, msz,
    moy, moz, mslot; core.hpp mirror_store): its stores of `fields` also land in a packed
    buffer [len(fields)][g planes].  Returns (mfs, msy, msz, moy, moz, slot); slot[f] is
    the position of field f in the buffer, -1 for a field that is not mirrored."""
    g, _ = axis_extent(lat, axis)
    px = lat.px
    if axis == 2:
        dims = (g * lat.NY * px, px, lat.NY * px, lat.gy, -r0)
    else:
        # g rows of every z plane; for NZ == 1, the only y slab NativeLoop.supported
        # admits, this is the native loop's [field][g rows]: mfs = g * px
        dims = (lat.NZ * g * px, px, g * px, -r0, lat.gz)
    slot = [-1] * MIRROR_FIELDS
    for j, f in enumerate(fields):
        slot[f] = j
    return dims + (slot,)


def stage_mode(k: int, st) -> int:
    """kind of the k-th stage of an action: 0 plain, 1 out of place (it reads, through a
    stencil, a field it also writes), 2 fixed point (FIXED_POINT_SWEEPS sweeps of 1)"""
    if k > 0 and st.fixed_point:
        return 2
    if k > 0 and st.snapshot_reads:
        return 1
    return 0
