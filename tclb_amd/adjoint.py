"""Discrete adjoint of the lattice time stepping (reference: Lattice::Iteration_Adj,
IterateTill and the snapshot hierarchy, src/Lattice.cu.Rt:46-61,542-613,843-890).

Every model is differentiable: the AD executor re-runs a stage with dual numbers and
applies the transposed local Jacobian — on the CPU (csrc/include/tclb/executor_ad.hpp,
OpenMP) or on the GPU (csrc/include/tclb_ad/executor_ad_hip.hpp: windowed tangents,
device fp64 atomics for the adjoint push), following the lattice's device.  This module
drives it over actions (reverse stage order, in-place stages pass the adjoint of the
fields they do not write through), returns ghost-plane contributions to their owners
(Lattice.reverse_halo: the periodic image on one rank, the neighbour rank over the
communicator otherwise — every rank runs the adjoint of its own slab), and runs
unsteady adjoints with checkpointed recomputation of the primal trajectory.

Objective:  J = sum over the recorded iterations of the ``Objective`` global (the
weighted sum of the model's globals, ``<G>InObj`` zonal weights), as in the reference.
Gradients:  d J / d (initial state) — including parameter densities such as design
fields, which are carried unchanged through the iterations — and d J / d (selected
global or zonal settings).
"""
from __future__ import annotations

import ctypes
import math
import os
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .ops import abi
from .parallel.halo import runs


class AdjointError(RuntimeError):
    pass


class _AdSegPlan(ctypes.Structure):
    """mirror of tclb::AdSegPlan (csrc/include/tclb_rt/ad_loop.hpp)"""
    _fields_ = [("nsteps", ctypes.c_int), ("par0", ctypes.c_int), ("dual_count", ctypes.c_int),
                ("mode", ctypes.c_int), ("states", ctypes.c_void_p), ("iters", ctypes.c_void_p),
                ("abuf", ctypes.c_void_p * 2), ("ctx", ctypes.c_void_p * 2), ("abytes", ctypes.c_longlong)]


class Adjoint:
    def __init__(self, lat, settings: Sequence[str] = (), zonal: Sequence[str] = (), reverse: bool = True):
        if lat.sdtype != torch.float64:
            raise AdjointError("adjoint needs double precision storage")
        self.lat = lat
        self.lib = abi.load_ad(lat.model.name, gpu=lat.is_gpu)
        dev = lat.device
        self.set_mask = torch.tensor([1 if s in settings else 0 for s in lat.gsettings] or [0], dtype=torch.int32,
                                     device=dev)
        self.zon_mask = torch.tensor([1 if s in zonal else 0 for s in lat.zsettings] or [0], dtype=torch.int32,
                                     device=dev)
        self.gset = torch.zeros(max(1, len(lat.gsettings)), dtype=torch.float64, device=dev)
        self.gzon = torch.zeros(lat.zvals.size if lat.zvals.size else 1, dtype=torch.float64, device=dev)
        self.scratch = torch.zeros_like(lat.snaps[0])
        self.series_grads = {}
        self.ctx = abi.AdCtx()
        # the GPU executor reads its context from device memory
        self._ad_cover = {}   # stage -> largest input count of a node (GPU pass sizing)
        self._ctx_dev = torch.zeros(ctypes.sizeof(abi.AdCtx), dtype=torch.uint8, device=dev) if lat.is_gpu else None
        # reverse sweeps of the model (Model.set_reverse) are used when no setting is seeded;
        # reverse=False forces the dual-number passes everywhere (tests, A/B)
        self.reverse = bool(lat.model.reverse) and reverse
        self._seeded = bool(list(settings) or list(zonal))
        self._abuf = None             # persistent (aout, ain) ping-pong buffers of _ad_stage
        # GPU: per stage, the nodes without a reverse sweep (recorded on the stage's first
        # call, index list + count); invalidated when the node flags change
        self._dual_bufs: Dict[int, torch.Tensor] = {}
        self._dual_count: Dict[int, int] = {}
        self._dual_flags = None
        self._ctx_bytes = [b"", b""]
        self._ctx_devs = ([self._ctx_dev, torch.zeros_like(self._ctx_dev)] if self._ctx_dev is not None
                          else [None, None])
        self._ovf = torch.zeros(1, dtype=torch.int32, device=dev) if lat.is_gpu else None
        self.native_steps = 0         # reverse steps run by the native segment loop

    # ------------------------------------------------------------------ one action
    def _ad_stage(self, si: int, inp: torch.Tensor, aout: torch.Tensor, obj_weight: float) -> torch.Tensor:
        """adjoint of one stage launch: returns a new tensor dJ/d(stage inputs).

        The adjoint buffers the executor reads and writes are persistent (their addresses
        sit in the AdCtx, which is uploaded only when it changes) and the AdCtx is read
        back only on the first call of a stage (to size the tangent windows): the later
        calls of an adjoint sweep run without a host synchronisation; window overflow is
        accumulated on the device and checked once per sweep (check_overflow)."""
        lat = self.lat
        if self._abuf is None:
            self._abuf = (torch.zeros_like(aout), torch.zeros_like(aout))
        # ping-pong: the output adjoint of one call is the input of the next, so in a sweep
        # no adjoint snapshot is copied; each parity has its own device AdCtx
        if aout is self._abuf[1]:
            par = 1
        else:
            par = 0
            if aout is not self._abuf[0]:
                self._abuf[0].copy_(aout)
        aout_b, ain = self._abuf[par], self._abuf[1 - par]
        ain.zero_()
        L = self._stage_launch(si, inp)
        c = self.ctx
        c.aout = aout_b.data_ptr()
        c.ain = ain.data_ptr()
        c.gset = self.gset.data_ptr()
        c.gzon = self.gzon.data_ptr()
        c.set_mask = self.set_mask.data_ptr()
        c.zon_mask = self.zon_mask.data_ptr()
        c.obj_weight = obj_weight
        c.overflow = 0
        c.reserved = 0
        # GPU: tangent windows up to the largest input count a node of this stage read in an
        # earlier call (0 = all TCLB_AD_K); the device reports the count in AdCtx.reserved
        cover = self._ad_cover.get(si, 0) if self._ctx_dev is not None else 0
        L.reserved0 = cover
        # hand-written reverse sweeps (Model.set_reverse) on the nodes they cover, unless a
        # setting gradient is asked for (the sweeps push state adjoints only).  CPU: one
        # pass, reverse or dual per node; GPU: launch mode 1 (reverse sweeps, recording the
        # other nodes once) then mode 2 (dual windows over the recorded nodes only), so no
        # wave mixes the two (executor_ad_hip.hpp)
        rev = self.reverse and not self._seeded
        L.next[5] = 1 if rev else 0
        first = si not in self._ad_cover
        if self._ctx_dev is not None:
            raw = bytes(c)
            dev_ctx = self._ctx_devs[par]
            if first or raw != self._ctx_bytes[par]:
                dev_ctx.copy_(torch.frombuffer(bytearray(raw), dtype=torch.uint8))
                self._ctx_bytes[par] = raw
            self._ctx_dev = dev_ctx
            L.ext[5] = dev_ctx.data_ptr()
        else:
            L.ext[5] = ctypes.cast(ctypes.pointer(c), ctypes.c_void_p)
        if rev and self._ctx_dev is not None:
            if self._dual_flags != lat.flags_version:
                self._dual_bufs.clear()
                self._dual_count.clear()
                self._dual_flags = lat.flags_version
            nodes = (L.xhi - L.xlo) * (L.yhi - L.ylo) * (L.zhi - L.zlo)
            buf = self._dual_bufs.get(si)
            if buf is None or buf.numel() < nodes + 1:
                buf = self._dual_bufs[si] = torch.zeros(nodes + 1, dtype=torch.int32, device=lat.device)
                self._dual_count.pop(si, None)
            count = self._dual_count.get(si)
            if count is None:
                buf[0] = 0
            L.aux = buf.data_ptr()
            L.qcomp = 0 if count is None else 1          # record the dual nodes on the first call
            self.lib.run(L)
            if count is None:
                count = self._dual_count[si] = int(buf[0].item())
            L.next[5], L.qcomp = 2, count
            if count > 0:
                self.lib.run(L)
            elif first:
                self._ad_cover[si] = -1                   # nothing for the dual windows
                first = False
        else:
            self.lib.run(L)
        if self._ctx_dev is not None:
            if first:
                c = abi.AdCtx.from_buffer_copy(bytes(self._ctx_dev.cpu().numpy()))
                w = self.lib.window
                covered = -(-cover // w) * w if cover > 0 else self.lib.tangents
                if c.reserved > covered:
                    # a node read more inputs than the windows covered: the windows partition
                    # the Jacobian columns, so the missing ones are added by the remaining windows
                    L.reserved2, L.reserved0 = covered, 0
                    self.lib.run(L)
                    c = abi.AdCtx.from_buffer_copy(bytes(self._ctx_dev.cpu().numpy()))
                self._ad_cover[si] = max(cover, c.reserved)
                if c.overflow:
                    raise AdjointError(f"model {lat.model.name}: a node needed more than "
                                       f"{self.lib.tangents} AD tangents")
            else:
                # the device sets AdCtx.overflow; keep it (the next upload resets it)
                o = abi.ADCTX_OVERFLOW_OFFSET
                flag = self._ctx_dev[o:o + 4].view(torch.int32)
                torch.maximum(self._ovf, flag, out=self._ovf)
        elif c.overflow:
            raise AdjointError(f"model {lat.model.name}: a node needed more than {self.lib.tangents} AD tangents")
        lat.reverse_halo(ain)
        return ain

    def _stage_launch(self, si: int, inp: torch.Tensor) -> abi.Launch:
        """the Launch of one AD stage call (everything but the executor context / mode)"""
        lat = self.lat
        L = lat._base_launch()
        lat._sync_settings()
        L.settings = lat.settings_t.data_ptr()
        L.zonal = lat.zonal_t.data_ptr()
        L.nzones = lat.zvals.shape[1]
        L.flags = lat.flags.data_ptr()
        L.flags_gen = lat.flags_version
        L.in_ = inp.data_ptr()
        L.out = self.scratch.data_ptr()
        L.stage = si
        L.glob = 1
        L.iter = lat.iter
        L.globals_ = lat.globals_t.data_ptr()
        L.reserved2 = 0
        L.stream = lat._stream()
        if lat.turb_t is not None:
            L.ext[0] = lat.turb_t.data_ptr()
            L.next[0] = lat.turb_t.shape[0]
            L.time_shift = lat.turb_time_wn
        if lat.cuts is not None:
            L.ext[1] = lat.cuts.data_ptr()
            L.next[1] = lat.cuts.numel()
        return L

    def _native_ready(self, action: str) -> bool:
        """the executor of the action's (single) stage has been sized by a first call"""
        m = self.lat.model
        act = m.action(action)
        if len(act.stages) != 1:
            return False
        si = m.stage_index(act.stages[0])
        if self._ctx_dev is None:
            return True                  # the CPU executor needs no sizing
        if si not in self._ad_cover:
            return False
        return not (self.reverse and not self._seeded and si not in self._dual_count)

    def _segment_native(self, a: torch.Tensor, states: List[torch.Tensor], iters: List[int],
                        action: str, obj_weight: float = 1.0) -> Optional[torch.Tensor]:
        """the reverse steps of one checkpoint segment in one native call
        (tclb_rt/ad_loop.hpp ad_segment): states[i] / iters[i] are the input state and
        iteration of the i-th reverse step.  Taken for single-stage actions that save every
        field, on a rank without ghost planes and without zonal series, once the stage's
        executor sizing is known (its first call, through _ad_stage); None otherwise."""
        lat = self.lat
        m = lat.model
        act = m.action(action)
        if (len(act.stages) != 1 or lat.g != 0 or lat.zseries or not states or self._abuf is None
                or os.environ.get("TCLB_AD_NATIVE", "1") == "0"):
            return None
        si = m.stage_index(act.stages[0])
        gpu = self._ctx_dev is not None
        if len(lat._saved_fields(m.stage(act.stages[0]))) != lat.nf or not self._native_ready(action):
            return None
        rev = self.reverse and not self._seeded
        if a is self._abuf[1]:
            par0 = 1
        else:
            par0 = 0
            if a is not self._abuf[0]:
                self._abuf[0].copy_(a)
        L = self._stage_launch(si, states[0])
        cover = self._ad_cover.get(si, 0) if gpu else 0
        L.reserved0 = max(0, cover)
        # one executor context per parity: aout = abuf[par], ain = abuf[1 - par]
        ctxs = []
        for par in (0, 1):
            c = abi.AdCtx.from_buffer_copy(bytes(self.ctx))
            c.aout, c.ain = self._abuf[par].data_ptr(), self._abuf[1 - par].data_ptr()
            c.gset, c.gzon = self.gset.data_ptr(), self.gzon.data_ptr()
            c.set_mask, c.zon_mask = self.set_mask.data_ptr(), self.zon_mask.data_ptr()
            c.obj_weight, c.overflow, c.reserved = obj_weight, 0, 0
            if gpu:
                raw = bytes(c)
                if raw != self._ctx_bytes[par]:
                    self._ctx_devs[par].copy_(torch.frombuffer(bytearray(raw), dtype=torch.uint8))
                    self._ctx_bytes[par] = raw
                ctxs.append(self._ctx_devs[par].data_ptr())
            else:
                ctxs.append(c)
        P = _AdSegPlan()
        n = len(states)
        P.nsteps, P.par0 = n, par0
        if rev:
            P.mode = 1
            P.dual_count = self._dual_count.get(si, 0) if gpu else 0
            if gpu:
                L.aux = self._dual_bufs[si].data_ptr()
            else:
                P.mode = 2               # CPU: one pass, reverse or dual per node (next[5] = 1)
        st = (ctypes.c_longlong * n)(*[s.data_ptr() for s in states])
        it = (ctypes.c_int * n)(*iters)
        P.states = ctypes.cast(st, ctypes.c_void_p)
        P.iters = ctypes.cast(it, ctypes.c_void_p)
        P.abuf[0], P.abuf[1] = self._abuf[0].data_ptr(), self._abuf[1].data_ptr()
        for par in (0, 1):
            P.ctx[par] = ctxs[par] if gpu else ctypes.cast(ctypes.pointer(ctxs[par]), ctypes.c_void_p).value
        P.abytes = self._abuf[0].numel() * self._abuf[0].element_size()
        run = ctypes.cast(self.lib._adj, ctypes.c_void_p)
        if gpu:
            from .parallel.native import _dev_lib
            r = _dev_lib().tclb_ad_segment(ctypes.byref(L), ctypes.byref(P), run)
        else:
            from .parallel.native import _host_lib
            r = _host_lib().tclb_ad_segment_cpu(ctypes.byref(L), ctypes.byref(P), run)
        if r != 0:
            raise AdjointError(f"native adjoint segment failed ({r})")
        self.native_steps += n
        if gpu:
            o = abi.ADCTX_OVERFLOW_OFFSET
            for par in (0, 1):
                flag = self._ctx_devs[par][o:o + 4].view(torch.int32)
                torch.maximum(self._ovf, flag, out=self._ovf)
        elif any(c.overflow for c in ctxs):
            raise AdjointError(f"model {lat.model.name}: a node needed more than {self.lib.tangents} AD tangents")
        return self._abuf[1 - (par0 ^ ((n - 1) & 1))]

    def _free_bytes(self) -> float:
        if self.lat.is_gpu:
            return float(torch.cuda.mem_get_info(self.lat.device)[0])
        try:
            import psutil
            return float(psutil.virtual_memory().available)
        except ImportError:      # pragma: no cover
            return 8e9

    def check_overflow(self):
        """raise if any dual-number node of the sweeps since the last check needed more
        tangents than the executor has (one host synchronisation)"""
        if self._ovf is not None and int(self._ovf.item()):
            self._ovf.zero_()
            raise AdjointError(f"model {self.lat.model.name}: a node needed more than {self.lib.tangents} AD tangents")

    def step_back(self, a_next: torch.Tensor, action: str = "Iteration", obj_weight: float = 1.0,
                  state: Optional[torch.Tensor] = None, _buffer: bool = False,
                  other: Optional[torch.Tensor] = None) -> torch.Tensor:
        """adjoint of one `action` applied to the primal state `state` (default: the
        current snapshot): given a_next = dJ/d(state after the action) return
        dJ/d(state before), adding this step's Objective derivative (weight obj_weight)
        and setting gradients.  `other`: what the step's output snapshot held before the
        step (default: the other snapshot of the lattice) — read by a multi-stage action
        only for the fields of Model.late_reads.  (_buffer: the result may be one of the
        adjoint's internal ping-pong buffers, valid until the next call — the unsteady
        sweep's own loop.)"""
        a = self._step_back(a_next, action, obj_weight, state, other)
        if not _buffer and self._abuf is not None and any(a is b for b in self._abuf):
            a = a.clone()
        return a

    def _step_back(self, a_next, action, obj_weight, state, other=None):
        if (len(self.lat.model.action(action).stages) > 1 and self._abuf is not None
                and any(a_next is b for b in self._abuf)):
            # a_next is read again after the first stage's adjoint reuses the buffers
            a_next = a_next.clone()
        lat = self.lat
        m = lat.model
        act = m.action(action)
        src = lat.snaps[lat.cur] if state is None else state
        # forward recompute of the intermediate in-place states of multi-stage actions,
        # in a work copy of the snapshot the primal step wrote into (fields no stage has
        # written yet keep what it held: Model.late_reads are read from it, as in the
        # primal step; for every other field its contents do not matter)
        inputs: List[torch.Tensor] = [src]
        if len(act.stages) > 1:
            glob = lat.globals_t.clone()
            if other is None:
                if state is not None and m.late_reads(action):
                    raise AdjointError(f"model {m.name}: action {action} reads {m.late_reads(action)} from the "
                                       "output snapshot's previous contents; step_back(state=...) needs other=")
                other = lat.snaps[1 - lat.cur] if state is None else lat.snaps[lat.cur]
            dst = other.clone()
            for k, sname in enumerate(act.stages[:-1]):
                si = m.stage_index(sname)
                lat._launch_stage(si, src if k == 0 else dst, dst, False)
                lat._halo_finish(lat._halo_start(dst, lat._saved_fields(m.stage(sname))))
                inputs.append(dst.clone())
            lat.globals_t.copy_(glob)
        a = a_next
        for k in range(len(act.stages) - 1, -1, -1):
            st = m.stage(act.stages[k])
            si = m.stage_index(act.stages[k])
            saved = lat._saved_fields(st)
            if len(saved) == a.shape[0]:
                aout = a                 # every field is an output of the stage
            else:
                aout = torch.zeros_like(a)
                for r0, r1 in runs(saved):
                    aout[r0:r1] = a[r0:r1]
            ain = self._ad_stage(si, inputs[k], aout, obj_weight)
            if k > 0:
                keep = a.clone()
                for r0, r1 in runs(saved):
                    keep[r0:r1] = 0      # written in place: the old values are overwritten
                a = ain + keep
            else:
                a = ain                  # B's unwritten fields do not depend on A
        return a

    # ------------------------------------------------------------------ unsteady
    def unsteady(self, steps: int, action: str = "Iteration", checkpoint: int = 0,
                 a_final: Optional[torch.Tensor] = None, keep_segment: Optional[bool] = None) -> torch.Tensor:
        """run `steps` primal iterations from the current state recording checkpoints,
        then sweep backwards; returns dJ/d(initial state).  The primal ends at its final
        state (as the reference's record/rewind leaves it).

        Two-level checkpointing: a snapshot every `checkpoint` (default sqrt(steps))
        iterations; the reverse sweep re-runs each segment once, keeping its states (the
        288 GB of HBM hold sqrt(steps) snapshots easily), so every primal step is
        recomputed once instead of once per later step of its segment.  The Objective is
        summed on the device (no host round trip per recorded step)."""
        lat = self.lat
        checkpoint = checkpoint or max(1, int(math.sqrt(steps)))
        # memory: (steps / checkpoint) checkpoints + one segment of states; when that does
        # not fit in half the free memory, keep only checkpoints and re-run each reverse
        # step from its checkpoint instead (no segment states)
        snap_bytes = lat.snaps[0].numel() * lat.snaps[0].element_size()
        if keep_segment is None:
            keep_segment = (steps // checkpoint + checkpoint + 2) * snap_bytes <= 0.5 * self._free_bytes()
        it0 = lat.iter
        snaps: Dict[int, torch.Tensor] = {0: lat.snaps[lat.cur].clone()}
        # with late reads (Model.late_reads) a step also depends on what its output
        # snapshot held: keep that next to every checkpoint
        late = bool(lat.model.late_reads(action))
        prev: Dict[int, torch.Tensor] = {0: lat.snaps[1 - lat.cur].clone()} if late else {}
        obj = next((i for i, g in enumerate(lat.model.globals_) if g.name == "Objective"), None)
        J = torch.zeros((), dtype=torch.float64, device=lat.device)
        for t in range(steps):
            lat.iterate(1, glob_last=True, action=action, reduce=False)
            if obj is not None:
                J += lat.globals_vector()[obj]
            if (t + 1) % checkpoint == 0 and t + 1 < steps:
                snaps[t + 1] = lat.snaps[lat.cur].clone()
                if late:
                    prev[t + 1] = lat.snaps[1 - lat.cur].clone()
        lat._reduce_globals()
        self.J = lat.comm.allreduce_scalar(float(J.item()), "sum") if obj is not None else 0.0
        final = lat.snaps[lat.cur].clone()
        cur_final = lat.cur
        a = torch.zeros_like(final) if a_final is None else a_final
        bases = sorted(snaps)
        for si, base in reversed(list(enumerate(bases))):
            end = bases[si + 1] if si + 1 < len(bases) else steps
            # re-run the segment once, keeping the state before every step: each step
            # writes a fresh snapshot buffer, which is kept (no copies)
            lat.snaps[lat.cur].copy_(snaps[base])
            if late:
                lat.snaps[1 - lat.cur].copy_(prev[base])
            lat.iter = it0 + base
            states = [snaps[base]]
            # a single rank reads no ghost plane, and a step that writes every field
            # overwrites the whole interior: the recompute buffers need no zero fill
            uninit = not lat.ghosts and lat.writes_all_fields(action)
            for t in range(base + 1, end if keep_segment else base + 1):
                if late:
                    # the step reads what its output snapshot held in the primal run: the
                    # state two steps back (prev[base] before the segment's first step)
                    lat.snaps[1 - lat.cur] = (states[-2] if len(states) > 1 else prev[base]).clone()
                else:
                    lat.snaps[1 - lat.cur] = lat.new_snapshot(uninit)
                lat.iterate(1, glob_last=False, action=action)
                states.append(lat.snaps[lat.cur])
            t_lo = end - 1
            if keep_segment and not lat.zseries and len(lat.model.action(action).stages) == 1:
                # the reverse steps of the segment in one native call; a stage the executor
                # has not run yet goes through _ad_stage once first (it sizes the windows)
                seg = list(range(end - 1, base - 1, -1))
                if not self._native_ready(action):
                    t = seg.pop(0)
                    lat.iter = it0 + t
                    a = self.step_back(a, action, state=states[t - base], _buffer=True)
                r = self._segment_native(a, [states[t - base] for t in seg], [it0 + t for t in seg], action) \
                    if seg else None
                if r is not None or not seg:
                    a = r if r is not None else a
                    t_lo = base - 1
                else:
                    t_lo = seg[0]
            for t in range(t_lo, base - 1, -1):
                other = None
                if keep_segment:
                    state = states[t - base]
                    if late:
                        other = states[t - base - 1] if t > base else prev[base]
                else:
                    lat.snaps[lat.cur].copy_(snaps[base])
                    if late:
                        lat.snaps[1 - lat.cur].copy_(prev[base])
                    lat.iter = it0 + base
                    for _ in range(t - base):
                        lat.iterate(1, glob_last=False, action=action)
                    state = None
                lat.iter = it0 + t
                if lat.zseries:
                    lat.apply_series()
                    before = self.gzon.cpu().numpy().copy()
                a = self.step_back(a, action, state=state, _buffer=True, other=other)
                if lat.zseries:
                    self._series_grad(before, lat)
            del states
        self.check_overflow()
        a = a.clone()
        lat.snaps = [lat.new_snapshot(), lat.new_snapshot()]
        lat.snaps[cur_final].copy_(final)
        lat.cur = cur_final
        lat.iter = it0 + steps
        self.a0 = a
        lat.adjoint_state = a
        return a

    def _series_grad(self, before: np.ndarray, lat):
        """attribute this reverse step's zonal-setting gradient to the active entry of
        each zonal time series (reference zSet gradient tables per time index)"""
        nz = lat.zvals.shape[1]
        d = self.gzon.cpu().numpy() - before
        for key, v in lat.zseries.items():
            g = self.series_grads.setdefault(key, np.zeros(len(v)))
            g[lat.series_index(key)] += d[key[0] * nz + key[1]]

    def series_gradient(self, name: str, zone: Optional[str] = None) -> np.ndarray:
        lat = self.lat
        key = (lat.zsettings.index(name), lat.zone_index(zone or "DefaultZone"))
        g = self.series_grads.get(key, np.zeros(len(lat.zseries.get(key, [0.0])))).copy()
        if lat.comm.size > 1:
            g = np.array([lat.comm.allreduce_scalar(float(v), "sum") for v in g])
        return g

    def param_fields(self) -> List[int]:
        return [i for i, f in enumerate(self.lat.model.fields) if f.parameter]

    def steady_step(self, a: torch.Tensor, action: str = "Iteration",
                    state: Optional[torch.Tensor] = None) -> torch.Tensor:
        """one steady-adjoint iteration (reference SteadyAdjoint kernels, "SAdj" dispatch
        with zeropar, src/conf.R:831-839): the adjoint of the parameter densities is
        zeroed on entry, so on exit it holds this iteration's gradient contribution
        lambda^T dF/dp + dJ/dp — the steady design gradient once lambda has converged"""
        a = a.clone()
        pf = self.param_fields()
        if pf:
            a[pf] = 0
        self.gset.zero_()
        self.gzon.zero_()
        return self.step_back(a, action, state=state)

    def steady(self, iterations: int, action: str = "Iteration", tol: float = 0.0) -> torch.Tensor:
        """fixed-point adjoint at the current (converged) primal state: a <- A^T a + dJ/df"""
        a = torch.zeros_like(self.lat.snaps[self.lat.cur])
        for _ in range(iterations):
            b = self.steady_step(a, action)
            d = self.lat.comm.allreduce_scalar(float((b - a).abs().max()), "max") if tol else 0.0
            a = b
            if tol and d < tol:
                break
        self.check_overflow()
        self.a0 = a
        self.lat.adjoint_state = a
        return a

    # ------------------------------------------------------------------ results
    def field_gradient(self, name: str) -> np.ndarray:
        """dJ/d(field) on the interior (nz, ny, nx) — e.g. a design parameter density"""
        lat = self.lat
        i = lat.model.field_index(name)
        nx, ny, nz = lat.shape
        return self.a0[i, lat.gz:lat.gz + nz, lat.gy:lat.gy + ny, :nx].cpu().numpy().copy()

    def setting_gradient(self, name: str, zone: Optional[str] = None) -> float:
        """d J / d setting, summed over the ranks (each accumulates its own nodes)"""
        lat = self.lat
        if name in lat.gsettings:
            v = float(self.gset[lat.gsettings.index(name)])
        else:
            zi = lat.zone_index(zone or "DefaultZone")
            v = float(self.gzon[lat.zsettings.index(name) * lat.zvals.shape[1] + zi])
        return lat.comm.allreduce_scalar(v, "sum")
