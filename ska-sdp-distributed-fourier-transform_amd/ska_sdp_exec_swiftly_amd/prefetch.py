"""
Planned-wave prefetch of the contiguous-axis-first forward pipeline (r4 / r5): K2 of the waves a caller that walks its
plan will ask for next, enqueued on the core's side stream while the subgrid side of the wave being served runs.  A
mix-in of :class:`SwiftlyForward`; the multi-GPU classes drive the same object through ``wave_blocks_into``
(distributed.DistributedForward), so they get the same free-running K2 chain.

Where the state lives: the walk of the caller over its plan in a :class:`WavePredictor` (pure Python), the K2s in flight
in the attributes :class:`WavePrefetch` declares, and what holds for one set of band buffers (the bands-ready event, the
chain flag) with the band buffers, in :class:`SwiftlyForward`.

The knobs live in the ``api`` module namespace (``api._PREFETCH`` ...; the tests switch them at run time).
"""
import logging
import os
import sys
from functools import cached_property

from .tasks import _torch

log = logging.getLogger("fourier-logger")

# tuning knob: SWIFTLY_PREFETCH=0 turns the planned-wave prefetch of SwiftlyForward off (A/B runs)
PREFETCH_DEFAULT = os.environ.get("SWIFTLY_PREFETCH", "1") != "0"


def _env_int(name, default, lowest):
    """integer knob from the environment; anything unparsable falls back to the default (r5 advisor)"""
    try:
        return max(lowest, int(os.environ.get(name, default)))
    except (TypeError, ValueError):
        return default


# how many planned waves K2 may run ahead of the wave being served (_prefetch_wave): 1 = the r4 schedule
PREFETCH_DEPTH_DEFAULT = _env_int("SWIFTLY_PREFETCH_DEPTH", 2, 1)
# SWIFTLY_CHAIN_K2=0: every prefetched K2 forks its chunk streams behind the side stream again (A/B runs)
CHAIN_K2_DEFAULT = os.environ.get("SWIFTLY_CHAIN_K2", "1") != "0"
# SWIFTLY_K2_SLABS=0: K2 on every wave's whole window, not once per column slab of the padded axis (slabs.py; A/B runs)
K2_SLABS_DEFAULT = os.environ.get("SWIFTLY_K2_SLABS", "1") != "0"


_REARM_AFTER = 4  # requests in plan order after which a switched-off prefetch is switched on again


def _knobs():
    """the module whose ``_PREFETCH`` / ``_knobs()._PREFETCH_DEPTH`` / ``_knobs()._CHAIN_K2`` are the live values"""
    return sys.modules[__package__ + ".api"]


class WavePredictor:
    """The walk of a caller over its planned waves: positions are those of ``keys`` (the wave keys in order of first
    appearance in the plan, or the order announced with :py:meth:`set_order`): a caller that walks its own plan forwards
    or backwards is predicted whatever the numeric order of the keys; a repeated key keeps the direction of the walk."""

    def __init__(self, keys):
        self.order = list(dict.fromkeys(int(k) for k in keys))
        self.pos = {k: i for i, k in enumerate(self.order)}
        self.last, self.step = None, 1  # position of the last request, direction of the walk
        self.off, self.missed, self.streak = False, 0, 0

    def set_order(self, keys, planned):
        """the order the caller announces; keys outside ``planned`` and repeats are dropped, the walk restarts"""
        self.order = [k for k in dict.fromkeys(int(k) for k in keys) if k in planned]
        self.pos = {k: i for i, k in enumerate(self.order)}
        self.last, self.step = None, 1

    def next(self, key, depth):
        """the waves asked for after ``key``, nearest first, at most ``depth`` of them ([]: end / unknown key / off)"""
        pos, last, order = self.pos.get(int(key)), self.last, self.order
        if self.off:
            # switched off after two mispredictions (miss): a caller that follows the order again for _REARM_AFTER
            # requests gets the prefetch back (r5 advisor: the switch used to be for the life of the object)
            follows = pos is not None and last is not None and pos - last == self.step
            self.streak = self.streak + 1 if follows else 0
            if pos is not None:
                self.last = last = pos
            if self.streak < _REARM_AFTER:
                return []
            self.off, self.missed, self.streak = False, 0, 0
        if pos is None:
            return []
        if last is not None and pos != last:
            # a jump from one end of the order to the other is the next PASS of the same walk (an object that is reused
            # for several passes), not a turn: the direction is kept (r5 advisor)
            wrapped = len(order) > 2 and {pos, last} == {0, len(order) - 1} and (pos == 0) == (self.step > 0)
            if not wrapped:
                self.step = 1 if pos > last else -1
        self.last = pos
        ahead = range(pos + self.step, pos + (int(depth) + 1) * self.step, self.step)
        return [order[i] for i in ahead if 0 <= i < len(order)]

    def hit(self):
        """a prefetched wave was asked for: the walk follows the order"""
        self.missed = 0

    def miss(self):
        """a wave other than the prefetched ones had to be computed; True when this miss (the second in a row) switched
        the predictor off"""
        self.missed += 1
        if self.missed < 2 or self.off:
            return False
        self.off = True
        return True


class WavePrefetch:
    """Side-stream K2 of the next planned waves: the in-flight side.  The host class provides ``_plan`` /
    ``_planned_keys``, ``lru``, ``core``, ``_wave_rows`` / ``_k2_wave`` / ``_axis1`` and the band-lifetime fields
    ``_bands_ready`` / ``_side_waited`` / ``_k2_chain_forked``, which it resets when band buffers are installed; for the
    slab form of K2 also ``_slab_plan`` / ``_slab_rows`` / ``_compute_slab`` and the slab cache ``_slab_has`` / ``_slab_cached``
    / ``_slab_store``."""

    def __init__(self):
        self._prefetched = {}  # K2s in flight: {off1: (Q, rowmap, done event)}
        self._prefetched_slabs = {}  # the same for column slabs: {slab: (Q, rowmap, done event, n_rows)}
        self._prefetch_parked = []  # mispredicted ones, kept referenced until their done events have fired
        self.prefetch_issued = 0  # K2s enqueued on the side stream so far

    @cached_property
    def _predictor(self):
        """the walk over the plan's waves (built on first use: one walk over the plan, none for objects that never predict)"""
        return WavePredictor(sg.off1 for sg in self._plan)

    # -- planned-wave prefetch (r4): K2 of the NEXT planned wave(s) on the core's side stream ------------------------
    def _predict_next_waves(self, off1, depth):
        """the planned waves a caller that walks the plan asks for after ``off1``, nearest first, at most ``depth`` of
        them ([]: no plan / end / prefetch off; :py:meth:`WavePredictor.next`)"""
        if self._plan is None or not _knobs()._PREFETCH:
            return []
        return self._predictor.next(off1, depth)

    def set_wave_order(self, keys):
        """Tell the predictor the order in which the caller will ask for the planned waves (wave keys = ``off1``), when
        it is not the order of first appearance in ``subgrid_configs`` -- e.g. the group order of the multi-GPU pass
        (distributed.DistributedForward).  Keys outside the plan are ignored; the walk restarts."""
        if self._plan is not None:
            self._predictor.set_order(keys, self._planned_keys)

    def _predict_next_wave(self, off1):
        """the nearest of :py:meth:`_predict_next_waves` (None: nothing to predict)"""
        nxt = self._predict_next_waves(off1, 1)
        return nxt[0] if nxt else None

    def _take_prefetched(self, off1):
        """hand a prefetched ``Q`` of wave ``off1`` over to the LRU cache (the current stream waits for its K2).  When a
        wave that is neither prefetched nor cached has to be computed, the prefetched ones were mispredictions: their
        buffers are dropped, and after two such misses the prefetch is switched off for this object (a wasted K2 per
        wave costs more than the overlap gains)."""
        pending = self._prefetched
        if not pending:
            return
        pf = pending.pop(int(off1), None)
        if pf is None:
            if self.lru.get(("b", off1)) is None:  # a different wave has to be computed: the guess was wrong
                # the K2 kernels of the dropped waves may still be running (they read the band buffers and write these Q
                # blocks): keep the blocks referenced until their `done` events have fired
                parked = self._prefetch_parked
                parked[:] = [p for p in parked if p[2] is not None and not p[2].query()]
                parked.extend(pending.values())
                pending.clear()
                if self._predictor.miss():
                    log.info("SwiftlyForward: two mispredicted waves in a row -- planned-wave prefetch switched off "
                             "until %d requests have followed the plan again", _REARM_AFTER)
            return
        self._predictor.hit()  # the walk follows the plan
        if self.lru.get(("b", off1)) is None:
            cur = _torch().cuda.current_stream(self.core.device)
            cur.wait_event(pf[2])
            # Q was allocated under the side stream and is read by kernels of the caller's stream from now on: tell the
            # caching allocator, so that a freed Q is not handed to the next side-stream allocation while `cur` reads it
            pf[0].record_stream(cur)
            self.lru.set(("b", off1), (pf[0], pf[1]))

    def _prefetch_wave(self, off1):
        """Enqueue K2 of planned wave ``off1`` on the side stream: it runs next to the subgrid side (K3-K5) of the wave
        the caller is being served now.  The bandwidth-bound column passes and the issue-bound ``sum_finish`` share
        the chip better than they follow each other (measured r4, 64k workload: 25.5 -> 24.2 ms for the 25 waves).

        Depth 1 (r4): the side stream starts behind everything queued on the caller's stream so far, i.e. K2 of wave
        w + 1 begins when K2 of wave w AND the subgrid side of wave w - 1 have finished -- one cross-stream hand-over
        (a 20-50 us idle gap, tools/trace_timeline.py) per wave.  Depth >= 2 (r5, SWIFTLY_PREFETCH_DEPTH): the side
        stream waits for the band buffers only (an event recorded behind K1), so the K2s of consecutive waves follow
        each other without a hand-over, up to ``depth`` waves ahead of the wave being served; ``Q`` is allocated under
        the side stream and handed over with ``record_stream``, which is what keeps a recycled block from being
        written while the caller's stream still reads it."""
        torch = _torch()
        core = self.core
        pending = self._prefetched
        if off1 is None or int(off1) in pending or self.lru.get(("b", off1)) is not None:
            return
        rowmap, n_rows = self._wave_rows(off1)
        side, chain = self._side_behind_bands()
        with torch.cuda.stream(side):
            Q = torch.empty((len(self.facet_configs), n_rows, core.xM_yN_size), dtype=self.dtype, device=core.device)
            core.chain_chunk_streams(chain)
            try:
                self._k2_wave(off1, rowmap, n_rows, out=Q)
            finally:
                core.chain_chunk_streams(False)
            done = torch.cuda.Event()
            done.record(side)
        self._k2_chain_forked = True
        pending[int(off1)] = (Q, rowmap, done)
        self.prefetch_issued += 1

    def _side_behind_bands(self):
        """``(side stream, chain)``: the core's side stream put in order behind the band buffers, and whether the next K2
        on it may run its chunk streams on from the previous one (see :py:meth:`_prefetch_wave`)"""
        torch = _torch()
        core = self.core
        side = core.side_stream()
        ready = self._bands_ready
        if _knobs()._PREFETCH_DEPTH >= 2 and ready is not None:
            if self._side_waited is not ready:  # once per pass: the side stream is in order behind it
                side.wait_event(ready)  # K1 of every facet (recorded by _prepare_all_bands)
                self._side_waited = ready
        else:
            ev = torch.cuda.Event()
            # bands ready; every reader of a Q buffer that the allocator may hand out again has been enqueued
            ev.record(torch.cuda.current_stream(core.device))
            side.wait_event(ev)
        # (r5) second and later K2 of the free-running chain: the chunk streams of the four-step run on from the previous
        # wave's chunks instead of being forked behind its join -- the band buffers were complete before the first (forking)
        # call of this object, Q is a fresh block (swiftly_hip_chain_chunk_streams; 40 us of idle GPU per wave otherwise)
        # (axis-1-first pipeline with a row pass per wave: K2 reads rows that finish_axis1_rows has just written on the side
        # stream -- its chunk streams must fork behind them every time)
        chain = (_knobs()._PREFETCH_DEPTH >= 2 and ready is not None and _knobs()._CHAIN_K2
                 and self._k2_chain_forked and self._axis1() != 1)
        return side, chain

    # -- the slab form (slabs.py): the same side-stream chain, issued per column slab instead of per wave ---------------
    def _slab_hit(self, j):
        """cached slab ``j`` as ``(Q, rowmap, n_rows)``, a prefetched one taken over first (the current stream waits for
        its K2; hand-over as in :py:meth:`_take_prefetched`); None when it has to be computed"""
        pf = self._prefetched_slabs.pop(j, None)
        if pf is not None and not self._slab_has(j):
            cur = _torch().cuda.current_stream(self.core.device)
            cur.wait_event(pf[2])
            pf[0].record_stream(cur)
            self._slab_store(j, (pf[0], pf[1], pf[3]))
        return self._slab_cached(j)

    def _check_slab_prediction(self, needed):
        """the misprediction rule of :py:meth:`_take_prefetched` for a wave that needs the slabs ``needed``: when one of
        them is neither cached nor in flight although slabs are in flight, the guess was wrong -- the slabs in flight that
        this wave does not use are dropped, and two such misses in a row switch the prefetch off"""
        pending = self._prefetched_slabs
        if not pending:
            return
        if all(j in pending or self._slab_has(j) for j in needed):
            self._predictor.hit()
            return
        parked = self._prefetch_parked  # (kept referenced until their K2 has run, as the waves' blocks are)
        parked[:] = [p for p in parked if p[2] is not None and not p[2].query()]
        for j in [j for j in pending if j not in needed]:
            parked.append(pending.pop(j))
        if self._predictor.miss():
            log.info("SwiftlyForward: two mispredicted waves in a row -- planned-wave prefetch switched off "
                     "until %d requests have followed the plan again", _REARM_AFTER)

    def _prefetch_slab(self, j):
        """K2 of slab ``j`` on the side stream (:py:meth:`_prefetch_wave` for a slab), unless cached or in flight"""
        torch = _torch()
        core = self.core
        pending = self._prefetched_slabs
        if j in pending or self._slab_has(j):
            return
        rowmap, n_rows = self._slab_rows(j)
        side, chain = self._side_behind_bands()
        with torch.cuda.stream(side):
            Q = torch.empty((len(self.facet_configs), n_rows, core.xM_yN_size), dtype=self.dtype, device=core.device)
            core.chain_chunk_streams(chain)
            try:
                calls = self._compute_slab(j, Q, rowmap)
            finally:
                core.chain_chunk_streams(False)
            done = torch.cuda.Event()
            done.record(side)
        self._k2_chain_forked = True
        pending[j] = (Q, rowmap, done, n_rows)
        self.prefetch_issued += calls

    def _prefetch_slabs_of(self, waves):
        """the slabs the predicted ``waves`` need, in the order the walk meets them"""
        for off1 in waves:
            for j, _, _ in self._slab_plan.pieces(off1):
                self._prefetch_slab(j)

    def _prefetch_waves(self, waves):
        """:py:meth:`_prefetch_wave` for the predicted waves, nearest first, at most SWIFTLY_PREFETCH_DEPTH in flight"""
        for off1 in waves:
            if len(self._prefetched) >= _knobs()._PREFETCH_DEPTH:
                break
            self._prefetch_wave(off1)
