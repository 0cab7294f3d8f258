"""
``SwiftlyBackward``: the subgrid -> facet direction of the streaming API (reference src/ska_sdp_exec_swiftly/api.py:327-463,
task bodies api_helper.py:115-197) on one MI355X, with the reference's schedule (``wave_axis=0``) and the band schedule
(``wave_axis=1``).  The class is the front -- keywords, schedule and dtype rules, staging of partial
waves, ``finish()`` -- of three roles: ``splitter.SubgridSplitter`` (a wave's contributions to every facet) and the facet
owner's accumulators of either schedule, ``ColumnAccumulators`` and ``BandAccumulators``.
"""
import logging

import numpy

from . import _lib, facet_dtype as fdt
from .b8_form import B8Facts, choose_b8
from .core_hip import band_range
from .ingest import _mask_table
from .splitter import SubgridSplitter
from .tasks import DeviceTask, LRUCache, TaskQueue, _torch, _unwrap

log = logging.getLogger("fourier-logger")


class ColumnAccumulators:
    """The reference's schedule (``wave_axis=0``) for the facets ``facet_configs``: partial sums ``NAF_MNAF [F, m, yN]`` per
    subgrid ``off0`` column in an LRU of ``lru_backward`` columns (reference api.py:402-438), evicted columns folded into the
    facet accumulators ``MNAF_BMNAFs_persist [yN, yB]``, strided-axis transform at the end."""

    def __init__(self, core, facet_configs, lru_backward=1):
        self.core, self.facet_configs = core, facet_configs
        self.lru = LRUCache(lru_backward)
        self.MNAF_BMNAFs_persist = [None for _ in facet_configs]

    def accumulate_wave(self, sgs, parts):
        """:py:meth:`accumulate` of the one chunk ``parts[F, S, m, m]`` of subgrids ``sgs`` that share ``off0``"""
        off0 = sgs[0].off0
        if any(int(sg.off0) != int(off0) for sg in sgs):
            raise ValueError(f"reference schedule (wave_axis=0): all subgrids of a wave must share off0={off0}")
        return self.accumulate(off0, [(sgs, parts)])

    def accumulate(self, off0, chunks):
        """``accumulate_column`` (reference api_helper.py:142-152): add ``chunks = [(subgrid configs, parts[F, S_c, m, m]),
        ...]`` into the partial sums of column ``off0``; the column this evicts goes to the facet accumulators"""
        core = self.core
        m, yN = core.xM_yN_size, core.yN_size
        F = len(self.facet_configs)
        col = self.lru.get(off0)
        for sgs, parts in chunks:
            if col is None:
                col = _torch().zeros((F, m, yN), dtype=parts.dtype, device=core.device)
            # one launch per subgrid (batched over facets): launches are ordered on the stream, so subgrids whose
            # windows overlap never update the same element concurrently
            for b, sg in enumerate(sgs):
                core.launch("add_to_facet", parts[:, b], m, m, 1, col, yN, 1, sg.off1,
                            nbatch=F, in_bs=parts.stride(0), out_bs=m * yN)
        if col is None:
            return None
        old_off0, old_col = self.lru.set(off0, col)
        if old_off0 is not None and old_col is not None:
            self.update_MNAF_BMNAFs(old_off0, old_col)
        return col

    def update_MNAF_BMNAFs(self, off0, NAF_MNAFs):
        """accumulate_facet for every facet (reference api.py:440-463,
        api_helper.py:155-179): finish axis 1 (+mask1), add along axis 0."""
        torch = _torch()
        core = self.core
        yN = core.yN_size
        dev, dt = core.device, NAF_MNAFs.dtype
        for j, cfg in enumerate(self.facet_configs):
            yB = cfg.size
            t = core.finish_facet(NAF_MNAFs[j], cfg.off1, yB, axis=1, mask=cfg.mask1)
            if self.MNAF_BMNAFs_persist[j] is None:
                self.MNAF_BMNAFs_persist[j] = torch.zeros((yN, yB), dtype=dt, device=dev)
            core.launch("add_to_facet", t, yB, 1, yB, self.MNAF_BMNAFs_persist[j], 1, yB, off0)
        return self.MNAF_BMNAFs_persist

    def finish(self, empty_dtype, handed_out):
        """flush the column cache and finish every facet along axis 0 (reference api_helper.py:182-197): ``handed_out(facet)``
        per facet as it is finished, zeros of ``empty_dtype`` for a facet without contributions"""
        core = self.core
        for old_off0, old_col in self.lru.pop_all():
            self.update_MNAF_BMNAFs(old_off0, old_col)
        out = []
        for cfg, acc in zip(self.facet_configs, self.MNAF_BMNAFs_persist):
            if acc is None:
                out.append(_torch().zeros((cfg.size, cfg.size), dtype=empty_dtype, device=core.device))
            else:
                out.append(handed_out(core.finish_facet(acc, cfg.off0, cfg.size, axis=0, mask=cfg.mask0)))
        return out


class BandAccumulators:
    """The band schedule (``wave_axis=1``) for the facets ``facet_configs``: accumulators
    ``bands [F, yB, band length]`` over the columns ``band`` that the waves of ``plan`` touch (no plan: the whole padded axis),
    first-write flags ``touched`` per column, the facet mask table and the scratch of ``accumulate_facet_columns`` -- all
    created by the first wave.  ``fixed_dtype``: the dtype a ``SwiftlyBackward`` was constructed with (the explicit gate)."""

    def __init__(self, core, facet_configs, plan=None, fixed_dtype=None):
        self.core, self.facet_configs, self._plan, self._fixed_dtype = core, facet_configs, plan, fixed_dtype
        self.band = self.bands = self.touched = self.masks0 = self.work = None
        self._planned = {sg.off1 for sg in plan} if plan else None
        self._facet_off0s = [cfg.off0 for cfg in facet_configs]

    def _create(self, dtype):
        torch = _torch()
        core = self.core
        if self._fixed_dtype is not None:
            # explicit dtype: complex128 runs through the explicit gate (complex64: the same answer as without)
            if dtype != self._fixed_dtype:
                raise ValueError(f"SwiftlyBackward(wave_axis=1, dtype={self._fixed_dtype}) got {dtype} contributions")
            if not core.supports_backward_band(dtype, explicit=True):
                raise ValueError(f"SwiftlyBackward(wave_axis=1, dtype={dtype}): {_lib.last_error()}")
        elif dtype != torch.complex64 or not core.supports_backward_band(dtype):
            raise ValueError("SwiftlyBackward(wave_axis=1) needs complex64 data and power-of-two yN_size / xM_yN_size")
        sizes = {cfg.size for cfg in self.facet_configs}
        if len(sizes) != 1:
            raise ValueError("SwiftlyBackward(wave_axis=1) needs facets of one size")
        yB = sizes.pop()
        # (the backward accumulators are plain-order bands for every yN: band_range, not the forward layout rule)
        self.band = (
            band_range(core.N, core.yN_size, core.xM_yN_size, [sg.off1 for sg in self._plan])
            if self._plan else (0, core.yN_size)
        )
        F = len(self.facet_configs)
        # uninitialised: first-write flags per band column replace the zero fill
        self.bands = torch.empty((F, yB, self.band[1]), dtype=dtype, device=core.device)
        self.touched = torch.zeros((self.band[1],), dtype=torch.uint8, device=core.device)
        self.masks0 = _mask_table(core, self.facet_configs, "mask0", yB, dtype)
        # four-step scratch of accumulate_facet_columns (+ the radix-Q pass's output when yN = Q * 2^k)
        esz = 16 if dtype == torch.complex128 else 8
        self.work = torch.empty((core._k2_scratch_bytes(F, element_size=esz) // esz,), dtype=dtype, device=core.device)

    def accumulate(self, off1, chunks, first=None):
        """accumulate_column + accumulate_facet (reference api_helper.py:142-179) with the axes swapped, for the
        contributions ``chunks = [(subgrid configs, parts[F, S_c, m, m]), ...]`` of subgrids sharing ``off1``.
        ``first(dtype)``: called with the contributions' dtype once the wave has passed its key check, before anything is
        created (the owner's first-data rules)."""
        core = self.core
        m = core.xM_yN_size
        chunks = [(sgs, parts) for sgs, parts in chunks if len(sgs)]
        if not chunks:
            return None
        for sgs, _parts in chunks:
            # (r4 advice) the band schedule folds a wave under ONE off1: a caller that follows the reference's per-off0
            # flow (accumulate_column, api_helper.py:142-152) on an object whose schedule resolved to wave_axis=1 must
            # hear about it instead of getting every subgrid placed at the first one's off1
            bad = [sg for sg in sgs if int(sg.off1) != int(off1)]
            if bad:
                raise ValueError(
                    f"band schedule (wave_axis=1): all subgrids of a wave must share off1={off1}, got off1={bad[0].off1}; "
                    "group the subgrids by off1, or construct SwiftlyBackward(wave_axis=0) for the reference's per-off0 flow"
                )
        if first is not None:
            first(chunks[0][1].dtype)
        if self.bands is None:
            self._create(chunks[0][1].dtype)
        bands = self.bands
        for _sgs, parts in chunks:
            # on EVERY call, not only the one that creates the accumulators: the native side reads `parts` with the
            # accumulators' element size
            if parts.dtype != bands.dtype:
                raise ValueError(f"band accumulators are {bands.dtype}, got {parts.dtype} contributions")
        if self._planned is not None and off1 not in self._planned:
            raise ValueError(f"subgrid off1={off1} is not in the subgrid_configs this SwiftlyBackward was planned for")
        F = len(self.facet_configs)
        dt0 = chunks[0][1].dtype
        fstr, off0s, locs = [], [], []
        fixed = []
        for c, (sgs, parts) in enumerate(chunks):
            if parts.shape[0] != F or parts.dtype != dt0:
                raise ValueError("contribution chunk does not match the facet list / dtype")
            if parts.stride(3) != 1 or parts.stride(2) != m or (parts.shape[1] > 1 and parts.stride(1) != m * m):
                parts = parts.contiguous()
            fixed.append(parts)  # keeps a contiguous copy alive until the launch is queued
            fstr.append(parts.stride(0) if F > 1 else 0)
            for b, sg in enumerate(sgs):
                off0s.append(sg.off0)
                locs.append((c, b))
        # chunk offsets are relative to the LOWEST chunk address: the gather-sum kernel reads a negative 64-bit offset
        # as "no source row", so a chunk allocated below the base (a contiguous copy, a separately allocated chunk
        # handed to accumulate_chunks) would otherwise be dropped silently
        base = min(fixed, key=lambda t: t.data_ptr())
        offs = [(t.data_ptr() - base.data_ptr()) // base.element_size() for t in fixed]
        if len(chunks) > core.GS_MAX_CHUNKS:
            raise ValueError(f"at most {core.GS_MAX_CHUNKS} contribution chunks per wave")
        for _members, table in core.column_row_sources(off0s, locs):
            core.accumulate_facet_columns(base, m, offs, fstr, table, self._facet_off0s, bands.shape[1], self.masks0,
                                          off1, bands, self.band, workspace=self.work, touched=self.touched)
        return bands

    def hand_out(self):
        """the accumulators ``[F, yB, band length]`` with the columns no wave touched zero-filled, ready for the
        contiguous-axis finish; ``None`` when no wave arrived"""
        if self.bands is not None:
            self.core.band_zero_untouched(self.bands, self.touched)
        return self.bands

    def release(self):
        """drop the accumulators and the scratch (the finished facets replace them)"""
        self.bands = self.work = None


class SwiftlyBackward:
    """Subgrid -> facet streaming transform (reference api.py:327-463).

    :param swiftly_config: SwiftlyConfig
    :param facets_config_list: list of FacetConfig
    :param lru_backward: number of subgrid columns (distinct ``off0``) whose
        partial sums ``NAF_MNAF [m, yN]`` per facet stay in HBM before they are
        folded into the facet accumulators
    :param queue_size: bound on unfinished subgrid tasks (reference
        ``TaskQueue``, api.py:466-522)
    :param wave_axis: 0 (default) = the reference's schedule: partial sums per subgrid ``off0`` column, facet
        accumulators ``[yN, yB]``, strided-axis transform at the end.  1 (complex64, power-of-two sizes) = the
        mirror of the forward ``wave_axis=1`` pipeline: subgrids sharing ``off1`` form a wave, the strided-axis
        ``finish_facet`` runs per wave on ``m`` columns with ``add_to_facet`` fused into its load and its store
        (no column accumulator in HBM), the facet accumulators are bands ``[yB, band]`` and the full-facet
        transform at the end runs along the contiguous axis in one kernel.  Any request order is correct.
    :param subgrid_configs: (wave_axis=1) the subgrids that will be added: sizes the band accumulators to the
        columns they touch; without it the band is the whole padded axis
    :param dtype: ``None`` (default): the dtype is the first data's, and the band schedule takes complex64 only.
        A torch or numpy complex dtype fixes the accumulator and staging dtype at construction; data of another
        dtype then raises ``ValueError`` on the band schedule.  ``wave_axis=1, dtype=torch.complex128`` is the
        explicit request that runs the band schedule in complex128 (power-of-two ``yN_size`` 64 .. 32768); nothing
        picks it on its own: with ``wave_axis=None`` complex128 stays on the reference's schedule.
    :param facet_dtype: ``None`` (default) or the complex dtype of the data: :py:meth:`finish` returns complex facets.
        ``torch.float32`` (complex64 data) / ``torch.float64`` (complex128 data): the facets are images and
        :py:meth:`finish` returns their real parts, ``[size, size]`` in that dtype -- bit for bit the ``.real`` of the complex
        result.  On the band schedule in complex64, where ``core.supports_real_facets_out()`` holds, the finishing row
        kernels store float32 themselves and no complex facet is ever allocated (:py:attr:`real_finish_native`); likewise
        float64 from complex128 accumulators where ``core.supports_real_facets_out_f64()`` holds;
        everywhere else each facet is finished complex, its real part copied out and the complex one released before
        the next facet is finished.  A dtype that does not match the data's precision raises ``ValueError`` -- at
        construction when ``dtype`` is given, else at the first data.
    :param half_length_finish: (``facet_dtype=torch.float32`` only, else ``ValueError``) finish the float32 facets through
        the half-length form of the contiguous-axis kernel (``core.finish_facet_band(..., real=True, half_length=True)``):
        one 16384-point transform per 32768-point band row (``_lib.FEATURE_REAL_FACETS_OUT_C2R``), one 32768-point
        transform per 65536-point band row (``_lib.FEATURE_REAL_FACETS_OUT_C2R_64K``).  The same facets within the same error bound, not the same
        bits as without it.  Taken where :py:attr:`half_length_finish` says so; everywhere else the pass runs exactly
        what it runs without the keyword.
    """

    # pylint: disable=too-many-arguments,too-many-instance-attributes
    def __init__(self, swiftly_config, facets_config_list, lru_backward=1, queue_size=20, client=None,
                 subgrid_configs=None, wave_axis=None, delayed=False, dtype=None, facet_dtype=None, half_length_finish=False):
        # (before anything touches the configuration or a device)
        self._want_half_length = bool(half_length_finish)
        self._facet_dtype = fdt.backward_keywords(facet_dtype, self._want_half_length)
        self.delayed = bool(delayed)  # finish() hands out DeviceTask handles instead of bare device tensors
        # wave_axis=None: the reference's schedule, unless the caller hands over the plan of subgrids it will add and
        # the band kernels exist -- decided when the first subgrid shows the dtype (complex64 only)
        self._auto_axis = wave_axis is None
        self.wave_axis = 0 if wave_axis is None else int(wave_axis)
        if self.wave_axis not in (0, 1):
            raise ValueError("wave_axis must be 0 or 1")
        self._plan = list(subgrid_configs) if subgrid_configs is not None else None
        self._plan_counts = None
        self.config = swiftly_config
        self.core = swiftly_config.core
        self.facets_config_list = facets_config_list
        self.queue_size = queue_size
        self.task_queue = TaskQueue(queue_size)
        self._client = client
        self.lru = LRUCache(lru_backward)  # the staged partial waves of the band schedule (wave_axis=0: unused, see columns.lru)
        self.dtype = None
        self._fixed_dtype = None
        if dtype is not None:
            torch = _torch()
            if not isinstance(dtype, torch.dtype):
                dtype = {numpy.dtype(numpy.complex64): torch.complex64, numpy.dtype(numpy.complex128): torch.complex128}.get(
                    numpy.dtype(dtype)
                )
            if dtype not in (torch.complex64, torch.complex128):
                raise ValueError("dtype must be complex64 or complex128")
            self._fixed_dtype = self.dtype = dtype
            # an explicit request for the band schedule is answered at once (complex128: the explicit gate)
            if self.wave_axis == 1 and not self._auto_axis and not self.core.supports_backward_band(dtype, explicit=True):
                raise ValueError(f"SwiftlyBackward(wave_axis=1, dtype={dtype}): {_lib.last_error()}")
            self._check_facet_dtype(dtype)
        # the three roles: the subgrid holder's half, and the facet owner's half in either schedule
        self.splitter = SubgridSplitter(self.core, facets_config_list)  # (the dtype goes with each call)
        self.columns = ColumnAccumulators(self.core, facets_config_list, lru_backward)
        self.bands = BandAccumulators(self.core, facets_config_list, self._plan, self._fixed_dtype)

    def __getattr__(self, name):
        """the band state (``_band``, ``_bands``, ``_work``, ``_masks0``) and the splitter's workspaces (``_wsbuf``) read under
        the names they had on this class"""
        role = {"_band": "bands", "_bands": "bands", "_work": "bands", "_masks0": "bands", "_wsbuf": "splitter"}.get(name)
        if role not in self.__dict__:
            raise AttributeError(f"'{type(self).__name__}' object has no attribute '{name}'")
        return getattr(self.__dict__[role], name if role == "splitter" else name[1:])

    @property
    def MNAF_BMNAFs_persist(self):
        """the reference schedule's facet accumulators (reference api.py:341)"""
        return self.columns.MNAF_BMNAFs_persist

    def update_MNAF_BMNAFs(self, off0, NAF_MNAFs):
        """:py:meth:`ColumnAccumulators.update_MNAF_BMNAFs` (reference api.py:440-463)"""
        return self.columns.update_MNAF_BMNAFs(off0, NAF_MNAFs)

    def _check_facet_dtype(self, data_dtype):
        """``facet_dtype`` has the precision of the data (called wherever the data's dtype becomes known)"""
        fdt.check_precision("SwiftlyBackward", self._facet_dtype, data_dtype)

    @property
    def facet_dtype(self):
        """dtype of the facets :py:meth:`finish` returns: the ``facet_dtype`` asked for, else the data's complex dtype
        (``None`` while no data has shown it)"""
        return self._facet_dtype if self._facet_dtype is not None else self.dtype

    def _decide_b8(self, accumulators=None):
        """The B8 form of this object: gathers the facts of ``b8_form.B8Facts`` and asks ``b8_form.choose_b8``.  Asked on every
        read, never stored: the schedule may still be open.  ``accumulators``: the band accumulators a finish is about to
        read (:py:meth:`_finish_bands`); the properties answer for the object."""
        # (``reals`` / ``half``: only then does what is asked of the library and of the facets matter)
        core = self.core
        reals = not self._auto_axis and self.wave_axis == 1 and self._facet_dtype == _torch().float32
        half = reals and self._want_half_length
        reals64 = not self._auto_axis and self.wave_axis == 1 and self._facet_dtype == _torch().float64
        f64 = getattr(core, "supports_real_facets_out_f64", None)  # (a core without the method has no such form)
        return choose_b8(B8Facts(
            resolved=not self._auto_axis, wave_axis=self.wave_axis, facet_dtype=fdt.name_of(self._facet_dtype),
            half_length_asked=self._want_half_length, real_facets_out=reals and core.supports_real_facets_out(),
            real_facets_out_c2r=half and core.supports_real_facets_out_c2r(),
            pairs=half and all(fdt.loads_as_pairs(cfg.size, cfg.off1, core.yN_size) for cfg in self.facets_config_list),
            accumulators_complex64=None if accumulators is None else accumulators.dtype == _torch().complex64,
            real_facets_out_f64=bool(reals64 and f64 is not None and f64())))

    @property
    def real_finish_native(self):
        """By which path :py:meth:`finish` produces real facets: True = the finishing row kernels store float32 (band
        schedule, complex64, ``core.supports_real_facets_out()``) or float64 (band schedule, complex128,
        ``core.supports_real_facets_out_f64()``), False = complex finish and a copy of the real part per
        facet (also: the facets are complex).  ``None`` until the schedule is resolved."""
        return self._decide_b8().native

    @property
    def half_length_finish(self):
        """True when :py:meth:`finish` runs the half-length form of the contiguous-axis kernel: asked for
        (``half_length_finish=True``), :py:attr:`real_finish_native` holds, ``core.supports_real_facets_out_c2r()``, and every
        facet has an even size at an even position of the padded row (the kernel stores aligned pairs of pixels).
        Otherwise False: the real-store form, bit for bit what the pass gives without the keyword."""
        return self._decide_b8().half_length

    def _handed_out(self, facet):
        """a facet finished complex as :py:meth:`finish` hands it out: itself, or -- real facets -- its real part as a tensor of
        its own.  The caller keeps no name for the complex one: it is gone before the next facet is finished"""
        if not self._decide_b8().real_facets:
            return facet
        self._check_facet_dtype(facet.dtype)  # (contributions handed straight to accumulate_wave show their dtype only here)
        return facet.real.contiguous()

    def add_new_subgrid_task(self, subgrid_config, new_subgrid_task):
        """Fold one subgrid into the facet sums (reference api.py:347-372)."""
        return self.add_new_subgrid_tasks([subgrid_config], [new_subgrid_task])

    def _resolve_axis(self, first_subgrid):
        """Fix the automatic schedule on the FIRST data this object sees, whichever public entry point it arrives
        through (add_new_subgrid_task(s), wave_contributions, accumulate_wave / accumulate_chunks); it never changes
        afterwards (r3 advice: the low-level entry points used to leave it open, and a later add flipped the schedule
        under accumulators of the other kind)."""
        if not self._auto_axis:
            return
        self._auto_axis = False
        torch = _torch()
        dt = first_subgrid.dtype
        is_c64 = dt in (torch.complex64, torch.float32) if isinstance(first_subgrid, torch.Tensor) else (
            numpy.asarray(first_subgrid).dtype in (numpy.complex64, numpy.float32)
        )
        if self._fixed_dtype is not None:  # the accumulators' dtype, not the data's, decides
            is_c64 = self._fixed_dtype == torch.complex64
        sizes = {cfg.size for cfg in self.facets_config_list}
        if self._plan is not None and is_c64 and len(sizes) == 1 and self.core.supports_backward_band(torch.complex64):
            self.wave_axis = 1

    def add_new_subgrid_tasks(self, subgrid_configs, new_subgrid_tasks):
        """Fold a list of subgrids into the facet sums (extension: consecutive
        subgrids sharing the wave key -- ``off0``, or ``off1`` with ``wave_axis=1`` -- and ``size`` are processed
        as one wave with batched launches).

        Band schedule (``wave_axis=1``): the per-wave kernels run over ALL subgrids of a wave at once, so subgrids
        that arrive one by one (or in pieces of a planned wave) are first staged -- a device copy into a per-key
        buffer held in ``LRUCache(lru_backward)``, the counterpart of the reference's per-column partial sums
        (api.py:402-438) -- and the wave is folded into the band accumulators when it is complete (plan known),
        evicted from the cache, or at :py:meth:`finish`."""
        new_subgrid_tasks = [_unwrap(t) for t in new_subgrid_tasks]
        if len(subgrid_configs) and self._auto_axis:
            self._resolve_axis(new_subgrid_tasks[0])
        col = None
        i = 0
        key = "off1" if self.wave_axis == 1 else "off0"
        while i < len(subgrid_configs):
            j = i + 1
            while (
                j < len(subgrid_configs)
                and getattr(subgrid_configs[j], key) == getattr(subgrid_configs[i], key)
                and subgrid_configs[j].size == subgrid_configs[i].size
            ):
                j += 1
            if self.wave_axis == 1:
                col = self._add_band_group(subgrid_configs[i:j], new_subgrid_tasks[i:j])
            else:
                col = self._add_wave(subgrid_configs[i:j], new_subgrid_tasks[i:j])
            i = j
        return col

    # ---- wave_axis = 1: staging of partial waves (the role of lru_backward in the band schedule)
    def _planned_count(self, off1, size):
        if self._plan is None:
            return None
        if self._plan_counts is None:
            counts = {}
            for c in self._plan:
                k = (int(c.off1), int(c.size))
                counts[k] = counts.get(k, 0) + 1
            self._plan_counts = counts
        return self._plan_counts.get((int(off1), int(size)))

    def _add_band_group(self, sgs, subgrids):
        key = (int(sgs[0].off1), int(sgs[0].size))
        if self._plan is not None and not any(int(c.off1) == key[0] for c in self._plan):
            raise ValueError(f"subgrid off1={key[0]} is not in the subgrid_configs this SwiftlyBackward was planned for")
        staged = self.lru.get(key)
        planned = self._planned_count(*key)
        if staged is None and (len(sgs) == planned or (planned is None and len(sgs) > 1)):
            return self._add_wave(list(sgs), list(subgrids))  # a whole wave at once: no staging copy
        torch = _torch()
        core = self.core
        xA = sgs[0].size
        sdt = self._fixed_dtype or torch.complex64  # staging dtype
        if staged is None:
            cap = planned if planned is not None else 8
            staged = dict(cfgs=[], buf=torch.empty((max(cap, len(sgs)), xA, xA), dtype=sdt, device=core.device))
        need = len(staged["cfgs"]) + len(sgs)
        if need > staged["buf"].shape[0]:
            grown = torch.empty((max(need, 2 * staged["buf"].shape[0]), xA, xA), dtype=sdt, device=core.device)
            grown[: len(staged["cfgs"])].copy_(staged["buf"][: len(staged["cfgs"])])
            staged["buf"] = grown
        for sg, data in zip(sgs, subgrids):
            ten, _ = core._as_device(data)  # pylint: disable=protected-access
            if tuple(ten.shape) != (xA, xA):
                raise ValueError(f"subgrid has shape {tuple(ten.shape)}, expected {(xA, xA)}")
            if ten.dtype != sdt:
                if self._fixed_dtype is not None:
                    raise ValueError(f"SwiftlyBackward(wave_axis=1, dtype={sdt}) got {ten.dtype} data")
                raise ValueError("SwiftlyBackward(wave_axis=1) needs complex64 data and power-of-two yN_size / xM_yN_size")
            staged["buf"][len(staged["cfgs"])].copy_(ten)
            staged["cfgs"].append(sg)
        if planned is not None and len(staged["cfgs"]) >= planned:
            self.lru.discard(key)
            return self._flush_staged(staged)
        old_key, old = self.lru.set(key, staged)
        if old_key is not None and old is not None:
            self._flush_staged(old)
        return self.bands.bands

    def _flush_staged(self, staged):
        n = len(staged["cfgs"])
        return self._add_wave(staged["cfgs"], [staged["buf"][k] for k in range(n)])

    def _first_dtype(self, dtype):
        """the first data shows the dtype, where none was fixed: ``facet_dtype`` has its precision"""
        if self.dtype is None:
            self.dtype = dtype
            self._check_facet_dtype(dtype)

    def wave_contributions(self, sgs, subgrids):
        """``prepare_and_split_subgrid`` (reference api_helper.py:115-139) for a
        wave: contributions ``[F, S, m, m]`` of the subgrids ``sgs`` (same size)
        to every facet -- what the reference ships from the subgrid's worker to
        the facets' workers (api.py:357-364).  On the fused route the result lives in one of two alternating
        workspaces of this object: it stays valid until the second-next call."""
        if self._auto_axis and len(subgrids):
            self._resolve_axis(_unwrap(subgrids[0]))
        if self.dtype is None and len(subgrids):
            first, _ = self.core._as_device(subgrids[0])  # pylint: disable=protected-access
            self._first_dtype(first.dtype)
            subgrids = [first, *subgrids[1:]]  # (uploaded once)
        return self.splitter.contributions(sgs, subgrids, self.wave_axis == 1 and self._fixed_dtype is not None, self.dtype)

    def accumulate_wave(self, sgs, parts):
        """``accumulate_column`` (reference api_helper.py:142-152) for a wave:
        add the contributions ``parts[F, S, m, m]`` of subgrids sharing the wave key
        into that wave's partial sums.  Grouping key: ``off0`` with ``wave_axis=0`` (the reference's schedule: LRU
        cache keyed by ``off0``, reference api.py:402-438; evicted columns go to the facet accumulators), ``off1``
        with ``wave_axis=1`` (band schedule: the wave is folded straight into the band accumulators).  With
        ``wave_axis=None`` the schedule is fixed by the first data this object sees (:py:meth:`_resolve_axis`); a wave
        whose subgrids do not share the key of the resolved schedule raises ``ValueError``."""
        self._resolve_axis(parts)
        if self.wave_axis == 1:
            return self.bands.accumulate(sgs[0].off1, [(sgs, parts)], self._first_dtype)
        return self.columns.accumulate_wave(sgs, parts)

    def accumulate_chunks(self, off0, chunks):
        """:py:meth:`accumulate_wave` for contributions that arrive in several pieces (one per source rank of
        the multi-GPU exchange): ``chunks = [(subgrid configs, parts[F, S_c, m, m]), ...]``, all of wave ``off0`` --
        the wave KEY: the subgrids' ``off0`` with ``wave_axis=0``, their ``off1`` with ``wave_axis=1`` (checked)."""
        if self._auto_axis and len(chunks):
            self._resolve_axis(chunks[0][1])
        if self.wave_axis == 1:  # ``off0`` is the wave key: the subgrids' off1
            return self.bands.accumulate(off0, chunks, self._first_dtype)
        if len(chunks):
            self._first_dtype(chunks[0][1].dtype)
        return self.columns.accumulate(off0, chunks)

    def _add_wave(self, sgs, subgrids):
        parts = self.wave_contributions(sgs, subgrids)
        col = self.accumulate_wave(sgs, parts)
        self.task_queue.process([col])
        return col

    def _finish_bands(self):
        torch = _torch()
        core = self.core
        out = []
        bands = self.bands.hand_out()
        if bands is None:
            dt = self.facet_dtype or torch.complex64
            return [torch.zeros((cfg.size, cfg.size), dtype=dt, device=core.device) for cfg in self.facets_config_list]
        form = self._decide_b8(bands)
        for j, cfg in enumerate(self.facets_config_list):
            if form.native and self._facet_dtype == torch.float64:  # float64 straight from the complex128 row kernels
                out.append(core.finish_facet_band_float64(bands[j], self.bands.band, cfg.off1, cfg.size, mask=cfg.mask1))
            elif form.native:  # float32 straight from the row kernels: no complex facet exists
                out.append(core.finish_facet_band(bands[j], self.bands.band, cfg.off1, cfg.size, mask=cfg.mask1, real=True,
                                                  half_length=form.half_length))
            else:
                out.append(self._handed_out(core.finish_facet_band(bands[j], self.bands.band, cfg.off1, cfg.size,
                                                                   mask=cfg.mask1)))
        self.bands.release()
        return out

    def finish(self):
        """Flush the column cache and finish all facets (reference
        api.py:374-400, api_helper.py:182-197).  A facet that never received a
        contribution is all zeros (the reference raises AttributeError there,
        api_helper.py:184-187)."""
        if self.wave_axis == 1:
            for _key, staged in self.lru.pop_all():
                self._flush_staged(staged)
            out = self._finish_bands()
        else:
            out = self.columns.finish(self.facet_dtype or _torch().complex64, self._handed_out)
        self.task_queue.wait_all_done()
        return [DeviceTask(t) for t in out] if self.delayed else out
