"""
``SwiftlyForward``: the facet -> subgrid direction of the streaming API (reference src/ska_sdp_exec_swiftly/api.py:217-324,
task bodies api_helper.py:73-112, 200-210) on one MI355X, with the reference's schedule (``wave_axis=0``) and the
contiguous-axis-first band pipeline (``wave_axis=1``).
"""
import logging
import os
from functools import cached_property

from . import _lib, slabs
from .core_hip import band_range
from .facet_dtype import loads_as_pairs, single_forward_keywords
from .ingest import _FacetIngest, _mask_table
from .k1_form import K1Facts, axis1_active, choose_k1, may_fuse
from .prefetch import WavePrefetch, _knobs
from .tasks import DeviceTask, LRUCache, TaskQueue, _torch, _unwrap

log = logging.getLogger("fourier-logger")


def preferred_wave_axis(swiftly_config, dtype=None, n_facets=None):
    """Which subgrid offset the forward engine should group "waves" by for
    row-major facets: 0 = ``off0`` (the reference's column cache key,
    api.py:300-324; full-facet transform along the strided axis 0 first),
    1 = ``off1`` (full-facet transform along the CONTIGUOUS axis first: one
    kernel instead of a four-step with a facet-sized scratch; the axis order is
    free because the transforms are separable).  1 when the kernels of that
    pipeline exist for the configuration's sizes, dtype and -- when given -- the TOTAL number of facets of the
    cover (the fused subgrid side sums all facets in one kernel, at most ``core.MAX_FUSED_FACETS``)."""
    return 1 if swiftly_config.core.supports_band_pipeline(dtype, n_facets) else 0


K1_DESCRIPTION = {
    0: "K1 prepare_facet(axis=0) per facet = col_pass<n1=128, mapped load> + col_pass<n2=256, mapped store>",
    1: "K1 prepare_facet(axis=1) of all facet rows, band-compacted parity-split store = row_pass_band_kernel (2 workgroups per row)",
}

class SwiftlyForward(WavePrefetch):
    """Facet -> subgrid streaming transform (reference api.py:217-324).

    :param swiftly_config: SwiftlyConfig
    :param facet_tasks: list of ``(FacetConfig, facet_data)``; data may be a
        numpy array or a torch tensor (complex64 or complex128; it is uploaded
        once and stays in HBM).  Real-valued facets given as float32 stay float32 -- on the host, on the wire and in HBM,
        half the bytes -- when every facet is float32, the object runs ``wave_axis == 1`` with a K1 that loads reals
        (``core.supports_real_facets()``; under ``axis1_first=True``, whose whole-row K1 finishes the contiguous axis, only
        when ``facet_dtype`` asks for it); see :py:attr:`facet_dtype`.  In every other case they are promoted to complex64
    :param lru_forward: number of subgrid columns (distinct ``off0``) whose
        prepared facet columns ``NMBF_BF`` are kept
    :param queue_size: bound on unfinished subgrid tasks (reference
        ``TaskQueue``, api.py:466-522): ``get_subgrid_task`` blocks the host
        while that many earlier results are still being computed
    :param subgrid_configs: optional (extension) list of all subgrids that will
        be requested; enables row-compacted ``BF_F`` for sparse subgrid sets
    :param facet_dtype: ``None`` (default), or ``torch.float32`` / ``"float32"``: "my facets are real-valued, keep them
        float32 wherever a real K1 exists" -- the accurate order included (``SwiftlyConfig(axis1_first=True)`` with a plan:
        the real window-rows form of the whole-row K1, ``core.supports_window_rows(..., real=True)``), which the default
        leaves on promoted complex64 facets.  Every facet must then be float32 (``ValueError`` otherwise).  Where no real K1
        exists (``wave_axis=0``, ``yN_size`` = Q * 2^k, facets above 23552 pixels at ``yN_size`` 32768, device rows that
        are not 8-byte aligned at an even pitch under the accurate order, the multi-GPU classes without their own
        ``facet_dtype`` keyword) the facets are promoted as
        before and :py:attr:`facet_dtype` says complex64.  The results are those of the promoted facets bit for bit.
        ``torch.float64`` / ``"float64"``: "my facets are real-valued float64 images, keep them float64 through the
        complex128 band pipeline" (``wave_axis=1``; ``core.supports_band_pipeline(torch.complex128, n, explicit=True)`` and
        ``core.supports_real_facets_f64()``): every facet must be a float64 host array or a row-major 2-D float64 tensor
        (``ValueError`` otherwise); they stay float64 on the host, on the wire and in HBM -- 8 bytes per pixel where the
        promoted facet holds 16 -- and K1 is ``core.prepare_facet_band_float64``.  The subgrids are those of the promoted
        facets bit for bit.  Where no float64 K1 exists (``wave_axis=0``, other sizes) the facets are promoted as before and
        :py:attr:`facet_dtype` says complex128; without the keyword float64 facets are always promoted.
        Any other value: ``ValueError``
    :param half_length_k1: ``True`` (with ``facet_dtype=float32``, ``ValueError`` without): K1 of the real facets as ONE
        half-length transform per row (``core.prepare_facet_band(..., half_length=True)``) where that form exists
        (``core.supports_real_facets_rfft()``: ``yN_size`` 32768, ``_lib.FEATURE_REAL_FACETS_RFFT``, or 65536,
        ``_lib.FEATURE_REAL_FACETS_RFFT_64K``) and every facet can be loaded as pairs -- an even facet
        size, even positions in the padded row, device rows 8-byte aligned at an even pitch -- in the modes that store the
        band (axis-1-first mode 2 keeps its window-rows K1).  The results are those of the promoted facets within the same
        bound, not bit for bit; such facets stay float32 whatever their size.  Where the form is not available the object
        runs exactly what it runs without the keyword; :py:attr:`half_length_k1` says which happened
    """

    # pylint: disable=too-many-arguments,too-many-instance-attributes
    def __init__(
        self, swiftly_config, facet_tasks, lru_forward=1, queue_size=20, client=None, subgrid_configs=None,
        wave_axis=None, delayed=False, facet_dtype=None, half_length_k1=False,
    ):
        facet_tasks = list(facet_tasks)
        self._facet_dtype_asked = single_forward_keywords(facet_dtype, half_length_k1, (_unwrap(t[1]) for t in facet_tasks))
        self._half_length_asked, self._k1 = bool(half_length_k1), None  # (the K1 form: _decide_k1)
        WavePrefetch.__init__(self)
        self.delayed = bool(delayed)  # hand out DeviceTask handles instead of bare device tensors
        facet_tasks = [(cfg, _unwrap(data)) for cfg, data in facet_tasks]
        self.config = swiftly_config
        self.core = swiftly_config.core
        self.facet_tasks = facet_tasks
        self.task_queue = TaskQueue(queue_size)
        self.facet_configs = [cfg for cfg, _ in facet_tasks]
        self.queue_size = queue_size
        self._client = client
        self.lru = LRUCache(lru_forward)
        # valid for one set of band buffers (set_band / install_bands): the buffers, their band (with it the axis-1-first mode
        # of ``_k1``) and mode 2's {wave key: window}; the event behind K1, the one the side stream waited for, "a prefetched
        # K2 has forked"
        self.BF_Fs_persist, self._band, self._window_of = None, None, None
        self._bands_ready, self._side_waited, self._k2_chain_forked = None, None, False
        self._bands_own = False  # the band buffers are this object's own K1 output (not injected through install_bands)
        # column slabs of K2 (slabs.py): a cache of their own, so that the two slabs of the wave being served fit whatever
        # ``lru_forward`` is
        self._slab_lru = LRUCache(max(1, int(lru_forward)) + 1)
        # slabs the cache pushed out while a planned wave that reads them has not been served yet (the wave at the wrap of
        # the cyclic axis shares a slab with the first one of the walk), and {slab: waves served from its present copy}
        self._slab_kept, self._slab_served = {}, {}
        self._slab_rowmaps = {}
        self._prewindowed = False
        torch = _torch()
        # facet ingestion (host <-> device edge): device tensors are used in place; host (numpy) facets are
        # uploaded on a dedicated copy stream through a small ring of pinned staging buffers, and the compute
        # stream waits per facet only when a kernel first needs it -- the PCIe transfer of facet j+1 overlaps
        # the full-facet transform of facet j
        self._ingest = _FacetIngest(self.core, float64=self._facet_dtype_asked == torch.float64)
        self._facet_info = [self._ingest.add(data) for _, data in facet_tasks]
        dtypes = {info[0] for info in self._facet_info}
        if len(dtypes) > 1:
            raise ValueError("all facets must have the same dtype")
        self.dtype = dtypes.pop() if dtypes else torch.complex64
        if self._facet_dtype_asked == torch.float32 and not self._ingest.all_float32:
            raise ValueError("facet_dtype=float32 needs every facet as a row-major float32 array")
        if self._facet_dtype_asked == torch.float64 and (self.dtype != torch.complex128 or not self._ingest.all_float64):
            raise ValueError(f"facet_dtype=float64 needs float64 facets in a complex128 pass, got a {self.dtype} pass")
        if wave_axis is None:
            # default: the reference's schedule (waves keyed by off0) -- unless the caller hands over the plan of
            # subgrids it is going to request AND the contiguous-axis-first kernels exist for this configuration:
            # then that pipeline is used, and requests that cover only part of a planned wave are served from a
            # bounded cache of finished subgrids (below), so that ANY request order stays cheap
            self.wave_axis = 1 if subgrid_configs is not None and self._band_pipeline_ok() else 0
        else:
            self.wave_axis = int(wave_axis)
        if self.wave_axis not in (0, 1):
            raise ValueError("wave_axis must be 0 or 1")
        # optional plan (extension): when the caller knows up front which subgrids it will ask for (sparse
        # covers, scripts/demo_sparse_facet.py style), the facet-sized intermediate only keeps what those read
        self._rowmap, self._n_rows = None, None
        self._plan, self._planned_keys = None, None
        if subgrid_configs is not None:
            self._plan = list(subgrid_configs)
            if self.wave_axis == 0:
                self._rowmap, self._n_rows = self.core.subgrid_column_rows([sg.off0 for sg in subgrid_configs])
            self._planned_keys = {int(self._key(sg)) for sg in subgrid_configs}
        self._wave_rowmaps = {}
        # finished subgrids computed ahead of their request (see get_subgrid_tasks): (off0, off1, size, id) -> tensor
        self._results = {}
        self._result_bytes = 0
        self._result_budget = int(float(os.environ.get("SWIFTLY_RESULT_CACHE_GB", "16")) * 2**30)
        # float32 facets: kept as they are when this object's K1 loads reals, promoted to complex64 otherwise (float64 facets
        # of a caller who asked: float64 or complex128) -- decided before the first upload, for the band its own K1 will get
        self._ingest.settle(self._decide_k1(own=True).facets_real)
        self._ingest.prefetch(0)

    @property
    def facet_dtype(self):
        """dtype of the facets as they are resident: ``torch.float32`` (in a complex128 pass ``torch.float64``) when
        real-valued facets were kept real, else :py:attr:`dtype` (the complex dtype everything downstream of K1 computes in)"""
        torch = _torch()
        if not self._ingest.real:
            return self.dtype
        return torch.float64 if self.dtype == torch.complex128 else torch.float32

    @property
    def half_length_k1(self):
        """does K1 of this object run the half-length transform of real rows (the ``half_length_k1`` keyword, where the form
        exists and every facet can be loaded as pairs)?"""
        return self._k1.half_length

    def _own_band(self):
        """the band this object's own K1 stores: the plan's (complex128, or no plan: the whole padded axis, plain band layout)"""
        planned = self._plan is not None and self.dtype == _torch().complex64
        return self.core.band_for_offsets([sg.off1 for sg in self._plan]) if planned else (0, self.core.yN_size)

    def _decide_k1(self, band=None, own=False):
        """The K1 form of this object for ``band`` (``own``: the band of its own K1, worked out only where it matters): gathers
        the facts of ``k1_form.K1Facts``, asks ``k1_form.choose_k1`` and stores the answer.  The first call (the constructor's)
        decides whether float32 facets stay float32 and whether K1 runs the half-length form; later ones (``set_band``) only
        the axis-1-first mode."""
        # (``reals``: only then does what is asked of the library and of the tensors matter)
        core, ingest, reals = self.core, self._ingest, self._ingest.all_float32 and self.wave_axis == 1
        torch = _torch()
        reals64 = getattr(ingest, "all_float64", False) and self.wave_axis == 1
        sizes, off1s = [info[1][-1] for info in self._facet_info], [int(cfg.off1) for cfg in self.facet_configs]
        facts = K1Facts(
            wave_axis=self.wave_axis, complex64=self.dtype == torch.complex64, all_float32=ingest.all_float32,
            float32_asked=self._facet_dtype_asked == torch.float32, half_length_asked=self._half_length_asked,
            keeps_real=self._keep_real_facets, axis1_first=getattr(core, "axis1_first", False), axis1_fused=self.axis1_fused,
            planned=self._plan is not None, real_facets=reals and core.supports_real_facets(),
            real_facets_rfft=reals and core.supports_real_facets_rfft(),
            rows_match_promoted=all(core._real_rows_match_promoted(n) for n in sizes),  # pylint: disable=protected-access
            even=all(loads_as_pairs(n, off1, core.yN_size) for n, off1 in zip(sizes, off1s)),
            # (device facets are read in place: two adjacent reals must be one aligned 8-byte load; uploads are contiguous)
            aligned=reals and all(t is None or t.device != core.device or (t.stride(0) % 2 == 0 and t.data_ptr() % 8 == 0)
                                  for t in ingest.tensors), settled=self._k1,
            all_float64=getattr(ingest, "all_float64", False), float64_asked=self._facet_dtype_asked == torch.float64,
            real_facets_f64=bool(reals64 and core.supports_real_facets_f64()))
        # (only then are the window rows asked about: they need the plan's waves and a facet -- a rank may own none)
        if (own or band is not None) and sizes and may_fuse(facts):
            band = self._own_band() if own else band
            rows = [core.supports_window_rows(band, sizes[0], off1s, len(self._planned_keys), real) for real in (False, True)]
            facts = facts._replace(window_rows=rows[0], window_rows_real=rows[1])
        self._k1 = choose_k1(facts)
        return self._k1

    # -- tables derived from the plan: each built on first use by ONE walk over the plan (505 configs x 25 waves on every
    # pass otherwise), and not at all for objects that never need it
    @cached_property
    def _plan_waves(self):
        """({(wave key, size): planned subgrids in plan order, duplicates dropped}, {identities of the planned subgrids})"""
        waves, seen = {}, set()
        for c in self._plan:
            r = self._rid(c)
            if r not in seen:
                seen.add(r)
                waves.setdefault((int(self._key(c)), int(c.size)), []).append(c)
        return waves, seen

    @cached_property
    def _plan_off0s(self):
        """{off1: the off0 of the planned subgrids of that wave}"""
        by_key = {}
        for sg in self._plan:
            by_key.setdefault(int(sg.off1), []).append(sg.off0)
        return by_key

    @cached_property
    def _plan_set(self):
        """{(off0, off1) of the planned subgrids}"""
        return {(int(sg.off0), int(sg.off1)) for sg in self._plan}

    def _band_pipeline_ok(self):
        """the contiguous-axis-first pipeline can serve these facets (sizes, dtype, layout, facet count)"""
        torch = _torch()
        sizes = {info[1] for info in self._facet_info}
        return (
            self.dtype == torch.complex64
            and len(sizes) == 1
            and all(info[2] for info in self._facet_info)
            and self.core.supports_band_pipeline(self.dtype, len(self._facet_info))
        )

    # -- stage 1: BF_F = prepare_facet(axis 0), once per facet (api.py:281-298)
    def _prepare_one_facet(self, j):
        """BF_F of facet ``j`` as the streaming classes keep it: (optionally) row-compacted and with the
        axis-1 window of extract_column already applied (it commutes with the axis-0 transform), so the
        column kernel has no window loads; complex128 and unsupported sizes use the plain primitive."""
        cfg, data = self.facet_configs[j], self._ingest.ready(j)
        n_rows = self._n_rows if self._rowmap is not None else self.core.yN_size
        if self._prewindowed or self._rowmap is not None:
            return self.core.prepare_facet_rows(
                data, cfg.off0, self._rowmap, n_rows, fold_axis1_window=self._prewindowed
            )
        return self.core.prepare_facet(data, cfg.off0, axis=0)

    def prepare_all_facets(self, timer=None):
        """Stage 1 for every facet (idempotent).  ``timer`` (optional, bench.py's
        StageTimer) brackets each facet's launch group with HIP events."""
        if self.wave_axis == 1:
            return self._prepare_all_bands(timer)
        if self.BF_Fs_persist is None:
            self._prewindowed = self.dtype == _torch().complex64
            out = []
            for j in range(len(self.facet_configs)):
                t0 = timer.start() if timer is not None else None
                out.append(self._prepare_one_facet(j))
                self._ingest.prefetch(j + 1)
                if timer is not None:
                    timer.stop("K1_full_facet_transform", t0)
            self.BF_Fs_persist = out
        return self.BF_Fs_persist

    def _get_BF_Fs(self):
        return self.prepare_all_facets()

    # -- stage 2: per subgrid column (api.py:300-324)
    def get_NMBF_BFs_off0(self, off0, BF_Fs=None):
        """prepared facet columns for subgrid column ``off0`` (LRU cached)"""
        if self.wave_axis != 0:
            raise ValueError(
                "get_NMBF_BFs_off0 belongs to the reference schedule (wave_axis=0); this SwiftlyForward runs the "
                "contiguous-axis-first pipeline (wave_axis=1, the default with a subgrid plan): construct it with wave_axis=0"
            )
        if BF_Fs is None:
            BF_Fs = self._get_BF_Fs()
        elif BF_Fs is not self.BF_Fs_persist:
            # BF_Fs_persist holds pre-windowed / row-compacted data (see _prepare_one_facet); a plain
            # prepare_facet(axis=0) result would silently miss the axis-1 window
            raise ValueError("get_NMBF_BFs_off0 only accepts the BF_Fs this object prepared itself")
        cols = self.lru.get(off0)
        if cols is None:
            if self._plan is not None and int(off0) not in self._planned_keys:
                raise ValueError(f"subgrid column off0={off0} was not in the subgrid_configs plan")
            torch = _torch()
            core = self.core
            cols = torch.empty(
                (len(BF_Fs), core.xM_yN_size, core.yN_size), dtype=self.dtype, device=core.device
            )
            for j, (cfg, BF_F) in enumerate(zip(self.facet_configs, BF_Fs)):
                core.extract_column(BF_F, off0, cfg.off1, out=cols[j], rowmap=self._rowmap, prewindowed=self._prewindowed)
            self.lru.set(off0, cols)
        return cols

    # -- stage 3: per subgrid (api.py:255-279 + api_helper.py:73-112)
    def get_subgrid_task(self, subgrid_config):
        """Finished (masked) subgrid ``[size, size]`` as a device tensor
        (reference api.py:238-253)."""
        return self.get_subgrid_tasks([subgrid_config])[0]

    def _key(self, sg):
        return sg.off1 if self.wave_axis == 1 else sg.off0

    def get_subgrid_tasks(self, subgrid_configs):
        """Finished subgrids for a list of configs; consecutive configs with the
        same wave key (``off0``, or ``off1`` when ``wave_axis == 1``) and
        ``size`` are processed as one wave.  Each result is registered with the
        task queue (``queue_size``).

        With a ``subgrid_configs`` plan, a request that covers only PART of a planned wave (e.g. the reference's
        natural ``off0``-major loop over a cover while the waves are keyed by ``off1``) computes the whole
        planned wave once and keeps the subgrids that were not asked for yet in a cache bounded by
        ``SWIFTLY_RESULT_CACHE_GB`` (default 16); each cached subgrid is handed out once.  Beyond the budget the
        request is computed on its own (correct, slower)."""
        out = []
        i = 0
        while i < len(subgrid_configs):
            j = i + 1
            while (
                j < len(subgrid_configs)
                and self._key(subgrid_configs[j]) == self._key(subgrid_configs[i])
                and subgrid_configs[j].size == subgrid_configs[i].size
            ):
                j += 1
            tasks = self._serve_group(list(subgrid_configs[i:j]))
            self.task_queue.process(tasks)
            out.extend(DeviceTask(t) for t in tasks) if self.delayed else out.extend(tasks)
            i = j
        return out

    @staticmethod
    def _rid(sg):
        """identity of a request: its VALUE (equal configs of a rebuilt cover match the plan, r3 advice)"""
        return (int(sg.off0), int(sg.off1), int(sg.size))

    def _planned_wave_of(self, sg):
        """the planned subgrids that share ``sg``'s wave key and size, in plan order, duplicates dropped (None without
        a plan or when ``sg`` is not in the plan)"""
        if self._plan is None:
            return None
        waves, seen = self._plan_waves
        if self._rid(sg) not in seen:
            return None
        return waves.get((int(self._key(sg)), int(sg.size)))

    def _drop_result(self, rid):
        hit = self._results.pop(rid, None)
        if hit is not None:
            self._result_bytes -= hit.numel() * hit.element_size()
        return hit

    def _serve_group(self, group):
        """results for consecutive requests sharing the wave key: cache hits, a whole planned wave computed ahead,
        or just the group"""
        rids = [self._rid(sg) for sg in group]
        distinct = len(set(rids)) == len(rids)
        if distinct and all(r in self._results for r in rids):
            return [self._drop_result(r) for r in rids]  # each cached subgrid is handed out once
        # partial hits: the whole group is recomputed below, so the cached copies of its members are released
        # (r3 advice: they used to stay behind and shrink the budget for good)
        for r in set(rids):
            self._drop_result(r)
        full = self._planned_wave_of(group[0])
        if full is not None and distinct:
            in_full = {self._rid(c) for c in full}
            if all(r in in_full for r in rids):
                asked = set(rids)
                extra = [c for c in full if self._rid(c) not in asked and self._rid(c) not in self._results]
                esize = _torch().empty((), dtype=self.dtype).element_size()
                nbytes = sum(c.size * c.size for c in extra) * esize
                if extra and self._result_bytes + nbytes <= self._result_budget:
                    # (the requested config objects take the place of their plan twins: their masks are the ones asked for)
                    req = dict(zip(rids, group))
                    full = [req.get(self._rid(c), c) for c in full]
                    res = self.get_wave(full)
                    by_rid = {self._rid(c): res[k] for k, c in enumerate(full)}
                    for c in extra:
                        self._results[self._rid(c)] = by_rid[self._rid(c)]
                    self._result_bytes += nbytes
                    return [by_rid[r] for r in rids]
        res = self.get_wave(group)
        return [res[k] for k in range(len(group))]

    def get_wave(self, sgs, timer=None):
        """Finished, masked subgrids ``[S, xA, xA]`` of one wave (configs sharing
        the wave key and size).  ``timer`` brackets the stages with HIP events."""
        self.prepare_all_facets()
        if timer is None and self.wave_axis == 1:
            return self._wave_b(sgs)  # two native calls per wave
        t0 = timer.start() if timer is not None else None
        if self.wave_axis == 1:
            self._get_wave_columns(sgs[0].off1)
        else:
            self.get_NMBF_BFs_off0(sgs[0].off0)
        if timer is not None:
            timer.stop("K2_wave_facet_transform", t0)
            t0 = timer.start()
        res = self._wave_b_staged(sgs) if self.wave_axis == 1 else self._wave(sgs)
        if timer is not None:
            timer.stop("K345_extract_sum_finish", t0)
        return res

    def wave_contributions(self, sgs):
        """Contributions of every (local) facet to the subgrids ``sgs`` (same
        ``off0``): tensor ``[F, S, m, m]`` -- the data the reference ships
        between Dask workers (api.py:263-277) and the multi-GPU path ships
        through the all-to-all."""
        if self.wave_axis != 0:
            raise ValueError(
                "wave_contributions belongs to the reference schedule (wave_axis=0); with wave_axis=1 use "
                "distributed.DistributedForward.pack_wave / wave_blocks_into"
            )
        torch = _torch()
        core = self.core
        m, yN = core.xM_yN_size, core.yN_size
        S, F = len(sgs), len(self.facet_configs)
        cols = self.get_NMBF_BFs_off0(sgs[0].off0)
        contrib = torch.empty((F, S, m, m), dtype=self.dtype, device=core.device)
        off1s = [sg.off1 for sg in sgs]
        for j in range(F):
            core.launch("extract_from_facet", cols[j], m, yN, 1, contrib[j], m, 1,
                        nbatch=S, in_bs=0, out_bs=m * m, offs=off1s)
        return contrib

    def supports_fused_subgrid_side(self):
        """transform_contributions / sum_finish_facets available for this configuration and dtype"""
        return self.core.supports_fused_subgrid(self.dtype)

    def _wave_source(self, sgs):
        """(source tensor, layout, window offsets, row map) of the wave for transform_contributions"""
        if self.wave_axis == 1:
            Q, rowmap = self._get_wave_columns(sgs[0].off1)
            return Q, 1, [sg.off0 for sg in sgs], rowmap
        return self.get_NMBF_BFs_off0(sgs[0].off0), 0, [sg.off1 for sg in sgs], None

    def wave_blocks(self, sgs, out=None, transformed=True):
        """Per-(facet, subgrid) ``[m, m]`` blocks of THIS object's facets for the subgrids ``sgs`` of one wave,
        ``[F, S, m, m]`` written into ``out`` (e.g. a slice of an all-to-all send buffer).  ``transformed``:
        the axis-0-transformed blocks ``G`` of transform_contributions (what the fused subgrid side consumes)
        instead of the raw contributions (reference api.py:263-277)."""
        torch = _torch()
        core = self.core
        m = core.xM_yN_size
        F, S = len(self.facet_configs), len(sgs)
        if out is None:
            out = torch.empty((F, S, m, m), dtype=self.dtype, device=core.device)
        if transformed:
            src, layout, offs, rowmap = self._wave_source(sgs)
            core.transform_contributions(src, layout, [cfg.off0 for cfg in self.facet_configs], offs, out=out, rowmap=rowmap)
            return out
        if self.wave_axis != 0:
            raise NotImplementedError("raw contributions are only produced by the wave_axis=0 pipeline")
        cols = self.get_NMBF_BFs_off0(sgs[0].off0)
        off1s = [sg.off1 for sg in sgs]
        for j in range(F):
            core.launch("extract_from_facet", cols[j], m, core.yN_size, 1, out[j], m, 1,
                        nbatch=S, in_bs=0, out_bs=out.stride(1), offs=off1s)
        return out

    def wave_blocks_into(self, sgs, flat, layout):
        """:py:meth:`wave_blocks` (transformed) of a whole wave with per-subgrid placement inside the flat buffer
        ``flat``: block (f, i) at ``layout[0][i] + f * layout[1][i]`` elements -- one native call
        (contiguous-axis-first pipeline only)."""
        self._check_planned(sgs)
        self._facet_side(sgs, flat, layout)

    def _wave(self, sgs):
        # single-GPU route: the [m, m] contributions are never materialised -- the window gather is
        # folded into the axis-0 transform kernel reading the column buffers directly
        cols = self.get_NMBF_BFs_off0(sgs[0].off0)
        try:
            return _finish_from_columns(self.core, cols, 0, self.facet_configs, sgs, [sg.off1 for sg in sgs])
        except NotImplementedError:
            pass
        try:
            colacc = _colacc_from_columns(self.core, cols, self.facet_configs, sgs)
        except NotImplementedError:
            return sum_and_finish_wave(self.core, self.wave_contributions(sgs), self.facet_configs, sgs)
        return _finish_from_colacc(self.core, colacc, self.facet_configs, sgs)

    # -- contiguous-axis-first pipeline (wave_axis == 1) ---------------------------
    def _check_band_pipeline(self):
        torch = _torch()
        if not self.core.supports_band_pipeline(self.dtype, explicit=True):
            if self.dtype == torch.complex128:
                raise ValueError(f"wave_axis=1 is not available for complex128 facets of this configuration: {_lib.last_error()}")
            raise ValueError("wave_axis=1 is not available for this configuration / dtype (see preferred_wave_axis)")
        if len(self.facet_configs) > self.core.MAX_FUSED_FACETS:
            raise ValueError(
                f"wave_axis=1 sums at most {self.core.MAX_FUSED_FACETS} facets per subgrid in its fused kernel, "
                f"got {len(self.facet_configs)}; use wave_axis=0 (preferred_wave_axis(config, dtype, n_facets=...))"
            )
        sizes = {info[1] for info in self._facet_info}
        if len(sizes) != 1 or not all(info[2] for info in self._facet_info) or self.dtype not in (torch.complex64,
                                                                                                  torch.complex128):
            raise ValueError("wave_axis=1 needs equally sized row-major complex64 or complex128 facets")

    def _prepare_all_bands(self, timer=None):
        """K1: band buffers ``[F, yB, band columns]`` -- prepare_facet along axis 1 of every facet row, only the
        columns some planned subgrid window reads, axis-0 window pre-applied.

        (r2's "facet-major schedule" -- K2 of all planned waves per facet on a second stream behind its K1 -- was measured
        no faster than the plain wave loop, K1 and K2 contend for the same HBM / fabric; removed in r4, numbers in
        DESIGN.md section 4.)"""
        if self.BF_Fs_persist is None:
            self._check_band_pipeline()
            torch = _torch()
            core = self.core
            mode = self.set_band(self._own_band())
            F, yB = len(self._facet_info), self._facet_info[0][1][0]
            if mode == 2:
                # axis-1-first pipeline, contiguous-axis finish fused into K1: per facet row, for every planned window, the
                # finished window row (core.prepare_facet_window_rows) instead of the band
                keys = list(self._window_of)
                starts = torch.tensor(core.window_starts(self._band, keys), dtype=torch.int32, device=core.device)
                # wave-major: K2 of wave w reads the contiguous block [f, w] (side by side in a row measured the same)
                bands = torch.empty((F, len(keys), yB, core.xM_yN_size), dtype=self.dtype, device=core.device)
            else:
                bands = torch.empty((F, yB, core.band_columns(self._band)), dtype=self.dtype, device=core.device)
            for j, cfg in enumerate(self.facet_configs):
                data = self._ingest.ready(j)
                t0 = timer.start() if timer is not None else None
                if mode == 2:
                    core.prepare_facet_window_rows(data, cfg.off1, self._band, starts, bands[j])
                elif data.dtype == torch.float64:  # (float64 facets kept real: the float64-load K1 of complex128)
                    core.prepare_facet_band_float64(data, cfg.off1, self._band, out=bands[j])
                else:
                    core.prepare_facet_band(data, cfg.off1, self._band, out=bands[j], half_length=self._k1.half_length)
                if timer is not None:
                    timer.stop("K1_full_facet_transform", t0)
                self._ingest.prefetch(j + 1)
            ready = None
            if self._plan is not None and _knobs()._PREFETCH and _knobs()._PREFETCH_DEPTH >= 2:
                ready = torch.cuda.Event()
                ready.record(torch.cuda.current_stream(core.device))
            self.install_bands(bands, ready)
            self._bands_own = True
        return self.BF_Fs_persist

    def set_band(self, band):
        """First step of installing band buffers: the band they cover decides the axis-1-first mode (returned) and, in mode
        2, the window table -- and with them the shape of the buffers (``[F, W, yB, m]`` against ``[F, yB, band columns]``)."""
        self._band = band
        self._window_of = {k: w for w, k in enumerate(sorted(self._planned_keys))} if self._decide_k1(band).axis1_mode == 2 else None
        return self._k1.axis1_mode

    def install_bands(self, bands, ready=None):
        """Second step: the finished buffers (this object's own K1 output, or what the band-row exchange of the multi-GPU
        pass assembled).  ``ready``: an event recorded behind K1, which lets the side stream run K2 ahead without a hand-over
        per wave (_prefetch_wave); without it every prefetched K2 waits for the caller's stream and none is chained."""
        self.BF_Fs_persist, self._bands_ready = bands, ready
        self._k2_chain_forked = False  # new band buffers: the next prefetched K2 forks behind K1 again
        self._bands_own = False  # (_prepare_all_bands says otherwise for its own)

    def _wave_rows(self, off1):
        """(rowmap, n_rows) of the axis-0 rows the planned subgrids of wave ``off1`` read (None = all rows)."""
        if self._plan is None:
            return None, self.core.yN_size
        key = int(off1)
        if key not in self._wave_rowmaps:
            self._wave_rowmaps[key] = self.core.subgrid_column_rows(self._plan_off0s.get(key, []))
        return self._wave_rowmaps[key]

    #: may the axis-1-first pipeline fuse the contiguous-axis finish into K1?  The multi-GPU classes switch this off for the
    #: objects whose band buffers come from the band-row exchange (cooperative facets).
    axis1_fused = True
    #: may float32 facets stay float32 (see the constructor)?  The multi-GPU classes, which have no real form, switch it off.
    _keep_real_facets = True

    def _axis1(self):
        """the axis-1-first mode of this object (``SwiftlyConfig(axis1_first=True)``, wave_axis = 1): 0 = off, 1 = row pass
        per wave, 2 = fused into K1 (decided when the facets are prepared)"""
        if self._band is None:  # before set_band: without a band there are no window rows, so never mode 2 (a row pass per
            # wave where the pipeline is on) -- or band buffers installed without set_band
            return int(axis1_first_active(self.core, self.wave_axis, self.dtype)) if self.BF_Fs_persist is None else 0
        return self._k1.axis1_mode

    def _placed(self):
        """the ``placed`` argument of the subgrid side: in both axis-1-first modes the blocks arrive finished along axis 1"""
        return bool(self._axis1())

    def _k2_source(self, off1):
        """``(bands, band)`` that K2 of wave ``off1`` reads: the K1 band buffers and the plan's band -- or, in the
        axis-1-first pipeline (``SwiftlyConfig(axis1_first=True)``), the rows finished along the contiguous axis for this
        wave (core.finish_axis1_rows, on the current stream) with the band that is exactly the wave's window."""
        bands = self.BF_Fs_persist
        mode = self._axis1()
        if not mode:
            return bands, self._band
        if mode == 2:  # the window's finished rows: m columns of the K1 output, read as a band that is exactly the window
            core = self.core
            m, w = core.xM_yN_size, self._window_of[int(off1)]
            start = (core.window_starts(self._band, [off1])[0] + self._band[0]) % core.yN_size
            return bands[:, w], (start, m)
        return self.core.finish_axis1_rows(bands, [cfg.off1 for cfg in self.facet_configs], self._band, off1)

    def _k2_finishes_axis1(self):
        """does K2 itself finish the contiguous axis (``SwiftlyConfig(axis1_first="k2")`` in the row-pass mode, on a core
        that has ``prepare_facet_columns_axis1`` for its sizes)?  Else ``"k2"`` runs as ``"rows"`` does.  The gate is asked
        only for the value ``"k2"``."""
        core = self.core
        return (getattr(core, "axis1_first", False) == "k2" and self._axis1() == 1
                and core.supports_axis1_columns(self.dtype))

    def _k2_wave(self, off1, rowmap, n_rows, out=None):
        """K2 of wave ``off1`` on the current stream, the one call both K2 call sites make (here and ``_prefetch_wave``):
        ``core.prepare_facet_columns`` on :py:meth:`_k2_source` -- or, with ``axis1_first="k2"``, ONE call of
        ``core.prepare_facet_columns_axis1`` on the K1 band buffers and the pass's band, which finishes the contiguous axis
        inside K2's first pass instead of a row pass in front of it."""
        off0s = [cfg.off0 for cfg in self.facet_configs]
        if self._k2_finishes_axis1():
            return self.core.prepare_facet_columns_axis1(self.BF_Fs_persist, off0s, [cfg.off1 for cfg in self.facet_configs],
                                                         self._band, off1, rowmap, n_rows, out=out)
        bands, band = self._k2_source(off1)
        return self.core.prepare_facet_columns(bands, off0s, band, off1, rowmap, n_rows, out=out)

    def _get_wave_columns(self, off1):
        """K2: ``(Q[F, rows, m], rowmap)`` for the subgrid wave ``off1`` (LRU cached like the reference's per-off0 columns).  A
        prefetched ``Q`` is taken over; one that has to be computed is checked against the plan first and enters the cache
        after its K2 has been enqueued."""
        self._take_prefetched(off1)
        hit = self.lru.get(("b", off1))
        if hit is None:
            if self._plan is not None and int(off1) not in self._planned_keys:
                raise ValueError(f"subgrid wave off1={off1} was not in the subgrid_configs plan")
            self.prepare_all_facets()
            rowmap, n_rows = self._wave_rows(off1)
            hit = (self._k2_wave(off1, rowmap, n_rows), rowmap)
            self.lru.set(("b", off1), hit)
        return hit

    def _check_planned(self, sgs):
        if self._plan is not None and any((int(sg.off0), int(sg.off1)) not in self._plan_set for sg in sgs):
            raise ValueError("subgrid was not in the subgrid_configs plan")

    def _wave_b_staged(self, sgs):
        """:py:meth:`_wave_b` with K2 always per wave (never per slab) and without the prefetch: what the stage timers of
        ``get_wave`` bracket"""
        Q, rowmap = self._get_wave_columns(sgs[0].off1)
        self._check_planned(sgs)
        return _finish_window(self.core, [(Q, rowmap, Q.shape[1], 0, self.core.xM_yN_size)], self.facet_configs, sgs,
                              placed=self._placed())

    # -- K2 once per column slab of the padded axis instead of once per wave (slabs.py; DESIGN.md sections 3 and 4) --
    @cached_property
    def _slab_plan(self):
        """what the plan needs of every slab (None: no plan, or sizes / offsets the slab grid does not fit)"""
        core = self.core
        N, yN, m = core.N, core.yN_size, core.xM_yN_size
        if self._plan is None or yN & (yN - 1) or not slabs.supported(N, yN, m, self._planned_keys):
            return None
        return slabs.SlabPlan(N, yN, m, ((sg.off0, sg.off1) for sg in self._plan))

    def _slabs_on(self):
        """does the facet side of this object run K2 per slab?  Only the configuration the benchmark's timed pass runs:
        planned complex64 waves keyed by off1 in the default order, on band buffers of this object's own K1
        (``api._K2_SLABS`` / SWIFTLY_K2_SLABS=0 switches it off); everything else keeps K2 per wave."""
        return bool(
            _knobs()._K2_SLABS and self.wave_axis == 1 and self._plan is not None and self._bands_own
            and self.dtype == _torch().complex64 and self._axis1() == 0 and self._slab_plan is not None
        )

    def _slab_rows(self, j):
        """(rowmap, n_rows) of slab ``j``: the rows the planned subgrids of EVERY planned wave that meets the slab read"""
        if j not in self._slab_rowmaps:
            self._slab_rowmaps[j] = self.core.subgrid_column_rows(self._slab_plan.off0s[j])
        return self._slab_rowmaps[j]

    def _slab_has(self, j):
        """is slab ``j`` cached?  (no effect on the recency order)"""
        return ("q", j) in self._slab_lru._items or j in self._slab_kept  # pylint: disable=protected-access

    def _slab_cached(self, j):
        """cached slab ``j`` as ``(Q, rowmap, n_rows)``, or None"""
        hit = self._slab_lru.get(("q", j))
        if hit is None and j in self._slab_kept:
            hit = self._slab_kept.pop(j)
            self._slab_store(j, hit, fresh=False)
        return hit

    def _slab_store(self, j, hit, fresh=True):
        """Slab ``j`` enters the cache.  The slab this pushes out is kept aside while a planned wave that reads it has not
        been served from it yet -- as many such slabs as the cache holds, the oldest dropped first: a walk along the axis
        then computes every slab once although its first and last wave share one; any other order only recomputes."""
        if fresh:
            self._slab_served[j] = set()
        key, old = self._slab_lru.set(("q", j), hit)
        if key is not None and set(self._slab_plan.users[key[1]]) - self._slab_served.get(key[1], set()):
            kept = self._slab_kept
            kept[key[1]] = old
            while len(kept) > self._slab_lru.cache_size:
                kept.pop(next(iter(kept)))

    def _compute_slab(self, j, Q, rowmap):
        """K2 of the planned positions of slab ``j`` into ``Q`` on the current stream; returns the number of native calls"""
        plan = self._slab_plan
        off0s = [cfg.off0 for cfg in self.facet_configs]
        for first, count in plan.ranges[j]:
            self.core.prepare_facet_columns_range(self.BF_Fs_persist, off0s, self._band, plan.off1(j), first, count, Q, rowmap)
        return len(plan.ranges[j])

    def _slab_pieces(self, sgs):
        """K2 per slab: the window of the wave as the pieces of ``core.transform_contributions_pieces``.  The wave's one or
        two slabs are taken from the cache or the prefetch (a missing one is computed on the current stream), the slabs of
        the next predicted waves go to the side stream."""
        core, off1 = self.core, sgs[0].off1
        if int(off1) not in self._planned_keys:
            raise ValueError(f"subgrid wave off1={off1} was not in the subgrid_configs plan")
        torch = _torch()
        wanted = self._slab_plan.pieces(off1)
        self._check_slab_prediction([j for j, _, _ in wanted])
        nxt = self._predict_next_waves(off1, _knobs()._PREFETCH_DEPTH)
        pieces = []
        for j, first, count in wanted:
            hit = self._slab_hit(j)
            if hit is None:
                rowmap, n_rows = self._slab_rows(j)
                Q = torch.empty((len(self.facet_configs), n_rows, core.xM_yN_size), dtype=self.dtype, device=core.device)
                self._compute_slab(j, Q, rowmap)
                hit = (Q, rowmap, n_rows)
                self._slab_store(j, hit)
            self._slab_served.setdefault(j, set()).add(int(off1))
            pieces.append((*hit, first, count))
        self._prefetch_slabs_of(nxt)  # (behind this wave's own K2, if it had to run, and before its K3)
        return pieces

    def _wave_pieces(self, sgs):
        """K2 of one wave without K3 -- the one place a wave's window comes from: the pieces of
        ``core.transform_contributions_pieces`` / ``core.wave_group_finish_pieces`` (the two slabs, or the wave's own ``Q``).
        K2 of the next waves of the announced order (set_wave_order; the plan's own order otherwise) goes to the side stream
        behind this wave's K2 and before its K3 (_prefetch_wave), for every caller (r6: the multi-GPU pass used to compute
        every K2 on the caller's stream, 41.4 against 35.5 ms at world 1)."""
        off1 = sgs[0].off1
        self.prepare_all_facets()
        if self._slabs_on():
            return self._slab_pieces(sgs)
        Q, rowmap = self._get_wave_columns(off1)
        self._prefetch_waves(self._predict_next_waves(off1, _knobs()._PREFETCH_DEPTH))
        return [(Q, rowmap, Q.shape[1], 0, self.core.xM_yN_size)]

    def _facet_side(self, sgs, g_out=None, g_layout=None):
        """Facet side of one wave: K2 (:py:meth:`_wave_pieces`), then K3 + K4a from its pieces into the blocks
        ``G[F, S, m, m]`` (returned), or placed by ``g_layout`` inside the flat buffer ``g_out`` (wave_blocks_into)."""
        core = self.core
        pieces = self._wave_pieces(sgs)
        if g_out is None:
            m = core.xM_yN_size
            g_out = _torch().empty((len(self.facet_configs), len(sgs), m, m), dtype=self.dtype, device=core.device)
        return core.transform_contributions_pieces(pieces, [cfg.off0 for cfg in self.facet_configs], [sg.off0 for sg in sgs],
                                                   g_out, g_layout=g_layout)

    def _wave_b(self, sgs):
        """One wave: K2 (:py:meth:`_wave_pieces`), then the subgrid side from its pieces (:py:func:`_finish_window`)."""
        self._check_planned(sgs)
        return _finish_window(self.core, self._wave_pieces(sgs), self.facet_configs, sgs, placed=self._placed())


class _PromotingForward(SwiftlyForward):
    """``SwiftlyForward`` as the multi-GPU classes own it without ``facet_dtype=torch.float32``: float32 facets are always
    promoted to complex64"""

    _keep_real_facets = False


def axis1_first_active(core, wave_axis, dtype):
    """does a forward object of this core, wave axis and dtype send blocks finished along axis 1 (axis-1-first pipeline,
    either form)?  One rule (``k1_form.axis1_active``) for the senders and for whoever finishes their blocks (``placed``)."""
    return axis1_active(wave_axis, getattr(core, "axis1_first", False), dtype == _torch().complex64)


def _finish_from_columns(core, src, layout, facet_configs, sgs, window_offs, rowmap=None, band=None, placed=False):
    """K3..K5 without any HBM accumulator: per-(facet, subgrid) axis-0 transforms gathered straight from the
    wave's facet buffers (``src``), facet sum + axis-1 finish on chip, axis-0 finish."""
    if layout == 1:  # the row-window layout: ``src`` is the wave's whole window, served as every wave of the band pipeline is
        return _finish_window(core, [(src, rowmap, src.shape[1], 0, core.xM_yN_size)], facet_configs, sgs, placed=placed)
    if src.dtype != _torch().complex64:  # (the column-buffer layout 0 stays complex64)
        raise NotImplementedError("fused subgrid path is complex64 only")
    G = core.transform_contributions(src, layout, [cfg.off0 for cfg in facet_configs], window_offs, rowmap=rowmap, band=band)
    return _finish_from_G(core, G, facet_configs, sgs, placed=placed)


def group_finish_active(core, dtype, n_facets, placed=False):
    """Does a path that owns both K3 and the finish of a wave run the grouped subgrid side?  Asked by :py:func:`_finish_window`
    alone, through which all of them go (``SwiftlyForward._wave_b``, its staged twin, ``_finish_from_columns`` on the
    row-window layout), so that their results stay bit-identical to each other: complex64 blocks of the default order, an
    instance for the sizes (``core.supports_group_finish``), and the process-wide switch (``swiftly_hip_group_finish``,
    SWIFTLY_GROUP_FINISH=0) on.  Paths that hand ``G[F, S, m, m]`` to someone else (wave_blocks, finish_from_blocks, the
    multi-GPU classes) keep K3 + wave_subgrid_side."""
    if placed or dtype != _torch().complex64 or not _lib.load().swiftly_hip_group_finish(-1):
        return False
    return core.supports_group_finish(dtype, n_facets)


def _finish_window(core, pieces, facet_configs, sgs, placed=False):
    """Finished, masked subgrids ``[S, xA, xA]`` of one wave from the pieces of its K2 window (``SwiftlyForward._wave_pieces``).
    Where the grouped subgrid side exists (:py:func:`group_finish_active`): group_finish + sum_finish_facets from the pieces
    -- the strided axis finished first per facet off1 group, 49 instead of 79 MB per subgrid.  Else K3 + K4a into
    ``G[F, S, m, m]`` and the subgrid side K4b + K5 (:py:func:`_finish_from_G`)."""
    dt = pieces[0][0].dtype
    if group_finish_active(core, dt, len(facet_configs), placed):
        return _finish_from_pieces(core, pieces, facet_configs, sgs)
    m = core.xM_yN_size
    G = _torch().empty((len(facet_configs), len(sgs), m, m), dtype=dt, device=core.device)
    core.transform_contributions_pieces(pieces, [cfg.off0 for cfg in facet_configs], [sg.off0 for sg in sgs], G)
    return _finish_from_G(core, G, facet_configs, sgs, placed=placed)


def _finish_from_pieces(core, pieces, facet_configs, sgs):
    """group_finish + sum_finish_facets of one wave from the pieces of its K2 window (``core.wave_group_finish_pieces``)"""
    torch = _torch()
    xA, S = sgs[0].size, len(sgs)
    dt = pieces[0][0].dtype
    mask1 = _mask_table(core, sgs, "mask1", xA, dt)
    mask0 = _mask_table(core, sgs, "mask0", xA, dt)
    res = torch.empty((S, xA, xA), dtype=dt, device=core.device)
    return core.wave_group_finish_pieces(pieces, [cfg.off0 for cfg in facet_configs], [cfg.off1 for cfg in facet_configs],
                                         [sg.off0 for sg in sgs], [sg.off1 for sg in sgs], xA, mask0, mask1, res)


def _finish_from_G(core, G, facet_configs, sgs, placed=False):
    """facet sum + axis-1 finish on chip (sum_finish_facets), then the axis-0 finish, for ``G[F, S, m, m]``.  ``placed``:
    blocks of the axis-1-first pipeline (their contiguous axis is already finished up to the placement)."""
    torch = _torch()
    xM, xA, S = core.xM_size, sgs[0].size, len(sgs)
    dt, dev = G.dtype, core.device
    off0s = [cfg.off0 for cfg in facet_configs]
    off1s = [cfg.off1 for cfg in facet_configs]
    mask1 = _mask_table(core, sgs, "mask1", xA, dt)
    mask0 = _mask_table(core, sgs, "mask0", xA, dt)
    tmp = torch.empty((S, xM, xA), dtype=dt, device=dev)
    res = torch.empty((S, xA, xA), dtype=dt, device=dev)
    return core.wave_subgrid_side(G, off0s, off1s, [sg.off0 for sg in sgs], [sg.off1 for sg in sgs], xA, mask0, mask1,
                                  tmp, res, placed=placed)


def finish_from_blocks(core, blocks, facet_configs, sgs, transformed=True, placed=False):
    """Finished, masked subgrids ``[S, xA, xA]`` from the per-(facet, subgrid) blocks ``[F, S, m, m]`` of ALL
    facets (``facet_configs`` in the blocks' facet order): the receiving side of the multi-GPU exchange.
    ``transformed`` as in :py:meth:`SwiftlyForward.wave_blocks`; ``placed``: the senders ran the axis-1-first pipeline."""
    if transformed:
        return _finish_from_G(core, blocks, facet_configs, sgs, placed=placed)
    return sum_and_finish_wave(core, blocks, facet_configs, sgs)


def _facet_grid(facet_configs):
    """(off0 values, off1 values) when the facets form an off0 x off1 grid in row-major order
    (make_full_facet_cover), else None."""
    off0s = sorted({cfg.off0 for cfg in facet_configs})
    off1s = sorted({cfg.off1 for cfg in facet_configs})
    if [(cfg.off0, cfg.off1) for cfg in facet_configs] == [(a, b) for a in off0s for b in off1s]:
        return off0s, off1s
    return None


def _colacc_from_columns(core, cols, facet_configs, sgs):
    """K3+K4a fused: per-off1-group axis-0 sums ``colacc[G, S, xM, m]`` straight from the column
    buffers ``cols[F, m, yN]``."""
    torch = _torch()
    grid = _facet_grid(facet_configs)
    if grid is None:
        raise NotImplementedError("fused path needs an off0 x off1 facet grid")
    off0s, groups = grid
    m, xM, S, G = core.xM_yN_size, core.xM_size, len(sgs), len(groups)
    colacc = torch.zeros((G, S, xM, m), dtype=cols.dtype, device=core.device)
    off1s = [sg.off1 for sg in sgs]
    for i, off0_f in enumerate(off0s):
        core.add_to_subgrid_from_columns(cols[i * G : (i + 1) * G], off0_f, colacc, off1s)
    return colacc


def sum_and_finish_wave(core, contrib, facet_configs, sgs):
    """``sum_and_finish_subgrid`` (reference api_helper.py:73-112) for a wave of
    subgrids that share ``off0`` and ``size``: ``contrib[F, S, m, m]`` (facet
    order = ``facet_configs``) -> finished, masked subgrids ``[S, xA, xA]``."""
    torch = _torch()
    m, xM = core.xM_yN_size, core.xM_size
    S = len(sgs)
    dev, dt = core.device, contrib.dtype
    groups = sorted({cfg.off1 for cfg in facet_configs})  # facets grouped by off1 (api_helper.py:83)
    # K4a: axis-0 transform + placement, summed over the facets of one off1 group
    colacc = torch.zeros((len(groups), S, xM, m), dtype=dt, device=dev)
    grid = _facet_grid(facet_configs)
    if grid is not None and contrib.is_contiguous():
        # facets with the same off0 belong to different groups, so ONE launch per off0 handles all
        # (group, subgrid) pairs -- batch item z = g*S + b reads contrib[i*G + g, b], adds into colacc[g, b]
        G = len(groups)
        for i, off0_f in enumerate(grid[0]):
            core.launch("add_to_subgrid", contrib[i * G], m, 1, m, colacc, 1, m, off0_f,
                        nbatch=G * S, in_bs=m * m, out_bs=xM * m)
    else:
        for j, cfg in enumerate(facet_configs):
            core.launch("add_to_subgrid", contrib[j], m, 1, m, colacc[groups.index(cfg.off1)], 1, m, cfg.off0,
                        nbatch=S, in_bs=m * m, out_bs=xM * m)
    return _finish_from_colacc(core, colacc, facet_configs, sgs)


def _finish_from_colacc(core, colacc, facet_configs, sgs):
    """axis-1 sum over groups + finish (fused where available), then finish along axis 0."""
    torch = _torch()
    m, xM = core.xM_yN_size, core.xM_size
    off0, xA, S = sgs[0].off0, sgs[0].size, len(sgs)
    dev, dt = core.device, colacc.dtype
    groups = sorted({cfg.off1 for cfg in facet_configs})
    off1s = [sg.off1 for sg in sgs]
    mask1 = _mask_table(core, sgs, "mask1", xA, dt)
    mask0 = _mask_table(core, sgs, "mask0", xA, dt)
    tmp = torch.empty((S, xM, xA), dtype=dt, device=dev)
    try:
        core.sum_finish_rows(colacc, groups, tmp, off1s, xA, mask=mask1)
    except NotImplementedError:
        acc = torch.zeros((S, xM, xM), dtype=dt, device=dev)
        for g, off1 in enumerate(groups):
            core.launch("add_to_subgrid", colacc[g], xM, m, 1, acc, xM, 1, off1,
                        nbatch=S, in_bs=xM * m, out_bs=xM * xM)
        core.launch("finish_subgrid", acc, xM, xM, 1, tmp, xA, 1, 0, size=xA, mask=mask1,
                    nbatch=S, in_bs=xM * xM, out_bs=xM * xA, offs=off1s, mask_bs=xA if mask1 is not None else 0)
    res = torch.empty((S, xA, xA), dtype=dt, device=dev)
    core.launch("finish_subgrid", tmp, xA, 1, xA, res, 1, xA, off0, size=xA, mask=mask0,
                nbatch=S, in_bs=xM * xA, out_bs=xA * xA, mask_bs=xA if mask0 is not None else 0)
    return res
