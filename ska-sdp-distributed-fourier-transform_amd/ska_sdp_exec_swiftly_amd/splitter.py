"""
``SubgridSplitter``: ``prepare_and_split_subgrid`` (reference api_helper.py:115-139) for a wave of subgrids -- the subgrid
holder's half of the backward pass, shared by ``SwiftlyBackward`` and ``DistributedBackward``.
"""
from .tasks import _torch


class SubgridSplitter:
    """Contributions of waves of subgrids to the facets ``facet_configs``, in that order, and the workspaces they live in.

    :param dtype: complex dtype of the contributions; data of another dtype is converted.  ``None``: each call's first data's.

    On the fused route the result of :py:meth:`contributions` lives in one of two alternating workspaces of this object:
    it stays valid until the second-next call."""

    def __init__(self, core, facet_configs, dtype=None):
        self.core, self.facet_configs, self.dtype = core, facet_configs, dtype
        self._off0s = sorted({cfg.off0 for cfg in facet_configs})
        self._off0_of = [self._off0s.index(cfg.off0) for cfg in facet_configs]
        self._wsbuf = {}
        self._ring = 0

    def _ws(self, name, shape, dtype):
        """Grow-only persistent workspace (per-wave allocations of changing size are kept away from the caching
        allocator: its misses are synchronous hipMallocs)."""
        torch = _torch()
        n = 1
        for d in shape:
            n *= int(d)
        buf = self._wsbuf.get(name)
        if buf is None or buf.numel() < n or buf.dtype != dtype:
            buf = self._wsbuf[name] = torch.empty((n,), dtype=dtype, device=self.core.device)
        return buf[:n].view(*shape)

    def contributions(self, sgs, subgrids, explicit_band=False, dtype=None):
        """``[F, S, m, m]`` of the subgrids ``sgs`` (same size) with the data ``subgrids``.  ``explicit_band``: the caller is a
        ``SwiftlyBackward`` on the explicitly requested band schedule -- data of another dtype raises ``ValueError`` instead
        of being converted, and complex128 may take the split kernel.  ``dtype``: of this call's contributions (default: the
        one the splitter was built with)."""
        torch = _torch()
        core = self.core
        m, xM = core.xM_yN_size, core.xM_size
        F, S, D = len(self.facet_configs), len(sgs), len(self._off0s)
        xA = sgs[0].size
        dt = dtype if dtype is not None else self.dtype
        subs = []
        for data in subgrids:
            ten, _ = core._as_device(data)  # pylint: disable=protected-access
            if dt is None:
                dt = ten.dtype
            elif ten.dtype != dt:
                if explicit_band:  # no silent conversion on the explicit band schedule
                    raise ValueError(f"SwiftlyBackward(wave_axis=1, dtype={dt}) got {ten.dtype} data")
                ten = ten.to(dt)
            if tuple(ten.shape) != (xA, xA):
                raise ValueError(f"subgrid has shape {tuple(ten.shape)}, expected {(xA, xA)}")
            subs.append(ten)
        dev = core.device
        # complex128 takes the split kernel only on the explicitly requested band schedule: every path that existed before
        # keeps its launch sequence (and its rounding)
        explicit128 = explicit_band and dt == torch.complex128
        if core.supports_fused_subgrid(dt, n_facets=F) or (explicit128 and core.supports_split_prepare(dt, n_facets=F)):
            # prepare_subgrid along axis 0 on the xA columns, then ONE kernel per padded row for the contiguous-axis
            # half (prepare axis 1 + extract axis 1 for every facet, on chip) and one column pass for the rest
            step = xA * xA * subs[0].element_size()
            base = subs[0].untyped_storage().data_ptr()
            if all(
                t.is_contiguous() and t.data_ptr() == subs[0].data_ptr() + i * step
                and t.untyped_storage().data_ptr() == base  # views of ONE allocation, not neighbours by chance
                for i, t in enumerate(subs)
            ):
                # the subgrids already sit back to back (slices of one wave tensor, e.g. what get_wave returned)
                sub = torch.as_strided(subs[0], (S, xA, xA), (xA * xA, xA, 1))
            else:
                sub = self._ws("stack", (S, xA, xA), dt)
                torch.stack(subs, out=sub)
            work = self._ws("work", (2 * S * xM * xA,), dt)
            self._ring ^= 1
            parts = self._ws(f"parts{self._ring}", (F, S, m, m), dt)
            return core.wave_split_subgrids(sub, [sg.off0 for sg in sgs], [sg.off1 for sg in sgs],
                                            [c.off0 for c in self.facet_configs],
                                            [c.off1 for c in self.facet_configs], work, parts)
        sub = subs[0].unsqueeze(0) if S == 1 else torch.stack(subs)
        sub = sub.contiguous()
        # prepare_subgrid (core.py:328-368): axis 1 on the xA rows, then axis 0 on all xM columns
        tmp = torch.empty((S, xA, xM), dtype=dt, device=dev)
        core.launch("prepare_subgrid", sub, xA, xA, 1, tmp, xM, 1, 0, size=xA,
                    nbatch=S, in_bs=xA * xA, out_bs=xA * xM, offs=[sg.off1 for sg in sgs])
        prepared = torch.empty((S, xM, xM), dtype=dt, device=dev)
        core.launch("prepare_subgrid", tmp, xM, 1, xM, prepared, 1, xM, 0, size=xA,
                    nbatch=S, in_bs=xA * xM, out_bs=xM * xM, offs=[sg.off0 for sg in sgs])
        # extract_from_subgrid along axis 0 once per distinct facet off0 (api_helper.py:125-131) ...
        e0 = torch.empty((D, S, m, xM), dtype=dt, device=dev)
        for d, off0_f in enumerate(self._off0s):
            core.launch("extract_from_subgrid", prepared, xM, 1, xM, e0[d], 1, xM, off0_f,
                        nbatch=S, in_bs=xM * xM, out_bs=m * xM)
        # ... and along axis 1 per facet (api_helper.py:133-138)
        parts = torch.empty((F, S, m, m), dtype=dt, device=dev)
        for j, cfg in enumerate(self.facet_configs):
            core.launch("extract_from_subgrid", e0[self._off0_of[j]], m, xM, 1, parts[j], m, 1, cfg.off1,
                        nbatch=S, in_bs=m * xM, out_bs=m * m)
        return parts
