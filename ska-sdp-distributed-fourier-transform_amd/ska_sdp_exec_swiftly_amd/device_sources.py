"""
Point-source truths and RMSE checks on the device.

The reference checks itself with point sources: ``make_facet`` builds the
inputs, ``check_subgrid`` compares every subgrid with the direct Fourier sum of
the sources and ``check_facet`` every finished facet with the scattered
sources (reference api_helper.py:15-70, fourier_algorithm.py:218-315).  The
numpy versions in ``api_helper`` pull every array to the host and spend
``S * size**2`` complex exponentials per subgrid there; ``DeviceSources`` does
the same work with native kernels (csrc/swiftly_sources.h) on arrays that stay
on the device.

The device truth is also the more accurate one: ``exp(2 pi i c u / N)`` in
double carries a phase error that grows with ``c * u / N``; the kernels reduce
``(c * u) mod N`` exactly in 64-bit integers before the angle is formed.
"""
import ctypes

import numpy

from . import _lib

__all__ = ["DeviceSources", "source_table", "SOURCE_DTYPE", "MAX_IMAGE_SIZE"]

# one record of the device table (csrc/swiftly_sources.h, SourceRec): complex intensity, integer image coordinates
SOURCE_DTYPE = numpy.dtype([("re", "<f8"), ("im", "<f8"), ("c0", "<i4"), ("c1", "<i4")])
MAX_IMAGE_SIZE = 1 << 31


def _torch():
    import torch  # pylint: disable=import-outside-toplevel

    return torch


def source_table(sources, image_size):
    """The normalised source table of ``sources = [(intensity, c0, c1), ...]`` as a numpy record array of
    ``SOURCE_DTYPE``: coordinates reduced modulo ``image_size`` into ``[-image_size // 2, image_size // 2)``, sources
    that land on one pixel merged by adding their intensities (in the order given).  ``ValueError`` for a coordinate
    that is not an integer (a facet cannot hold such a source) and for a source that is not two-dimensional."""
    N = int(image_size)
    if N <= 0 or N > MAX_IMAGE_SIZE:
        raise ValueError(f"image size {image_size} must be in [1, 2^31]")
    merged = {}
    for source in sources:
        intensity, *coord = source
        if len(coord) != 2:
            raise ValueError(f"source {source!r} has {len(coord)} coordinate(s), expected 2")
        pixel = []
        for c in coord:
            if isinstance(c, (bool, numpy.bool_)) or c != int(c):
                raise ValueError(f"source coordinate {c!r} is not an integer")
            pixel.append((int(c) + N // 2) % N - N // 2)
        key = tuple(pixel)
        merged[key] = merged.get(key, 0) + complex(intensity)
    table = numpy.zeros(len(merged), dtype=SOURCE_DTYPE)
    for k, ((c0, c1), intensity) in enumerate(merged.items()):
        table[k] = (intensity.real, intensity.imag, c0, c1)
    return table


def facet_row_lists(table, image_size, size, off0, off1):
    """Per-row source lists of one facet (CSR): ``row_start`` (int32, ``size + 1``) and ``row_sources`` (int32): the
    sources of facet row ``r`` are ``row_sources[row_start[r]:row_start[r + 1]]``, ascending in their column.  The
    pixel follows the reference: ``(c - (off - size // 2)) mod image_size < size`` on both axes
    (fourier_algorithm.py:253-256)."""
    p0 = (table["c0"].astype(numpy.int64) - (int(off0) - size // 2)) % image_size
    p1 = (table["c1"].astype(numpy.int64) - (int(off1) - size // 2)) % image_size
    inside = numpy.flatnonzero((p0 < size) & (p1 < size))
    order = inside[numpy.lexsort((p1[inside], p0[inside]))]
    row_start = numpy.zeros(size + 1, dtype=numpy.int32)
    row_start[1:] = numpy.cumsum(numpy.bincount(p0[order], minlength=size))
    return row_start, order.astype(numpy.int32)


class DeviceSources:
    """Point sources ``[(intensity, c0, c1), ...]`` (real or complex intensity, integer coordinates relative to the
    image centre) of an ``image_size`` x ``image_size`` image, held on ``device`` for truths and checks."""

    def __init__(self, sources, image_size, device=None):
        torch = _torch()
        self.image_size = int(image_size)
        self.table = source_table(sources, image_size)
        self._lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("DeviceSources needs a HIP device: there is no CPU fallback (api_helper has the numpy forms)")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        raw = numpy.ascontiguousarray(self.table).view(numpy.uint8)
        self._table_dev = torch.from_numpy(raw.copy()).to(self.device)
        self._mask_cache = {}
        self._row_cache = {}

    def __len__(self):
        return len(self.table)

    # ------------------------------------------------------------------ marshalling
    @staticmethod
    def _cdtype(dtype, real_ok=False):
        """``dtype`` (torch or numpy) as a torch dtype: complex64 / complex128; ``real_ok``: float32 / float64 too"""
        torch = _torch()
        names = ("complex64", "complex128", "float32", "float64") if real_ok else ("complex64", "complex128")
        if not isinstance(dtype, torch.dtype):
            try:
                dtype = getattr(torch, numpy.dtype(dtype).name, None)
            except TypeError:
                dtype = None
        if dtype in [getattr(torch, name) for name in names]:
            return dtype
        raise ValueError(f"dtype must be {' or '.join(names[:2])}{', float32 or float64' if real_ok else ''}, not {dtype!r}")

    @staticmethod
    def _code(dtype):
        """the library's precision code: C64 for complex64 and float32 data, C128 for complex128 and float64"""
        torch = _torch()
        return _lib.C64 if dtype in (torch.complex64, torch.float32) else _lib.C128

    def _stream(self):
        return ctypes.c_void_p(int(_torch().cuda.current_stream(self.device).cuda_stream))

    def _masks(self, configs, axis, size):
        """device double [n][size] of the configs' masks along ``axis`` (``None`` = ones), or None when all are None"""
        masks = [c.mask1 if axis else c.mask0 for c in configs]
        if all(m is None for m in masks):
            return None
        host = numpy.ones((len(masks), size))
        for k, m in enumerate(masks):
            if m is None:
                continue
            m = numpy.asarray(m.detach().cpu() if hasattr(m, "detach") else m, dtype=float)
            if m.shape != (size,):
                raise ValueError(f"Mask has shape {m.shape}, expected ({size},)!")
            host[k] = m
        key = host.tobytes()
        hit = self._mask_cache.get(key)
        if hit is None:
            if len(self._mask_cache) >= 64:
                self._mask_cache.pop(next(iter(self._mask_cache)))
            hit = self._mask_cache[key] = _torch().from_numpy(host).to(self.device)
        return hit

    def _approx(self, approx, ndim, real_ok=False):
        """``approx`` as a complex device tensor with unit stride along the last axis: no copy for a contiguous or
        row-strided device tensor; a host array is uploaded.  ``real_ok``: float32 / float64 pass as they are."""
        torch = _torch()
        if isinstance(approx, (list, tuple)):
            approx = torch.stack([self._approx(a, ndim - 1) for a in approx])
        if not isinstance(approx, torch.Tensor):
            approx = numpy.asarray(approx)
            if real_ok and approx.dtype in (numpy.float32, numpy.float64):
                pass
            elif not numpy.iscomplexobj(approx):
                raise ValueError(f"approx must be complex, not {approx.dtype}")
            elif approx.dtype not in (numpy.complex64, numpy.complex128):
                approx = approx.astype(numpy.complex128)
            approx = torch.from_numpy(numpy.ascontiguousarray(approx)).to(self.device)
        if real_ok and approx.dtype in (torch.float32, torch.float64):
            pass
        elif approx.dtype not in (torch.complex64, torch.complex128):
            raise ValueError(f"approx must be complex64 or complex128, not {approx.dtype}")
        if approx.device != self.device:
            approx = approx.to(self.device)
        if approx.dim() != ndim or approx.shape[-1] != approx.shape[-2]:
            raise ValueError(f"approx has shape {tuple(approx.shape)}, expected {ndim} dimensions with square chunks")
        if approx.is_conj():
            approx = approx.resolve_conj()
        if approx.stride(-1) != 1 or approx.stride(-2) < approx.shape[-1] or (ndim == 3 and approx.stride(0) < 0):
            approx = approx.contiguous()
        return approx

    def _out(self, out, shape, dtype, real_ok=False):
        torch = _torch()
        dtype = self._cdtype(dtype if out is None else out.dtype, real_ok)
        if out is None:
            return torch.empty(shape, dtype=dtype, device=self.device)
        if tuple(out.shape) != tuple(shape) or out.device != self.device:
            raise ValueError(f"out has shape {tuple(out.shape)} on {out.device}, expected {tuple(shape)} on {self.device}")
        if out.stride(-1) != 1 or out.stride(-2) < shape[-1]:
            raise ValueError("out must have unit stride along its last axis and non-overlapping rows")
        return out

    @staticmethod
    def _offsets(configs):
        n = len(configs)
        return (ctypes.c_int64 * n)(*[int(c.off0) for c in configs]), (ctypes.c_int64 * n)(*[int(c.off1) for c in configs])

    @staticmethod
    def _ptr(tensor):
        return ctypes.c_void_p(tensor.data_ptr()) if tensor is not None else None

    # ------------------------------------------------------------------ subgrids
    def subgrids(self, sg_configs, dtype=None, out=None):
        """``[n, size, size]``: the direct Fourier sums of the sources on ``sg_configs`` (all of one size, masks
        applied), one launch (reference ``make_subgrid``, api_helper.py:15-24)."""
        torch = _torch()
        sg_configs = list(sg_configs)
        sizes = {int(c.size) for c in sg_configs}
        if len(sizes) > 1:
            raise ValueError(f"subgrids of one batch must share one size, got {sorted(sizes)}")
        size = sizes.pop() if sizes else 0
        n = len(sg_configs)
        out = self._out(out, (n, size, size), torch.complex128 if dtype is None else dtype)
        if n == 0:
            return out
        off0s, off1s = self._offsets(sg_configs)
        m0, m1 = self._masks(sg_configs, 0, size), self._masks(sg_configs, 1, size)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.swiftly_hip_subgrids_from_sources(
                self._code(out.dtype), self._ptr(self._table_dev), len(self.table), self.image_size, size, off0s, off1s, n,
                self._ptr(m0), self._ptr(m1), self._ptr(out), out.stride(0), out.stride(1), self._stream(),
            ))
        return out

    def subgrid(self, sg_config, dtype=None, out=None):
        """``[size, size]``: ``subgrids`` for one subgrid"""
        return self.subgrids([sg_config], dtype, None if out is None else out[None])[0]

    def check_subgrids(self, sg_configs, approx):
        """float64 device tensor ``[n, 2]``: per subgrid the RMSE between ``approx[k]`` and the direct Fourier sum, and the
        RMS of that truth.  ``approx``: ``[n, size, size]`` complex (device tensor of either complex dtype, contiguous
        or strided between rows and subgrids: read in place; a host array or a list of chunks is gathered first).  The
        subgrid size is ``approx.shape[-1]``, as in the reference's ``check_subgrid`` (api_helper.py:58-70); the truth
        is never stored."""
        torch = _torch()
        sg_configs = list(sg_configs)
        approx = self._approx(approx, 3)
        n, size = len(sg_configs), int(approx.shape[-1])
        if approx.shape[0] != n:
            raise ValueError(f"{n} subgrid configurations for {approx.shape[0]} subgrids")
        result = torch.zeros((n, 2), dtype=torch.float64, device=self.device)
        if n == 0 or size == 0:
            return result
        off0s, off1s = self._offsets(sg_configs)
        m0, m1 = self._masks(sg_configs, 0, size), self._masks(sg_configs, 1, size)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.swiftly_hip_check_subgrids_from_sources(
                self._code(approx.dtype), self._ptr(self._table_dev), len(self.table), self.image_size, size, off0s, off1s,
                n, self._ptr(m0), self._ptr(m1), self._ptr(approx), approx.stride(0), approx.stride(1),
                self._ptr(result), self._stream(),
            ))
        return torch.sqrt(result) / size  # sqrt(sum / size^2)

    def check_subgrid(self, sg_config, approx):
        """RMSE between a computed subgrid and the direct Fourier sum, as ``api_helper.check_subgrid``"""
        approx = self._approx(approx, 2)
        return float(self.check_subgrids([sg_config], approx[None])[0, 0])

    # ------------------------------------------------------------------ facets
    def _facet_call(self, facet_config, size):
        m0, m1 = self._masks([facet_config], 0, size), self._masks([facet_config], 1, size)
        return [self._ptr(self._table_dev), len(self.table), self.image_size, size, int(facet_config.off0),
                int(facet_config.off1), self._ptr(m0), self._ptr(m1)]

    def facet(self, facet_config, dtype=None, out=None):
        """``[size, size]``: the facet holding the sources (reference ``make_facet``, api_helper.py:27-36).  ``dtype`` (or
        ``out``) float32 / float64: the facet of a real-valued image as reals, bit for bit the real part of the complex
        one (``swiftly_hip_facet_from_sources_real``) -- ``ValueError``, and nothing written, when an intensity has a
        non-zero imaginary part."""
        torch = _torch()
        size = int(facet_config.size)
        out = self._out(out, (size, size), torch.complex128 if dtype is None else dtype, real_ok=True)
        entry = self._lib.swiftly_hip_facet_from_sources
        if not out.dtype.is_complex:
            if numpy.any(self.table["im"] != 0):
                raise ValueError(f"a {out.dtype} facet needs real intensities: a source has a non-zero imaginary part")
            entry = self._lib.swiftly_hip_facet_from_sources_real
        with torch.cuda.device(self.device):
            _lib.check(entry(
                self._code(out.dtype), *self._facet_call(facet_config, size), self._ptr(out), out.stride(0), self._stream(),
            ))
        return out

    def _facet_rows(self, facet_config, size):
        """device ``(row_start, row_sources)`` of ``facet_row_lists`` for a facet of ``size`` pixels at these offsets (cached)"""
        torch = _torch()
        key = (size, int(facet_config.off0), int(facet_config.off1))
        rows = self._row_cache.get(key)
        if rows is None:
            if len(self._row_cache) >= 256:
                self._row_cache.pop(next(iter(self._row_cache)))
            start, srcs = facet_row_lists(self.table, self.image_size, size, key[1], key[2])
            srcs = numpy.concatenate([srcs, numpy.zeros(1, dtype=numpy.int32)])  # never an empty allocation
            rows = self._row_cache[key] = (torch.from_numpy(start).to(self.device), torch.from_numpy(srcs).to(self.device))
        return rows

    def _check_facet_into(self, facet_config, approx, result):
        """enqueue the sums of one facet check into the two doubles ``result`` (complex or real ``approx``)"""
        size = int(approx.shape[-1])
        rows = self._facet_rows(facet_config, size)
        entry = (self._lib.swiftly_hip_check_facet_from_sources if approx.dtype.is_complex
                 else self._lib.swiftly_hip_check_facet_from_sources_real)
        with _torch().cuda.device(self.device):
            _lib.check(entry(
                self._code(approx.dtype), *self._facet_call(facet_config, size), self._ptr(approx), approx.stride(0),
                self._ptr(rows[0]), self._ptr(rows[1]), self._ptr(result), self._stream(),
            ))

    def check_facet(self, facet_config, approx):
        """RMSE between a computed facet and the one generated from the sources, as ``api_helper.check_facet``: every
        pixel is differenced on its own (no cancellation between the facet's power and the sources')."""
        torch = _torch()
        approx = self._approx(approx, 2)
        result = torch.zeros(2, dtype=torch.float64, device=self.device)
        self._check_facet_into(facet_config, approx, result)
        return float(torch.sqrt(result[0]) / int(approx.shape[-1]))

    def check_facets(self, facet_configs, approx):
        """float64 device tensor ``[n, 2]``: per facet the RMSE between ``approx[k]`` and the facet generated from the
        sources, and the RMS of that truth -- the facet counterpart of :py:meth:`check_subgrids`, without a host
        synchronisation per facet.  ``approx``: one ``[size, size]`` tensor per facet, complex64 / complex128 or, for a
        real-valued image, float32 / float64 (the truth's imaginary part then counts as zero;
        ``swiftly_hip_check_facet_from_sources_real``); device tensors with unit stride along their rows are read in
        place.  For facets with zero imaginary parts the real form gives the bits of the complex one."""
        torch = _torch()
        facet_configs = list(facet_configs)
        if isinstance(approx, torch.Tensor) or not isinstance(approx, (list, tuple)):
            approx = list(approx)
        if len(approx) != len(facet_configs):
            raise ValueError(f"{len(facet_configs)} facet configurations for {len(approx)} facets")
        for a in approx:  # (a facet is large: never gathered into a contiguous copy behind the caller's back)
            if isinstance(a, torch.Tensor) and a.dim() == 2 and (a.stride(1) != 1 or a.stride(0) < a.shape[1]):
                raise ValueError("check_facets reads facets in place: unit stride along the rows, rows that do not overlap")
        approx = [self._approx(a, 2, real_ok=True) for a in approx]
        result = torch.zeros((len(approx), 2), dtype=torch.float64, device=self.device)
        for k, (cfg, a) in enumerate(zip(facet_configs, approx)):
            if a.shape[-1]:
                self._check_facet_into(cfg, a, result[k])
        sizes = [max(int(a.shape[-1]), 1) for a in approx]
        if len(set(sizes)) <= 1:
            return torch.sqrt(result) / (sizes[0] if sizes else 1)  # sqrt(sum / size^2)
        return torch.sqrt(result) / torch.tensor(sizes, dtype=torch.float64, device=self.device)[:, None]
