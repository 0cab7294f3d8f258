"""
Host -> device edges of the streaming classes: cached device tables of the config masks and the pinned staging ring that
uploads host facets one ahead of the kernels that use them.
"""
import numpy

from .facet_dtype import is_float32_facet, is_float64_facet
from .tasks import _torch

_MASK_CACHE = {}
_MASK_CACHE_MAX = 4096


def _mask_cache_put(key, value):
    if len(_MASK_CACHE) >= _MASK_CACHE_MAX:
        _MASK_CACHE.pop(next(iter(_MASK_CACHE)))
    _MASK_CACHE[key] = value


def _mask_table(core, configs, which, size, cdtype):
    """[len(configs), size] real device table of the masks (ones where a config
    has no mask), or None when no config has one.  Tables are cached per
    (device, precision, mask contents): an upload from pageable host memory is
    ordered behind everything already queued on the stream, i.e. it would stall
    the host once per wave."""
    torch = _torch()
    # fast path: the same config objects as last time (waves are re-requested every pass); the cache entry
    # keeps the configs alive, so their ids cannot be recycled while it exists
    idkey = (str(core.device), str(cdtype), which, size, tuple(id(c) for c in configs))
    hit = _MASK_CACHE.get(idkey)
    if hit is not None:
        return hit[1]
    masks = [getattr(c, which) for c in configs]
    if all(m is None for m in masks):
        _mask_cache_put(idkey, (tuple(configs), None))
        return None
    tab = numpy.ones((len(configs), size))
    for i, m in enumerate(masks):
        if m is not None:
            tab[i] = numpy.asarray(m, dtype=float)
    key = (str(core.device), str(cdtype), tab.shape, tab.tobytes())
    hit = _MASK_CACHE.get(key)
    if hit is None:
        rdtype = torch.float32 if cdtype == torch.complex64 else torch.float64
        hit = (None, torch.from_numpy(tab).to(device=core.device, dtype=rdtype).contiguous())
        _mask_cache_put(key, hit)
    _mask_cache_put(idkey, (tuple(configs), hit[1]))
    return hit[1]


class _FacetIngest:
    """Host -> device facet upload overlapped with compute.

    Device tensors are used in place.  Host (numpy) facets are uploaded LAZILY on a separate HIP stream in slabs of
    ``SLAB`` bytes through two pinned staging buffers (pageable memory cannot be copied asynchronously, and pinning
    a whole 4 GB facet would cost more than the copy): ``ready(j)`` makes the CURRENT stream wait for facet ``j``
    (a stream-side wait) and returns the tensor; ``prefetch(j)`` starts the upload of facet ``j`` -- the streaming
    classes call it for facet j+1 right after queueing the full-facet transform of facet j, so the transfer runs
    under that kernel.

    Real-valued facets: a float32 facet (host array or device tensor) is registered as it is and reported with the complex
    dtype it computes in; ``settle(keep_real)`` -- called by the owner once all facets are registered, before the first upload
    -- either keeps all of them float32 (the owner's K1 loads reals: half the resident bytes and half the upload) or promotes
    them to complex64 the way every other real input is.  ``float64=True`` (an owner whose caller asked for float64 facets):
    the same for float64 facets, which compute in complex128 -- kept float64 or promoted to complex128; without it a float64
    facet is promoted when it is registered, as ever."""

    SLAB = 128 << 20

    def __init__(self, core, float64=False):
        self.core = core
        self.host, self.tensors, self.events = [], [], []
        self._float32 = []    # per facet: registered as float32 (promotion pending until settle)
        self._float64 = []    # per facet: registered as float64 (only an owner that asked: promotion pending until settle)
        self._keep_float64 = bool(float64)
        self._settled = False
        self.real = False     # the facets stay float32 / float64 (settle(True))
        self._stream = None
        self._staging = None
        self._staging_free = None

    def add(self, data):
        """register a facet; returns (dtype, shape, is_row_major)"""
        torch = _torch()
        if self._settled:
            raise RuntimeError("facets must be registered before settle()")
        is_float32 = is_float32_facet(data)
        is_float64 = self._keep_float64 and is_float64_facet(data)
        is_real = is_float32 or is_float64
        if isinstance(data, torch.Tensor):
            # (a float32 tensor K1 could not read in place -- not 2-D row-major -- is promoted at once, as it always was)
            ten = data if is_real else self.core._as_device(data)[0]  # pylint: disable=protected-access
            self.host.append(None)
            self.tensors.append(ten)
        else:
            arr = numpy.asarray(data)
            if is_real:
                pass
            elif not numpy.iscomplexobj(arr):
                arr = arr.astype(numpy.complex128)
            elif arr.dtype not in (numpy.complex64, numpy.complex128):
                arr = arr.astype(numpy.complex128)
            self.host.append(arr if is_real else numpy.ascontiguousarray(arr))
            self.tensors.append(None)
        self.events.append(None)
        self._float32.append(is_float32)
        self._float64.append(is_float64)
        j = len(self.tensors) - 1
        src = self.tensors[j] if self.tensors[j] is not None else self.host[j]
        if is_real:
            tdt = torch.complex64 if is_float32 else torch.complex128  # the dtype it computes in, kept real or not
        else:
            tdt = src.dtype if self.tensors[j] is not None else (
                torch.complex64 if src.dtype == numpy.complex64 else torch.complex128
            )
        row_major = src.stride(-1) == 1 if self.tensors[j] is not None else True
        return tdt, tuple(src.shape), row_major

    @property
    def all_float32(self):
        """every registered facet is float32 (and there is one)"""
        return bool(self._float32) and all(self._float32)

    @property
    def all_float64(self):
        """every registered facet is float64, registered by an owner that asked (and there is one)"""
        return bool(self._float64) and all(self._float64)

    def settle(self, keep_real):
        """Decide what the float32 facets become: with ``keep_real`` (all of them must be float32) they stay float32 -- a
        device tensor in place, a host array staged and uploaded as float32; otherwise each is promoted to complex64 exactly as
        a real input always was.  Float64 facets of an owner that asked: the same, float64 or complex128.  Idempotent; the
        first upload settles with ``False`` when the owner never asked."""
        if self._settled:
            return
        self._settled = True
        self.real = bool(keep_real) and (self.all_float32 or self.all_float64)
        for j, (is_float32, is_float64) in enumerate(zip(self._float32, self._float64)):
            if not (is_float32 or is_float64):
                continue
            if self.tensors[j] is not None:
                ten = self.tensors[j]
                if self.real:
                    self.tensors[j] = ten if ten.device == self.core.device else ten.to(self.core.device)
                else:
                    self.tensors[j] = self.core._as_device(ten)[0]  # pylint: disable=protected-access
            else:
                arr = self.host[j] if self.real else self.host[j].astype(numpy.complex64 if is_float32 else numpy.complex128)
                self.host[j] = numpy.ascontiguousarray(arr)

    def prefetch(self, j):
        """start the upload of facet ``j`` (no-op for device facets / out of range / already started)"""
        torch = _torch()
        self.settle(False)
        if j < 0 or j >= len(self.tensors) or self.tensors[j] is not None:
            return
        core = self.core
        arr = self.host[j]
        tdt = {numpy.dtype(numpy.float32): torch.float32, numpy.dtype(numpy.float64): torch.float64,
               numpy.dtype(numpy.complex64): torch.complex64}.get(arr.dtype, torch.complex128)
        dev = torch.empty(arr.shape, dtype=tdt, device=core.device)
        if self._stream is None:
            self._stream = torch.cuda.Stream(device=core.device)
            self._staging = [torch.empty(self.SLAB, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
            self._staging_free = [None, None]
        src = torch.from_numpy(arr.reshape(-1).view(numpy.uint8))
        dst = dev.reshape(-1).view(torch.uint8)
        nbytes = src.numel()
        # the new tensor's memory may still be in use by work queued on the current stream (caching allocator)
        self._stream.wait_stream(torch.cuda.current_stream(core.device))
        with torch.cuda.stream(self._stream):
            for k, pos in enumerate(range(0, nbytes, self.SLAB)):
                n = min(self.SLAB, nbytes - pos)
                slot = k % 2
                if self._staging_free[slot] is not None:
                    self._staging_free[slot].synchronize()  # staging slot still in flight
                self._staging[slot][:n].copy_(src[pos : pos + n])  # host memcpy into pinned memory
                dst[pos : pos + n].copy_(self._staging[slot][:n], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(self._stream)
                self._staging_free[slot] = ev
            done = torch.cuda.Event()
            done.record(self._stream)
        dev.record_stream(self._stream)
        self.tensors[j] = dev
        self.events[j] = done
        self.host[j] = None

    def ready(self, j):
        """facet ``j`` on the device with the current stream ordered behind its upload"""
        self.prefetch(j)
        ev = self.events[j]
        if ev is not None:
            _torch().cuda.current_stream(self.core.device).wait_event(ev)
            self.events[j] = None
        return self.tensors[j]
