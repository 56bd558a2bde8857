"""The codec-neutral host staging layer under the SLQ and stochastic channels (quant.py, stoch.py).

A channel call packs a state dict's tensors back to back into one flat bucket, moves it to the GPU, runs the
codec's kernels over it and hands the results back as owned per-tensor tensors. What of that does not depend
on the codec is here: the per-process, per-device cache of reused buffers, layouts, streams and events
(``_staging()``, one caller at a time: ``_serialized``); the split of a bucket into staging ranges and each
range's byte-copy list (``_ranges``, ``_range_copies``); the pipeline itself — the native pool gathers range
r + 1 into the pinned bucket while the copy engine moves range r (``_stage_in``), and on the way back every
range is scattered into the outputs as its D2H lands, the outputs being created meanwhile (``_PendingD2H``,
``_hand_out``); K clients' payloads as device rows (``_stage_rows``); and the phase clock (``phase_clock``).

The switches ``_PIPELINE`` (ADFL_HOST_PIPELINE=0: create all outputs, then scatter — the A/B of the pipelined
paths) and ``_PIECE_BYTES`` are read at call time, by both codecs, as attributes of this module.
"""

import ctypes
import os
import threading
import time
from collections import OrderedDict
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from .. import _lib, _torchhost, hostcopy, ops
from .._lib import check

_LAYOUT_CACHE_MAX = 16


class _DeviceStaging:
    """Per-process, per-device reusable buffers (pinned host + device), grown on demand."""

    def __init__(self, device: torch.device):
        self.device = device
        self.cpus = hostcopy.bind_to_device(device)   # the copy pool on the GPU's NUMA node
        self.lock = threading.RLock()
        self._bufs: Dict[str, torch.Tensor] = {}
        self.layouts: "OrderedDict[Tuple[int, ...], ops.BucketLayout]" = OrderedDict()
        self._d2h: Optional[torch.cuda.Stream] = None
        self._h2d: Optional[torch.cuda.Stream] = None
        self._events: List[int] = []

    def d2h_stream(self) -> torch.cuda.Stream:
        """The range-pipelined host paths' copy-back stream: a range's D2H runs here, behind an event on the
        compute stream, so it overlaps the next range's H2D (one stream would serialise them)."""
        if self._d2h is None:
            self._d2h = torch.cuda.Stream(self.device)
        return self._d2h

    def h2d_stream(self) -> torch.cuda.Stream:
        """The stochastic host encode's staging stream: each range's H2D runs here and the compute stream waits
        only for the ranges its kernels read, so the copies run at the link's rate however long the calling
        thread spends on a range's kernels and outputs."""
        if self._h2d is None:
            self._h2d = torch.cuda.Stream(self.device)
        return self._h2d

    def events(self, n: int) -> List[int]:
        """n hipEvent_t handles (timing-free, on this device) for the range-pipelined host paths: a range's
        kernel-done and copied-back events (adfl_stage_*_range). Kept for the staging's life: every call waits
        for all its ranges' scatters before it returns, so the next call may record them again."""
        if len(self._events) < n:
            more = n - len(self._events)
            arr = (ctypes.c_void_p * more)()
            with torch.cuda.device(self.device):
                check(_lib.load().adfl_stage_events_create(more, arr))
            self._events.extend(int(a) for a in arr)
        return self._events

    def buf(self, key: str, numel: int, dtype: torch.dtype, pinned: bool = False) -> torch.Tensor:
        t = self._bufs.get(key)
        if t is None or t.numel() < numel:
            numel = max(numel, 1)
            if pinned:
                with hostcopy.on_cpus(self.cpus):   # pages on the GPU's NUMA node
                    t = torch.empty(numel, dtype=dtype, pin_memory=True)
            else:
                t = torch.empty(numel, dtype=dtype, device=self.device)
            self._bufs[key] = t
        return t[:numel]

    def layout(self, sizes: Tuple[int, ...], align: int = 1) -> ops.BucketLayout:
        """align=1: compact (the host gather is one concatenation); align=2 for packed int4 buckets."""
        key = (sizes, align)
        lay = self.layouts.get(key)
        if lay is None:
            lay = ops.BucketLayout(sizes, align=align)
            self.layouts[key] = lay
            if len(self.layouts) > _LAYOUT_CACHE_MAX:
                self.layouts.popitem(last=False)
        else:
            self.layouts.move_to_end(key)
        return lay


_STAGING: Dict[int, _DeviceStaging] = {}


_STAGING_LOCK = threading.Lock()


def _staging() -> _DeviceStaging:
    idx = torch.cuda.current_device()
    with _STAGING_LOCK:
        st = _STAGING.get(idx)
        if st is None:
            st = _DeviceStaging(torch.device("cuda", idx))
            _STAGING[idx] = st
    return st


def _serialized(fn):
    """Staging buffers are per device and reused: calls from several threads of one actor (ADFL's peer
    clients receive on one thread while training on another, Examples/ray_ad.py) take turns. (Running the
    calling thread on the GPU's NUMA node as well, not only the copy pool, measured no faster:
    profiles/r04/host_channel/caller_*.json.)"""
    def wrapper(*args, **kwargs):
        with _staging().lock:
            return fn(*args, **kwargs)
    wrapper.__name__, wrapper.__doc__ = fn.__name__, fn.__doc__
    return wrapper


def _gather(tensors: List[torch.Tensor], lay: ops.BucketLayout, out: torch.Tensor) -> None:
    """Copy `tensors` (all on out's device) into the 1-D bucket `out` at lay.offsets with ONE torch.cat
    (zero pads between tensors only for an aligned layout; the Channel's compact layout has none)."""
    if lay.align == 1:
        torch.cat([t.reshape(-1) for t in tensors], out=out)
        return
    zeros = torch.zeros(lay.align, dtype=out.dtype, device=out.device)
    pieces = []
    for t, n, padded in zip(tensors, lay.sizes.tolist(), lay.padded.tolist()):
        pieces.append(t.reshape(-1))
        if padded > n:
            pieces.append(zeros[:padded - n])
    torch.cat(pieces, out=out)


_PIECE_BYTES = 4 << 20  # staging pieces of at least this size: one gather + one H2D each
_PIECES = 8             # ... and at most this many per bucket


def _ranges(lay: ops.BucketLayout, elem_bytes: int) -> List[Tuple[int, int]]:
    """The bucket split into element ranges [lo, hi) of about max(_PIECE_BYTES, total / _PIECES) bytes.
    Ranges may cut through a tensor (one 1 GiB tensor still stages in pipelined pieces). Eight pieces: the
    copy engine starts after the first eighth is gathered, and the last eighth's copy is the exposed tail."""
    step = max(_PIECE_BYTES // elem_bytes, -(-lay.total // _PIECES))
    return [(lo, min(lo + step, lay.total)) for lo in range(0, lay.total, step)]


class _RangePlan:
    """For one layout and staging range [lo, hi): which tensor each copy piece belongs to, where it starts in
    that tensor and in the bucket, and its length — everything but the call's pointers, computed once per
    (layout, range) and cached on the layout (the per-call numpy work was ~20 us per range)."""

    __slots__ = ("k", "t_off", "b_off", "n", "ku")

    def __init__(self, lay: ops.BucketLayout, lo: int, hi: int):
        a = np.maximum(lay.offsets, lo)
        b = np.minimum(lay.offsets + lay.sizes, hi)
        k = np.nonzero(a < b)[0]
        self.k = k
        self.ku = k.astype(np.uint64)
        self.t_off = (a[k] - lay.offsets[k]).astype(np.uint64)
        self.b_off = a[k].astype(np.uint64)
        self.n = (b[k] - a[k]).astype(np.int64)

    def copies(self, ptrs: np.ndarray, base: int, es: int, to_bucket: bool):
        t_ptr = ptrs[self.k] + self.t_off * np.uint64(es)
        b_ptr = np.uint64(base) + self.b_off * np.uint64(es)
        nbytes = self.n * es
        return (b_ptr, t_ptr, nbytes) if to_bucket else (t_ptr, b_ptr, nbytes)


def _plan(lay: ops.BucketLayout, lo: int, hi: int) -> _RangePlan:
    cache = lay.__dict__.setdefault("_range_plans", {})
    p = cache.get((lo, hi))
    if p is None:
        p = cache[(lo, hi)] = _RangePlan(lay, lo, hi)
    return p


def _range_copies(ptrs: np.ndarray, lay: ops.BucketLayout, base: int, es: int, lo: int, hi: int, to_bucket: bool,
                  with_tensors: bool = False):
    """Byte-copy lists moving bucket elements [lo, hi) between the host bucket at `base` and the tensors
    whose data pointers are `ptrs` (tensor k at lay.offsets[k]; pads are never copied). with_tensors: the
    tensor index of every piece is returned too."""
    p = _plan(lay, lo, hi)
    out = p.copies(ptrs, base, es, to_bucket)
    return out + (p.k,) if with_tensors else out


_CHUNK_DT = np.dtype([("start", "<i8"), ("len", "<i4"), ("tensor", "<i4"), ("first_chunk", "<i4"),
                      ("nchunks", "<i4")])   # adfl_slq_chunk


class _ChunkMeta:
    """A layout's chunk table as arrays (cached on the layout): every chunk's [start, end) and, per tensor, its
    first chunk and one past its last — what the range-pipelined host paths launch chunk ranges with."""

    __slots__ = ("start", "end", "first", "cend")

    def __init__(self, lay: ops.BucketLayout):
        c = np.frombuffer(lay.chunks, dtype=_CHUNK_DT)
        self.start = c["start"].astype(np.int64)
        self.end = self.start + c["len"]
        t_first = np.zeros(lay.ntensors, dtype=np.int64)
        t_first[c["tensor"][c["first_chunk"] == np.arange(len(c))]] = np.nonzero(c["first_chunk"] == np.arange(len(c)))[0]
        self.first = t_first
        self.cend = t_first + c["nchunks"][t_first]


def _chunk_meta(lay: ops.BucketLayout) -> _ChunkMeta:
    m = lay.__dict__.get("_chunk_meta")
    if m is None:
        m = lay.__dict__["_chunk_meta"] = _ChunkMeta(lay)
    return m


def _ptrs(tensors: List[torch.Tensor]) -> np.ndarray:
    return np.fromiter((t.data_ptr() for t in tensors), dtype=np.uint64, count=len(tensors))


def _host_heap(lay: ops.BucketLayout) -> None:
    """A host-resident call: the process heap sized for this layout's fp32 outputs (hostcopy.keep_host_heap:
    raised only as layouts grow; ADFL_KEEP_HOST_HEAP=0 leaves the allocator alone). Device-resident callers
    never change the allocator."""
    hostcopy.keep_host_heap(4 * lay.total, 4 * int(lay.sizes.max()))


def _stage_in(tensors: List[torch.Tensor], lay: ops.BucketLayout, st: _DeviceStaging, key: str,
              dtype: torch.dtype, host_ptrs: Optional[np.ndarray] = None) -> torch.Tensor:
    """The bucket on the device: one gather + one H2D for CPU tensors, one device gather otherwise.
    host_ptrs: the tensors' data pointers when the caller knows them all to be contiguous CPU tensors of the
    bucket's element size (adfl_torchhost.qint8_meta checked them in one call)."""
    dev_buf = st.buf(key, lay.total, dtype)
    if host_ptrs is None and tensors and tensors[0].is_cuda:
        # a device dict: its pointers and sizes checked in one native call, then one gather launch
        ok, numel, dptrs = _torchhost.get().device_ptrs(tensors, st.device.index, dev_buf.element_size())
        if ok and np.array_equal(numel.numpy(), lay.sizes):
            ops.bucket_gather(tensors, lay, dev_buf, checked=False, ptrs=dptrs)
            return dev_buf
    kinds = {False} if host_ptrs is not None else {t.is_cuda for t in tensors}
    if kinds == {False}:
        _host_heap(lay)
        host = st.buf(key + "_host", lay.total, dtype, pinned=True)
        es = host.element_size()
        if host_ptrs is not None or all(t.is_contiguous() and t.element_size() == es for t in tensors):
            # Native parallel gather (csrc/host_copy.cpp) in element ranges, each range's H2D enqueued as
            # soon as it is staged so the copy engine overlaps the next range's host copy. Pads of an
            # aligned layout are never read.
            ptrs = _ptrs(tensors) if host_ptrs is None else host_ptrs
            for lo, hi in _ranges(lay, es):
                hostcopy.copy_pieces(*_range_copies(ptrs, lay, host.data_ptr(), es, lo, hi, to_bucket=True))
                dev_buf[lo:hi].copy_(host[lo:hi], non_blocking=True)
        else:
            _gather(tensors, lay, host)
            dev_buf.copy_(host, non_blocking=True)
    elif kinds == {True}:
        es = dev_buf.element_size()
        if all(t.device == st.device and t.is_contiguous() and t.element_size() == es and t.numel() == n
               for t, n in zip(tensors, lay.sizes.tolist())):
            # one launch; quantized payloads read from their storage (checked just above)
            ops.bucket_gather(tensors, lay, dev_buf, checked=False)
        else:
            _gather([t.to(st.device) for t in tensors], lay, dev_buf)
    else:  # mixed host / device dict: per-tensor copies (rare)
        for t, off, n in zip(tensors, lay.offsets.tolist(), lay.sizes.tolist()):
            dev_buf[off:off + n].view(t.shape).copy_(t)
    return dev_buf


_PIPELINE = os.environ.get("ADFL_HOST_PIPELINE", "1") != "0"


def _drain(*streams) -> None:
    """A pipelined host path that fails part-way (an output allocation, a caller's emit / idle callback, a
    native call) may leave H2D copies reading, and kernels and D2H copies writing, the staging buffers it
    shares with the next call (the pinned buckets, the device buckets): wait for every stream it enqueued on
    before the exception leaves, so the next call's gathers cannot overwrite a buffer still in use."""
    for s in streams:
        if s is not None:
            try:
                s.synchronize()
            except Exception:   # the original exception is the one to report
                pass


class PhaseClock:
    """Wall milliseconds the calling thread spends in each phase of the host-to-host path (exclusive, no extra
    synchronisation): filled while a `phase_clock()` block is active, e.g. bench.py's channel_c3_dict."""

    def __init__(self):
        self.ms: Dict[str, float] = {}


_CLOCK: Optional[PhaseClock] = None


class _Phase:
    __slots__ = ("name", "t0")

    def __init__(self, name: str):
        self.name = name

    def __enter__(self):
        self.t0 = time.perf_counter()

    def __exit__(self, *exc):
        c = _CLOCK
        if c is not None:
            c.ms[self.name] = c.ms.get(self.name, 0.0) + (time.perf_counter() - self.t0) * 1e3


class _NoPhase:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return None


_NO_PHASE = _NoPhase()


def _ph(name: str):
    return _NO_PHASE if _CLOCK is None else _Phase(name)


class phase_clock:
    """`with phase_clock() as c:` — c.ms holds the phase split of the channel calls made inside."""

    def __enter__(self) -> PhaseClock:
        global _CLOCK
        self.prev = _CLOCK
        _CLOCK = PhaseClock()
        return _CLOCK

    def __exit__(self, *exc):
        global _CLOCK
        _CLOCK = self.prev


class _PendingD2H:
    """D2H of a device bucket into the reused pinned staging, enqueued range by range with an event each;
    finish() scatters every range into the per-tensor CPU storages as soon as its copy lands (the native
    pool copies while the copy engine moves the next range). Whatever the caller does between the two —
    allocating the output tensors — overlaps the copies."""

    def __init__(self, dev_buf: torch.Tensor, lay: ops.BucketLayout, st: _DeviceStaging, key: str):
        self.host = st.buf(key + "_host", lay.total, dev_buf.dtype, pinned=True)
        self.lay = lay
        stream = torch.cuda.current_stream(st.device)
        self.stream = stream
        self.ranges = _ranges(lay, self.host.element_size())
        self.events = []
        for lo, hi in self.ranges:
            self.host[lo:hi].copy_(dev_buf[lo:hi], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(stream)
            self.events.append(ev)

    def finish_building(self, make, count: int, make_batch=None) -> List[torch.Tensor]:
        """Create the `count` outputs (make(k): a fresh contiguous CPU tensor for tensor k of the layout) in
        offset order while the D2H runs, and hand each staging range's scatter to the native pool as soon as
        its copy has landed and every output it touches exists; the pool copies while this thread goes on
        creating the next outputs (their creation was otherwise serial with the scatter). Returns the outputs
        once every byte has landed in them. ADFL_HOST_PIPELINE=0: create all, then finish() (the A/B)."""
        lay = self.lay
        offs = lay.offsets
        if make is None:  # batched creation only: make(k) from it when the slow path needs one
            make = lambda k: make_batch(k, k + 1)[0][0]  # noqa: E731
        if not _PIPELINE or count != lay.ntensors or (count > 1 and (np.diff(offs) < 0).any()):
            outs = [make(k) for k in range(count)]
            hostcopy.advise_huge(outs)
            self.finish(outs)
            return outs
        es = self.host.element_size()
        base = self.host.data_ptr()
        ptrs = np.zeros(count, dtype=np.uint64)
        outs: List[torch.Tensor] = []
        pending = []
        k = 0
        try:
            for (lo, hi), ev in zip(self.ranges, self.events):
                with _ph("out.alloc"):
                    if make_batch is not None:   # the range's new outputs in one native call (adfl_torchhost)
                        k_end = int(np.searchsorted(offs, hi, side="left"))
                        if k_end > k:
                            ts, pt = make_batch(k, k_end)
                            outs.extend(ts)
                            ptrs[k:k_end] = pt.numpy().view(np.uint64)
                            for j in np.nonzero(lay.sizes[k:k_end] * es >= (4 << 20))[0].tolist():
                                hostcopy.advise_huge([ts[j]])
                            k = k_end
                    while k < count and offs[k] < hi:   # every tensor the range [lo, hi) touches starts below hi
                        t = make(k)
                        if t.is_cuda or not t.is_contiguous() or t.element_size() != es:
                            raise ValueError("staging: outputs must be contiguous CPU tensors of the bucket's "
                                             "element size")
                        if t.numel() * es >= (4 << 20):
                            hostcopy.advise_huge([t])
                        ptrs[k] = t.data_ptr()
                        outs.append(t)
                        k += 1
                with _ph("out.d2h_wait"):
                    ev.synchronize()   # usually landed already: the outputs took longer than the copy
                with _ph("out.scatter_submit"):
                    pending.append(hostcopy.submit_pieces(*_range_copies(ptrs, lay, base, es, lo, hi,
                                                                         to_bucket=False),
                                                          stream=True, keep=self.host))
            while k < count:   # tensors past the last range (none for a bucket layout; kept for safety)
                outs.append(make(k))
                k += 1
        except BaseException:
            _drain(self.stream)
            raise
        finally:
            with _ph("out.scatter_wait"):
                for pd in pending:
                    pd.wait()
        return outs

    def finish(self, outs: List[torch.Tensor], ptrs: Optional[np.ndarray] = None) -> None:
        """outs: contiguous CPU tensors owned by the caller, tensor k receiving bucket elements at offsets[k].
        ptrs: their data pointers when the caller made them (adfl_torchhost) and knows them to fit."""
        es = self.host.element_size()
        if ptrs is None:
            for t in outs:
                if t.is_cuda or not t.is_contiguous() or t.element_size() != es:
                    raise ValueError("staging: outputs must be contiguous CPU tensors of the bucket's element size")
            ptrs = _ptrs(outs)
        for (lo, hi), ev in zip(self.ranges, self.events):
            ev.synchronize()
            hostcopy.copy_pieces(*_range_copies(ptrs, self.lay, self.host.data_ptr(), es, lo, hi, to_bucket=False),
                                 stream=True)


def _stage_out(dev_buf: torch.Tensor, lay: ops.BucketLayout, st: _DeviceStaging, key: str,
               outs: List[torch.Tensor]) -> None:
    """Copy the bucket `dev_buf` (on the device) into the per-tensor CPU storages `outs` (_PendingD2H)."""
    _PendingD2H(dev_buf, lay, st, key).finish(outs)


def _hand_out(out_dev: torch.Tensor, lay: ops.BucketLayout, shapes: List[torch.Size], on_cpu: List[bool],
              st: _DeviceStaging, key: str, like: Optional[List[torch.Tensor]] = None) -> List[torch.Tensor]:
    """Decoded tensors as the reference returns them (quant.py:107-112): one new, owned, writable tensor
    per entry — pageable CPU tensors for CPU payloads, device tensors for device payloads — never views
    of a shared bucket (a strategy keeps single updates alive, Src/ADFL/Strategy/fed_buff.py:75,90, and
    pickling one must not ship the whole bucket). For an all-CPU dict the D2H is enqueued first and the
    output tensors are allocated while it runs."""
    outs: List[Optional[torch.Tensor]] = [None] * len(shapes)
    if all(on_cpu):
        pending = _PendingD2H(out_dev, lay, st, key)
        dt = out_dev.dtype
        if like is not None and dt == torch.float32:   # `like`: tensors of the outputs' shapes (the payloads)
            th = _torchhost.get()
            return pending.finish_building(None, len(shapes), make_batch=lambda a, b: th.empty_f32_like(like[a:b]))
        return pending.finish_building(lambda k: torch.empty(shapes[k], dtype=dt), len(shapes))
    if not any(on_cpu) and out_dev.device == st.device:
        # device dict: fresh owned tensors filled from the bucket by one launch (not one clone per tensor)
        th = _torchhost.get()
        if (like is not None and out_dev.dtype == torch.float32
                and th.device_ptrs(like, st.device.index, like[0].element_size())[0]):
            dev_outs, ptrs = th.empty_f32_like(like)   # one native call, on like's (= the staging's) device
            ops.bucket_scatter(out_dev, lay, dev_outs, checked=False, ptrs=ptrs)
        else:
            dev_outs = [torch.empty(s, dtype=out_dev.dtype, device=st.device) for s in shapes]
            ops.bucket_scatter(out_dev, lay, dev_outs, checked=False)
        torch.cuda.current_stream(st.device).synchronize()
        return dev_outs
    for i, (off, n, s) in enumerate(zip(lay.offsets.tolist(), lay.sizes.tolist(), shapes)):
        if on_cpu[i]:  # mixed host / device dict (rare): per-tensor copies
            outs[i] = torch.empty(s, dtype=out_dev.dtype)
            outs[i].view(-1).copy_(out_dev[off:off + n])
        else:
            outs[i] = out_dev[off:off + n].view(s).clone()
    torch.cuda.current_stream(st.device).synchronize()
    return outs


def _int8_view(q: torch.Tensor) -> torch.Tensor:
    """The int8 bytes of a qint8 tensor without the copy `int_repr()` makes."""
    return torch.empty(0, dtype=torch.int8, device=q.device).set_(q.untyped_storage(), q.storage_offset(),
                                                                  q.shape, q.stride())


def _byte_view(t: torch.Tensor) -> torch.Tensor:
    """The bytes of an int8 / uint8 / qint8 tensor as a uint8 tensor over the same storage."""
    if t.is_quantized:
        t = _int8_view(t)
    return t if t.dtype == torch.uint8 else t.view(torch.uint8)


def _rows_from_ptrs(ptrs, lay: ops.BucketLayout, st: _DeviceStaging, key: str) -> torch.Tensor:
    """K clients' one-byte-per-element payloads, given as one array of data pointers per client (contiguous
    CPU storages, client k's tensor j at lay.offsets[j]) -> device rows [K, pad16(lay.total)] uint8: one
    native gather per client into its pinned row, that row's H2D enqueued as soon as it is staged (the copy
    engine overlaps the next client's gather)."""
    k = len(ptrs)
    row = (lay.total + 15) // 16 * 16
    dev = st.buf(key, k * row, torch.uint8).view(k, row)
    host = st.buf(key + "_host", k * row, torch.uint8, pinned=True).view(k, row)
    for r, p in enumerate(ptrs):
        hostcopy.copy_pieces(*_range_copies(p, lay, host[r].data_ptr(), 1, 0, lay.total, to_bucket=True))
        dev[r].copy_(host[r], non_blocking=True)
    return dev


def _stage_rows(clients: List[List[torch.Tensor]], lay: ops.BucketLayout, st: _DeviceStaging,
                key: str) -> torch.Tensor:
    """K clients' payload tensors of one byte per element (int8 / uint8 / qint8; client k's tensor j at
    lay.offsets[j]) -> device rows [K, pad16(lay.total)] uint8. All on the CPU: _rows_from_ptrs."""
    if all(not t.is_cuda and t.is_contiguous() and t.element_size() == 1 for c in clients for t in c):
        # byte copies from the tensors' storages: qint8 payloads need no int8 view object here
        return _rows_from_ptrs([_ptrs(c) for c in clients], lay, st, key)
    k = len(clients)
    row = (lay.total + 15) // 16 * 16
    dev = st.buf(key, k * row, torch.uint8).view(k, row)
    if all(t.device == st.device and t.is_contiguous() and t.element_size() == 1 and t.numel() == n
           for c in clients for t, n in zip(c, lay.sizes.tolist())):
        for r, c in enumerate(clients):   # device payloads: one gather launch per client row
            ops.bucket_gather(c, lay, dev[r], checked=False)
    else:  # mixed payloads: per-tensor copies into the device rows
        for r, c in enumerate(clients):
            for t, off, n in zip(c, lay.offsets.tolist(), lay.sizes.tolist()):
                dev[r, off:off + n].copy_(_byte_view(t).reshape(-1).to(st.device))
    return dev
