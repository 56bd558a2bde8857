"""SLQ channels backed by the MI355X HIP codec — drop-in for ``Src/ADFL/Channel/quant.py:15-137``.

``SLQChannel`` / ``USLQChannel`` keep the reference's names, constructor, six-method surface,
``to_json`` output, ``simulate_bandwidth`` formula, payload types and error behaviour. What changes is
where the arithmetic runs: the reference loops over the state dict calling ATen CPU ops per tensor
(quant.py:74-112); here the whole dict is packed back to back into one flat buffer, moved to
the GPU once, encoded by two HIP launches (absmax partials -> scale + quantize, per-tensor scales),
and the int8 payload comes back in one copy. Decode is one HIP launch. Output is bit-identical to the
reference: int8 payload, fp32 scale and dequantized floats (tests/golden).

Contract kept from the reference:
* inputs are CPU tensors (callers ``.cpu()``, Src/ADFL/model.py:195-197) — CUDA tensors are also
  accepted and then stay on the device;
* ``ndim <= 1`` tensors pass through untouched with ``scale = 1`` (quant.py:80-81, same object);
* ``QuantParameter.data`` is a ``torch.qint8`` tensor (zero point 0) and ``scale`` a Python float;
* decode returns new, owned, writable fp32 tensors (strategies mutate them in place);
* a non-fp32 ``ndim > 1`` tensor raises ``RuntimeError: Quantize only works on Float Tensor, got …``;
  an empty one raises torch.max's ``RuntimeError``; ``_receive`` asserts ``QuantParameters``;
* the channel object holds no device state (it is pickled into every Ray actor): buffers live in a
  per-process, per-device cache created lazily on first use (_staging.py).

This module is the SLQ codec's side of a call: which kernels run over the bucket and how the qint8 payloads
and scales are built. How the bucket gets to the device and the results back into owned tensors is
_staging.py's; the class skeleton shared with the stochastic channels (stoch.py) is _base.py's. The six
stochastic channels are importable from here as well, as they are from the reference's quant.py.

There is no CPU fallback: without a GPU and the built HIP library these methods raise.
"""

import time
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from .. import _lib, _torchhost, hostcopy, ops, qerror
from .._lib import check
from ..model import CompressedParameters, Parameters, QuantParameter, QuantParameters
from . import _staging as _stg
from ._base import (_broadcast_groups, _CodecChannel, _delta_on_device, _delta_pairs, _mean_axpby_out, _passthrough_idle,
                    _Unidirectional)
from ._staging import (_DeviceStaging, _PendingD2H, _chunk_meta, _drain, _hand_out, _host_heap, _int8_view, _ph,
                       _plan, _range_copies, _ranges, _rows_from_ptrs, _serialized, _stage_in, _stage_rows,
                       _staging, phase_clock)  # noqa: F401  (phase_clock: re-exported, bench.py uses it from here)
from .stoch import (CNATChannel, QSGDChannel, RQSGDChannel, UCNATChannel, UQSGDChannel,  # noqa: F401
                    URQSGDChannel)   # beside the SLQ channels, as in the reference (quant.py:140-570)
from .stoch import (PackedQSGDChannel, PackedRQSGDChannel, UPackedQSGDChannel,  # noqa: F401
                    UPackedRQSGDChannel)   # their packed wire format (bits + 1 bits per weight)


def _host_scales(amax_bits: np.ndarray, bits: int) -> np.ndarray:
    """fp32(max|x| / q_max) from the magnitude bits the staging gather reduced (quant.py:99-100: fp32 tensor
    math, correctly rounded; a NaN magnitude gives a NaN scale) — what the device encode computes."""
    return (amax_bits.view(np.float32) / np.float32((1 << (bits - 1)) - 1)).astype(np.float32)


def _qerror_sums(x_dev: torch.Tensor, d_dev: torch.Tensor, lay: ops.BucketLayout):
    """The reference's q-error sums of a bucket against its decode (qerror.reference_sums): over the
    tensors back to back, so a padded layout (int4 buckets: align 2) is compacted first."""
    sizes = lay.sizes.tolist()
    if (lay.offsets != np.concatenate([[0], np.cumsum(lay.sizes)[:-1]])).any():
        x_dev = torch.cat([x_dev[o:o + n] for o, n in zip(lay.offsets.tolist(), sizes)])
        d_dev = torch.cat([d_dev[o:o + n] for o, n in zip(lay.offsets.tolist(), sizes)])
    return qerror.reference_sums(x_dev, d_dev, sizes)


def _encode_host_dict(tensors: List[torch.Tensor], lay: ops.BucketLayout, st: _DeviceStaging, bits: int,
                      stats: Optional[list], emit, idle):
    """The all-CPU fp32 dict's encode, pipelined range by range across the host, the link and the GPU.

    The gather into the pinned bucket is queued on the native pool range by range. As each range lands (the
    thread enqueues every landed range before it builds outputs), one native call (adfl_stage_encode_range)
    enqueues its H2D and, for the tensors whose every byte is now staged, the device's absmax and quantize
    over their chunks (adfl_slq_absmax_batched_range + adfl_slq_quantize_batched_range: the two-pass encode's
    kernels, so the same payload and scales), then their payload bytes' D2H on a side stream behind an event.
    The D2H and scatter of range r overlap the H2D of range r + 1.
    The outputs are built while the copies run: the gather also reduces max|x| per tensor as it copies
    (adfl_host_copy_submit_absmax), so the host knows each scale in time to create the qint8 outputs (one
    native call per range) and emit(k, q, scale) each payload object, and the scatter into them is queued on
    the pool behind the range's event. `idle()` (the caller's other payload objects) runs in between. The
    payload bytes and scales are the device's: its scales are compared with the host's at the end and any
    output whose host scale differed is rebuilt with the device's. Returns [(q, scale)] per tensor."""
    with _ph("enc.heap"):
        _host_heap(lay)
    dev = st.device
    stream = torch.cuda.current_stream(dev)
    sh = stream.cuda_stream
    lib = _lib.load()
    x_dev = st.buf("x", lay.total, torch.float32)
    host = st.buf("x_host", lay.total, torch.float32, pinned=True)
    q_dev = st.buf("q", lay.total, torch.int8)
    q_host = st.buf("q_host", lay.total, torch.int8, pinned=True)
    s_dev = st.buf("scales", lay.ntensors, torch.float32)
    part_dev = st.buf("partials", lay.nchunks, torch.int32)
    chunks_ptr = lay.device_chunks(dev).data_ptr()
    d2h = st.d2h_stream()
    cm = _chunk_meta(lay)
    amax = np.zeros(lay.ntensors, dtype=np.uint32)
    a_base = amax.ctypes.data
    th = _torchhost.get()
    ptrs = th.data_ptrs(tensors).numpy().view(np.uint64)
    ranges = _ranges(lay, 4)
    evs = st.events(2 * len(ranges))
    d2h_h = d2h.cuda_stream
    hx, dx, qd, qh = host.data_ptr(), x_dev.data_ptr(), q_dev.data_ptr(), q_host.data_ptr()
    pd, sd = part_dev.data_ptr(), s_dev.data_ptr()
    jobs = []
    with _ph("enc.gather_submit"):
        for lo, hi in ranges:
            plan = _plan(lay, lo, hi)
            b_ptr, t_ptr, nb = plan.copies(ptrs, host.data_ptr(), 4, True)
            jobs.append(hostcopy.submit_pieces(b_ptr, t_ptr, nb,
                                               absmax_ptrs=np.uint64(a_base) + plan.ku * np.uint64(4),
                                               keep=(host, amax)))
    ends = lay.offsets + lay.sizes
    outs: List[torch.Tensor] = []
    out_ptrs = np.zeros(lay.ntensors, dtype=np.uint64)
    scales = np.zeros(lay.ntensors, dtype=np.float32)
    scatters = []
    made = 0
    staged: List[Tuple[int, int, int, int, int]] = []   # ranges on the device whose outputs are not built yet
    r = 0
    try:
        while r < len(ranges) or staged:
            # every range whose gather has landed goes to the device at once (the link, not this thread, then
            # paces the H2D); the thread waits on a gather only when it has no outputs left to build
            while r < len(ranges) and (not staged or jobs[r].done()):
                lo, hi = ranges[r]
                with _ph("enc.gather_absmax_wait"):
                    jobs[r].wait()
                done = int(np.searchsorted(ends, hi, side="right"))   # tensors whose every byte is staged
                with _ph("enc.kernel_launch"):
                    # one native call: the range's H2D; the device's absmax and quantize of the tensors it
                    # completes; their payload bytes back D2H on the side stream behind an event (host_stage.hip)
                    c0 = c1 = e0 = e1 = 0
                    if done > made:
                        c0, c1 = int(cm.first[made]), int(cm.cend[done - 1])
                        e0, e1 = int(lay.offsets[made]), int(ends[done - 1])
                    check(lib.adfl_stage_encode_range(hx, dx, lo, hi, pd, chunks_ptr, c0, c1 - c0, bits, qd, sd, qh,
                                                      e0, e1, sh, d2h_h, evs[2 * r], evs[2 * r + 1]))
                if done > made:
                    staged.append((made, done, e0, e1, evs[2 * r + 1]))
                    made = done
                r += 1
            if not staged:
                continue
            t0, t1, e0, e1, ev = staged.pop(0)
            with _ph("enc.outputs"):
                scales[t0:t1] = _host_scales(amax[t0:t1], bits)
                # the range's payload tensors in one native call (adfl_torchhost): the qint8 tensors
                # torch.quantize_per_tensor(x, scale, 0, torch.qint8) would return, still to be filled
                qs, qp = th.empty_qint8_like(tensors[t0:t1], torch.from_numpy(scales[t0:t1]))
                out_ptrs[t0:t1] = qp.numpy().view(np.uint64)
                sl = scales[t0:t1].tolist()
                for j, q in enumerate(qs):
                    outs.append(q)
                    emit(t0 + j, q, sl[j])
            with _ph("enc.scatter_submit"):
                scatters.append(hostcopy.submit_pieces(
                    *_range_copies(out_ptrs, lay, q_host.data_ptr(), 1, e0, e1, to_bucket=False),
                    stream=True, event=ev, keep=q_host))
            with _ph("enc.passthrough"):
                idle()
    except BaseException:
        _drain(stream, d2h)
        raise
    finally:
        for j in jobs:
            j.wait()
        with _ph("enc.scatter_wait"):
            for j in scatters:
                j.wait()
    if stats is not None:
        stats.append(_qerror_sums(x_dev, ops.decode_batched(q_dev, s_dev, lay, out=st.buf("qe_d", lay.total, torch.float32)),
                                  lay))
    scales_host = st.buf("scales_host", lay.ntensors, torch.float32, pinned=True)
    scales_host.copy_(s_dev, non_blocking=True)
    scales_ready = torch.cuda.Event()
    scales_ready.record(stream)
    with _ph("enc.passthrough"):
        while idle():   # the caller's remaining objects
            pass
    scales_ready.synchronize()
    dev_scales = scales_host.numpy()
    bad = np.nonzero(dev_scales.view(np.uint32) != scales.view(np.uint32))[0]
    res = [(q, float(sc)) for q, sc in zip(outs, scales)]
    for k in bad.tolist():   # never seen (both reduce the same magnitude bits and divide correctly rounded):
        # the device's scale is the one the payload was quantized with
        sc = float(dev_scales[k])
        q = torch._make_per_tensor_quantized_tensor(_int8_view(outs[k]), sc, 0)
        res[k] = (q, sc)
        emit(k, q, sc)
    return res


@_serialized
def _encode_dict(params: Parameters, names: List[str], bits: int, stats: Optional[list] = None,
                 emit=None, idle=None, meta=None):
    """Encode the ndim>1 tensors `names` of `params` in one bucketed pass.

    Returns {name: (qint8 tensor on the input's device, python float scale)}. With `stats` (a list), the
    four q-error sums of the bucket against its payload are appended to it (ops.qerror_batched). For a dict
    of contiguous CPU fp32 tensors the outputs are built while the copies run (_encode_host_dict): emit(k, q,
    scale) is called for each as it is created and idle() (returning True while it has work left) between
    the copy ranges."""
    st = _staging()
    tensors = [params[n] for n in names]
    # meta: (sizes, all contiguous CPU) from _quantize_params' native scan (every tensor already fp32)
    lay = st.layout(meta[0] if meta is not None else tuple(int(t.numel()) for t in tensors))
    all_host = meta[1] if meta is not None else all(not t.is_cuda and t.is_contiguous() for t in tensors)
    if _stg._PIPELINE and all_host and (meta is not None or all(t.dtype == torch.float32 for t in tensors)):
        res = _encode_host_dict(tensors, lay, st, bits, stats, emit or (lambda k, q, sc: None),
                                idle or (lambda: False))
        return {name: r for name, r in zip(names, res)}
    x_dev = _stage_in(tensors, lay, st, "x", torch.float32)
    q_dev, s_dev = ops.encode_batched(x_dev, lay, bits, q=st.buf("q", lay.total, torch.int8),
                                      scales=st.buf("scales", lay.ntensors, torch.float32),
                                      partials=st.buf("partials", lay.nchunks, torch.int32))
    if stats is not None:
        stats.append(_qerror_sums(x_dev, ops.decode_batched(q_dev, s_dev, lay, out=st.buf("qe_d", lay.total, torch.float32)),
                                  lay))
    return _payloads_out(names, tensors, lay, st, q_dev, s_dev)


def _payloads_out(names: List[str], tensors: List[torch.Tensor], lay: ops.BucketLayout, st: _DeviceStaging,
                  q_dev: torch.Tensor, s_dev: torch.Tensor):
    """The owned qint8 payloads of an encoded bucket (q_dev, s_dev in `lay`): {name: (qint8 tensor shaped like
    tensors[k] and on its device, python float scale)} — the output half of _encode_dict and _encode_delta_dict."""
    dev = st.device
    scales_host = st.buf("scales_host", lay.ntensors, torch.float32, pinned=True)
    scales_host.copy_(s_dev, non_blocking=True)
    on_cpu = [not t.is_cuda for t in tensors]
    if all(on_cpu):
        # every payload tensor owns its bytes (compact pickles; the staging buffer is reused by the next
        # call): the payload D2H is enqueued right behind the scales, and the qint8 tensors (which need the
        # scales) are allocated while it runs, then filled by the native scatter as its ranges land
        scales_ready = torch.cuda.Event()
        scales_ready.record(torch.cuda.current_stream(dev))
        pending = _PendingD2H(q_dev, lay, st, "q")
        scales_ready.synchronize()
        scales = scales_host.tolist()
        eaq, qint8 = torch._empty_affine_quantized, torch.qint8
        qs = pending.finish_building(
            lambda k: eaq(tensors[k].shape, scale=scales[k], zero_point=0, dtype=qint8), len(tensors))
        return {name: (qt, sc) for name, qt, sc in zip(names, qs, scales)}
    torch.cuda.current_stream(dev).synchronize()
    scales = scales_host.tolist()
    if not any(on_cpu) and all(t.device == dev for t in tensors):
        # device dict: the qint8 payloads allocated by one native call (on the tensors' device, no launch each)
        # and filled from the bucket by one launch
        qs, qp = _torchhost.get().empty_qint8_like(tensors, scales_host)
        ops.bucket_scatter(q_dev, lay, qs, checked=False, ptrs=qp)
        torch.cuda.current_stream(dev).synchronize()
        return {name: (qt, sc) for name, qt, sc in zip(names, qs, scales)}
    out = {}
    offs, sizes = lay.offsets.tolist(), lay.sizes.tolist()
    for i, (name, t) in enumerate(zip(names, tensors)):
        src = q_dev[offs[i]:offs[i] + sizes[i]].view(t.shape)
        if on_cpu[i]:
            src = src.cpu()
        # _make_per_tensor_quantized_tensor copies into a fresh qint8 storage of the source's device
        out[name] = (torch._make_per_tensor_quantized_tensor(src, scales[i], 0), scales[i])
    return out


@_serialized
def _decode_dict(items: List[Tuple[str, torch.Tensor]], idle=None) -> Dict[str, torch.Tensor]:
    """Decode qint8 tensors (per-tensor affine, zero point 0) in one bucketed pass. idle(): the caller's
    other entries, run by the pipelined host path while its last copies are in flight (else not at all)."""
    st = _staging()
    dev = st.device
    qlist = [q for _, q in items]
    with _ph("dec.meta"):
        # every payload's quantizer, size, place and data pointer in one native call (adfl_torchhost)
        ok, all_host, numel, scales, ptrs = _torchhost.get().qint8_meta(qlist)
    if not ok:
        qint8, pta = torch.qint8, torch.per_tensor_affine
        for name, q in items:
            if not q.is_quantized or q.dtype != qint8 or q.qscheme() != pta or q.q_zero_point() != 0:
                raise ValueError(f"SLQChannel: '{name}' is not a per-tensor qint8 payload with zero point 0")
    lay = st.layout(tuple(numel.tolist()))
    if all_host and _stg._PIPELINE:
        decoded = _decode_host_dict(qlist, lay, st, ptrs.numpy().view(np.uint64), scales, idle)
        return {name: t for (name, _), t in zip(items, decoded)}
    # CPU qint8 payloads are gathered byte-wise straight from their storage; device ones through int8 views
    all_dev = not all_host and all(q.is_cuda and q.device == dev and q.is_contiguous() for q in qlist)
    # host payloads are gathered byte-wise from their storages, device ones by one gather launch: neither
    # needs an int8 view object per tensor
    qs = qlist if all_host or all_dev else [_int8_view(q) for q in qlist]
    with _ph("dec.gather_h2d"):
        q_dev = _stage_in(qs, lay, st, "dq", torch.int8, host_ptrs=ptrs.numpy().view(np.uint64) if all_host else None)
    with _ph("dec.scales"):
        # q_scale() is a double; fbgemm's dequantize uses it as fp32 (quant.py:110): qint8_meta rounded it so
        s_dev = scales.to(dev, non_blocking=True)
    on_cpu = [True] * len(qlist) if all_host else [not q.is_cuda for q in qlist]
    with _ph("dec.kernel_launch"):
        out_dev = ops.decode_batched(q_dev, s_dev, lay, out=st.buf("d_out", lay.total, torch.float32))
    decoded = _hand_out(out_dev, lay, [q.shape for q in qlist] if not all_host else [None] * len(qlist), on_cpu, st,
                        "d_out", like=qlist if all_host or all_dev else None)
    return {name: t for (name, _), t in zip(items, decoded)}


def _decode_host_dict(qlist: List[torch.Tensor], lay: ops.BucketLayout, st: _DeviceStaging, ptrs: np.ndarray,
                      scales: torch.Tensor, idle=None) -> List[torch.Tensor]:
    """CPU qint8 payloads -> owned CPU fp32 tensors, pipelined range by range: the byte gather of every range
    is queued on the native pool at once; as range r lands, its H2D is enqueued, the chunks it completes are
    decoded (adfl_slq_dequantize_batched on that chunk range), their floats go back D2H behind an event, the
    outputs of the tensors they reach are created (one native call) and the scatter is queued on the pool
    behind the event — so the D2H of range r overlaps the H2D of range r + 1 and the scatters overlap the
    D2H. Bit-identical to the one-launch decode (each chunk is decoded by the same kernel)."""
    with _ph("dec.heap"):
        _host_heap(lay)
    dev = st.device
    stream = torch.cuda.current_stream(dev)
    sh = stream.cuda_stream
    lib = _lib.load()
    q_dev = st.buf("dq", lay.total, torch.int8)
    q_host = st.buf("dq_host", lay.total, torch.int8, pinned=True)
    out_dev = st.buf("d_out", lay.total, torch.float32)
    out_host = st.buf("d_out_host", lay.total, torch.float32, pinned=True)
    chunks_ptr = lay.device_chunks(dev).data_ptr()
    d2h = st.d2h_stream()
    cm = _chunk_meta(lay)
    th = _torchhost.get()
    ranges = _ranges(lay, 4)
    evs = st.events(2 * len(ranges))
    d2h_h = d2h.cuda_stream
    qh, qd, od, oh = q_host.data_ptr(), q_dev.data_ptr(), out_dev.data_ptr(), out_host.data_ptr()
    with _ph("dec.gather_submit"):
        jobs = [hostcopy.submit_pieces(*_range_copies(ptrs, lay, q_host.data_ptr(), 1, lo, hi, to_bucket=True),
                                       keep=q_host) for lo, hi in ranges]
    with _ph("dec.scales"):
        s_dev = scales.to(dev, non_blocking=True)
    offs = lay.offsets
    outs: List[torch.Tensor] = []
    out_ptrs = np.zeros(lay.ntensors, dtype=np.uint64)
    scatters = []
    c_made = 0
    t_made = 0
    try:
        sd = s_dev.data_ptr()
        for r, ((lo, hi), job) in enumerate(zip(ranges, jobs)):
            with _ph("dec.gather_wait"):
                job.wait()
            with _ph("dec.kernel_launch"):
                # one native call: the range's H2D; the decode of the chunks it completes; their floats back
                # D2H on the side stream behind an event (host_stage.hip)
                c_end = int(np.searchsorted(cm.end, hi, side="right"))   # chunks whose every byte is staged
                if c_end <= c_made:
                    check(lib.adfl_stage_decode_range(qh, qd, lo, hi, chunks_ptr, 0, 0, sd, od, oh, 0, 0, sh, d2h_h,
                                                      evs[2 * r], evs[2 * r + 1]))
                    continue
                e0, e1 = int(cm.start[c_made]), int(cm.end[c_end - 1])
                check(lib.adfl_stage_decode_range(qh, qd, lo, hi, chunks_ptr, c_made, c_end - c_made, sd, od, oh, e0,
                                                  e1, sh, d2h_h, evs[2 * r], evs[2 * r + 1]))
                ev = evs[2 * r + 1]
                c_made = c_end
            with _ph("out.alloc"):
                t_end = int(np.searchsorted(offs, e1, side="left"))    # tensors starting below e1
                if t_end > t_made:
                    ts, pt = th.empty_f32_like(qlist[t_made:t_end])
                    outs.extend(ts)
                    out_ptrs[t_made:t_end] = pt.numpy().view(np.uint64)
                    for j in np.nonzero(lay.sizes[t_made:t_end] * 4 >= (4 << 20))[0].tolist():
                        hostcopy.advise_huge([ts[j]])
                    t_made = t_end
            with _ph("out.scatter_submit"):
                scatters.append(hostcopy.submit_pieces(
                    *_range_copies(out_ptrs, lay, out_host.data_ptr(), 4, e0, e1, to_bucket=False),
                    stream=True, event=ev, keep=out_host))
        if idle is not None:
            with _ph("dec.passthrough"):
                idle()
    except BaseException:
        _drain(stream, d2h)
        raise
    finally:
        for j in jobs:
            j.wait()
        with _ph("out.scatter_wait"):
            for j in scatters:
                j.wait()
    return outs


@_serialized
def _decode_mean(clients: List[List[torch.Tensor]], scales: List[List[float]], shapes: List[torch.Size],
                 packed: bool, apply=None) -> List[torch.Tensor]:
    """The fp32 mean over K clients of their decoded tensors, tensor by tensor, in torch's CPU summation
    order for simple_aggregate (csrc/torch_sum_order.h), in ONE launch (ops.dequantize_mean_batched): clients[k][j] is client k's payload for tensor j (a qint8 tensor,
    or ceil(n/2) packed int8 bytes with packed=True), scales[k][j] its scale. Returns one
    owned tensor per entry (CPU when every client's payload is on the CPU). apply = (bases, where, alpha, beta):
    the fused decode-mean + axpby over the same rows instead (_mean_axpby_out), one owned tensor per entry where
    its base lives."""
    st = _staging()
    dev = st.device
    sizes = tuple(int(torch.Size(s).numel()) for s in shapes)
    if packed:   # element layout with even offsets; its bytes: every slot exactly ceil(n/2), back to back
        lay = st.layout(sizes, align=2)
        b_lay = st.layout(tuple((n + 1) // 2 for n in sizes), align=1)
    else:
        lay = b_lay = st.layout(sizes, align=1)
    rows = _stage_rows(clients, b_lay, st, "mq")
    s_dev = torch.tensor(scales, dtype=torch.float32).to(dev, non_blocking=True)
    if apply is not None:
        bases, where, alpha, beta = apply
        return _mean_axpby_out(st, lay, [torch.Size(s) for s in shapes], bases, where, "m_out",
                               lambda b, o: ops.dequantize_mean_axpby_batched(
                                   rows if packed else rows.view(torch.int8), s_dev, lay, b, o, alpha, beta,
                                   packed=packed))
    out_dev = ops.dequantize_mean_batched(rows if packed else rows.view(torch.int8), s_dev, lay,
                                          out=st.buf("m_out", lay.total, torch.float32), packed=packed)
    on_cpu = [not any(c[j].is_cuda for c in clients) for j in range(len(sizes))]
    return _hand_out(out_dev, lay, [torch.Size(s) for s in shapes], on_cpu, st, "m_out")


@_serialized
def _decode_mean_host(st: _DeviceStaging, like: List[torch.Tensor], numel: torch.Tensor, ptrs: List[np.ndarray],
                      scales: torch.Tensor, apply=None) -> List[torch.Tensor]:
    """_decode_mean for K CPU qint8 payload lists already checked (SLQChannel._mean_host_updates): each client's
    bytes gathered straight from the storages into its pinned row (_rows_from_ptrs), one decode-mean launch,
    and the fp32 means handed back as owned CPU tensors shaped like `like`, created by one native call per
    staging range while the D2H runs. apply: as _decode_mean's."""
    dev = st.device
    lay = st.layout(tuple(numel.tolist()), align=1)
    _host_heap(lay)
    rows = _rows_from_ptrs(ptrs, lay, st, "mq")
    s_dev = scales.to(dev, non_blocking=True)
    if apply is not None:
        bases, where, alpha, beta = apply
        return _mean_axpby_out(st, lay, [q.shape for q in like], bases, where, "m_out",
                               lambda b, o: ops.dequantize_mean_axpby_batched(rows.view(torch.int8), s_dev, lay, b, o,
                                                                              alpha, beta), like=like)
    out_dev = ops.dequantize_mean_batched(rows.view(torch.int8), s_dev, lay,
                                          out=st.buf("m_out", lay.total, torch.float32))
    return _hand_out(out_dev, lay, [None] * len(like), [True] * len(like), st, "m_out", like=like)


@_serialized
def _encode_dict_packed(params: Parameters, names: List[str], bits: int, stats: Optional[list] = None):
    """Packed int4 variant of _encode_dict: {name: (int8 tensor of ceil(n/2) packed bytes, scale)}; with
    `stats`, the bucket's four q-error sums against its packed payload are appended."""
    st = _staging()
    tensors = [params[n] for n in names]
    th = _torchhost.get()
    host_ok, numel, hptrs = th.host_bytes(tensors, 4)   # sizes, and contiguous CPU fp32 storages, in one call
    lay = st.layout(tuple(numel.tolist()), align=2)
    x_dev = _stage_in(tensors, lay, st, "x", torch.float32, host_ptrs=hptrs.numpy().view(np.uint64) if host_ok else None)
    p_dev, s_dev = ops.encode_batched_int4(x_dev, lay, bits, packed=st.buf("p", lay.total // 2, torch.uint8),
                                           scales=st.buf("scales", lay.ntensors, torch.float32),
                                           partials=st.buf("partials", lay.nchunks, torch.int32))
    if stats is not None:
        stats.append(_qerror_sums(x_dev, ops.decode_batched_int4(p_dev, s_dev, lay,
                                                                 out=st.buf("qe_d", lay.total, torch.float32)), lay))
    return _packed_out(names, tensors, lay, st, p_dev, s_dev, host_ok, numel)


def _packed_bytes_layout(lay: ops.BucketLayout, st: _DeviceStaging) -> ops.BucketLayout:
    """The packed-byte layout of an even-offset element layout: tensor k's ceil(n/2) bytes at offsets[k] / 2.
    With align=2 every slot is exactly that many bytes and the layout is the compact one of the staging cache;
    a wider alignment (send_delta's device route) keeps its pads out of the layout (cached on `lay`)."""
    if lay.align == 2:
        return st.layout(tuple(int(n) // 2 for n in lay.padded.tolist()), align=1)
    p_lay = lay.__dict__.get("_packed_bytes")
    if p_lay is None:
        p_lay = lay.__dict__["_packed_bytes"] = ops.BucketLayout(((lay.sizes + 1) // 2).tolist(),
                                                                 offsets=(lay.offsets // 2).tolist())
    return p_lay


def _packed_out(names: List[str], tensors: List[torch.Tensor], lay: ops.BucketLayout, st: _DeviceStaging,
                p_dev: torch.Tensor, s_dev: torch.Tensor, host_ok: bool, numel: torch.Tensor):
    """The owned packed payloads of an int4-encoded bucket: {name: (int8 tensor of ceil(n/2) packed bytes on
    tensors[k]'s device, python float scale)} — the output half of _encode_dict_packed and _encode_delta_dict_packed."""
    dev = st.device
    th = _torchhost.get()
    scales_host = st.buf("scales_host", lay.ntensors, torch.float32, pinned=True)
    scales_host.copy_(s_dev, non_blocking=True)
    torch.cuda.current_stream(dev).synchronize()
    scales = scales_host.tolist()
    p_lay = _packed_bytes_layout(lay, st)
    if host_ok:   # the owned int8 payloads created by one native call per staging range while the D2H runs
        p_numel = (numel + 1) // 2
        parts = _PendingD2H(p_dev.view(torch.int8), p_lay, st, "p").finish_building(
            None, len(tensors), make_batch=lambda a, b: th.empty_1d(p_numel[a:b], 1))
        return {name: (pt, sc) for name, pt, sc in zip(names, parts, scales)}
    on_cpu = [not t.is_cuda for t in tensors]
    shapes = [torch.Size([(int(t.numel()) + 1) // 2]) for t in tensors]
    # int8, as compression.py:pack_4bit returns; each tensor owns its bytes (the staging is reused)
    parts = _hand_out(p_dev.view(torch.int8), p_lay, shapes, on_cpu, st, "p")
    return {name: (pt, sc) for name, pt, sc in zip(names, parts, scales)}


@_serialized
def _decode_dict_packed(items: List[Tuple[str, torch.Tensor, torch.Size, float]]) -> Dict[str, torch.Tensor]:
    """Decode packed int4 payloads (name, packed int8 [ceil(n/2)], original shape, scale)."""
    st = _staging()
    dev = st.device
    sizes = tuple(int(torch.Size(shape).numel()) for _, _, shape, _ in items)
    lay = st.layout(sizes, align=2)
    for (name, p, _, _), n in zip(items, sizes):
        if p.numel() != (n + 1) // 2:
            raise ValueError(f"PackedSLQChannel: '{name}' holds {p.numel()} packed bytes, expected {(n + 1) // 2}")
    # with align=2 every tensor's slot is exactly ceil(n/2) packed bytes: the gather is one concatenation
    p_lay = st.layout(tuple((n + 1) // 2 for n in sizes), align=1)
    p_dev = _stage_in([p.view(torch.uint8) for _, p, _, _ in items], p_lay, st, "dp", torch.uint8)
    s_dev = torch.tensor([s for _, _, _, s in items], dtype=torch.float32).to(dev, non_blocking=True)
    on_cpu = [not p.is_cuda for _, p, _, _ in items]
    out_dev = ops.decode_batched_int4(p_dev, s_dev, lay, out=st.buf("d_out", lay.total, torch.float32))
    decoded = _hand_out(out_dev, lay, [torch.Size(shape) for _, _, shape, _ in items], on_cpu, st, "d_out")
    return {name: t for (name, _, _, _), t in zip(items, decoded)}


@_serialized
def _encode_delta_dict(prevs: List[torch.Tensor], news: List[torch.Tensor], names: List[str], bits: int):
    """SLQ-encode news[k] - prevs[k] (fp32, ndim > 1, equal shapes) for every k without materialising the
    difference: {name: (qint8 tensor shaped like news[k] and on its device, python float scale)}.

    Device dicts: the kernels read the tensors through two pointer tables (no bucket of either source and none
    of the difference exists), the payload goes to a 64-element-aligned bucket, so separately allocated
    tensors take the 16-byte path, and the qint8 outputs are filled from it by one scatter launch. CPU or mixed
    dicts: each dict is staged as a compact device bucket (two H2D copies; diffing on the host inside the
    gather, to keep one, is not done), the same kernels run over the two buckets, and the payloads come back
    through the D2H + scatter path of _encode_dict."""
    st = _staging()
    dev = st.device
    sizes = tuple(int(t.numel()) for t in news)
    ptrs = _delta_on_device(prevs, news, dev)
    if ptrs is not None:
        lay = st.layout(sizes, align=ops.ALIGN_ELEMS)
        src_new, src_prev = news, prevs
    else:
        lay = st.layout(sizes, align=1)
        src_new = _stage_in(news, lay, st, "x", torch.float32)
        src_prev = _stage_in(prevs, lay, st, "x_prev", torch.float32)
    q_dev, s_dev = ops.encode_delta_batched(src_new, src_prev, lay, bits, ptrs=ptrs,
                                            q=st.buf("q", lay.total, torch.int8),
                                            scales=st.buf("scales", lay.ntensors, torch.float32),
                                            partials=st.buf("partials", lay.nchunks, torch.int32))
    return _payloads_out(names, news, lay, st, q_dev, s_dev)


@_serialized
def _encode_delta_dict_packed(prevs: List[torch.Tensor], news: List[torch.Tensor], names: List[str], bits: int):
    """Packed int4 variant of _encode_delta_dict: {name: (int8 tensor of ceil(n/2) packed bytes, scale)}."""
    st = _staging()
    dev = st.device
    th = _torchhost.get()
    host_ok, numel, hptrs = th.host_bytes(news, 4)   # sizes, and contiguous CPU fp32 storages, in one call
    sizes = tuple(numel.tolist())
    ptrs = _delta_on_device(prevs, news, dev)
    if ptrs is not None:
        lay = st.layout(sizes, align=ops.ALIGN_ELEMS)
        src_new, src_prev = news, prevs
    else:
        lay = st.layout(sizes, align=2)
        src_new = _stage_in(news, lay, st, "x", torch.float32,
                            host_ptrs=hptrs.numpy().view(np.uint64) if host_ok else None)
        src_prev = _stage_in(prevs, lay, st, "x_prev", torch.float32)
    p_dev, s_dev = ops.encode_delta_batched_int4(src_new, src_prev, lay, bits, ptrs=ptrs,
                                                 packed=st.buf("p", lay.total // 2, torch.uint8),
                                                 scales=st.buf("scales", lay.ntensors, torch.float32),
                                                 partials=st.buf("partials", lay.nchunks, torch.int32))
    return _packed_out(names, news, lay, st, p_dev, s_dev, host_ok, numel)


@_serialized
def _encode_delta_update_dict(hiddens: List[torch.Tensor], news: List[torch.Tensor], names: List[str], bits: int,
                              packed: bool):
    """SLQ-encode news[k] - hiddens[k] and, in the same launch, hiddens[k] += decode(payload) (_broadcast_groups'
    entries; ops.encode_delta_update_batched): the payloads of _encode_delta_dict (packed: _encode_delta_dict_packed)
    for the same pair, on news[k]'s device.

    The hidden tensors are read and written where they are, through their pointer table. `news` on the device:
    a second pointer table, nothing staged. `news` on the CPU (get_model_parameters hands out CPU dicts): staged
    into a 64-element-aligned bucket by one H2D copy. Either way the payload goes to a 64-element-aligned bucket
    and from there into the owned outputs: one scatter launch on the device, the D2H + scatter path on the CPU."""
    st = _staging()
    dev = st.device
    th = _torchhost.get()
    host_ok, numel, hptrs = th.host_bytes(news, 4)   # sizes, and contiguous CPU fp32 storages, in one call
    lay = st.layout(tuple(numel.tolist()), align=ops.ALIGN_ELEMS)
    ok_h, _, h_ptrs = th.device_ptrs(hiddens, dev.index, 4)
    if not ok_h:
        raise ValueError("broadcast_delta_: the fused hidden tensors must be contiguous fp32 tensors on the device")
    if news[0].is_cuda:
        ok_n, _, n_ptrs = th.device_ptrs(news, dev.index, 4)
        if not ok_n:
            raise ValueError("broadcast_delta_: the fused new tensors must be contiguous fp32 tensors on the device")
    else:
        x_dev = _stage_in(news, lay, st, "x", torch.float32,
                          host_ptrs=hptrs.numpy().view(np.uint64) if host_ok else None)
        n_ptrs = torch.from_numpy(x_dev.data_ptr() + 4 * lay.offsets)
    scales = st.buf("scales", lay.ntensors, torch.float32)
    partials = st.buf("partials", lay.nchunks, torch.int32)
    with torch.no_grad():
        if packed:
            p_dev, s_dev = ops.encode_delta_update_batched_int4(news, hiddens, lay, bits, ptrs=(n_ptrs, h_ptrs),
                                                                packed=st.buf("p", lay.total // 2, torch.uint8),
                                                                scales=scales, partials=partials)
            return _packed_out(names, news, lay, st, p_dev, s_dev, host_ok, numel)
        q_dev, s_dev = ops.encode_delta_update_batched(news, hiddens, lay, bits, ptrs=(n_ptrs, h_ptrs),
                                                       q=st.buf("q", lay.total, torch.int8), scales=scales,
                                                       partials=partials)
        return _payloads_out(names, news, lay, st, q_dev, s_dev)


class SLQChannel(_CodecChannel):
    """Bi-directional symmetric linear quantization (quant.py:15-112) on the MI355X HIP codec:
    ``simulate_bandwidth`` counts self.bits for weights, 32 bits for biases, 32 bits per scale (quant.py:47-58).

    ``receive_add_``: quantized tensors whose targets all live on the GPU (``_apply_groups``' rule) are decoded
    once and accumulated into every model by one launch (ops.dequantize_axpby_batched in place with alpha = beta
    = 1: the payload is read once, each model read and written once, no decoded tensor is materialised; the
    packed int4 channel unpacks in the same launch). ``receive_mean``: tensors quantized in every update are
    decoded and averaged by one launch of ops.dequantize_mean_batched."""

    def _receive(self, c_params: CompressedParameters) -> Tuple[Parameters, float]:
        assert isinstance(c_params, QuantParameters)
        s_time = time.perf_counter()
        names = list(c_params.params.keys())
        datas = [p.data for p in c_params.params.values()]
        th = _torchhost.get()
        kinds = th.payload_kinds(datas).numpy()   # _dequantize_tensor's cases for every entry in one call
        qi = np.nonzero(kinds == 1)[0].tolist()
        vals: List[Optional[torch.Tensor]] = [None] * len(names)
        rest_done = []

        def rest():   # every entry but the decoded ones; the host decode runs it while its copies land
            if rest_done:
                return
            rest_done.append(True)
            pi = np.nonzero(kinds == 0)[0].tolist()
            for i, t in zip(pi, th.variable_data([datas[i] for i in pi])):
                vals[i] = t  # passthrough: q_param.data.data (quant.py:111-112)
            for i in np.nonzero(kinds == 2)[0].tolist():
                vals[i] = datas[i].data.dequantize()  # non-quantized ndim > 1 payload: what quant.py:110 does

        decoded = _decode_dict([(names[i], datas[i]) for i in qi], idle=rest) if qi else {}
        for i in qi:
            vals[i] = decoded[names[i]]
        rest()
        return dict(zip(names, vals)), time.perf_counter() - s_time

    def _apply_payload(self, c_params: QuantParameters, names: List[str], st: _DeviceStaging):
        """The qint8 payloads of `names` (``_fusable`` entries) in an aligned device bucket, and the fused decode
        + axpby over it (ops.dequantize_axpby_batched)."""
        lay, q_dev, s_dev = self._stage_payload(c_params, names, st)
        return lay, lambda bases, outs, alpha, beta: ops.dequantize_axpby_batched(q_dev, s_dev, lay, bases, outs,
                                                                                 alpha, beta)

    @staticmethod
    def _stage_payload(c_params: QuantParameters, names: List[str], st: _DeviceStaging):
        qs = [c_params.params[n].data for n in names]
        lay = st.layout(tuple(int(q.numel()) for q in qs), align=ops.ALIGN_ELEMS)
        q_dev = _stage_in([_int8_view(q) for q in qs], lay, st, "ax_q", torch.int8)
        # q_scale() is a double; fbgemm's dequantize uses it as fp32 (quant.py:110)
        s_dev = torch.tensor([q.q_scale() for q in qs], dtype=torch.float32).to(st.device, non_blocking=True)
        return lay, q_dev, s_dev

    def _flush_payload(self, c_params: QuantParameters, names: List[str], st: _DeviceStaging):
        """The same staged bucket, and the fused decode + accumulate + flush over it
        (ops.dequantize_fedbuff_flush_batched / dequantize_fadas_flush_batched)."""
        lay, q_dev, s_dev = self._stage_payload(c_params, names, st)
        return lay, (lambda buf, g, out, K, factor, lr: ops.dequantize_fedbuff_flush_batched(
                         q_dev, s_dev, lay, buf, g, out, K, factor, lr),
                     lambda buf, g, m, v, h, out, K, scalars: ops.dequantize_fadas_flush_batched(
                         q_dev, s_dev, lay, buf, g, m, v, h, out, K, scalars))

    @staticmethod
    def _mean_host_updates(all_c_params: List[QuantParameters], names: List[str]):
        """receive_mean's common case in a few native calls: K updates of one model whose entries come in the
        same order, every ndim > 1 payload a non-empty per-tensor qint8 CPU tensor with zero point 0 of the same
        shape in every update. Returns (fused names, their means, the ndim <= 1 names) — the means from one
        decode-mean launch over rows staged straight from the payloads' storages, the outputs created by one
        native call per staging range — or None when the updates are anything else (receive_mean then
        classifies entry by entry)."""
        cls = SLQChannel._mean_host_classify(all_c_params, names)
        if cls is None:
            return None
        fused, plain, like, numel, ptrs, scales = cls
        if not fused:
            return [], [], plain
        return fused, _decode_mean_host(_staging(), like, numel, ptrs, scales), plain

    @staticmethod
    def _mean_host_classify(all_c_params: List[QuantParameters], names: List[str]):
        """_mean_host_updates' classification: (fused names, the ndim <= 1 names, the first update's fused
        payloads, their element counts, every update's payload pointers, the [K, T] fp32 scales), or None."""
        if any(list(c.params.keys()) != names for c in all_c_params):
            return None
        th = _torchhost.get()
        datas = [[p.data for p in c.params.values()] for c in all_c_params]
        kinds = np.stack([th.payload_kinds(d).numpy() for d in datas])
        if (kinds == 2).any() or (kinds != kinds[0]).any():
            return None
        idx = np.nonzero(kinds[0] == 1)[0].tolist()
        plain = [names[i] for i in np.nonzero(kinds[0] == 0)[0].tolist()]   # ndim <= 1 in every update
        if not idx:
            return [], plain, [], None, [], None
        qs = [[d[i] for i in idx] for d in datas]
        metas = [th.qint8_meta(q) for q in qs]   # (ok, all contiguous CPU, numel, fp32 scales, data pointers)
        numel = metas[0][2]
        if not all(m[0] and m[1] and torch.equal(m[2], numel) for m in metas) or int(numel.min()) == 0:
            return None
        if not th.shapes_equal(qs):
            return None
        return ([names[i] for i in idx], plain, qs[0], numel, [m[4].numpy().view(np.uint64) for m in metas],
                torch.stack([m[3] for m in metas]))

    def _mean_apply(self, all_c_params: List[QuantParameters], names: List[str], bases: List[torch.Tensor],
                    where: str, alpha: float, beta: float, host) -> List[torch.Tensor]:
        apply = (bases, where, alpha, beta)
        if host is not None:   # K CPU updates, classified natively: rows staged straight from the storages
            _, _, like, numel, ptrs, scales = host
            return _decode_mean_host(_staging(), like, numel, ptrs, scales, apply=apply)
        qs = [[c.params[n].data for n in names] for c in all_c_params]
        return _decode_mean(qs, [[q.q_scale() for q in c] for c in qs], [q.shape for q in qs[0]], packed=False,
                            apply=apply)

    @staticmethod
    def _passthrough(p: QuantParameter) -> bool:
        """_receive hands this entry back as its own payload tensor (quant.py:111-112)."""
        return isinstance(p.data, torch.Tensor) and p.data.ndim <= 1

    @staticmethod
    def _fusable(p: QuantParameter) -> bool:
        d = p.data
        return (d.dtype == torch.qint8 and d.ndim > 1 and d.numel() > 0
                and d.qscheme() == torch.per_tensor_affine and d.q_zero_point() == 0)

    def _mean_payloads(self, all_c_params: List[QuantParameters], names: List[str]) -> List[torch.Tensor]:
        qs = [[c.params[n].data for n in names] for c in all_c_params]
        # q_scale() is a double; fbgemm's dequantize uses it as fp32 (quant.py:110)
        return _decode_mean(qs, [[q.q_scale() for q in c] for c in qs], [q.shape for q in qs[0]], packed=False)

    def send_with_q_error(self, params: Parameters) -> Tuple[CompressedParameters, float, float, float]:
        """`on_client_send` fused with the worker's quantization-error metrics.

        Returns (c_params, c_time, q_error_mse, q_error_cos): the values
        Src/ADFL/Client/worker.py:176,186-189 gets from on_client_send, an extra on_server_receive and
        parameter_relative_mse / parameter_cosine_similarity(exclude_bias=True)
        (Src/ADFL/model.py:256-323), bit for bit: the decode stays on the device (no extra transfer) and
        the fp32 sums run in torch's CPU order with this process's torch.get_num_threads() (qerror.py).
        c_time covers the encode only, as on_client_send's does."""
        s_time = time.perf_counter()
        stats: list = []
        q_params = self._quantize_params(params, self.bits, stats)
        c_time = time.perf_counter() - s_time
        if not stats:  # nothing quantized: parameter_relative_mse returns 0.0; cosine of empty vectors raises
            raise RuntimeError("send_with_q_error: no ndim > 1 tensors to measure (torch.cat of an empty list)")
        e, s, c = stats[0]
        count = sum(int(p.numel()) for p in params.values() if p.ndim > 1)
        rel_mse, cos = qerror.metrics(e, s, c, count)
        return q_params, c_time, rel_mse, cos

    def send_delta(self, params_prev: Parameters, params_new: Parameters) -> Tuple[CompressedParameters, float]:
        """``on_client_send(diff_parameters(params_prev, params_new))`` — what every CommType.DELTA strategy
        sends (the clients, Src/ADFL/Client/async_sc.py:106-114,318-324; QAFeL's server,
        Src/ADFL/Server/qafel.py:160-161) — with the difference of the ndim > 1 tensors formed inside the encode
        kernels and never written (ops.encode_delta_batched). Returns (c_params, seconds); c_params equals the
        two-step result bit for bit and field for field (payload, scale, shape, dtypes, bits, size), in
        params_prev's key order (model.py:356). ndim <= 1 entries carry ``new - prev`` computed by torch on
        their own device, with scale 1. Neither input is modified. The same errors are raised: the key-set
        assertion, torch's for shapes that do not match, quantize's for an ndim > 1 entry that is empty or
        whose difference is not fp32."""
        s_time = time.perf_counter()
        q_params = self._quantize_delta(params_prev, params_new, self.bits)
        return q_params, time.perf_counter() - s_time

    def broadcast_delta_(self, hidden_state: Parameters,
                         params_new: Parameters) -> Tuple[CompressedParameters, float]:
        """``_CodecChannel.broadcast_delta_`` (QAFeL's broadcast: send_delta(hidden_state, params_new), then
        receive_add_(c_params, [hidden_state])) with the two fused for a device-resident hidden state: the ndim > 1
        entries ``_broadcast_groups`` names are encoded and their hidden tensors updated by the same launch
        (ops.encode_delta_update_batched: read g, read h, write the payload, write h — the payload never comes
        back in), whether params_new is on the device (pointer tables, nothing staged) or on the CPU (staged by
        one H2D copy). The payload tensors live where params_new's do, as with send_delta. ndim <= 1 entries
        keep torch's own statements (``new - prev`` with scale 1, then ``mul_(1).add_``); a CPU hidden state and
        every other entry take send_delta's encode and receive_add_'s update."""
        s_time = time.perf_counter()
        q_params = self._quantize_delta(hidden_state, params_new, self.bits, update=True)
        return q_params, time.perf_counter() - s_time

    _PACKED_DELTA = False   # PackedSLQChannel: the int4-packed delta encodes

    def _encode_delta_pairs(self, params_prev: Parameters, pairs, bits: int, update: bool):
        """({name: (payload, scale)} of _delta_pairs' ndim > 1 pairs, the names whose params_prev tensor the
        encode has already updated: broadcast_delta_'s fused entries, none without `update`)."""
        encoded: Dict[str, Tuple[torch.Tensor, float]] = {}
        if update and pairs:
            for grp in _broadcast_groups(params_prev, pairs, _staging().device):
                encoded.update(_encode_delta_update_dict([pairs[n][0] for n in grp], [pairs[n][1] for n in grp], grp,
                                                         bits, self._PACKED_DELTA))
        done = set(encoded)
        rest = [n for n in pairs if n not in done]
        if rest:
            enc = _encode_delta_dict_packed if self._PACKED_DELTA else _encode_delta_dict
            encoded.update(enc([pairs[n][0] for n in rest], [pairs[n][1] for n in rest], rest, bits))
        return encoded, done

    def _update_rest(self, params_prev: Parameters, out: Dict[str, QuantParameter], done) -> None:
        """broadcast_delta_'s entries the fused launch did not take: receive_add_ of their payloads."""
        rest = {n: p for n, p in out.items() if n not in done}
        if rest:
            self.receive_add_(QuantParameters(rest, 0), [{n: params_prev[n] for n in rest}])

    def _quantize_delta(self, params_prev: Parameters, params_new: Parameters, bits: int,
                        update: bool = False) -> QuantParameters:
        names, plain, pairs = _delta_pairs(params_prev, params_new)
        encoded, done = self._encode_delta_pairs(params_prev, pairs, bits, update)
        signs = torch.zeros(1, dtype=torch.uint8)  # the unused field (quant.py:91), one object per call
        qp = QuantParameter
        out: Dict[str, QuantParameter] = {}
        size = 0
        for n in names:
            # positional: QuantParameter(data, bits, scale, signs, shape, dtype, q_dtype) (model.py:21-31)
            if n in encoded:
                q, scale = encoded[n]
                out[n] = qp(q, bits, scale, signs, q.shape, torch.float32, torch.qint8)
                size += q.numel()             # a qint8 payload: one byte per element
            else:
                t = plain[n]                  # passthrough (quant.py:80-81: scale 1)
                out[n] = qp(t, bits, 1, signs, t.shape, t.dtype, t.dtype)
                size += t.nbytes
        if update:
            self._update_rest(params_prev, out, done)
        return QuantParameters(out, size)

    def _quantize_params(self, params: Parameters, bits: int, stats: Optional[list] = None) -> QuantParameters:
        """Biases and running metrics (ndim <= 1) are not quantized (quant.py:74-94)."""
        items = list(params.items())
        # every entry's ndim / numel / dtype / placement in one native call (adfl_torchhost.tensor_meta)
        ndim, numel, f32, host = (a.numpy() for a in _torchhost.get().tensor_meta([p for _, p in items]))
        qi = np.nonzero(ndim > 1)[0]
        names = [items[i][0] for i in qi.tolist()]
        bad = qi[(numel[qi] == 0) | ~f32[qi]]
        if bad.size:
            ops.require_quantizable(items[int(bad[0])][1])   # raises the reference's error for that tensor
        sizes = numel[qi].tolist()
        meta = (tuple(sizes), bool(host[qi].all()))
        signs = torch.zeros(1, dtype=torch.uint8)  # the unused field (quant.py:91), one object per call
        qp = QuantParameter
        made: Dict[str, QuantParameter] = {}
        size = [0]
        # positional: QuantParameter(data, bits, scale, signs, shape, dtype, q_dtype) (model.py:21-31)

        f32t, qint8 = torch.float32, torch.qint8

        def emit(k, q, scale):   # a quantized entry, built as soon as its output exists
            n = names[k]
            if n not in made:
                size[0] += sizes[k]           # a qint8 payload: one byte per element
            made[n] = qp(q, bits, scale, signs, q.shape, f32t, qint8)
        # passthrough entries (quant.py:80-81: scale 1), a batch per copy range
        idle = _passthrough_idle([items[i] for i in np.nonzero(ndim <= 1)[0].tolist()], made, size, bits, 1, signs)
        encoded = _encode_dict(params, names, bits, stats, emit=emit, idle=idle, meta=meta) if names else {}
        for k, n in enumerate(names):
            if n not in made:    # device dicts and the other staging paths: built here
                emit(k, *encoded[n])
        while idle():
            pass
        return QuantParameters({name: made[name] for name in params}, size[0])


class USLQChannel(_Unidirectional, SLQChannel):
    """Uni-directional SLQ (quant.py:115-137): only client -> server is quantized."""


class PackedSLQChannel(SLQChannel):
    """SLQ with the 4-bit payload actually packed two values per byte — the end-to-end int4 path the
    reference meant to provide but cannot run (Src/ADFL/compression.py:91-94 passes a qint8 tensor to
    pack_4bit and raises; its dequantize_tensor never unpacks, :71-74).

    Encode = SLQ quantize (bit-exact with SLQChannel(bits)) + pack_4bit's nibble layout
    (compression.py:35-48); decode = unpack_4bit (:51-66) + dequantize. Payload entries:
    QuantParameter(data = int8 tensor of ceil(n/2) packed bytes, bits, scale, shape = original shape,
    dtype = float32, q_dtype = int8) — what compression.quantize_params builds for bits == 4 (:86-110).
    bits must be <= 4 (larger codes do not fit a nibble). Values 127 from an all-zero / NaN tensor alias
    exactly as pack_4bit makes them alias (nibbles 7, -1); they dequantize to +-0.0 / NaN."""

    def __init__(self, bits: int) -> None:
        if not 1 <= bits <= 4:
            raise ValueError(f"PackedSLQChannel: bits must be in [1, 4], got {bits}")
        super().__init__(bits)

    @staticmethod
    def _is_packed(p: QuantParameter) -> bool:
        return p.dtype == torch.float32 and p.q_dtype == torch.int8 and len(p.shape) > 1 and p.data.ndim == 1

    def _receive(self, c_params: CompressedParameters) -> Tuple[Parameters, float]:
        assert isinstance(c_params, QuantParameters)
        s_time = time.perf_counter()
        packed = [(name, p.data, p.shape, p.scale) for name, p in c_params.params.items() if self._is_packed(p)]
        decoded = _decode_dict_packed(packed) if packed else {}
        params = {name: decoded[name] if name in decoded else p.data.data for name, p in c_params.params.items()}
        return params, time.perf_counter() - s_time

    def _fusable(self, p: QuantParameter) -> bool:
        return self._is_packed(p) and p.data.numel() == (torch.Size(p.shape).numel() + 1) // 2

    def _passthrough(self, p: QuantParameter) -> bool:
        return isinstance(p.data, torch.Tensor) and p.data.ndim <= 1 and not self._is_packed(p)

    def _apply_payload(self, c_params: QuantParameters, names: List[str], st: _DeviceStaging):
        """The packed int4 payloads of `names` in an aligned device bucket (element offsets multiples of 64, so
        tensor k's ceil(n/2) bytes start at offset / 2), and the fused unpack + decode + axpby over it."""
        lay, p_dev, s_dev = self._stage_payload(c_params, names, st)
        return lay, lambda bases, outs, alpha, beta: ops.dequantize_axpby_batched(p_dev, s_dev, lay, bases, outs,
                                                                                 alpha, beta, packed=True)

    @staticmethod
    def _stage_payload(c_params: QuantParameters, names: List[str], st: _DeviceStaging):
        ps = [c_params.params[n] for n in names]
        sizes = tuple(int(torch.Size(p.shape).numel()) for p in ps)
        lay = st.layout(sizes, align=ops.ALIGN_ELEMS)
        p_lay = st.layout(tuple((n + 1) // 2 for n in sizes), align=ops.ALIGN_ELEMS // 2)
        p_dev = _stage_in([p.data.view(torch.uint8) for p in ps], p_lay, st, "ax_p", torch.uint8)
        s_dev = torch.tensor([float(p.scale) for p in ps], dtype=torch.float32).to(st.device, non_blocking=True)
        return lay, p_dev, s_dev

    def _flush_payload(self, c_params: QuantParameters, names: List[str], st: _DeviceStaging):
        """The same staged packed bucket, and the fused unpack + decode + accumulate + flush over it."""
        lay, p_dev, s_dev = self._stage_payload(c_params, names, st)
        return lay, (lambda buf, g, out, K, factor, lr: ops.dequantize_fedbuff_flush_batched(
                         p_dev, s_dev, lay, buf, g, out, K, factor, lr, packed=True),
                     lambda buf, g, m, v, h, out, K, scalars: ops.dequantize_fadas_flush_batched(
                         p_dev, s_dev, lay, buf, g, m, v, h, out, K, scalars, packed=True))

    @staticmethod
    def _mean_host_updates(all_c_params: List[QuantParameters], names: List[str]):
        """Packed payloads are 1-D byte buffers whose shape lives in the payload object: the native
        classification of SLQChannel's qint8 updates does not apply (receive_mean classifies entry by entry)."""
        return None

    @staticmethod
    def _mean_host_classify(all_c_params: List[QuantParameters], names: List[str]):
        return None

    def _mean_payloads(self, all_c_params: List[QuantParameters], names: List[str]) -> List[torch.Tensor]:
        return self._mean_apply(all_c_params, names, None, None, 1.0, 1.0, None)

    def _mean_apply(self, all_c_params: List[QuantParameters], names: List[str], bases, where, alpha: float,
                    beta: float, host) -> List[torch.Tensor]:
        """bases None: the plain mean (_mean_payloads)."""
        return _decode_mean([[c.params[n].data for n in names] for c in all_c_params],
                            [[c.params[n].scale for n in names] for c in all_c_params],
                            [torch.Size(all_c_params[0].params[n].shape) for n in names], packed=True,
                            apply=None if bases is None else (bases, where, alpha, beta))

    _PACKED_DELTA = True

    def _quantize_delta(self, params_prev: Parameters, params_new: Parameters, bits: int,
                        update: bool = False) -> QuantParameters:
        names, plain, pairs = _delta_pairs(params_prev, params_new)
        encoded, done = self._encode_delta_pairs(params_prev, pairs, bits, update)
        signs = torch.zeros(1, dtype=torch.uint8)  # the unused field (compression.py:102), one object per call
        qp = QuantParameter
        out: Dict[str, QuantParameter] = {}
        size = 0
        for n in names:
            if n in encoded:
                q_param, scale = encoded[n]
                shape, dtype = pairs[n][1].shape, torch.float32
            else:
                q_param, scale = plain[n], 1
                shape, dtype = q_param.shape, q_param.dtype
            out[n] = qp(q_param, bits, scale, signs, shape, dtype, q_param.dtype)
            size += q_param.nbytes
        if update:
            self._update_rest(params_prev, out, done)
        return QuantParameters(out, size)

    def _quantize_params(self, params: Parameters, bits: int, stats: Optional[list] = None) -> QuantParameters:
        items = list(params.items())
        # every entry's ndim / numel / dtype in one native call (adfl_torchhost.tensor_meta)
        ndim, numel, f32, _ = (a.numpy() for a in _torchhost.get().tensor_meta([p for _, p in items]))
        qi = np.nonzero(ndim > 1)[0]
        names = [items[i][0] for i in qi.tolist()]
        bad = qi[(numel[qi] == 0) | ~f32[qi]]
        if bad.size:
            ops.require_quantizable(items[int(bad[0])][1])   # raises the reference's error for that tensor
        encoded = _encode_dict_packed(params, names, bits, stats) if names else {}
        signs = torch.zeros(1, dtype=torch.uint8)  # the unused field (compression.py:102), one object per call
        qp = QuantParameter
        out: Dict[str, QuantParameter] = {}
        size = 0
        for name, param in items:
            q_param, scale = encoded[name] if name in encoded else (param, 1)
            # positional: QuantParameter(data, bits, scale, signs, shape, dtype, q_dtype) (model.py:21-31)
            out[name] = qp(q_param, bits, scale, signs, param.shape, param.dtype, q_param.dtype)
            size += q_param.nbytes
        return QuantParameters(out, size)


HipSLQChannel = SLQChannel
HipUSLQChannel = USLQChannel
