"""Device-resident stochastic codec ops (QSGD / RQSGD / CNAT) over the HIP C ABI (include/adfl_stoch.h).

Every function takes and returns CUDA (HIP) tensors over a bucketed flat buffer described by an
``ops.BucketLayout``, launches on the current stream and never synchronises:

* ``qsgd_encode_batched`` / ``qsgd_decode_batched``   — QSGDChannel._quantize_tensor / _dequantize_tensor
  (Src/ADFL/Channel/quant.py:223-252)
* ``rqsgd_encode_batched`` / ``rqsgd_decode_batched`` — RQSGDChannel (quant.py:364-398)
* ``cnat_encode_batched`` / ``cnat_decode_batched``   — CNATChannel (quant.py:509-545)
* ``rqsgd_encode_delta_batched`` — RQSGD of ``new - prev`` from two sources; ``rqsgd_encode_delta_update_batched``
  / ``qsgd_quantize_update_batched`` — QAFeL's broadcast: the encode that also leaves ``hidden += decode(payload)``
* ``norms_batched`` — per-tensor ||x||_2 or (max|x|, min|x|); ``qsgd_quantize_batched`` — levels from
  given norms (what the parity tests use to inject the reference's own norm)
* ``quantize_packed_batched`` / ``encode_packed_batched`` / ``dequantize_packed_batched`` /
  ``dequantize_axpby_packed_batched`` — QSGD / RQSGD over the packed planes, bits + 1 bits per weight
  (``packed_plane_bytes``; DESIGN.md §10 "Packed wire format")

Randomness: pass ``uniforms`` (fp32 plane indexed like x, values in [0, 1)) to inject the reference's
``torch.rand_like`` draws, or leave it None to draw from the Philox4x32-7 stream ``(seed, counter)``.
``RngStream`` hands out (seed, counter) pairs seeded from torch's default CPU generator, so
``torch.manual_seed`` makes a run reproducible the way it does for the reference.
"""

import os
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import (CODEC_CNAT, CODEC_QSGD, CODEC_RQSGD, DTYPE_BF16, DTYPE_F16, DTYPE_F32, DTYPE_F64, NORM_L2, NORM_L2_TORCH,
                   NORM_LINF, check)
from .ops import BucketLayout, _dev, _stream

__all__ = ["RngStream", "norms_batched", "qsgd_quantize_batched", "qsgd_encode_batched", "rqsgd_encode_batched",
           "qsgd_decode_batched", "rqsgd_decode_batched", "cnat_encode_batched", "cnat_decode_batched",
           "philox_uniforms", "workspace", "rqsgd_encode_delta_batched",
           "rqsgd_encode_delta_update_batched", "qsgd_quantize_update_batched",
           "torch_norms", "NORM_L2", "NORM_LINF", "NORM_L2_TORCH", "DT_DTYPES", "encode_batched_dt",
           "quantize_batched_dt", "norms_batched_dt", "philox_uniforms_dt", "dequantize_mean_batched",
           "packed_plane_bytes", "quantize_packed_batched", "encode_packed_batched", "dequantize_packed_batched",
           "dequantize_axpby_packed_batched"]


class RngStream:
    """(seed, counter) pairs for successive encode calls. The seed is drawn from torch's default CPU
    generator at construction (the generator the reference's torch.rand_like consumes); each call
    advances the counter past the uniforms it used, so no two calls share a uniform."""

    def __init__(self, seed: Optional[int] = None):
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
        self.seed = int(seed) & (2 ** 64 - 1)
        self.counter = 0

    def take(self, numel: int) -> Tuple[int, int]:
        c = self.counter
        self.counter += (int(numel) + 3) // 4
        return self.seed, c


def workspace(layout: BucketLayout, device) -> torch.Tensor:
    return torch.empty(int(_lib.load().adfl_stoch_workspace_bytes(layout.nchunks)), dtype=torch.uint8, device=device)


def _check_flat(flat: torch.Tensor, layout: BucketLayout) -> torch.Tensor:
    if flat.dtype != torch.float32:
        raise ValueError(f"adfl_amd.stoch: the HIP stochastic codecs take fp32 buckets, got {flat.dtype}")
    flat = _dev(flat, "flat")
    if flat.numel() < layout.total:
        raise ValueError("adfl_amd.stoch: flat buffer smaller than the layout")
    return flat


def _uniforms(u: Optional[torch.Tensor], layout: BucketLayout) -> int:
    if u is None:
        return 0
    if u.dtype != torch.float32 or u.numel() < layout.total:
        raise ValueError("adfl_amd.stoch: uniforms must be an fp32 plane covering the layout")
    if not u.is_cuda or not u.is_contiguous() or u.data_ptr() % 16:
        raise ValueError("adfl_amd.stoch: uniforms must be a contiguous, 16-byte aligned device tensor")
    return u.data_ptr()


def _ws(ws: Optional[torch.Tensor], layout: BucketLayout, dev) -> torch.Tensor:
    return workspace(layout, dev) if ws is None else ws


def _work(layout: BucketLayout, dev, resident: Optional[bool] = None):
    """(work list pointer, count) for the *_encode_batched_work entries: the one-launch register-resident
    encode when every tensor of the layout fits a block (layout.nwork > 0), else (any, 0) = multi-launch.
    ADFL_STOCH_RESIDENT=0 in the environment forces the multi-launch path (A/B runs)."""
    if resident is None:
        resident = os.environ.get("ADFL_STOCH_RESIDENT", "1") != "0"
    if not resident or layout.nwork == 0:
        return 0, 0
    return layout.device_work(dev).data_ptr(), layout.nwork


def norms_batched(flat: torch.Tensor, layout: BucketLayout, mode: int = NORM_L2, *,
                  norms: Optional[torch.Tensor] = None, mins: Optional[torch.Tensor] = None,
                  ws: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """Per-tensor ||x||_2 (mode NORM_L2: fp64 accumulation, correctly rounded; NORM_L2_TORCH: torch's own
    fp32 reduction order, bit-identical to the reference's norm, sequential per tensor) or
    (max|x|, min|x|) (NORM_LINF)."""
    flat = _check_flat(flat, layout)
    dev = flat.device
    norms = torch.empty(layout.ntensors, dtype=torch.float32, device=dev) if norms is None else norms
    if mode == NORM_LINF and mins is None:
        mins = torch.empty(layout.ntensors, dtype=torch.float32, device=dev)
    ws = _ws(ws, layout, dev)
    check(_lib.load().adfl_stoch_norms_batched(flat.data_ptr(), layout.device_chunks(dev).data_ptr(), layout.nchunks,
                                               mode, ws.data_ptr(), ws.numel(), norms.data_ptr(),
                                               mins.data_ptr() if mins is not None else None, _stream(dev)))
    return norms, mins


def torch_norms(flat: torch.Tensor, layout: BucketLayout, *, norms: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-tensor ||x||_2 of an fp32 bucket bit-identical to torch's CPU vector_norm (the reference's QSGD /
    CNAT norm, quant.py:226,512): reference_norms' fp32 output. Same bits as norms_batched(...,
    NORM_L2_TORCH), the in-order kernel."""
    flat = _check_flat(flat, layout)
    norms = torch.empty(layout.ntensors, dtype=torch.float32, device=flat.device) if norms is None else norms
    reference_norms(flat, layout, out32=_dev(norms, "norms"))
    return norms


_REF_NORM_DTYPES = {torch.float32: DTYPE_F32, torch.float16: DTYPE_F16, torch.bfloat16: DTYPE_BF16,
                    torch.float64: DTYPE_F64}


def reference_norms(flat: torch.Tensor, layout: BucketLayout, *, threads: Optional[int] = None,
                    out64: Optional[torch.Tensor] = None, out32: Optional[torch.Tensor] = None):
    """Per-tensor ``torch.linalg.vector_norm(x, ord=2)`` of an fp32 / fp16 / bf16 / fp64 bucket, bit-identical
    to torch 2.10's CPU kernel — the reference's QSGD / CNAT norm in the tensor's own dtype (quant.py:226,512)
    — by adfl_torch_norms (csrc/torch_norm.hip: phases with no cross-block waits).

    threads: the torch.get_num_threads() whose fp16 split is reproduced (default: this process's, which is
    what the reference's own call would use). Returns (out64, out32): fp64 norms (the dtype's exact value)
    and fp32 ones; pass either to fill it (the other stays None unless passed too); with neither, out64 is
    allocated."""
    if flat.dtype not in _REF_NORM_DTYPES:
        raise ValueError(f"adfl_amd.stoch: reference_norms takes fp32 / fp16 / bf16 / fp64 buckets, got {flat.dtype}")
    flat = _dev(flat, "flat")
    if flat.numel() < layout.total:
        raise ValueError("adfl_amd.stoch: flat buffer smaller than the layout")
    dev = flat.device
    if out64 is None and out32 is None:
        out64 = torch.empty(layout.ntensors, dtype=torch.float64, device=dev)
    for o, dt in ((out64, torch.float64), (out32, torch.float32)):
        if o is not None and (o.dtype != dt or o.numel() < layout.ntensors or not o.is_contiguous() or o.device != dev):
            raise ValueError(f"adfl_amd.stoch: norm outputs must be contiguous {dt} device tensors of >= ntensors")
    if layout.nchunks == 0:
        return out64, out32
    L = _lib.load()
    threads = torch.get_num_threads() if threads is None else int(threads)
    if threads < 1:
        raise ValueError("adfl_amd.stoch: threads must be >= 1")
    if flat.dtype == torch.float16:   # at::parallel_for splits a tensor into at most ceil(n / GRAIN) pieces
        threads = min(threads, max(1, -(-int(max(layout.sizes)) // 32768)))
    short_max = L.adfl_torch_norm_short_max_dt(_REF_NORM_DTYPES[flat.dtype])
    kinds = (1 if min(layout.sizes) <= short_max else 0) | (2 if max(layout.sizes) > short_max else 0)
    need = L.adfl_torch_norm_scratch_bytes(layout.nchunks, layout.ntensors)
    scratch = torch.empty(need, dtype=torch.uint8, device=dev)  # stream-ordered: no initialisation needed
    check(L.adfl_torch_norms_work(_REF_NORM_DTYPES[flat.dtype], flat.data_ptr(), layout.device_chunks(dev).data_ptr(),
                                  layout.nchunks, layout.device_tfirst(dev).data_ptr(), layout.ntensors, kinds, threads,
                                  scratch.data_ptr(), need, out64.data_ptr() if out64 is not None else None,
                                  out32.data_ptr() if out32 is not None else None, _stream(dev)))
    return out64, out32


def _planes(layout, dev, levels, signs, ldtype):
    levels = torch.empty(layout.total, dtype=ldtype, device=dev) if levels is None else levels
    signs = torch.empty(layout.total, dtype=torch.int8, device=dev) if signs is None else signs
    return levels, signs


def qsgd_quantize_batched(flat: torch.Tensor, layout: BucketLayout, bits: int, norms: torch.Tensor, *,
                          uniforms: Optional[torch.Tensor] = None, seed: int = 0, counter: int = 0,
                          levels: Optional[torch.Tensor] = None,
                          signs: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Levels + signs from given per-tensor norms (QSGD: L2 norms; RQSGD: max|x|)."""
    flat = _check_flat(flat, layout)
    dev = flat.device
    levels, signs = _planes(layout, dev, levels, signs, torch.uint8)
    check(_lib.load().adfl_qsgd_quantize_batched(flat.data_ptr(), layout.device_chunks(dev).data_ptr(),
                                                 layout.nchunks, bits, _dev(norms, "norms").data_ptr(),
                                                 _uniforms(uniforms, layout), seed, counter, levels.data_ptr(),
                                                 signs.data_ptr(), _stream(dev)))
    return levels, signs


def qsgd_encode_batched(flat: torch.Tensor, layout: BucketLayout, bits: int, *,
                        uniforms: Optional[torch.Tensor] = None, seed: int = 0, counter: int = 0,
                        levels: Optional[torch.Tensor] = None, signs: Optional[torch.Tensor] = None,
                        norms: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None,
                        torch_norm: bool = False, resident: Optional[bool] = None):
    """QSGD encode of every tensor of a bucket: (levels u8, signs i8, L2 norms f32). torch_norm=True takes
    the norm in torch's reduction order (the reference's norm bit for bit: reference_norms, then the
    given-norm quantize); False, the one-launch encode's correctly rounded norm.
    resident: None = the one-launch register-resident encode whenever the layout allows it (same bytes as
    the multi-launch path), False = always the multi-launch path."""
    flat = _check_flat(flat, layout)
    dev = flat.device
    levels, signs = _planes(layout, dev, levels, signs, torch.uint8)
    norms = torch.empty(layout.ntensors, dtype=torch.float32, device=dev) if norms is None else norms
    ws = _ws(ws, layout, dev)
    if torch_norm:
        reference_norms(flat, layout, out32=norms)
        qsgd_quantize_batched(flat, layout, bits, norms, uniforms=uniforms, seed=seed, counter=counter,
                              levels=levels, signs=signs)
        return levels, signs, norms
    check(_lib.load().adfl_qsgd_encode_batched_work(flat.data_ptr(), layout.device_chunks(dev).data_ptr(),
                                                    layout.nchunks, *_work(layout, dev, resident), bits,
                                                    _uniforms(uniforms, layout), seed, counter, ws.data_ptr(),
                                                    ws.numel(), levels.data_ptr(), signs.data_ptr(), norms.data_ptr(),
                                                    _stream(dev)))
    return levels, signs, norms


def rqsgd_encode_batched(flat: torch.Tensor, layout: BucketLayout, bits: int, *,
                         uniforms: Optional[torch.Tensor] = None, seed: int = 0, counter: int = 0,
                         levels: Optional[torch.Tensor] = None, signs: Optional[torch.Tensor] = None,
                         norms: Optional[torch.Tensor] = None, mins: Optional[torch.Tensor] = None,
                         ws: Optional[torch.Tensor] = None, resident: Optional[bool] = None):
    """RQSGD encode: (levels u8, signs i8, max|x| norms f32, min|x| factors f32). resident as for QSGD."""
    flat = _check_flat(flat, layout)
    dev = flat.device
    levels, signs = _planes(layout, dev, levels, signs, torch.uint8)
    norms = torch.empty(layout.ntensors, dtype=torch.float32, device=dev) if norms is None else norms
    mins = torch.empty(layout.ntensors, dtype=torch.float32, device=dev) if mins is None else mins
    ws = _ws(ws, layout, dev)
    check(_lib.load().adfl_rqsgd_encode_batched_work(flat.data_ptr(), layout.device_chunks(dev).data_ptr(),
                                                     layout.nchunks, *_work(layout, dev, resident), bits,
                                                     _uniforms(uniforms, layout), seed, counter, ws.data_ptr(),
                                                     ws.numel(), levels.data_ptr(), signs.data_ptr(),
                                                     norms.data_ptr(), mins.data_ptr(), _stream(dev)))
    return levels, signs, norms, mins


def _delta_f32(src, what: str) -> None:
    for x in ([src] if isinstance(src, torch.Tensor) else list(src)):
        if isinstance(x, torch.Tensor) and x.dtype != torch.float32:
            raise ValueError(f"adfl_amd.stoch: the two-source encode takes fp32 sources, `{what}` holds {x.dtype}")


def _ushift(ushift, layout: BucketLayout, dev):
    """The per-tensor uniform-index shifts as (device int64 tensor or None: no shift, host array or 0), after the check the C ABI
    cannot make: every tensor's first uniform index, offset + shift, must be >= 0."""
    if ushift is None:
        return None, 0
    us = np.ascontiguousarray(ushift.cpu().numpy() if isinstance(ushift, torch.Tensor) else ushift, dtype=np.int64)
    cache = layout.__dict__.setdefault("_ushift_dev", {})   # the last shifts used with this layout, already checked
    key = (us.tobytes(), dev.index)
    if key not in cache:
        if us.shape != (layout.ntensors,):
            raise ValueError(f"adfl_amd.stoch: ushift must hold one int64 per tensor ({layout.ntensors}), got {us.shape}")
        if ((layout.offsets + us) < 0).any():
            raise ValueError("adfl_amd.stoch: ushift puts a tensor's first uniform index below 0")
        cache.clear()
        cache[key] = torch.from_numpy(us).to(dev)
    return cache[key], us


def _rqsgd_delta(entry: str, n_tab, p_tab, dev, layout: BucketLayout, bits: int, ushift, uniforms, seed, counter,
                 levels, signs, norms, mins, ws, work):
    """The shared tail of rqsgd_encode_delta_batched / rqsgd_encode_delta_update_batched: the checks the C ABI
    cannot make, the outputs, and the launch of `entry`."""
    us, us_host = _ushift(ushift, layout, dev)
    if uniforms is not None:
        top = int((layout.offsets + layout.sizes + us_host).max())
        if uniforms.dtype != torch.float32 or uniforms.numel() < top:
            raise ValueError("adfl_amd.stoch: uniforms must be an fp32 plane covering the shifted layout")
        if not uniforms.is_cuda or not uniforms.is_contiguous() or uniforms.data_ptr() % 16:
            raise ValueError("adfl_amd.stoch: uniforms must be a contiguous, 16-byte aligned device tensor")
    levels, signs = _planes(layout, dev, levels, signs, torch.uint8)
    norms = torch.empty(layout.ntensors, dtype=torch.float32, device=dev) if norms is None else norms
    mins = torch.empty(layout.ntensors, dtype=torch.float32, device=dev) if mins is None else mins
    ws = _ws(ws, layout, dev)
    check(getattr(_lib.load(), entry)(
        n_tab.data_ptr(), p_tab.data_ptr(), layout.device_chunks(dev).data_ptr(), layout.nchunks,
        *work, bits, uniforms.data_ptr() if uniforms is not None else None,
        us.data_ptr() if us is not None else None, seed, counter, ws.data_ptr(), ws.numel(), levels.data_ptr(),
        signs.data_ptr(), norms.data_ptr(), mins.data_ptr(), _stream(dev)))
    return levels, signs, norms, mins


# rqsgd_encode_delta_update_batched over a resident-eligible layout with resident=None: "resident" (one launch, h
# re-read stage by stage) or "twopass". DESIGN.md §10 has the measurement that chose it.
_UPDATE_RESIDENT_FORM = "resident"


def rqsgd_encode_delta_update_batched(new, hidden, layout: BucketLayout, bits: int, *, ptrs=None, ushift=None,
                                      uniforms: Optional[torch.Tensor] = None, seed: int = 0, counter: int = 0,
                                      levels: Optional[torch.Tensor] = None, signs: Optional[torch.Tensor] = None,
                                      norms: Optional[torch.Tensor] = None, mins: Optional[torch.Tensor] = None,
                                      ws: Optional[torch.Tensor] = None, resident: Optional[bool] = None):
    """QAFeL's broadcast (Src/ADFL/Server/qafel.py:156-180) for RQSGD: ``rqsgd_encode_delta_batched(new, hidden)``
    and, in place, ``hidden += rqsgd_decode(payload)`` — per element fp32(h + d), d the decode kernel's value for
    the stored level and sign bytes under the tensor's max and min (+0 for a zero norm, still added) —
    bit-identical to the encode followed by rqsgd_decode_batched and an fp32 add
    (adfl_rqsgd_encode_delta_update_batched_work). Sources, ushift, uniforms and outputs as
    rqsgd_encode_delta_batched takes them; `hidden` must be writable fp32 on the device (a contiguous flat buffer
    in `layout`, or a list of contiguous tensors of its sizes), must not overlap `new`, and is the only thing
    modified besides the outputs. resident: None = the form measured faster where both apply
    (_UPDATE_RESIDENT_FORM), True = the one launch whenever the layout allows it, False = the two passes; the
    same bytes. ptrs: see ops._delta_tables."""
    from .ops import _delta_nwork, _update_tables
    if ptrs is None:
        _delta_f32(new, "new")
        _delta_f32(hidden, "hidden")
    dev, n_tab, h_tab, _keep = _update_tables(new, hidden, layout, ptrs, "rqsgd_encode_delta_update_batched")
    if resident is None and _UPDATE_RESIDENT_FORM != "resident":
        resident = False
    work = _work(layout, dev, resident) if _delta_nwork(layout) else (0, 0)
    return _rqsgd_delta("adfl_rqsgd_encode_delta_update_batched_work", n_tab, h_tab, dev, layout, bits, ushift,
                        uniforms, seed, counter, levels, signs, norms, mins, ws, work)


def qsgd_quantize_update_batched(flat: torch.Tensor, layout: BucketLayout, bits: int, norms: torch.Tensor, hidden, *,
                                 ptrs=None, uniforms: Optional[torch.Tensor] = None, seed: int = 0, counter: int = 0,
                                 levels: Optional[torch.Tensor] = None,
                                 signs: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """QAFeL's broadcast for QSGD under given norms: ``qsgd_quantize_batched(flat, ...)`` over the difference
    bucket flat = new - hidden (ops.bucket_diff) and, in place, ``hidden += qsgd_decode(payload)`` — fp32(h + d)
    per element, bit-identical to the quantize followed by qsgd_decode_batched and an fp32 add
    (adfl_qsgd_quantize_update_batched). `hidden`: a contiguous flat fp32 device buffer in `layout` or a list of
    contiguous fp32 device tensors of its sizes, any addresses, not overlapping `flat`; the only thing modified
    besides the outputs. ptrs: hidden's data pointers as a CPU int64 tensor when the caller has checked the list."""
    from .ops import _delta_sources
    flat = _check_flat(flat, layout)
    dev = flat.device
    if ptrs is not None:
        if len(hidden) != layout.ntensors:
            raise ValueError(f"qsgd_quantize_update_batched: {len(hidden)} tensors for a layout of {layout.ntensors}")
        h_tab = ptrs.to(dev, non_blocking=True)
    else:
        _delta_f32(hidden, "hidden")
        if isinstance(hidden, torch.Tensor) and not hidden.is_contiguous():
            raise ValueError("qsgd_quantize_update_batched: hidden must be contiguous (it is updated in place)")
        h_tab, _keep = _delta_sources(hidden, layout, dev, "hidden")
    levels, signs = _planes(layout, dev, levels, signs, torch.uint8)
    check(_lib.load().adfl_qsgd_quantize_update_batched(flat.data_ptr(), layout.device_chunks(dev).data_ptr(),
                                                        layout.nchunks, bits, _dev(norms, "norms").data_ptr(),
                                                        _uniforms(uniforms, layout), seed, counter, levels.data_ptr(),
                                                        signs.data_ptr(), h_tab.data_ptr(), layout.ntensors,
                                                        _stream(dev)))
    return levels, signs


def rqsgd_encode_delta_batched(new, prev, layout: BucketLayout, bits: int, *, ptrs=None, ushift=None,
                               uniforms: Optional[torch.Tensor] = None, seed: int = 0, counter: int = 0,
                               levels: Optional[torch.Tensor] = None, signs: Optional[torch.Tensor] = None,
                               norms: Optional[torch.Tensor] = None, mins: Optional[torch.Tensor] = None,
                               ws: Optional[torch.Tensor] = None, resident: Optional[bool] = None):
    """``rqsgd_encode_batched`` of ``new - prev`` without writing the difference (adfl_rqsgd_encode_delta_batched_work):
    (levels u8, signs i8, max|x| norms f32, min|x| factors f32) in `layout`, bit-identical to the two steps.
    `new` / `prev`: two flat fp32 device buffers in `layout`, or two lists of fp32 device tensors of its sizes
    (validated as ops.encode_delta_batched validates them; any addresses). ushift: per tensor, the element at
    layout index g draws uniform g + ushift[t] (the Philox word, or uniforms[g + ushift[t]]) — with the planes
    in a 64-aligned layout and ushift = compact offset - aligned offset the payload is the compact layout's.
    Injected `uniforms` cover the indices the shifted elements use. resident: as for the other encodes (None =
    the one-launch form whenever every tensor of the layout fits a block, False = always the two passes; the
    same bytes).
    ptrs: see ops._delta_tables."""
    from .ops import _delta_device, _delta_nwork, _delta_tables
    if ptrs is None:   # a caller that passes `ptrs` has checked its lists (the channel: fp32 by _delta_pairs)
        _delta_f32(new, "new")
        _delta_f32(prev, "prev")
    dev = _delta_device(new, prev)
    n_tab, p_tab, _keep = _delta_tables(new, prev, layout, dev, ptrs)
    # the work list is the resident encodes' (ADFL_SLQ_RESIDENT_CHUNKS); the delta kernel takes tensors up to
    # ADFL_SLQ_DELTA_RESIDENT_CHUNKS, so a layout beyond that bound runs the two passes (ops._delta_nwork's guard)
    work = _work(layout, dev, resident) if _delta_nwork(layout) else (0, 0)
    return _rqsgd_delta("adfl_rqsgd_encode_delta_batched_work", n_tab, p_tab, dev, layout, bits, ushift, uniforms,
                        seed, counter, levels, signs, norms, mins, ws, work)


def qsgd_decode_batched(levels: torch.Tensor, signs: torch.Tensor, norms: torch.Tensor, layout: BucketLayout,
                        bits: int, *, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    levels, signs = _dev(levels, "levels"), _dev(signs, "signs")
    dev = levels.device
    out = torch.empty(layout.total, dtype=torch.float32, device=dev) if out is None else out
    check(_lib.load().adfl_qsgd_dequantize_batched(levels.data_ptr(), signs.data_ptr(),
                                                   layout.device_chunks(dev).data_ptr(), layout.nchunks, bits,
                                                   _dev(norms, "norms").data_ptr(), out.data_ptr(), _stream(dev)))
    return out


def rqsgd_decode_batched(levels: torch.Tensor, signs: torch.Tensor, norms: torch.Tensor, mins: torch.Tensor,
                         layout: BucketLayout, bits: int, *, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    levels, signs = _dev(levels, "levels"), _dev(signs, "signs")
    dev = levels.device
    out = torch.empty(layout.total, dtype=torch.float32, device=dev) if out is None else out
    check(_lib.load().adfl_rqsgd_dequantize_batched(levels.data_ptr(), signs.data_ptr(),
                                                    layout.device_chunks(dev).data_ptr(), layout.nchunks, bits,
                                                    _dev(norms, "norms").data_ptr(), _dev(mins, "mins").data_ptr(),
                                                    out.data_ptr(), _stream(dev)))
    return out


def cnat_encode_batched(flat: torch.Tensor, layout: BucketLayout, bits: int, *,
                        uniforms: Optional[torch.Tensor] = None, seed: int = 0, counter: int = 0,
                        exps: Optional[torch.Tensor] = None, signs: Optional[torch.Tensor] = None,
                        norms: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None,
                        torch_norm: bool = False, resident: Optional[bool] = None):
    """CNAT encode (x read once; resident as for QSGD): (exponents i8, signs i8, L2 norms f32). A tensor
    whose norm is 0 gets the reference's zero-branch bytes (0 / 1). torch_norm=True then replaces the norms
    with torch's own (the exponents do not depend on the norm; both norms are 0 for exactly the same tensors)."""
    flat = _check_flat(flat, layout)
    dev = flat.device
    exps, signs = _planes(layout, dev, exps, signs, torch.int8)
    norms = torch.empty(layout.ntensors, dtype=torch.float32, device=dev) if norms is None else norms
    ws = _ws(ws, layout, dev)
    check(_lib.load().adfl_cnat_encode_batched_work(flat.data_ptr(), layout.device_chunks(dev).data_ptr(),
                                                    layout.nchunks, *_work(layout, dev, resident), bits,
                                                    _uniforms(uniforms, layout), seed, counter, ws.data_ptr(),
                                                    ws.numel(), exps.data_ptr(), signs.data_ptr(), norms.data_ptr(),
                                                    _stream(dev)))
    if torch_norm:
        reference_norms(flat, layout, out32=norms)
    return exps, signs, norms


def cnat_decode_batched(exps: torch.Tensor, signs: torch.Tensor, norms: torch.Tensor, layout: BucketLayout, *,
                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
    exps, signs = _dev(exps, "exps"), _dev(signs, "signs")
    dev = exps.device
    out = torch.empty(layout.total, dtype=torch.float32, device=dev) if out is None else out
    check(_lib.load().adfl_cnat_dequantize_batched(exps.data_ptr(), signs.data_ptr(),
                                                   layout.device_chunks(dev).data_ptr(), layout.nchunks,
                                                   _dev(norms, "norms").data_ptr(), out.data_ptr(), _stream(dev)))
    return out


def philox_uniforms(n: int, seed: int, counter: int, start: int = 0, *, device=None) -> torch.Tensor:
    """The uniforms elements start .. start+n-1 of stream (seed, counter) draw."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    out = torch.empty(n, dtype=torch.float32, device=dev)
    check(_lib.load().adfl_philox_uniforms(out.data_ptr(), n, start, seed & (2 ** 64 - 1), counter, _stream(dev)))
    return out


# ------------------------------------------------------------------------------------------------
def dequantize_mean_batched(codec: str, levels: torch.Tensor, signs: torch.Tensor, norms: torch.Tensor,
                            layout: BucketLayout, bits: int, *, mins: Optional[torch.Tensor] = None,
                            out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """simple_aggregate of K clients' decodes in one launch (adfl_stoch_dequantize_mean_batched): levels /
    signs are [K, row] byte planes (uint8 / int8; row >= layout.total, a multiple of 16), norms (RQSGD: mins)
    [K, ntensors] fp32. Returns the fp32 mean bucket."""
    if codec not in _CODEC_IDS:
        raise ValueError(f"adfl_amd.stoch: codec must be one of {sorted(_CODEC_IDS)}, got {codec!r}")
    levels, signs, norms = _dev(levels, "levels"), _dev(signs, "signs"), _dev(norms, "norms")
    if levels.dim() != 2 or signs.shape != levels.shape or levels.element_size() != 1 or signs.element_size() != 1:
        raise ValueError("adfl_amd.stoch: levels / signs must be [K, row] byte planes of one shape")
    k, row = levels.shape
    if row < layout.total or not levels.is_contiguous() or not signs.is_contiguous():
        raise ValueError(f"adfl_amd.stoch: rows of {row} bytes cannot hold the {layout.total}-element bucket")
    if norms.shape != (k, layout.ntensors) or norms.dtype != torch.float32 or not norms.is_contiguous():
        raise ValueError(f"adfl_amd.stoch: norms must be contiguous fp32 [{k}, {layout.ntensors}]")
    if codec == "rqsgd":
        if mins is None:
            raise ValueError("adfl_amd.stoch: RQSGD needs mins")
        mins = _dev(mins, "mins")
        if mins.shape != norms.shape or mins.dtype != torch.float32 or not mins.is_contiguous():
            raise ValueError("adfl_amd.stoch: mins must match norms")
    dev = levels.device
    out = torch.empty(layout.total, dtype=torch.float32, device=dev) if out is None else out
    if out.dtype != torch.float32 or out.numel() < layout.total or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"adfl_amd.stoch: out must be a contiguous fp32 device tensor of >= {layout.total}")
    check(_lib.load().adfl_stoch_dequantize_mean_batched(
        _CODEC_IDS[codec], levels.data_ptr(), signs.data_ptr(), row, k, layout.device_chunks(dev).data_ptr(),
        layout.nchunks, bits, norms.data_ptr(), mins.data_ptr() if mins is not None else None, layout.ntensors,
        out.data_ptr(), _stream(dev)))
    return out


# fp16 / bf16 / fp64 buckets (include/adfl_stoch.h *_dt): the reference's arithmetic in the tensor's dtype
# ------------------------------------------------------------------------------------------------
DT_DTYPES = {torch.float16: DTYPE_F16, torch.bfloat16: DTYPE_BF16, torch.float64: DTYPE_F64}
_CODEC_IDS = {"qsgd": CODEC_QSGD, "rqsgd": CODEC_RQSGD, "cnat": CODEC_CNAT}


def _check_flat_dt(flat: torch.Tensor, layout: BucketLayout) -> Tuple[torch.Tensor, int]:
    if flat.dtype not in DT_DTYPES:
        raise ValueError(f"adfl_amd.stoch: the *_dt codecs take fp16 / bf16 / fp64 buckets, got {flat.dtype}")
    flat = _dev(flat, "flat")
    if flat.numel() < layout.total:
        raise ValueError("adfl_amd.stoch: flat buffer smaller than the layout")
    return flat, DT_DTYPES[flat.dtype]


def _uniforms_dt(u: Optional[torch.Tensor], layout: BucketLayout, dtype: torch.dtype) -> int:
    if u is None:
        return 0
    if u.dtype != dtype or u.numel() < layout.total:
        raise ValueError(f"adfl_amd.stoch: uniforms must be a {dtype} plane covering the layout")
    if not u.is_cuda or not u.is_contiguous() or u.data_ptr() % 16:
        raise ValueError("adfl_amd.stoch: uniforms must be a contiguous, 16-byte aligned device tensor")
    return u.data_ptr()


def norms_batched_dt(flat: torch.Tensor, layout: BucketLayout, mode: int = NORM_L2, *,
                     ws: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """Per-tensor norms of an fp16 / bf16 / fp64 bucket as fp64 values of the dtype's norm: L2 (fp16 / bf16:
    fp32 squares summed in fp64, rounded to fp32, sqrt, rounded to the dtype; fp64: fp64 sum) or
    (max|x|, min|x|) with mode NORM_LINF."""
    flat, dt = _check_flat_dt(flat, layout)
    dev = flat.device
    norms = torch.empty(layout.ntensors, dtype=torch.float64, device=dev)
    mins = torch.empty(layout.ntensors, dtype=torch.float64, device=dev) if mode == NORM_LINF else None
    ws = _ws(ws, layout, dev)
    check(_lib.load().adfl_stoch_norms_batched_dt(dt, flat.data_ptr(), layout.device_chunks(dev).data_ptr(),
                                                  layout.nchunks, mode, ws.data_ptr(), ws.numel(), norms.data_ptr(),
                                                  mins.data_ptr() if mins is not None else None, _stream(dev)))
    return norms, mins


def quantize_batched_dt(codec: str, flat: torch.Tensor, layout: BucketLayout, bits: int, norms: torch.Tensor, *,
                        uniforms: Optional[torch.Tensor] = None, seed: int = 0, counter: int = 0,
                        levels: Optional[torch.Tensor] = None,
                        signs: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Levels (QSGD / RQSGD; uint8) or exponents (CNAT; int8) + signs of an fp16 / bf16 / fp64 bucket from
    given fp64 per-tensor norms (the parity tests inject the reference's)."""
    flat, dt = _check_flat_dt(flat, layout)
    dev = flat.device
    levels, signs = _planes(layout, dev, levels, signs, torch.int8 if codec == "cnat" else torch.uint8)
    norms = _dev(norms, "norms")
    if norms.dtype != torch.float64 or norms.numel() < layout.ntensors:
        raise ValueError("adfl_amd.stoch: norms must be fp64, one per tensor")
    check(_lib.load().adfl_stoch_quantize_batched_dt(_CODEC_IDS[codec], dt, flat.data_ptr(),
                                                     layout.device_chunks(dev).data_ptr(), layout.nchunks, bits,
                                                     norms.data_ptr(), _uniforms_dt(uniforms, layout, flat.dtype),
                                                     seed, counter, levels.data_ptr(), signs.data_ptr(), _stream(dev)))
    return levels, signs


def encode_batched_dt(codec: str, flat: torch.Tensor, layout: BucketLayout, bits: int, *,
                      uniforms: Optional[torch.Tensor] = None, seed: int = 0, counter: int = 0,
                      levels: Optional[torch.Tensor] = None, signs: Optional[torch.Tensor] = None,
                      ws: Optional[torch.Tensor] = None):
    """QSGD / RQSGD / CNAT encode of an fp16 / bf16 / fp64 bucket in the dtype's arithmetic
    (quant.py:223-240, :364-382, :509-534): (levels, signs, norms f64, mins f64 or None)."""
    flat, dt = _check_flat_dt(flat, layout)
    dev = flat.device
    levels, signs = _planes(layout, dev, levels, signs, torch.int8 if codec == "cnat" else torch.uint8)
    norms = torch.empty(layout.ntensors, dtype=torch.float64, device=dev)
    mins = torch.empty(layout.ntensors, dtype=torch.float64, device=dev) if codec == "rqsgd" else None
    ws = _ws(ws, layout, dev)
    check(_lib.load().adfl_stoch_encode_batched_dt(_CODEC_IDS[codec], dt, flat.data_ptr(),
                                                   layout.device_chunks(dev).data_ptr(), layout.nchunks, bits,
                                                   _uniforms_dt(uniforms, layout, flat.dtype), seed, counter,
                                                   ws.data_ptr(), ws.numel(), levels.data_ptr(), signs.data_ptr(),
                                                   norms.data_ptr(), mins.data_ptr() if mins is not None else None,
                                                   _stream(dev)))
    return levels, signs, norms, mins


def philox_uniforms_dt(dtype: torch.dtype, n: int, seed: int, counter: int, start: int = 0, *,
                       device=None) -> torch.Tensor:
    """The uniforms (in `dtype`) elements start .. start+n-1 of stream (seed, counter) draw."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    out = torch.empty(n, dtype=dtype, device=dev)
    check(_lib.load().adfl_philox_uniforms_dt(DT_DTYPES[dtype], out.data_ptr(), n, start, seed & (2 ** 64 - 1),
                                              counter, _stream(dev)))
    return out


# ------------------------------------------------------------------------------------------------
# torch.ops.adfl stochastic ops over caller-placed tensors (offsets / sizes: host int64, as the SLQ batched
# ops take them, ops.layout_for): QSGDChannel / RQSGDChannel / CNATChannel's per-tensor loops
# (quant.py:223-252, :364-398, :509-545) as traceable ops. Positions no tensor owns are zero.
# ------------------------------------------------------------------------------------------------
def _check_codec(codec: str) -> None:
    if codec not in _CODEC_IDS:
        raise ValueError(f"adfl stochastic ops: codec must be one of {sorted(_CODEC_IDS)}, got {codec!r}")


def _stoch_encode_flat(flat: torch.Tensor, offsets: torch.Tensor, sizes: torch.Tensor, codec: str, bits: int,
                       seed: int, counter: int):
    """stoch_encode_batched's body (stoch_encode_delta_batched runs it over the difference bucket)."""
    from .ops import _filled, layout_for
    _check_codec(codec)
    lay = layout_for(offsets, sizes)
    flat = flat.reshape(-1)
    if flat.numel() < lay.total:
        raise ValueError("stoch_encode_batched: flat buffer smaller than the layout")
    dev = flat.device
    lv = _filled(flat.numel(), torch.int8 if codec == "cnat" else torch.uint8, dev, lay)
    sg = _filled(flat.numel(), torch.int8, dev, lay)
    mins = torch.zeros(lay.ntensors, dtype=torch.float32, device=dev)
    if flat.dtype in DT_DTYPES:
        lv, sg, nr, mn = encode_batched_dt(codec, flat, lay, bits, seed=seed, counter=counter, levels=lv, signs=sg)
        return lv, sg, nr.float(), (mn.float() if mn is not None else mins)
    if codec == "qsgd":
        lv, sg, nr = qsgd_encode_batched(flat, lay, bits, seed=seed, counter=counter, levels=lv, signs=sg)
    elif codec == "rqsgd":
        lv, sg, nr, mins = rqsgd_encode_batched(flat, lay, bits, seed=seed, counter=counter, levels=lv, signs=sg,
                                                mins=mins)
    else:
        lv, sg, nr = cnat_encode_batched(flat, lay, bits, seed=seed, counter=counter, exps=lv, signs=sg)
    return lv, sg, nr, mins


@torch.library.custom_op("adfl::stoch_encode_batched", mutates_args=())
def stoch_encode_batched_op(flat: torch.Tensor, offsets: torch.Tensor, sizes: torch.Tensor, codec: str, bits: int,
                            seed: int, counter: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(levels — uint8, CNAT: int8 exponents —, signs int8, norms f32, mins f32 — RQSGD's min|x|, else 0) of
    a flat buffer; uniforms from the Philox stream (seed, counter). fp32 buffers take the fp32 kernels;
    fp16 / bf16 / fp64 ones are encoded in their own dtype's arithmetic, as the reference computes them
    (encode_batched_dt), and their norms / mins come back as the fp32 values the decode multiplies by (the
    channels' Python-float norm as an fp32 scalar; exact for fp16 / bf16 norms)."""
    return _stoch_encode_flat(flat, offsets, sizes, codec, bits, seed, counter)


@stoch_encode_batched_op.register_fake
def _(flat, offsets, sizes, codec, bits, seed, counter):
    n, t = flat.numel(), sizes.numel()
    return (flat.new_empty((n,), dtype=torch.int8 if codec == "cnat" else torch.uint8),
            flat.new_empty((n,), dtype=torch.int8), flat.new_empty((t,), dtype=torch.float32),
            flat.new_empty((t,), dtype=torch.float32))


@torch.library.custom_op("adfl::stoch_encode_delta_batched", mutates_args=())
def stoch_encode_delta_batched_op(new: torch.Tensor, prev: torch.Tensor, offsets: torch.Tensor, sizes: torch.Tensor,
                                  codec: str, bits: int, seed: int,
                                  counter: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """stoch_encode_batched of (new - prev), two flat fp32 buffers in the same caller-placed layout. rqsgd: the
    two-source kernels (the difference is never written); qsgd / cnat: one bucket_diff launch, then exactly what
    stoch_encode_batched runs over it, its norm mode included."""
    from .ops import _filled, bucket_diff, layout_for
    _check_codec(codec)
    if new.dtype != torch.float32 or prev.dtype != torch.float32:
        raise ValueError(f"stoch_encode_delta_batched: fp32 buffers only, got {new.dtype} / {prev.dtype}")
    lay = layout_for(offsets, sizes)
    new, prev = new.reshape(-1), prev.reshape(-1)
    if new.numel() < lay.total or prev.numel() < lay.total:
        raise ValueError("stoch_encode_delta_batched: flat buffer smaller than the layout")
    dev = new.device
    if codec != "rqsgd":
        diff = bucket_diff(new, prev, lay, out=torch.empty(new.numel(), dtype=torch.float32, device=dev))
        return _stoch_encode_flat(diff, offsets, sizes, codec, bits, seed, counter)
    lv = _filled(new.numel(), torch.uint8, dev, lay)
    sg = _filled(new.numel(), torch.int8, dev, lay)
    return rqsgd_encode_delta_batched(new, prev, lay, bits, seed=seed, counter=counter, levels=lv, signs=sg)


@stoch_encode_delta_batched_op.register_fake
def _(new, prev, offsets, sizes, codec, bits, seed, counter):
    n, t = new.numel(), sizes.numel()
    return (new.new_empty((n,), dtype=torch.int8 if codec == "cnat" else torch.uint8),
            new.new_empty((n,), dtype=torch.int8), new.new_empty((t,), dtype=torch.float32),
            new.new_empty((t,), dtype=torch.float32))


# QAFeL's broadcast (torch.ops.adfl_apply.*, beside the other server steps).
@torch.library.custom_op("adfl_apply::stoch_encode_delta_update_batched", mutates_args=("hidden",))
def stoch_encode_delta_update_batched_op(new: torch.Tensor, hidden: torch.Tensor, offsets: torch.Tensor,
                                         sizes: torch.Tensor, codec: str, bits: int, seed: int,
                                         counter: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """stoch_encode_delta_batched(new, hidden), and in place hidden += decode(payload): fp32(h + d) per element of
    every tensor of the caller-placed layout, d the codec's decode of the stored bytes (+0 for a zero norm);
    positions no tensor owns are untouched. rqsgd: the two-source kernels that also write h'; qsgd under the
    reference norm (the default): bucket_diff, the reference-order norm, then the quantize that also writes h';
    cnat, and qsgd under ADFL_STOCH_NORM=fp64: stoch_encode_delta_batched's encode, then the fused decode + axpby
    (alpha = beta = 1) over the planes where the encode left them."""
    from .Channel.stoch import reference_norm
    from .ops import _filled, _update_flat, bucket_diff, layout_for
    _check_codec(codec)
    if new.dtype != torch.float32:
        raise ValueError(f"stoch_encode_delta_update_batched: fp32 buffers only, got {new.dtype} / {hidden.dtype}")
    lay = layout_for(offsets, sizes)
    new, hidden = _update_flat(new, hidden, lay, "stoch_encode_delta_update_batched")
    dev = new.device
    n = new.numel()
    lv = _filled(n, torch.int8 if codec == "cnat" else torch.uint8, dev, lay)
    sg = _filled(n, torch.int8, dev, lay)
    mins = torch.zeros(lay.ntensors, dtype=torch.float32, device=dev)
    if codec == "rqsgd":
        return rqsgd_encode_delta_update_batched(new, hidden, lay, bits, seed=seed, counter=counter, levels=lv,
                                                 signs=sg, mins=mins)
    diff = bucket_diff(new, hidden, lay, out=torch.empty(n, dtype=torch.float32, device=dev))
    if codec == "qsgd" and reference_norm():
        norms = torch_norms(diff, lay)
        qsgd_quantize_update_batched(diff, lay, bits, norms, hidden, seed=seed, counter=counter, levels=lv, signs=sg)
        return lv, sg, norms, mins
    if codec == "qsgd":
        lv, sg, norms = qsgd_encode_batched(diff, lay, bits, seed=seed, counter=counter, levels=lv, signs=sg)
    else:
        lv, sg, norms = cnat_encode_batched(diff, lay, bits, seed=seed, counter=counter, exps=lv, signs=sg)
    dequantize_axpby_batched(codec, lv, sg, norms, lay, bits, hidden, hidden, 1.0, 1.0)
    return lv, sg, norms, mins


@stoch_encode_delta_update_batched_op.register_fake
def _(new, hidden, offsets, sizes, codec, bits, seed, counter):
    n, t = new.numel(), sizes.numel()
    return (new.new_empty((n,), dtype=torch.int8 if codec == "cnat" else torch.uint8),
            new.new_empty((n,), dtype=torch.int8), new.new_empty((t,), dtype=torch.float32),
            new.new_empty((t,), dtype=torch.float32))


@torch.library.custom_op("adfl::stoch_decode_batched", mutates_args=())
def stoch_decode_batched_op(levels: torch.Tensor, signs: torch.Tensor, norms: torch.Tensor, mins: torch.Tensor,
                            offsets: torch.Tensor, sizes: torch.Tensor, codec: str, bits: int) -> torch.Tensor:
    """fp32 decode of stoch_encode_batched's planes (mins used by RQSGD only)."""
    from .ops import _filled, layout_for
    _check_codec(codec)
    lay = layout_for(offsets, sizes)
    levels, signs = levels.reshape(-1), signs.reshape(-1)
    if levels.numel() < lay.total or signs.numel() < lay.total:
        raise ValueError("stoch_decode_batched: planes smaller than the layout")
    out = _filled(levels.numel(), torch.float32, levels.device, lay)
    if codec == "qsgd":
        return qsgd_decode_batched(levels.view(torch.uint8), signs, norms, lay, bits, out=out)
    if codec == "rqsgd":
        return rqsgd_decode_batched(levels.view(torch.uint8), signs, norms, mins, lay, bits, out=out)
    return cnat_decode_batched(levels.view(torch.int8), signs, norms, lay, out=out)


@stoch_decode_batched_op.register_fake
def _(levels, signs, norms, mins, offsets, sizes, codec, bits):
    return levels.new_empty((levels.numel(),), dtype=torch.float32)


# ------------------------------------------------------------------------------------------------
# fused decode + axpby: the asynchronous server's update step (adfl_stoch_dequantize_axpby_batched)
# ------------------------------------------------------------------------------------------------
def dequantize_axpby_batched(codec: str, levels: torch.Tensor, signs: torch.Tensor, norms: torch.Tensor,
                             layout: BucketLayout, bits: int, bases, outs, alpha: float, beta: float, *,
                             mins: Optional[torch.Tensor] = None) -> None:
    """ops.dequantize_axpby_batched for the stochastic codecs: with d the codec's decode of one bucket payload
    (+0 for a tensor whose norm is 0), outs[k][t] = fp32(fp32(alpha * bases[k][t]) + fp32(beta * d)), or
    fp32(beta * d) when bases is None — FedAsync (Src/ADFL/Strategy/fed_async.py:80-81), Simple DELTA
    (simple.py:100) and FedBuff (fed_buff.py:72-80) over quant.py:243-252 / :385-398 / :537-545. bases / outs as
    ops.dequantize_axpby_batched takes them; levels / signs byte planes of >= layout.total, norms (RQSGD: mins)
    one fp32 per tensor."""
    from .ops import _f32_on, apply_tables
    _check_codec(codec)
    levels, signs = _dev(levels, "levels"), _dev(signs, "signs")
    dev = levels.device
    if (levels.element_size() != 1 or signs.element_size() != 1 or levels.numel() < layout.total
            or signs.numel() < layout.total or signs.device != dev):
        raise ValueError(f"adfl_amd.stoch: levels / signs must be byte planes of >= {layout.total} on one device")
    norms = _f32_on(norms, layout.ntensors, dev, "norms")
    if codec == "rqsgd":
        if mins is None:
            raise ValueError("adfl_amd.stoch: RQSGD needs mins")
        mins = _f32_on(mins, layout.ntensors, dev, "mins")
    else:
        mins = None
    b_tab, o_tab, k = apply_tables(bases, outs, layout, dev)
    check(_lib.load().adfl_stoch_dequantize_axpby_batched(
        _CODEC_IDS[codec], levels.data_ptr(), signs.data_ptr(), layout.device_chunks(dev).data_ptr(), layout.nchunks,
        bits, norms.data_ptr(), mins.data_ptr() if mins is not None else None,
        b_tab.data_ptr() if b_tab is not None else None, o_tab.data_ptr(), layout.ntensors, k, float(alpha),
        float(beta), _stream(dev)))


def dequantize_mean_axpby_batched(codec: str, levels: torch.Tensor, signs: torch.Tensor, norms: torch.Tensor,
                                  mins: Optional[torch.Tensor], layout: BucketLayout, bits: int, bases, outs,
                                  alpha: float, beta: float) -> None:
    """ops.dequantize_mean_axpby_batched for the stochastic codecs (adfl_stoch_dequantize_mean_axpby_batched): the
    synchronous DELTA server step, add_parameters(g, simple_aggregate(K decodes), alpha, beta)
    (Src/ADFL/Strategy/simple.py:87-89) in one launch. With m what dequantize_mean_batched writes for the same
    planes, outs[t] = fp32(fp32(alpha * bases[t]) + fp32(beta * m)). levels / signs: [K, row] byte planes, norms
    (RQSGD: mins, else None) [K, ntensors] fp32; bases / outs as ops.dequantize_mean_axpby_batched takes them."""
    from .ops import mean_axpby_tables
    _check_codec(codec)
    levels, signs, norms = _dev(levels, "levels"), _dev(signs, "signs"), _dev(norms, "norms")
    if levels.dim() != 2 or signs.shape != levels.shape or levels.element_size() != 1 or signs.element_size() != 1:
        raise ValueError("adfl_amd.stoch: levels / signs must be [K, row] byte planes of one shape")
    k, row = levels.shape
    if row < layout.total or not levels.is_contiguous() or not signs.is_contiguous():
        raise ValueError(f"adfl_amd.stoch: rows of {row} bytes cannot hold the {layout.total}-element bucket")
    if norms.shape != (k, layout.ntensors) or norms.dtype != torch.float32 or not norms.is_contiguous():
        raise ValueError(f"adfl_amd.stoch: norms must be contiguous fp32 [{k}, {layout.ntensors}]")
    if codec == "rqsgd":
        if mins is None:
            raise ValueError("adfl_amd.stoch: RQSGD needs mins")
        mins = _dev(mins, "mins")
        if mins.shape != norms.shape or mins.dtype != torch.float32 or not mins.is_contiguous():
            raise ValueError("adfl_amd.stoch: mins must match norms")
    else:
        mins = None
    dev = levels.device
    b_tab, o_tab = mean_axpby_tables(bases, outs, layout, dev)
    check(_lib.load().adfl_stoch_dequantize_mean_axpby_batched(
        _CODEC_IDS[codec], levels.data_ptr(), signs.data_ptr(), row, k, layout.device_chunks(dev).data_ptr(),
        layout.nchunks, bits, norms.data_ptr(), mins.data_ptr() if mins is not None else None, layout.ntensors,
        b_tab.data_ptr(), o_tab.data_ptr(), layout.ntensors, float(alpha), float(beta), _stream(dev)))


@torch.library.custom_op("adfl_apply::stoch_decode_mean_axpby_batched", mutates_args=())
def stoch_decode_mean_axpby_batched_op(levels: torch.Tensor, signs: torch.Tensor, norms: torch.Tensor,
                                       mins: torch.Tensor, base: torch.Tensor, offsets: torch.Tensor,
                                       sizes: torch.Tensor, codec: str, bits: int, alpha: float,
                                       beta: float) -> torch.Tensor:
    """fp32(fp32(alpha * base) + fp32(beta * mean of the K decodes)) per tensor of K rows of stoch_encode_batched's
    planes ([K, row]; norms / mins [K, T], mins used by RQSGD only), as a new bucket shaped like `base`
    (positions no tensor owns are zero)."""
    from .ops import _filled, layout_for
    _check_codec(codec)
    lay = layout_for(offsets, sizes)
    base = base.reshape(-1)
    if base.dtype != torch.float32 or base.numel() < lay.total:
        raise ValueError("stoch_decode_mean_axpby_batched: base must be an fp32 bucket of at least the layout's "
                         "extent")
    out = _filled(base.numel(), torch.float32, base.device, lay)
    dequantize_mean_axpby_batched(codec, levels.view(torch.uint8), signs, norms, mins if codec == "rqsgd" else None,
                                  lay, bits, _dev(base, "base"), out, alpha, beta)
    return out


@stoch_decode_mean_axpby_batched_op.register_fake
def _(levels, signs, norms, mins, base, offsets, sizes, codec, bits, alpha, beta):
    return base.new_empty((base.numel(),), dtype=torch.float32)


@torch.library.custom_op("adfl_apply::stoch_decode_axpby_batched", mutates_args=())
def stoch_decode_axpby_batched_op(levels: torch.Tensor, signs: torch.Tensor, norms: torch.Tensor, mins: torch.Tensor,
                                  base: torch.Tensor, offsets: torch.Tensor, sizes: torch.Tensor, codec: str,
                                  bits: int, alpha: float, beta: float) -> torch.Tensor:
    """fp32(fp32(alpha * base) + fp32(beta * decode)) per tensor of stoch_encode_batched's planes, as a new
    bucket shaped like `base` (mins used by RQSGD only; positions no tensor owns are zero)."""
    from .ops import _filled, layout_for
    _check_codec(codec)
    lay = layout_for(offsets, sizes)
    levels, signs, base = levels.reshape(-1), signs.reshape(-1), base.reshape(-1)
    if base.dtype != torch.float32 or base.numel() < lay.total:
        raise ValueError("stoch_decode_axpby_batched: base must be an fp32 bucket of at least the layout's extent")
    out = _filled(base.numel(), torch.float32, base.device, lay)
    dequantize_axpby_batched(codec, levels, signs, norms, lay, bits, _dev(base, "base"), out, alpha, beta, mins=mins)
    return out


@stoch_decode_axpby_batched_op.register_fake
def _(levels, signs, norms, mins, base, offsets, sizes, codec, bits, alpha, beta):
    return base.new_empty((base.numel(),), dtype=torch.float32)


# ------------------------------------------------------------------------------------------------
# the buffered servers' K-th update: fused decode + accumulate + flush (adfl_stoch_dequantize_*_flush_batched)
# ------------------------------------------------------------------------------------------------
def _flush_payload(codec: str, levels: torch.Tensor, signs: torch.Tensor, norms: torch.Tensor,
                   mins: Optional[torch.Tensor], layout: BucketLayout, bits: int):
    """The checked payload of a fused decode + accumulate + flush: (levels, signs, norms, mins or None, s)."""
    from .ops import _f32_on
    _check_codec(codec)
    levels, signs = _dev(levels, "levels"), _dev(signs, "signs")
    dev = levels.device
    if (levels.element_size() != 1 or signs.element_size() != 1 or levels.numel() < layout.total
            or signs.numel() < layout.total or signs.device != dev):
        raise ValueError(f"adfl_amd.stoch: levels / signs must be byte planes of >= {layout.total} on one device")
    norms = _f32_on(norms, layout.ntensors, dev, "norms")
    if codec == "rqsgd":
        if mins is None:
            raise ValueError("adfl_amd.stoch: RQSGD needs mins")
        mins = _f32_on(mins, layout.ntensors, dev, "mins")
    else:
        mins = None
    if codec != "cnat" and not 1 <= int(bits) <= 16:
        raise ValueError(f"adfl_amd.stoch: bits must be in [1, 16], got {bits}")
    s = 1.0 if codec == "cnat" else float(2 ** int(bits) - 1)   # self.levels = 2**bits - 1
    return levels, signs, norms, mins, s


def dequantize_fedbuff_flush_batched(codec: str, levels: torch.Tensor, signs: torch.Tensor, norms: torch.Tensor,
                                     layout: BucketLayout, bits: int, buf, g, out, K: int, factor: float, lr: float,
                                     *, mins: Optional[torch.Tensor] = None) -> None:
    """ops.dequantize_fedbuff_flush_batched for the stochastic codecs (adfl_stoch_dequantize_fedbuff_flush_batched):
    FedBuff's K-th client update (Src/ADFL/Strategy/fed_buff.py:68-100) in one launch, d the codec's decode of one
    bucket payload (+0 for a tensor whose norm is 0). Bit-identical to dequantize_axpby_batched on the buffer with
    (1.0, factor) followed by flush.fedbuff_flush_batched; `buf` (None: no buffer) is read and never written.
    buf / g / out as ops.dequantize_fedbuff_flush_batched takes them; the payload as dequantize_axpby_batched's."""
    from .flush import _check_k
    from .ops import flush_tables
    levels, signs, norms, mins, s = _flush_payload(codec, levels, signs, norms, mins, layout, bits)
    dev = levels.device
    K = _check_k(K)
    tab, (b, gp, o) = flush_tables([buf, g, out], ["buf", "g", "out"], layout, dev)
    check(_lib.load().adfl_stoch_dequantize_fedbuff_flush_batched(
        _CODEC_IDS[codec], levels.data_ptr(), signs.data_ptr(), layout.device_chunks(dev).data_ptr(), layout.nchunks,
        norms.data_ptr(), mins.data_ptr() if mins is not None else None, s, b, gp, o, layout.ntensors, K,
        float(factor), float(lr), _stream(dev)))


def dequantize_fadas_flush_batched(codec: str, levels: torch.Tensor, signs: torch.Tensor, norms: torch.Tensor,
                                   layout: BucketLayout, bits: int, buf, g, m, v, v_hat, out, K: int, fadas_scalars,
                                   *, mins: Optional[torch.Tensor] = None) -> None:
    """ops.dequantize_fadas_flush_batched for the stochastic codecs (adfl_stoch_dequantize_fadas_flush_batched):
    FADAS's K-th client update (Src/ADFL/Strategy/fadas.py:56-80) in one launch; m, v, v_hat updated in place.
    Bit-identical to dequantize_axpby_batched on the buffer with (1.0, 1.0) followed by flush.fadas_flush_batched."""
    from .flush import _check_k
    from .ops import flush_tables
    levels, signs, norms, mins, s = _flush_payload(codec, levels, signs, norms, mins, layout, bits)
    dev = levels.device
    K = _check_k(K)
    if len(fadas_scalars) != 7:
        raise ValueError("dequantize_fadas_flush_batched: scalars are flush.fadas_scalars()'s seven values")
    tab, ptrs = flush_tables([buf, g, m, v, v_hat, out], ["buf", "g", "m", "v", "v_hat", "out"], layout, dev)
    check(_lib.load().adfl_stoch_dequantize_fadas_flush_batched(
        _CODEC_IDS[codec], levels.data_ptr(), signs.data_ptr(), layout.device_chunks(dev).data_ptr(), layout.nchunks,
        norms.data_ptr(), mins.data_ptr() if mins is not None else None, s, *ptrs, layout.ntensors, K,
        *(float(x) for x in fadas_scalars), _stream(dev)))


@torch.library.custom_op("adfl_apply::stoch_dequantize_fedbuff_flush_batched", mutates_args=())
def stoch_dequantize_fedbuff_flush_batched_op(levels: torch.Tensor, signs: torch.Tensor, norms: torch.Tensor,
                                              mins: torch.Tensor, buf: Optional[torch.Tensor], g: torch.Tensor,
                                              offsets: torch.Tensor, sizes: torch.Tensor, codec: str, bits: int,
                                              K: int, factor: float, lr: float) -> torch.Tensor:
    """FedBuff's K-th client update per tensor of stoch_encode_batched's planes (mins used by RQSGD only): decode,
    scale by `factor`, add to `buf` (None: no buffer), divide by K and step from `g`, as a new bucket shaped like
    `g` (positions no tensor owns are zero). `buf` is not written."""
    from .ops import _filled, _flush_flat, layout_for
    _check_codec(codec)
    lay = layout_for(offsets, sizes)
    what = "stoch_dequantize_fedbuff_flush_batched: "
    g = _flush_flat(g, lay, what + "g")
    buf = None if buf is None else _flush_flat(buf, lay, what + "buf")
    out = _filled(g.numel(), torch.float32, g.device, lay)
    dequantize_fedbuff_flush_batched(codec, levels.reshape(-1).view(torch.uint8), signs.reshape(-1), norms, lay, bits,
                                     buf, g, out, K, factor, lr, mins=mins if codec == "rqsgd" else None)
    return out


@stoch_dequantize_fedbuff_flush_batched_op.register_fake
def _(levels, signs, norms, mins, buf, g, offsets, sizes, codec, bits, K, factor, lr):
    return g.new_empty((g.numel(),), dtype=torch.float32)


@torch.library.custom_op("adfl_apply::stoch_dequantize_fadas_flush_batched", mutates_args=("m", "v", "v_hat"))
def stoch_dequantize_fadas_flush_batched_op(levels: torch.Tensor, signs: torch.Tensor, norms: torch.Tensor,
                                            mins: torch.Tensor, buf: Optional[torch.Tensor], g: torch.Tensor,
                                            m: torch.Tensor, v: torch.Tensor, v_hat: torch.Tensor,
                                            offsets: torch.Tensor, sizes: torch.Tensor, codec: str, bits: int, K: int,
                                            beta1: float, one_minus_beta1: float, beta2: float,
                                            one_minus_beta2: float, sqrt_bc2: float, eps: float,
                                            step: float) -> torch.Tensor:
    """FADAS's K-th client update per tensor of stoch_encode_batched's planes: m, v, v_hat (flat fp32 buckets)
    updated in place, the new parameters returned as a bucket shaped like `g`. Scalars: flush.fadas_scalars()."""
    from .ops import _filled, _flush_flat, layout_for
    _check_codec(codec)
    lay = layout_for(offsets, sizes)
    what = "stoch_dequantize_fadas_flush_batched: "
    g = _flush_flat(g, lay, what + "g")
    buf = None if buf is None else _flush_flat(buf, lay, what + "buf")
    for name, t in (("m", m), ("v", v), ("v_hat", v_hat)):
        if t.dim() != 1:
            raise ValueError(f"{what}{name} must be one-dimensional (it is updated in place)")
        _flush_flat(t, lay, what + name)
    out = _filled(g.numel(), torch.float32, g.device, lay)
    dequantize_fadas_flush_batched(codec, levels.reshape(-1).view(torch.uint8), signs.reshape(-1), norms, lay, bits,
                                   buf, g, m, v, v_hat, out, K,
                                   (beta1, one_minus_beta1, beta2, one_minus_beta2, sqrt_bc2, eps, step),
                                   mins=mins if codec == "rqsgd" else None)
    return out


@stoch_dequantize_fadas_flush_batched_op.register_fake
def _(levels, signs, norms, mins, buf, g, m, v, v_hat, offsets, sizes, codec, bits, K, beta1, one_minus_beta1, beta2,
      one_minus_beta2, sqrt_bc2, eps, step):
    return g.new_empty((g.numel(),), dtype=torch.float32)


# ------------------------------------------------------------------------------------------------
# packed planes: bits + 1 bits per weight (adfl_stoch_*_packed_batched, csrc/stoch_packed.hip)
# ------------------------------------------------------------------------------------------------
_PACKED_CODECS = ("qsgd", "rqsgd")


def packed_plane_bytes(n: int, bits: int) -> Tuple[int, int]:
    """(level bytes, sign bytes) of an n-element tensor in the packed format: one level byte per element for
    bits > 4, two levels per byte (pack_4bit's nibble order) for bits <= 4; one sign bit per element."""
    n = int(n)
    return (n if bits > 4 else (n + 1) // 2), (n + 7) // 8


def _packed_args(codec: str, layout: BucketLayout, bits: int) -> Tuple[int, int]:
    """The checks the C ABI cannot make (it never sees the chunk table): (level bytes, sign bytes) of the
    layout's packed planes."""
    if codec not in _PACKED_CODECS:
        raise ValueError(f"adfl_amd.stoch: the packed planes carry {' / '.join(_PACKED_CODECS)}, got {codec!r} "
                         "(CNAT's zero elements need a third sign state)")
    if not 1 <= int(bits) <= 8:
        raise ValueError(f"adfl_amd.stoch: packed planes take bits in [1, 8], got {bits}")
    from .ops import ALIGN_ELEMS
    if (layout.offsets % ALIGN_ELEMS).any():
        raise ValueError(f"adfl_amd.stoch: packed planes need every tensor offset a multiple of {ALIGN_ELEMS} elements")
    return packed_plane_bytes(layout.total, bits)


def _packed_planes(levels: torch.Tensor, signbits: torch.Tensor, need: Tuple[int, int]):
    """Both planes as contiguous, 16-byte aligned uint8 device tensors of at least `need` bytes on one device."""
    for t, what in ((levels, "levels"), (signbits, "signbits")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
            raise ValueError(f"adfl_amd.stoch: packed {what} must be a uint8 tensor, got {getattr(t, 'dtype', type(t))}")
    levels, signbits = _dev(levels.reshape(-1), "levels"), _dev(signbits.reshape(-1), "signbits")
    if signbits.device != levels.device or levels.numel() < need[0] or signbits.numel() < need[1]:
        raise ValueError(f"adfl_amd.stoch: packed planes must hold >= {need[0]} level and >= {need[1]} sign bytes on "
                         "one device")
    return levels, signbits


def _packed_scales(codec: str, norms: torch.Tensor, mins: Optional[torch.Tensor], layout: BucketLayout, dev):
    from .ops import _f32_on
    norms = _f32_on(norms, layout.ntensors, dev, "norms")
    if codec != "rqsgd":
        return norms, None
    if mins is None:
        raise ValueError("adfl_amd.stoch: RQSGD needs mins")
    return norms, _f32_on(mins, layout.ntensors, dev, "mins")


def quantize_packed_batched(codec: str, flat: torch.Tensor, layout: BucketLayout, bits: int, norms: torch.Tensor, *,
                            uniforms: Optional[torch.Tensor] = None, ushift=None, seed: int = 0, counter: int = 0,
                            levels: Optional[torch.Tensor] = None,
                            signbits: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """qsgd_quantize_batched's levels and sign tests from given per-tensor norms (QSGD: L2 norms; RQSGD: max|x|),
    stored as packed planes (packed_plane_bytes; layout offsets multiples of 64 elements): (levels, signbits),
    uint8. ushift: per tensor, element g draws the uniform of index g + ushift[t] (rqsgd_encode_delta_batched's
    rule: the compact bucket's draws for planes in the aligned one); injected uniforms then cover the shifted
    layout."""
    need = _packed_args(codec, layout, bits)
    flat = _check_flat(flat, layout)
    dev = flat.device
    from .ops import _f32_on
    norms = _f32_on(norms, layout.ntensors, dev, "norms")
    us, us_host = _ushift(ushift, layout, dev)
    if uniforms is not None:
        top = int((layout.offsets + layout.sizes + us_host).max())
        if uniforms.dtype != torch.float32 or uniforms.numel() < top:
            raise ValueError("adfl_amd.stoch: uniforms must be an fp32 plane covering the shifted layout")
        if not uniforms.is_cuda or not uniforms.is_contiguous() or uniforms.data_ptr() % 16:
            raise ValueError("adfl_amd.stoch: uniforms must be a contiguous, 16-byte aligned device tensor")
    levels = torch.empty(need[0], dtype=torch.uint8, device=dev) if levels is None else levels
    signbits = torch.empty(need[1], dtype=torch.uint8, device=dev) if signbits is None else signbits
    lv, sb = _packed_planes(levels, signbits, need)
    if lv.data_ptr() != levels.data_ptr() or sb.data_ptr() != signbits.data_ptr():
        raise ValueError("adfl_amd.stoch: packed output planes must be contiguous and 16-byte aligned")
    check(_lib.load().adfl_stoch_quantize_packed_batched(
        _CODEC_IDS[codec], flat.data_ptr(), layout.device_chunks(dev).data_ptr(), layout.nchunks, bits,
        norms.data_ptr(), uniforms.data_ptr() if uniforms is not None else None,
        us.data_ptr() if us is not None else None, seed, counter, lv.data_ptr(), sb.data_ptr(), _stream(dev)))
    return levels, signbits


def encode_packed_batched(codec: str, flat: torch.Tensor, layout: BucketLayout, bits: int, *,
                          uniforms: Optional[torch.Tensor] = None, ushift=None, seed: int = 0, counter: int = 0,
                          levels: Optional[torch.Tensor] = None, signbits: Optional[torch.Tensor] = None,
                          norms: Optional[torch.Tensor] = None, mins: Optional[torch.Tensor] = None,
                          ws: Optional[torch.Tensor] = None, torch_norm: bool = True):
    """The norms the unpacked channels take (QSGD: the reference-order L2 norm, or the correctly rounded fp64 one
    with torch_norm=False; RQSGD: max|x| and min|x|), then quantize_packed_batched: (levels, signbits, norms,
    mins or None)."""
    _packed_args(codec, layout, bits)
    flat = _check_flat(flat, layout)
    dev = flat.device
    norms = torch.empty(layout.ntensors, dtype=torch.float32, device=dev) if norms is None else norms
    if codec == "rqsgd":
        norms, mins = norms_batched(flat, layout, NORM_LINF, norms=norms, mins=mins, ws=ws)
    else:
        mins = None
        if torch_norm:
            reference_norms(flat, layout, out32=norms)
        else:
            norms_batched(flat, layout, NORM_L2, norms=norms, ws=ws)
    levels, signbits = quantize_packed_batched(codec, flat, layout, bits, norms, uniforms=uniforms, ushift=ushift,
                                               seed=seed, counter=counter, levels=levels, signbits=signbits)
    return levels, signbits, norms, mins


def dequantize_packed_batched(codec: str, levels: torch.Tensor, signbits: torch.Tensor, norms: torch.Tensor,
                              layout: BucketLayout, bits: int, *, mins: Optional[torch.Tensor] = None,
                              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """qsgd_decode_batched / rqsgd_decode_batched from packed planes: the fp32 bucket (layout offsets multiples of
    64 elements), every value the unpacked decode's of the unpacked planes."""
    need = _packed_args(codec, layout, bits)
    levels, signbits = _packed_planes(levels, signbits, need)
    dev = levels.device
    norms, mins = _packed_scales(codec, norms, mins, layout, dev)
    if out is None:
        out = torch.empty(layout.total, dtype=torch.float32, device=dev)
    elif (out.dtype != torch.float32 or out.device != dev or out.numel() < layout.total or not out.is_contiguous()
          or out.data_ptr() % 16):
        raise ValueError(f"adfl_amd.stoch: out must be a contiguous, 16-byte aligned fp32 bucket of >= {layout.total} "
                         f"on {dev}")
    check(_lib.load().adfl_stoch_dequantize_packed_batched(
        _CODEC_IDS[codec], levels.data_ptr(), signbits.data_ptr(), layout.device_chunks(dev).data_ptr(),
        layout.nchunks, bits, norms.data_ptr(), mins.data_ptr() if mins is not None else None, out.data_ptr(),
        _stream(dev)))
    return out


def dequantize_axpby_packed_batched(codec: str, levels: torch.Tensor, signbits: torch.Tensor, norms: torch.Tensor,
                                    layout: BucketLayout, bits: int, bases, outs, alpha: float, beta: float, *,
                                    mins: Optional[torch.Tensor] = None) -> None:
    """dequantize_axpby_batched from packed planes: the same bases / outs, arithmetic and in-place rule."""
    from .ops import apply_tables
    need = _packed_args(codec, layout, bits)
    levels, signbits = _packed_planes(levels, signbits, need)
    dev = levels.device
    norms, mins = _packed_scales(codec, norms, mins, layout, dev)
    b_tab, o_tab, k = apply_tables(bases, outs, layout, dev)
    check(_lib.load().adfl_stoch_dequantize_axpby_packed_batched(
        _CODEC_IDS[codec], levels.data_ptr(), signbits.data_ptr(), layout.device_chunks(dev).data_ptr(),
        layout.nchunks, bits, norms.data_ptr(), mins.data_ptr() if mins is not None else None,
        b_tab.data_ptr() if b_tab is not None else None, o_tab.data_ptr(), layout.ntensors, k, float(alpha),
        float(beta), _stream(dev)))


@torch.library.custom_op("adfl_apply::stoch_encode_packed_batched", mutates_args=())
def stoch_encode_packed_batched_op(flat: torch.Tensor, offsets: torch.Tensor, sizes: torch.Tensor, codec: str, bits: int,
                                   seed: int, counter: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor,
                                                                     torch.Tensor]:
    """(packed levels uint8, sign bits uint8, norms f32, mins f32 — RQSGD's min|x|, else 0) of a flat fp32 buffer
    whose tensors sit at offsets that are multiples of 64: encode_packed_batched with the Philox stream (seed,
    counter). The planes are sized for the whole buffer (packed_plane_bytes(flat.numel(), bits)); bytes no tensor
    owns are zero."""
    from .ops import layout_for
    lay = layout_for(offsets, sizes)
    flat = flat.reshape(-1)
    if flat.dtype != torch.float32:
        raise ValueError(f"stoch_encode_packed_batched: fp32 buffers only, got {flat.dtype}")
    if flat.numel() < lay.total:
        raise ValueError("stoch_encode_packed_batched: flat buffer smaller than the layout")
    _packed_args(codec, lay, bits)
    nl, ns = packed_plane_bytes(flat.numel(), bits)
    lv = torch.zeros(nl, dtype=torch.uint8, device=flat.device)
    sb = torch.zeros(ns, dtype=torch.uint8, device=flat.device)
    lv, sb, nr, mn = encode_packed_batched(codec, flat, lay, bits, seed=seed, counter=counter, levels=lv, signbits=sb)
    return lv, sb, nr, (mn if mn is not None else torch.zeros(lay.ntensors, dtype=torch.float32, device=flat.device))


@stoch_encode_packed_batched_op.register_fake
def _(flat, offsets, sizes, codec, bits, seed, counter):
    n, t = flat.numel(), sizes.numel()
    nl, ns = (n if bits > 4 else (n + 1) // 2), (n + 7) // 8
    return (flat.new_empty((nl,), dtype=torch.uint8), flat.new_empty((ns,), dtype=torch.uint8),
            flat.new_empty((t,), dtype=torch.float32), flat.new_empty((t,), dtype=torch.float32))


def _packed_op_total(levels: torch.Tensor, bits: int, lay: BucketLayout) -> int:
    """The element extent a packed op's output bucket gets: what the level plane can hold, at least the layout's."""
    n = levels.numel() if bits > 4 else 2 * levels.numel()
    return max(int(n), lay.total)


@torch.library.custom_op("adfl_apply::stoch_decode_packed_batched", mutates_args=())
def stoch_decode_packed_batched_op(levels: torch.Tensor, signbits: torch.Tensor, norms: torch.Tensor,
                                   mins: torch.Tensor, offsets: torch.Tensor, sizes: torch.Tensor, codec: str,
                                   bits: int) -> torch.Tensor:
    """fp32 decode of stoch_encode_packed_batched's planes (mins used by RQSGD only), one float per element the
    level plane holds (positions no tensor owns are zero)."""
    from .ops import _filled, layout_for
    lay = layout_for(offsets, sizes)
    _packed_args(codec, lay, bits)
    out = _filled(_packed_op_total(levels.reshape(-1), bits, lay), torch.float32, levels.device, lay)
    return dequantize_packed_batched(codec, levels, signbits, norms, lay, bits, mins=mins if codec == "rqsgd" else None,
                                     out=out)


@stoch_decode_packed_batched_op.register_fake
def _(levels, signbits, norms, mins, offsets, sizes, codec, bits):
    n = levels.numel() if bits > 4 else 2 * levels.numel()
    return levels.new_empty((n,), dtype=torch.float32)


@torch.library.custom_op("adfl_apply::stoch_decode_axpby_packed_batched", mutates_args=())
def stoch_decode_axpby_packed_batched_op(levels: torch.Tensor, signbits: torch.Tensor, norms: torch.Tensor,
                                         mins: torch.Tensor, base: torch.Tensor, offsets: torch.Tensor,
                                         sizes: torch.Tensor, codec: str, bits: int, alpha: float,
                                         beta: float) -> torch.Tensor:
    """fp32(fp32(alpha * base) + fp32(beta * decode)) per tensor of stoch_encode_packed_batched's planes, as a new
    bucket shaped like `base` (mins used by RQSGD only; positions no tensor owns are zero)."""
    from .ops import _filled, layout_for
    lay = layout_for(offsets, sizes)
    _packed_args(codec, lay, bits)
    base = base.reshape(-1)
    if base.dtype != torch.float32 or base.numel() < lay.total:
        raise ValueError("stoch_decode_axpby_packed_batched: base must be an fp32 bucket of at least the layout's "
                         "extent")
    out = _filled(base.numel(), torch.float32, base.device, lay)
    dequantize_axpby_packed_batched(codec, levels, signbits, norms, lay, bits, _dev(base, "base"), out, alpha, beta,
                                    mins=mins if codec == "rqsgd" else None)
    return out


@stoch_decode_axpby_packed_batched_op.register_fake
def _(levels, signbits, norms, mins, base, offsets, sizes, codec, bits, alpha, beta):
    return base.new_empty((base.numel(),), dtype=torch.float32)
