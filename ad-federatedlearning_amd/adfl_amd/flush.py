"""The buffered asynchronous servers' flush on the GPU: what FedBuff and FADAS compute from a full buffer.

``receive_scaled`` / ``receive_scaled_add_`` (Channel/_base.py) keep a strategy's buffer up to date with one launch
per client update; this module is the step they feed. Both flushes are one launch for the whole state dict
(csrc/server_flush.hip, declared in include/adfl_slq.h):

* ``fedbuff_flush(buffer, g_params, K, lr)``  Src/ADFL/Strategy/fed_buff.py:88-92 —
  ``tensor.float().div_(K)`` then ``add_parameters(g_params, buffer, 1.0, lr)``;
* ``FadasMoments(...).flush(buffer, g_params, K, lr_t, round)``  Strategy/fadas.py:69-73 — the same average, then
  ``_update_amsgrad`` and ``_compute_model_step``, the moments m, v, v_hat resident on the device between rounds;
* ``FadasMoments(...).receive_flush(channel, c_params, buffer, g_params, K, lr_t, round)`` — the K-th client update
  and that flush in one launch (Strategy/fadas.py:56-80; FedBuff's is ``channel.receive_scaled_flush``): the payload
  is decoded and added to the buffer in registers, so the full buffer is never written or re-read.

Bit-identical to the reference's fp32 statements for FedBuff and for FADAS's moments. FADAS's ``params_prime``
uses the correctly rounded fp32 square root; torch's CPU ``sqrt`` returns the value one ulp below it on about
0.6 % of inputs, which moves about 0.3 % of ``params_prime`` by an ulp or two.

The fusing rule is the channels' (Channel/_base.py ``_apply_groups``): an entry is fused when its buffer and
g_params tensors are fp32, contiguous, 16-byte aligned, of equal shape and non-empty, and both on the staging
device (pointer tables straight to the tensors) or both on the CPU (staged as two buckets, the result handed out
as owned CPU tensors). Every other entry — int64 counters, other dtypes, empty or misaligned tensors, a pair on
two devices — runs the reference's own torch statements. One difference is deliberate: the reference's ``div_``
leaves the averaged buffer in the fp32 buffer tensors before it clears the buffer; the fused entries' buffer
tensors are left as they were (nothing reads them: fed_buff.py:96, fadas.py:75).

Custom ops over flat buckets: ``torch.ops.adfl_apply.fedbuff_flush_batched`` and ``fadas_flush_batched``.
"""

import math
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib, _torchhost, ops
from ._lib import check
from .Channel._staging import _hand_out, _stage_in, _staging

Parameters = Dict[str, torch.Tensor]
Side = Union[torch.Tensor, Sequence[torch.Tensor]]
_F32 = torch.float32


# ------------------------------------------------------------------------------------------------
# the two launches (device-resident operands)
# ------------------------------------------------------------------------------------------------
class _Ptrs:
    """Ready-made device pointers standing in for a side of a launch (the moments' slots of FadasMoments' buckets)."""

    def __init__(self, ptrs: np.ndarray):
        self.ptrs = np.asarray(ptrs, dtype=np.int64)


def _side(side: Side, layout: ops.BucketLayout, dev: torch.device, what: str) -> np.ndarray:
    """One operand's pointers (int64, one per tensor of the layout): `side` is one flat fp32 device bucket in
    `layout` (pointer t = bucket + offset t) or a sequence of T contiguous fp32 device tensors of the layout's
    sizes. Any 4-byte alignment: operands that are not 16-byte aligned take the kernels' element-wise path."""
    if isinstance(side, _Ptrs):
        if side.ptrs.shape != (layout.ntensors,):
            raise ValueError(f"flush: {what} has {side.ptrs.size} pointers, layout {layout.ntensors}")
        return side.ptrs
    if isinstance(side, torch.Tensor):
        if (not side.is_cuda or side.device != dev or side.dtype != _F32 or not side.is_contiguous()
                or side.numel() < layout.total):
            raise ValueError(f"flush: {what} bucket must be a contiguous fp32 tensor of >= {layout.total} elements "
                             f"on {dev}")
        return side.data_ptr() + 4 * layout.offsets
    tensors = list(side)
    if len(tensors) != layout.ntensors:
        raise ValueError(f"flush: {what} has {len(tensors)} tensors, layout {layout.ntensors}")
    try:   # one native call for a whole dict's device, contiguity, element size, counts and pointers
        ok, numel, ptrs = _torchhost.get().device_ptrs(tensors, dev.index, 4)
        if ok and all(x.dtype == _F32 for x in tensors) and np.array_equal(numel.numpy(), layout.sizes):
            return ptrs.numpy()
    except TypeError:
        pass
    for t, (x, n) in enumerate(zip(tensors, layout.sizes.tolist())):
        if (not isinstance(x, torch.Tensor) or not x.is_cuda or x.device != dev or x.dtype != _F32
                or not x.is_contiguous() or x.numel() != n):
            raise ValueError(f"flush: {what} {t} must be a contiguous fp32 tensor of {n} elements on {dev}")
    return np.fromiter((x.data_ptr() for x in tensors), dtype=np.int64, count=len(tensors))


def _device_of(side: Side) -> torch.device:
    t = side if isinstance(side, torch.Tensor) else next(iter(side))
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError("flush: operands must be device tensors")
    return t.device


def _tables(sides: List[Side], names: List[str], layout: ops.BucketLayout, dev: torch.device) -> torch.Tensor:
    """All operands' pointer tables as one device int64 tensor of len(sides) rows (one H2D copy)."""
    rows = np.stack([_side(s, layout, dev, n) for s, n in zip(sides, names)])
    return torch.from_numpy(np.ascontiguousarray(rows)).to(dev, non_blocking=True)


def _check_k(K: int) -> int:
    K = int(K)
    if K < 1 or K > 2**31 - 1:
        raise ValueError(f"flush: max_buffer_size must be in [1, 2^31), got {K}")
    return K


def fedbuff_flush_batched(buf: Side, g: Side, out: Side, layout: ops.BucketLayout, K: int, lr: float) -> None:
    """adfl_fedbuff_flush_batched: for every tensor of `layout`, out = fp32(fp32(1 * g) + fp32(lr * (buf / K)))
    (true division; three separately rounded operations after it). Each operand is a flat fp32 device bucket in
    `layout` or T fp32 device tensors; lr is rounded to fp32 once. The operands must not overlap."""
    dev = _device_of(buf)
    tab = _tables([buf, g, out], ["buf", "g", "out"], layout, dev)
    check(_lib.load().adfl_fedbuff_flush_batched(tab[0].data_ptr(), tab[1].data_ptr(), tab[2].data_ptr(),
                                                 layout.device_chunks(dev).data_ptr(), layout.nchunks,
                                                 layout.ntensors, _check_k(K), float(lr), ops._stream(dev)))
    # `tab` may be freed on return: the caching allocator only reuses it for later work on this stream


def fadas_scalars(beta_1: float, beta_2: float, eps: float, lr_t: float, round: int) -> Tuple[float, ...]:
    """(beta1, 1 - beta1, beta2, 1 - beta2, sqrt(bias_correction_2), eps, step_size) as the Python doubles
    Strategy/fadas.py:97-101,127-128 hands to torch; each is rounded to fp32 once, at the call."""
    bias_correction_1 = 1 - beta_1 ** round
    bias_correction_2 = 1 - beta_2 ** round
    return (beta_1, 1 - beta_1, beta_2, 1 - beta_2, math.sqrt(bias_correction_2), eps, lr_t / bias_correction_1)


def fadas_flush_batched(buf: Side, g: Side, m: Side, v: Side, v_hat: Side, out: Side, layout: ops.BucketLayout,
                        K: int, scalars: Sequence[float]) -> None:
    """adfl_fadas_flush_batched: m, v, v_hat updated in place and `out` written, per element as include/adfl_slq.h
    states it. scalars: fadas_scalars(...). Operands as fedbuff_flush_batched's."""
    dev = _device_of(buf)
    if len(scalars) != 7:
        raise ValueError("fadas_flush_batched: scalars are fadas_scalars()'s seven values")
    tab = _tables([buf, g, m, v, v_hat, out], ["buf", "g", "m", "v", "v_hat", "out"], layout, dev)
    check(_lib.load().adfl_fadas_flush_batched(*(tab[i].data_ptr() for i in range(6)),
                                               layout.device_chunks(dev).data_ptr(), layout.nchunks, layout.ntensors,
                                               _check_k(K), *(float(s) for s in scalars), ops._stream(dev)))


# ------------------------------------------------------------------------------------------------
# state dicts
# ------------------------------------------------------------------------------------------------
def _fusable(b, g) -> bool:
    return (isinstance(b, torch.Tensor) and isinstance(g, torch.Tensor) and b.dtype == _F32 and g.dtype == _F32
            and b.shape == g.shape and b.numel() > 0 and b.is_contiguous() and g.is_contiguous()
            and b.data_ptr() % 16 == 0 and g.data_ptr() % 16 == 0)


def _groups(buffer: Parameters, g_params: Parameters) -> Dict[str, List[str]]:
    """The fused entries as {"cuda": names, "cpu": names} (buffer's key order)."""
    groups: Dict[str, List[str]] = {"cuda": [], "cpu": []}
    if not torch.cuda.is_available():
        return groups
    idx = torch.cuda.current_device()
    for n, b in buffer.items():
        g = g_params[n]
        if not _fusable(b, g):
            continue
        if b.is_cuda and g.is_cuda and b.device.index == idx and g.device.index == idx:
            groups["cuda"].append(n)
        elif not b.is_cuda and not g.is_cuda:
            groups["cpu"].append(n)
    return groups


def _run_group(where: str, bufs: List[torch.Tensor], gs: List[torch.Tensor], launch) -> List[torch.Tensor]:
    """One fused launch over a group's entries: launch(layout, buf side, g side, out side). "cuda": pointer tables
    straight to the tensors, new device tensors out. "cpu": buffer and g staged as two device buckets of one
    64-aligned layout, the result bucket handed out as owned CPU tensors."""
    st = _staging()
    with st.lock, torch.no_grad():
        lay = st.layout(tuple(t.numel() for t in bufs), align=_lib.ALIGN_ELEMS)
        if where == "cuda":
            outs = [torch.empty_like(t) for t in gs]
            launch(lay, bufs, gs, outs)
            return outs
        buf_dev = _stage_in(bufs, lay, st, "fl_buf", _F32)
        g_dev = _stage_in(gs, lay, st, "fl_g", _F32)
        out_dev = st.buf("fl_out", lay.total, _F32)
        launch(lay, buf_dev, g_dev, out_dev)
        return _hand_out(out_dev, lay, [t.shape for t in gs], [True] * len(gs), st, "fl_out")


def fedbuff_flush(buffer: Parameters, g_params: Parameters, max_buffer_size: int, lr: float) -> Parameters:
    """FedBuff's flush, Src/ADFL/Strategy/fed_buff.py:88-92::

        for tensor in buffer.values():
            tensor.float().div_(max_buffer_size)          # fp32 entries only: .float() copies every other dtype
        params_prime = add_parameters(g_params, buffer, 1.0, lr)

    bit-identical to it. Returns params_prime: keys in `buffer`'s order, owned tensors on g_params' device,
    g_params untouched. Fused entries (module docstring) take one launch per device group and their buffer
    tensors are not written; every other entry runs the statements above."""
    assert set(g_params.keys()) == set(buffer.keys())   # add_parameters, model.py:327
    K = _check_k(max_buffer_size)
    out: Parameters = {}
    for where, names in _groups(buffer, g_params).items():
        if names:
            outs = _run_group(where, [buffer[n] for n in names], [g_params[n] for n in names],
                              lambda lay, b, g, o: fedbuff_flush_batched(b, g, o, lay, K, lr))
            out.update(zip(names, outs))
    with torch.no_grad():
        for n, t in buffer.items():
            if n not in out:
                t.float().div_(K)
                g = g_params[n]
                out[n] = (1.0 * g) + (lr * (t if t.device == g.device else t.to(g.device)))
    return {n: out[n] for n in buffer}


class FadasMoments:
    """FADAS's AMSGrad state and its flush (Src/ADFL/Strategy/fadas.py). The strategy keeps its buffer (with
    ``receive_scaled(c, 1.0)`` / ``receive_scaled_add_(c, [buffer], 1.0)`` or the reference's own statements),
    ``_apply_delay_correction`` and the round counter; ``flush`` replaces fadas.py:69-73::

        for tensor in self.buffer.values():
            tensor.float().div_(self.max_buffer_size)
        self._update_amsgrad(agg_info)
        params_prime = self._compute_model_step(agg_info.g_params)

    The moments of the fused entries are created as zeros at the first flush (``_init_moments_if_needed``) and live
    as three device buckets of one 64-aligned layout for the object's lifetime: ``flush`` never copies them to the
    host. Entries that are not fused at the first flush keep ordinary per-entry moment tensors and run the
    reference's statements, dtype promotion included. ``m``, ``v``, ``v_hat`` return CPU dicts on demand."""

    def __init__(self, beta_1: float = 0.9, beta_2: float = 0.999, eps: float = 1e-8) -> None:
        self.beta_1, self.beta_2, self.eps = beta_1, beta_2, eps
        self._order: Optional[List[str]] = None      # g_params' keys at the first flush
        self._fused: List[str] = []                   # ... those whose moments live in the buckets
        self._index: Dict[str, int] = {}
        self._shapes: List[torch.Size] = []
        self._lay: Optional[ops.BucketLayout] = None
        self._buckets: Optional[torch.Tensor] = None  # [3, total]: m, v, v_hat
        self._plain: Dict[str, Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = {}

    def _init(self, buffer: Parameters, g_params: Parameters) -> None:
        groups = _groups(buffer, g_params)
        fused = set(groups["cuda"]) | set(groups["cpu"])
        self._order = list(g_params.keys())
        self._fused = [n for n in buffer if n in fused]
        self._index = {n: i for i, n in enumerate(self._fused)}
        self._shapes = [g_params[n].shape for n in self._fused]
        if self._fused:
            st = _staging()
            self._lay = ops.BucketLayout([int(s.numel()) for s in self._shapes], align=_lib.ALIGN_ELEMS)
            self._buckets = torch.zeros(3, self._lay.total, dtype=_F32, device=st.device)
        for n, g in g_params.items():   # _init_moments_if_needed, for the entries the kernel does not take
            if n not in fused:
                self._plain[n] = tuple(torch.zeros_like(g, dtype=_F32) for _ in range(3))

    def flush(self, buffer: Parameters, g_params: Parameters, max_buffer_size: int, lr_t: float,
              round: int) -> Parameters:
        """params_prime for a full buffer: keys in g_params' order (``_compute_model_step`` walks g_params), owned
        tensors on g_params' device, g_params untouched, the moments advanced by one round. lr_t is
        ``_apply_delay_correction()``'s value and `round` the strategy's counter (1 at the first flush)."""
        assert set(g_params.keys()) == set(buffer.keys())
        K = _check_k(max_buffer_size)
        if self._order is None:
            self._init(buffer, g_params)
        if set(g_params.keys()) != set(self._order):
            raise ValueError("FadasMoments.flush: the state dict's keys changed since the first flush")
        out = self._step(buffer, g_params, K, fadas_scalars(self.beta_1, self.beta_2, self.eps, lr_t, round))
        return {n: out[n] for n in self._order}

    def _step(self, buffer: Parameters, g_params: Parameters, K: int, scalars: Tuple[float, ...]) -> Parameters:
        """``flush`` over the entries of `buffer` (all of the state dict's, or the subset ``receive_flush`` hands
        over): the entries whose moments live in the buckets through one fadas_flush_batched launch per device
        group, the others through ``_plain_step``."""
        out: Parameters = {}
        groups = _groups(buffer, g_params)
        taken = {n for names in groups.values() for n in names}
        for n in self._fused:
            if n in buffer and (n not in taken or g_params[n].shape != self._shapes[self._index[n]]):
                raise ValueError(f"FadasMoments.flush: '{n}' was fused at the first flush (its moments live in the "
                                 "device buckets) and is no longer an aligned fp32 pair of that shape on one side")
        for where, names in groups.items():
            names = [n for n in names if n in self._index]
            if not names:
                continue
            m, v, h = self._moment_ptrs(names)

            def launch(lay, b, g, o, m=m, v=v, h=h):
                fadas_flush_batched(b, g, _Ptrs(m), _Ptrs(v), _Ptrs(h), o, lay, K, scalars)
            out.update(zip(names, _run_group(where, [buffer[n] for n in names], [g_params[n] for n in names],
                                             launch)))
        with torch.no_grad():
            for n in self._order:
                if n in buffer and n not in out:
                    out[n] = self._plain_step(n, buffer[n], g_params[n], K, scalars[4], scalars[6])
        return out

    def _moment_ptrs(self, names: List[str]):
        """The device addresses of the moments of `names` (entries of the buckets): m, v, v_hat."""
        at = 4 * self._lay.offsets[[self._index[n] for n in names]]
        return tuple(int(self._buckets[i].data_ptr()) + at for i in range(3))

    def receive_flush(self, channel, c_params, buffer, g_params: Parameters, max_buffer_size: int, lr_t: float,
                      round: int, *, keep_non_fp32: bool = False) -> Parameters:
        """FADAS's K-th client update, the one that fills the buffer (Src/ADFL/Strategy/fadas.py:56-80):
        ``channel.receive_scaled_add_(c_params, [buffer], 1.0)`` followed by ``flush(buffer, g_params,
        max_buffer_size, lr_t, round)``, bit-identical to the pair, m, v and v_hat included. `buffer` None or empty
        (K = 1) stands for ``channel.receive_scaled(c_params, 1.0)[0]``. Returns params_prime as ``flush`` does.

        An entry the channel fuses (``_apply_groups(c_params, [buffer, g_params])``) whose moments live in the
        buckets is decoded, added to the buffer in registers and stepped by one launch per device group; its
        buffer tensor is left as it was. Every other entry takes today's route: the reference add into the
        caller's buffer tensors, then ``flush``'s launch (a passthrough bias whose moments are in the buckets) or
        its plain statements. The first call creates the moments by ``flush``'s rule; without a buffer the decoded
        update stands in for it: fresh fp32 tensors of the decoded shapes where the payloads live.

        keep_non_fp32=True: the buffer's entries of another dtype (the int64 counter) go into the flush as they were
        before this update, which is what ``add_parameters_inpace(buffer, update, 1, 1, to_float=True)`` leaves
        (fadas.py:60-63: ``.float()`` copies them) and what keeping and restoring them around
        ``receive_scaled_add_`` does."""
        from .Channel._base import _flush_fused
        from .model import QuantParameters
        assert isinstance(c_params, QuantParameters)
        names = list(c_params.params.keys())
        has_buf = bool(buffer)
        if has_buf:
            assert set(buffer.keys()) == set(names)
        assert set(g_params.keys()) == set(names)
        K = _check_k(max_buffer_size)
        if self._order is None:
            self._init(buffer if has_buf else self._stand_in(channel, c_params), g_params)
        if set(g_params.keys()) != set(self._order):
            raise ValueError("FadasMoments.receive_flush: the state dict's keys changed since the first flush")
        scalars = fadas_scalars(self.beta_1, self.beta_2, self.eps, lr_t, round)
        out: Parameters = {}
        for where, ns in channel._flush_groups(c_params, [buffer, g_params] if has_buf else [g_params]):
            ns = [n for n in ns if n in self._index and g_params[n].shape == self._shapes[self._index[n]]]
            if not ns:
                continue
            m, v, h = self._moment_ptrs(ns)
            outs = _flush_fused(channel, c_params, ns, where, buffer if has_buf else None, g_params,
                                lambda launch, b, g, o, m=m, v=v, h=h: launch[1](b, g, _Ptrs(m), _Ptrs(v), _Ptrs(h),
                                                                                o, K, scalars))
            out.update(zip(ns, outs))
        rest = [n for n in names if n not in out]
        if rest:
            sub = QuantParameters({n: c_params.params[n] for n in rest}, 0)
            if has_buf:
                rest_buf = {n: buffer[n] for n in buffer if n not in out}
                keep = {n: t.clone() for n, t in rest_buf.items() if keep_non_fp32 and t.dtype != _F32}
                channel.receive_scaled_add_(sub, [rest_buf], 1.0)
                rest_buf.update(keep)
            else:
                rest_buf, _ = channel.receive_scaled(sub, 1.0)
            out.update(self._step(rest_buf, {n: g_params[n] for n in rest}, K, scalars))
        return {n: out[n] for n in self._order}

    @staticmethod
    def _stand_in(channel, c_params) -> Parameters:
        """What ``channel.receive_scaled(c_params, 1.0)[0]`` would hand ``_init`` at a first flush without a
        buffer, for its classification only: the entries the channel decodes on the device as uninitialised fp32
        tensors of the decoded shape where the payload lives, the others decoded."""
        from .model import QuantParameters
        like: Parameters = {}
        other = {}
        for n, p in c_params.params.items():
            if channel._fusable(p):
                like[n] = torch.empty(torch.Size(channel._apply_shape(p)), dtype=_F32, device=p.data.device)
            else:
                other[n] = p
        if other:
            like.update(channel.receive_scaled(QuantParameters(other, 0), 1.0)[0])
        return {n: like[n] for n in c_params.params}

    def _plain_step(self, n: str, b: torch.Tensor, g: torch.Tensor, K: int, sqrt_bc2: float,
                    step_size: float) -> torch.Tensor:
        """fadas.py:69-70,105-106,127-129 for one entry, as written there."""
        m, v, v_hat = self._plain[n]
        b.float().div_(K)
        if b.device != m.device:
            b = b.to(m.device)
        m.mul_(self.beta_1).add_(b, alpha=(1 - self.beta_1))
        v.mul_(self.beta_2).addcmul_(b, b, value=(1 - self.beta_2))
        torch.maximum(v_hat, v, out=v_hat)
        denom = (v_hat.sqrt() / sqrt_bc2).add_(self.eps)
        return torch.addcdiv(g, m, denom, value=step_size)

    def _dict(self, which: int) -> Parameters:
        if self._order is None:
            return {}
        host = self._buckets[which].cpu() if self._fused else None
        out: Parameters = {}
        for n in self._order:
            if n in self._index:
                i = self._index[n]
                off, size = int(self._lay.offsets[i]), int(self._lay.sizes[i])
                out[n] = host[off:off + size].reshape(self._shapes[i]).clone()
            else:
                out[n] = self._plain[n][which].detach().cpu().clone()
        return out

    @property
    def m(self) -> Parameters:
        """FADAS.m as a CPU dict (a copy: for checkpoints and tests)."""
        return self._dict(0)

    @property
    def v(self) -> Parameters:
        return self._dict(1)

    @property
    def v_hat(self) -> Parameters:
        return self._dict(2)


# ------------------------------------------------------------------------------------------------
# custom ops over flat buckets (torch.ops.adfl_apply.*: the torch.ops.adfl.* set is the codec proper, ops.py)
# ------------------------------------------------------------------------------------------------
def _flat(t: torch.Tensor, lay: ops.BucketLayout, what: str) -> torch.Tensor:
    t = t.reshape(-1)
    if t.dtype != _F32 or not t.is_cuda or not t.is_contiguous() or t.numel() < lay.total:
        raise ValueError(f"{what} must be a contiguous float32 device bucket of >= {lay.total} elements")
    return t


@torch.library.custom_op("adfl_apply::fedbuff_flush_batched", mutates_args=())
def fedbuff_flush_batched_op(buf: torch.Tensor, g: torch.Tensor, offsets: torch.Tensor, sizes: torch.Tensor,
                             K: int, lr: float) -> torch.Tensor:
    """FedBuff's flush per tensor of a caller-placed layout (host int64 offsets / sizes), as a new bucket shaped
    like `g`; positions no tensor owns are zero."""
    lay = ops.layout_for(offsets, sizes)
    buf, g = _flat(buf, lay, "fedbuff_flush_batched: buf"), _flat(g, lay, "fedbuff_flush_batched: g")
    out = ops._filled(g.numel(), _F32, g.device, lay)
    fedbuff_flush_batched(buf, g, out, lay, K, lr)
    return out


@fedbuff_flush_batched_op.register_fake
def _(buf, g, offsets, sizes, K, lr):
    return g.new_empty((g.numel(),), dtype=torch.float32)


@torch.library.custom_op("adfl_apply::fadas_flush_batched", mutates_args=("m", "v", "v_hat"))
def fadas_flush_batched_op(buf: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, v_hat: torch.Tensor,
                           offsets: torch.Tensor, sizes: torch.Tensor, K: int, beta1: float, one_minus_beta1: float,
                           beta2: float, one_minus_beta2: float, sqrt_bc2: float, eps: float,
                           step: float) -> torch.Tensor:
    """FADAS's flush per tensor of a caller-placed layout: m, v, v_hat (flat fp32 buckets) updated in place, the
    new parameters returned as a bucket shaped like `g` (zero where no tensor owns). Scalars: fadas_scalars()."""
    lay = ops.layout_for(offsets, sizes)
    what = "fadas_flush_batched: "
    buf, g = _flat(buf, lay, what + "buf"), _flat(g, lay, what + "g")
    for name, t in (("m", m), ("v", v), ("v_hat", v_hat)):
        if t.dim() != 1:
            raise ValueError(f"{what}{name} must be one-dimensional (it is updated in place)")
        _flat(t, lay, what + name)
    out = ops._filled(g.numel(), _F32, g.device, lay)
    fadas_flush_batched(buf, g, m, v, v_hat, out, lay, K,
                        (beta1, one_minus_beta1, beta2, one_minus_beta2, sqrt_bc2, eps, step))
    return out


@fadas_flush_batched_op.register_fake
def _(buf, g, m, v, v_hat, offsets, sizes, K, beta1, one_minus_beta1, beta2, one_minus_beta2, sqrt_bc2, eps, step):
    return g.new_empty((g.numel(),), dtype=torch.float32)
