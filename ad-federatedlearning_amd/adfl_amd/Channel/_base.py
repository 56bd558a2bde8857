"""What the SLQ channels (quant.py) and the stochastic channels (stoch.py) share above the staging layer:
``_CodecChannel``, the class skeleton of a bi-directional codec channel (the reference's six-method surface,
``receive_add_``, ``receive_mean``, the synchronous DELTA server's ``receive_mean_axpby`` and the asynchronous
server's ``receive_axpby`` / ``receive_scaled`` / ``receive_scaled_add_`` / ``receive_scaled_flush`` around the
codec's hooks); ``_Unidirectional``, the mix-in of the
uni-directional variants; and the host aggregate of the entries no device kernel takes (``_aggregate_entries``,
``device_mean_order_ok``).

An instance holds only what its constructor was given (``bits``; the stochastic channels add ``levels``): it
is pickled into every Ray actor. Device state lives in the staging layer's per-process cache.
"""

import time
from typing import Dict, List, Tuple

import numpy as np
import torch

from .. import _torchhost, ops, sum_order
from ..model import CompressedParameters, Parameters, QuantParameter, QuantParameters, get_parameter_info
from ._staging import _hand_out, _serialized, _stage_in, _stage_out, _staging
from .channel import Channel, IdentityChannel


def _simple_aggregate(values: List[torch.Tensor]) -> torch.Tensor:
    """One entry of simple_aggregate (Src/ADFL/model.py:221-234), as the reference computes it."""
    with torch.no_grad():
        return torch.sum(torch.stack(values, dim=0), dim=0) / len(values)


def device_mean_order_ok() -> bool:
    """The device mean kernels follow torch's CPU sum(dim=0) order as ATen's AVX2 kernel takes it
    (csrc/torch_sum_order.h). If this process's torch sums in another order (sum_order.self_check fails:
    another torch build or CPU kernel), receive_mean decodes and aggregates every entry on the host the
    reference's way instead, so the device and host halves of one aggregate never disagree; warned once."""
    ok = sum_order.self_check()
    if not ok and not _ORDER_WARNED[0]:
        _ORDER_WARNED[0] = True
        import warnings
        warnings.warn("adfl_amd: this torch's CPU sum order differs from the one the device mean kernels "
                      "restate; receive_mean aggregates on the host (bit-identical, slower)", RuntimeWarning)
    return ok


_ORDER_WARNED = [False]


def _aggregate_entries(names: List[str], parts: List[Parameters]) -> Dict[str, torch.Tensor]:
    """simple_aggregate over the entries `names` of the K dicts `parts` (host tensors: biases, running
    statistics, counters), with the per-entry call's values but not its per-entry dispatch cost (256
    biases: about 3 ms of stack / sum / div). Entries of one dtype are concatenated into K rows and summed
    together: int64 with K elementwise adds (integer sums are exact in any order), fp32 in torch's own CPU
    summation order (adfl_amd.sum_order: each entry's columns in the order its own
    torch.sum(torch.stack(...), 0) takes, bit for bit; checked against torch once per process,
    sum_order.self_check). Then one division and a split into owned tensors. One-element fp32 entries at
    K >= 8 (torch's inner-sum kernel) and everything else go through simple_aggregate per entry."""
    k = len(parts)
    res: Dict[str, torch.Tensor] = {}
    f32_ok = sum_order.self_check()
    lists = [[p[n] for n in names] for p in parts]
    if names and all(isinstance(v, torch.Tensor) for row in lists for v in row):
        # the classification, the K rows and the owned results in native calls (adfl_torchhost)
        th = _torchhost.get()
        uni, code, numel = (a.numpy() for a in th.entry_meta_k(lists))
        f32 = uni & (code == 0) & f32_ok & (numel > 0) & ~((numel == 1) & (k >= 8))
        with torch.no_grad():
            for sel, is_f32 in ((f32, True), (uni & (code == 1), False)):
                idx = np.nonzero(sel)[0]
                if idx.size < 2:
                    continue
                rows = th.concat_rows(lists, torch.from_numpy(idx))
                if is_f32:
                    acc = sum_order.sum_rows(rows, numel[idx].tolist())
                else:   # int64: K elementwise adds from zero (exact in any order)
                    acc = torch.zeros_like(rows[0])
                    for r in rows.unbind(0):
                        acc = acc + r
                agg = acc / k
                for i, t in zip(idx.tolist(), th.split_owned(agg, [lists[0][i] for i in idx.tolist()])):
                    res[names[i]] = t
        for n in names:
            if n not in res:
                res[n] = _simple_aggregate([p[n] for p in parts])
        return res
    groups: Dict[torch.dtype, List[str]] = {}
    for n in names:
        vals = [p[n] for p in parts]
        t0 = vals[0]
        if not all(isinstance(v, torch.Tensor) and not v.is_cuda and v.is_contiguous() and v.dtype == t0.dtype
                   and v.shape == t0.shape for v in vals):
            continue
        if t0.dtype == torch.int64 or (t0.dtype == torch.float32 and f32_ok and t0.numel() > 0
                                       and not (t0.numel() == 1 and k >= 8)):
            groups.setdefault(t0.dtype, []).append(n)
    with torch.no_grad():
        for dt, ns in groups.items():
            if len(ns) < 2:
                continue
            sizes = [parts[0][n].numel() for n in ns]
            if dt == torch.int64:
                rows = [torch.cat([p[n].reshape(-1) for n in ns]) for p in parts]
                acc = torch.zeros_like(rows[0])
                for r in rows:
                    acc = acc + r
            else:
                stacked = torch.stack([torch.cat([p[n].reshape(-1) for n in ns]) for p in parts])
                acc = sum_order.sum_rows(stacked, sizes)
            agg = acc / k
            for n, piece in zip(ns, torch.split(agg, sizes)):
                shape = parts[0][n].shape
                res[n] = (piece if piece.shape == shape else piece.view(shape)).clone()
    for n in names:
        if n not in res:
            res[n] = _simple_aggregate([p[n] for p in parts])
    return res


def _passthrough_idle(entries, made: Dict[str, QuantParameter], size: List[int], bits: int, scale, signs, *tail):
    """_quantize_params' idle(): each call turns up to `batch` of the passthrough `entries` (name, tensor) into
    payload objects in `made` (the tensor itself as data, `scale`, the shared unused `signs`, `tail`: the
    fields after q_dtype), counts their bytes in size[0], and returns True while entries are left. The
    pipelined host encodes call it between staging ranges."""
    rest = iter(entries)
    qp = QuantParameter

    def idle(batch=32):
        for _ in range(batch):
            e = next(rest, None)
            if e is None:
                return False
            t = e[1]
            made[e[0]] = qp(t, bits, scale, signs, t.shape, t.dtype, t.dtype, *tail)
            size[0] += t.nbytes
        return True
    return idle


class _CodecChannel(Channel):
    """A bi-directional codec channel; ``receive_add_`` and ``receive_mean`` are written once around the
    codec's part, which a subclass supplies:

    * ``_quantize_params(params, bits)`` -> QuantParameters, ``_receive(c_params)`` -> (Parameters, seconds);
    * ``_mean_host_updates(all_c_params, names)``: receive_mean's common case (K CPU updates of one model)
      classified in a few native calls -> (fused names, their means, the passthrough names or None), or None
      when the updates are anything else (they are then classified entry by entry, with the hooks below);
    * ``_fusable(p)``: an entry the decode-mean launch takes; ``_mean_shape(p)``: its decoded shape (one shape
      across the updates fuses); ``_mean_payloads(all_c_params, names)``: the means of such entries;
    * ``_mean_host_classify(all_c_params, names)`` and ``_mean_apply(...)``: that classification without the launch,
      and the fused decode-mean + axpby over such entries and their base tensors (receive_mean_axpby);
    * ``_passthrough(p)``: _receive hands this entry back as its own payload tensor;
    * ``_apply_payload(c_params, names, st)``: the ``_fusable`` entries' payloads staged on the device and the
      codec's fused decode + axpby over them — what receive_axpby, receive_scaled, receive_scaled_add_ (the
      asynchronous server's update step) and receive_add_ (the same launch in place with alpha = beta = 1) are
      written around;
    * ``_flush_payload(c_params, names, st)``: the same staging with the codec's fused decode + accumulate + flush
      (receive_scaled_flush, FadasMoments.receive_flush), for the entries ``_flush_groups`` names."""

    SIGN_BITS = 0    # sent per weight beside its `bits` (the stochastic codecs' sign plane: 1)
    NORM_BYTES = 4   # sent per quantized tensor: its scale or norm (RQSGD: norm + minimum factor, 8)

    def __init__(self, bits: int) -> None:
        self.bits = bits

    def on_server_send(self, params: Parameters) -> Tuple[CompressedParameters, float]:
        return self._send(params)

    def on_server_receive(self, c_params: CompressedParameters) -> Tuple[Parameters, float]:
        return self._receive(c_params)

    def on_client_send(self, params: Parameters) -> Tuple[CompressedParameters, float]:
        return self._send(params)

    def on_client_receive(self, c_params: CompressedParameters) -> Tuple[Parameters, float]:
        return self._receive(c_params)

    def to_json(self) -> Dict:
        return {"name": self.__class__.__name__, "bits": self.bits}

    def simulate_bandwidth(self, params: Parameters, mbps: float) -> float:
        """self.bits (+ SIGN_BITS) for weights, 32 bits for biases, NORM_BYTES per quantized tensor
        (quant.py:47-58,173-184,313-324,459-470)."""
        p_info = get_parameter_info(params)
        num_bytes = p_info.num_non_bias_w * (self.bits + self.SIGN_BITS) / 8
        num_bytes += p_info.num_bias_w * 4
        num_bytes += p_info.num_non_bias_t * self.NORM_BYTES
        transfer_time = num_bytes / (mbps * 1_000_000 / 8)
        time.sleep(transfer_time)
        return transfer_time

    def _send(self, params: Parameters) -> Tuple[CompressedParameters, float]:
        s_time = time.perf_counter()
        q_params = self._quantize_params(params, self.bits)
        return q_params, time.perf_counter() - s_time

    def receive_add_(self, c_params: CompressedParameters, targets: List[Parameters]) -> float:
        """``on_client_receive(c_params)`` followed by ``add_parameters_inpace(t, decoded, 1, 1, False)`` for
        every ``t`` in ``targets`` — the client pool's ``add_to_model`` / ``add_to_model_all``
        (Src/ADFL/Client/pool.py:62-75) and QAFeL's hidden-state update (Src/ADFL/Server/qafel.py:176-179),
        bit-identical to them. Returns the seconds spent.

        The entries ``_apply_groups`` names whose targets all live on the staging device are decoded once there
        and added into every model by the codec's fused decode + axpby launch with alpha = beta = 1
        (``_apply_payload``: fp32(fp32(1 * t) + fp32(1 * d)) is fp32(t + d); no decoded tensor is written or crosses
        PCIe). Everything else, CPU targets included, takes the reference's route: decode, then
        ``mul_(1).add_(decoded, alpha=1)``."""
        return self._add_inplace(c_params, targets, None)

    def broadcast_delta_(self, hidden_state: Parameters,
                         params_new: Parameters) -> Tuple[CompressedParameters, float]:
        """QAFeL's broadcast (Src/ADFL/Server/qafel.py:156-180): ``_broadcast_update``'s encode and
        ``_update_hidden_state`` in one call. Returns (c_params, seconds):

        * c_params equals ``on_server_send(diff_parameters(hidden_state, params_new))[0]`` field for field, in
          hidden_state's key order, and the same errors are raised (send_delta's);
        * afterwards hidden_state holds what ``add_parameters_inpace(hidden_state,
          on_client_receive(c_params)[0], 1, 1, False)`` leaves: updated in place, the same tensor objects;
        * params_new is not modified.

        Here: ``send_delta`` then ``receive_add_(c_params, [hidden_state])``, drawing the one random stream that
        pair draws. The SLQ channels (quant.py) and the stochastic channels (stoch.py) fuse the two on a
        device-resident hidden state."""
        s_time = time.perf_counter()
        c_params, _ = self.send_delta(hidden_state, params_new)
        self.receive_add_(c_params, [hidden_state])
        return c_params, time.perf_counter() - s_time

    def receive_mean(self, all_c_params: List[CompressedParameters]) -> Tuple[Parameters, float]:
        """``simple_aggregate([self.on_server_receive(c)[0] for c in all_c_params])`` — a synchronous
        server decoding K client updates and averaging them (Src/ADFL/Strategy/simple.py:83-89 over
        Src/ADFL/model.py:221-234; the peer mean of Examples/ray_ad.py:188). Returns (aggregate, seconds).

        Entries encoded in every update (``_fusable``, one shape) are decoded and averaged on the device in
        one launch: the K payloads are read once and no decoded copy is materialised. Their mean is summed in
        torch's CPU order for ``torch.sum(torch.stack(...), dim=0)`` (csrc/torch_sum_order.h: per tensor, a
        16-row cascade over the SEQ columns, four interleaved partials over each tensor's last n % 32
        elements), then / K correctly rounded: bit-identical to simple_aggregate on CPU tensors (as the
        reference runs it, model.py:195-197) for every K (tests/golden/aggregate.npz: the reference executed
        at K = 1 .. 64; the stochastic codecs' own payloads at K = 5, 8, 16, 20). Everything else (biases,
        running statistics, empty or non-quantized payloads) is decoded and aggregated as the reference does,
        on the host, in the same order."""
        if not all_c_params:
            raise AssertionError("receive_mean: no updates")   # simple_aggregate asserts len > 0
        for c in all_c_params:
            assert isinstance(c, QuantParameters)
        s_time = time.perf_counter()
        names = list(all_c_params[0].params.keys())
        order_ok = device_mean_order_ok()
        out: Parameters = {}
        fast = self._mean_host_updates(all_c_params, names) if order_ok else None
        plain = None
        if fast is not None:   # every update a CPU dict of the same entries: classified in native calls
            fused, decoded, plain = fast
            out.update(zip(fused, decoded))
        else:
            fused = self._mean_fused_names(all_c_params, names) if order_ok else []
            if fused:
                out.update(zip(fused, self._mean_payloads(all_c_params, fused)))
        rest = [n for n in names if n not in out]
        if rest:
            # passthrough entries decode to their own payload tensor (quant.py:111-112): used as they are
            # (the values _receive hands back, without its per-entry work); the rest through _receive
            if plain is None:
                plain = [n for n in rest if all(self._passthrough(c.params[n]) for c in all_c_params)]
            skip = set(plain)
            other = [n for n in rest if n not in skip]
            parts = []
            for c in all_c_params:
                part = {n: c.params[n].data for n in plain}
                if other:
                    part.update(self._receive(QuantParameters({n: c.params[n] for n in other}, 0))[0])
                parts.append(part)
            out.update(_aggregate_entries(rest, parts))
        return {n: out[n] for n in names}, time.perf_counter() - s_time

    def _mean_fused_names(self, all_c_params: List[QuantParameters], names: List[str]) -> List[str]:
        """The entries the decode-mean launch takes: ``_fusable`` in every update, one decoded shape."""
        return [n for n in names if all(n in c.params and self._fusable(c.params[n]) for c in all_c_params)
                and len({tuple(self._mean_shape(c.params[n])) for c in all_c_params}) == 1]

    # -- the synchronous DELTA server's step: decode-mean + axpby ---------------------------------------------
    def receive_mean_axpby(self, all_c_params: List[CompressedParameters], base: Parameters, alpha: float = 1.0,
                           beta: float = 1.0) -> Tuple[Parameters, float]:
        """``add_parameters(base, simple_aggregate([self.on_server_receive(c)[0] for c in all_c_params]), alpha,
        beta)`` — ``Simple(CommType.DELTA, sync=True)._sync_update`` with (1.0, 1.0)
        (Src/ADFL/Strategy/simple.py:87-89 over Src/ADFL/model.py:221-234,326-334), bit-identical to it: per element
        fp32(fp32(alpha * base) + fp32(beta * mean)), the mean as ``receive_mean`` computes it. Returns (new
        parameters, seconds); keys in the first update's order, `base` and the payloads unmodified, every returned
        tensor its own storage, living where its base entry lives.

        An entry ``receive_mean`` would average on the device (``_fusable`` in every update, one shape, torch's
        sum order as the kernels restate it) whose base tensor is fp32, contiguous, 16-byte aligned and of the
        decoded shape is decoded, averaged and combined by one launch (``_mean_apply``): the K payloads and the
        base are read once, no mean is written. Bases on the staging device are read in place; CPU bases (ADFL's
        own pattern) are staged by one H2D into a bucket of the mean's layout and come back as owned CPU tensors.
        Every other entry takes ``receive_mean``, then the reference's statement ``(alpha * base) + (beta *
        mean)``, so dtype promotion is torch's (the int64 counter comes back fp32)."""
        if not all_c_params:
            raise AssertionError("receive_mean_axpby: no updates")   # simple_aggregate asserts len > 0
        for c in all_c_params:
            assert isinstance(c, QuantParameters)
        names = list(all_c_params[0].params.keys())
        assert set(base.keys()) == set(names)   # add_parameters, model.py:327
        s_time = time.perf_counter()
        out: Parameters = {}
        if device_mean_order_ok() and torch.cuda.is_available():
            cls = self._mean_host_classify(all_c_params, names)
            fused = cls[0] if cls is not None else self._mean_fused_names(all_c_params, names)
            dev_idx = torch.cuda.current_device()
            groups: Dict[str, List[str]] = {"cuda": [], "cpu": []}
            for n in fused:
                t = base[n]
                if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.is_contiguous()
                        and t.data_ptr() % 16 == 0
                        and t.shape == torch.Size(self._mean_shape(all_c_params[0].params[n]))):
                    continue
                if t.is_cuda and t.device.index == dev_idx:
                    groups["cuda"].append(n)
                elif not t.is_cuda:
                    groups["cpu"].append(n)
            for where, ns in groups.items():
                if ns:
                    host = cls if cls is not None and len(ns) == len(cls[0]) else None
                    out.update(zip(ns, self._mean_apply(all_c_params, ns, [base[n] for n in ns], where, alpha, beta,
                                                        host)))
        rest = {n for n in names if n not in out}
        if rest:
            agg, _ = self.receive_mean([QuantParameters({n: p for n, p in c.params.items() if n in rest}, 0)
                                        for c in all_c_params])
            with torch.no_grad():
                for n, m in agg.items():
                    out[n] = (alpha * base[n]) + (beta * m.to(base[n].device))
        return {n: out[n] for n in names}, time.perf_counter() - s_time

    def _mean_host_classify(self, all_c_params: List[QuantParameters], names: List[str]):
        """``_mean_host_updates``' classification without its launch, where a codec has one in native calls:
        (fused names, ...the codec's own staging arguments) for K CPU updates of one model, else None."""
        return None

    def _mean_apply(self, all_c_params: List[QuantParameters], names: List[str], bases: List[torch.Tensor],
                    where: str, alpha: float, beta: float, host) -> List[torch.Tensor]:
        """The fused decode-mean + axpby over the entries `names` (``_mean_fused_names``' kind) and their base
        tensors, all on the staging device (where == "cuda") or all on the CPU ("cpu"): one new owned tensor per
        entry, where its base lives. host: ``_mean_host_classify``'s result when it covers exactly `names`."""
        raise NotImplementedError

    # -- the asynchronous server's update step: decode + axpby / scale ---------------------------------------
    def receive_axpby(self, c_params: CompressedParameters, base: Parameters, alpha: float,
                      beta: float) -> Tuple[Parameters, float]:
        """``add_parameters(base, self.on_server_receive(c_params)[0], alpha, beta)`` (Src/ADFL/model.py:326-334)
        — FedAsync's update with (1 - alpha_t, alpha_t) (Src/ADFL/Strategy/fed_async.py:80-81) and Simple
        DELTA's with (1.0, 1.0) (Strategy/simple.py:100), bit-identical to them: per element
        fp32(fp32(alpha * base) + fp32(beta * decoded)). Returns (sum, seconds); keys in c_params' order, `base`
        unmodified, every returned tensor its own storage.

        The entries ``_receive`` decodes on the device whose base tensor is fp32, contiguous and 16-byte aligned
        (all of them on the staging device, or all on the CPU) are decoded and combined by one launch
        (``_apply_payload``): no decoded tensor is written. Every other entry takes the reference's route:
        decode, then ``(alpha * base) + (beta * decoded)``."""
        assert isinstance(c_params, QuantParameters)
        assert set(base.keys()) == set(c_params.params.keys())   # add_parameters, model.py:327
        s_time = time.perf_counter()
        out: Parameters = {}
        for where, names in self._apply_groups(c_params, [base]):
            out.update(zip(names, _apply_fused(self, c_params, names, where, [base], False, alpha, beta)))
        rest = QuantParameters({n: p for n, p in c_params.params.items() if n not in out}, 0)
        if rest.params:
            decoded, _ = self.on_server_receive(rest)
            with torch.no_grad():
                for n, d in decoded.items():
                    out[n] = (alpha * base[n]) + (beta * d.to(base[n].device))
        return {n: out[n] for n in c_params.params}, time.perf_counter() - s_time

    def receive_scaled(self, c_params: CompressedParameters, factor: float) -> Tuple[Parameters, float]:
        """``self.on_server_receive(c_params)[0]`` after FedBuff's staleness scaling ``for t in D.values():
        t.float().mul_(factor)`` (Src/ADFL/Strategy/fed_buff.py:72-75) — the update that becomes the buffer: per
        element fp32(factor * decoded), so a -0.0 stays -0.0. fp32 entries are scaled; ``.float()`` copies every
        other dtype, which is therefore left as it is, as in the reference. Returns (update, seconds)."""
        assert isinstance(c_params, QuantParameters)
        s_time = time.perf_counter()
        out: Parameters = {}
        for where, names in self._apply_groups(c_params, None):
            out.update(zip(names, _apply_fused(self, c_params, names, where, None, False, 1.0, factor)))
        rest = QuantParameters({n: p for n, p in c_params.params.items() if n not in out}, 0)
        if rest.params:
            decoded, _ = self.on_server_receive(rest)
            with torch.no_grad():
                for t in decoded.values():
                    t.float().mul_(factor)
            out.update(decoded)
        return {n: out[n] for n in c_params.params}, time.perf_counter() - s_time

    def receive_scaled_add_(self, c_params: CompressedParameters, targets: List[Parameters], factor: float) -> float:
        """For every ``t`` in ``targets``: FedBuff's scaling of the decoded update (receive_scaled) followed by
        ``add_parameters_inpace(t, decoded, 1, 1, False)`` (Src/ADFL/Strategy/fed_buff.py:72-80) — the later
        updates of a buffer: per element fp32(t + fp32(factor * decoded)). With factor == 1.0 it equals
        ``receive_add_``. Returns the seconds spent."""
        return self._add_inplace(c_params, targets, factor)

    def _add_inplace(self, c_params: CompressedParameters, targets: List[Parameters], factor) -> float:
        """The one body of receive_add_ (factor None: the client's side, ``on_client_receive``, and only the
        targets on the staging device fuse) and receive_scaled_add_ (the server's side, ``on_server_receive``, the
        decoded update scaled first): ``_apply_groups``' entries by the fused in-place decode + axpby
        (1.0, factor), the remainder by the reference's torch statements."""
        assert isinstance(c_params, QuantParameters)
        for t in targets:
            assert set(t.keys()) == set(c_params.params.keys())  # add_parameters_inpace, model.py:340
        s_time = time.perf_counter()
        scaled = factor is not None
        done = set()
        if targets:
            for where, names in self._apply_groups(c_params, targets):
                if scaled or where == "cuda":
                    _apply_fused(self, c_params, names, where, targets, True, 1.0, factor if scaled else 1.0)
                    done.update(names)
        rest = QuantParameters({n: p for n, p in c_params.params.items() if n not in done}, 0)
        if rest.params:
            decoded, _ = (self.on_server_receive if scaled else self.on_client_receive)(rest)
            with torch.no_grad():
                if scaled:
                    for d in decoded.values():
                        d.float().mul_(factor)
                for t in targets:
                    for n, d in decoded.items():
                        t[n].mul_(1).add_(d.to(t[n].device), alpha=1)
        return time.perf_counter() - s_time

    def receive_scaled_flush(self, c_params: CompressedParameters, buffer, g_params: Parameters, factor: float,
                             max_buffer_size: int, lr: float) -> Tuple[Parameters, float]:
        """FedBuff's K-th client update, the one that fills the buffer (Src/ADFL/Strategy/fed_buff.py:68-100):
        ``receive_scaled_add_(c_params, [buffer], factor)`` followed by ``flush.fedbuff_flush(buffer, g_params,
        max_buffer_size, lr)``, bit-identical to the pair. `buffer` None or empty — K = 1, or the moment a strategy
        would set ``self.buffer = c_update`` — stands for ``receive_scaled(c_params, factor)[0]``. Returns
        (params_prime, seconds): keys, devices and owned storages as ``fedbuff_flush`` returns them, g_params
        untouched.

        The entries ``_apply_groups(c_params, [buffer, g_params])`` names are decoded, scaled, added to the buffer
        in registers, averaged and stepped by one launch per device group (``_flush_payload``): their buffer
        tensors are read and left as they were, which is the flush's documented rule (the strategy clears the
        buffer next). Every other entry takes today's route restricted to those names: the reference add into the
        caller's buffer tensors, then ``fedbuff_flush``."""
        from .. import flush   # flush stages through this package
        assert isinstance(c_params, QuantParameters)
        names = list(c_params.params.keys())
        has_buf = bool(buffer)
        if has_buf:
            assert set(buffer.keys()) == set(names)      # add_parameters_inpace, model.py:340
        assert set(g_params.keys()) == set(names)        # add_parameters, model.py:327
        K = flush._check_k(max_buffer_size)
        s_time = time.perf_counter()
        out: Parameters = {}
        for where, ns in self._flush_groups(c_params, [buffer, g_params] if has_buf else [g_params]):
            outs = _flush_fused(self, c_params, ns, where, buffer if has_buf else None, g_params,
                                lambda launch, b, g, o: launch[0](b, g, o, K, factor, lr))
            out.update(zip(ns, outs))
        rest = [n for n in names if n not in out]
        if rest:
            sub = QuantParameters({n: c_params.params[n] for n in rest}, 0)
            if has_buf:
                rest_buf = {n: buffer[n] for n in buffer if n not in out}
                self.receive_scaled_add_(sub, [rest_buf], factor)
            else:
                rest_buf, _ = self.receive_scaled(sub, factor)
            out.update(flush.fedbuff_flush(rest_buf, {n: g_params[n] for n in rest}, K, lr))
        order = buffer if has_buf else c_params.params
        return {n: out[n] for n in order}, time.perf_counter() - s_time

    def _apply_groups(self, c_params: QuantParameters, models):
        """The fused entries of receive_axpby / receive_scaled / receive_scaled_add_ / receive_add_ as [("cuda" |
        "cpu", names)] (receive_add_ fuses the "cuda" group only):
        entries _receive would decode on the device (``_fusable``) whose tensor in every model of `models` is
        fp32, contiguous, 16-byte aligned, of the decoded shape, and with the others either on the staging device
        or on the CPU. models None (receive_scaled): grouped by where the payload, hence the decoded tensor,
        lives."""
        dev_idx = torch.cuda.current_device() if torch.cuda.is_available() else None
        groups: Dict[str, List[str]] = {"cuda": [], "cpu": []}
        if dev_idx is None:
            return []
        for n, p in c_params.params.items():
            if not self._fusable(p):
                continue
            shape = torch.Size(self._apply_shape(p))
            if models is None:
                ts = [p.data]
            else:
                ts = [m[n] for m in models]
                if not all(isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.shape == shape
                           and t.is_contiguous() and t.data_ptr() % 16 == 0 for t in ts):
                    continue
            if all(t.is_cuda and t.device.index == dev_idx for t in ts):
                groups["cuda"].append(n)
            elif not any(t.is_cuda for t in ts):
                groups["cpu"].append(n)
        return [(w, ns) for w, ns in groups.items() if ns]

    def _flush_groups(self, c_params: QuantParameters, models):
        """The fused entries of receive_scaled_flush and flush.FadasMoments.receive_flush: ``_apply_groups``' where
        the codec has a fused decode + accumulate + flush (``_flush_payload``); a codec without one returns []."""
        return self._apply_groups(c_params, models)

    def _apply_shape(self, p: QuantParameter):
        """The decoded shape of a ``_fusable`` entry."""
        return self._mean_shape(p)

    def _apply_payload(self, c_params: QuantParameters, names: List[str], st):
        """Stage the payloads of `names` on the device: (element layout, launch), launch(bases, outs, alpha, beta)
        running the codec's fused decode + axpby over them (ops.dequantize_axpby_batched's bases / outs)."""
        raise NotImplementedError

    def _flush_payload(self, c_params: QuantParameters, names: List[str], st):
        """``_apply_payload``'s staging of the payloads of `names`, and the codec's fused decode + accumulate + flush
        over them: (element layout, (fedbuff, fadas)) with fedbuff(buf, g, out, K, factor, lr) and fadas(buf, g, m,
        v, v_hat, out, K, scalars) taking ops.dequantize_fedbuff_flush_batched's operands (buf None: no buffer)."""
        raise NotImplementedError

    @staticmethod
    def _mean_shape(p: QuantParameter):
        return p.shape

    def _passthrough(self, p: QuantParameter) -> bool:
        return False


@_serialized
def _apply_fused(channel: "_CodecChannel", c_params: QuantParameters, names: List[str], where: str, models,
                 inplace: bool, alpha: float, beta: float):
    """One fused decode + axpby / scale over the entries `names` (receive_axpby, receive_scaled,
    receive_scaled_add_): the payload staged once into an aligned bucket (``_apply_payload``), then
      where == "cuda": one launch over pointer tables straight to the K models' tensors, writing the models
                       themselves (inplace) or new device tensors;
      where == "cpu":  ADFL's own pattern (get_model_parameters hands out CPU dicts): per model, its tensors
                       staged into a bucket of the same layout, one launch over the two flat buckets, and the
                       result copied back into the model (inplace) or handed out as owned CPU tensors.
    models None: SCALE (no base). Returns the new tensors of the one model (not inplace), else None."""
    st = _staging()
    dev = st.device
    stream = torch.cuda.current_stream(dev)
    lay, launch = channel._apply_payload(c_params, names, st)
    # the in-place device update (receive_add_, receive_scaled_add_) creates nothing
    shapes = None if where == "cuda" and inplace else [torch.Size(channel._apply_shape(c_params.params[n]))
                                                       for n in names]
    outs = None
    with torch.no_grad():
        if where == "cuda":
            bases = None if models is None else [[m[n] for n in names] for m in models]
            if inplace:
                launch(bases, bases, alpha, beta)
            else:
                outs = [torch.empty(s, dtype=torch.float32, device=dev) for s in shapes]
                launch(bases, [outs], alpha, beta)
            # the next call's host gather rewrites the pinned staging this call's H2D reads from
            stream.synchronize()
            return outs
        out_dev = st.buf("ax_out", lay.total, torch.float32)
        if models is None:
            launch(None, out_dev, alpha, beta)
            return _hand_out(out_dev, lay, shapes, [True] * len(names), st, "ax_out")
        for m in models:
            tensors = [m[n] for n in names]
            base_dev = _stage_in(tensors, lay, st, "ax_base", torch.float32)
            launch(base_dev, out_dev, alpha, beta)
            if inplace:
                _stage_out(out_dev, lay, st, "ax_out", tensors)
            else:
                outs = _hand_out(out_dev, lay, shapes, [True] * len(names), st, "ax_out")
    return outs


@_serialized
def _flush_fused(channel: "_CodecChannel", c_params: QuantParameters, names: List[str], where: str, buffer,
                 g_params: Parameters, run) -> List[torch.Tensor]:
    """One fused decode + accumulate + flush over the entries `names` (receive_scaled_flush,
    flush.FadasMoments.receive_flush): the payload staged once into an aligned bucket (``_flush_payload``), then
    run(launch, buf side, g side, out side) with launch the codec's (fedbuff, fadas) pair:
      where == "cuda": pointer tables straight to the buffer's and g_params' tensors, new device tensors out;
      where == "cpu":  the buffer and g_params staged as two device buckets of the payload's layout, the result
                       bucket handed out as owned CPU tensors — the updated buffer never exists, so the D2H of the
                       buffer and its H2D for the flush are gone with it.
    buffer None: no buffer. Returns the new tensors, one per name."""
    st = _staging()
    dev = st.device
    lay, launch = channel._flush_payload(c_params, names, st)
    shapes = [torch.Size(channel._apply_shape(c_params.params[n])) for n in names]
    gs = [g_params[n] for n in names]
    bufs = None if buffer is None else [buffer[n] for n in names]
    with torch.no_grad():
        if where == "cuda":
            outs = [torch.empty(s, dtype=torch.float32, device=dev) for s in shapes]
            run(launch, bufs, gs, outs)
            # the next call's host gather rewrites the pinned staging this call's H2D reads from
            torch.cuda.current_stream(dev).synchronize()
            return outs
        buf_dev = None if bufs is None else _stage_in(bufs, lay, st, "rf_buf", torch.float32)
        g_dev = _stage_in(gs, lay, st, "rf_g", torch.float32)
        out_dev = st.buf("rf_out", lay.total, torch.float32)
        run(launch, buf_dev, g_dev, out_dev)
        return _hand_out(out_dev, lay, shapes, [True] * len(names), st, "rf_out")


def _mean_axpby_out(st, lay: ops.BucketLayout, shapes, bases: List[torch.Tensor], where: str, key: str, launch,
                    like=None) -> List[torch.Tensor]:
    """The output side of a fused decode-mean + axpby whose payload rows are staged (``_mean_apply``):
    launch(bases, outs) runs the codec's kernel over ops.dequantize_mean_axpby_batched's bases / outs.
      where == "cuda": pointer tables straight to the base tensors and to new device tensors;
      where == "cpu":  the bases staged by one H2D into a bucket of the rows' element layout, one launch over the
                       two flat buckets, the result handed out as owned CPU tensors (`like`: as _hand_out)."""
    dev = st.device
    with torch.no_grad():
        if where == "cuda":
            outs = [torch.empty(s, dtype=torch.float32, device=dev) for s in shapes]
            launch(bases, outs)
            # the next call's host gather rewrites the pinned staging this call's H2D reads from
            torch.cuda.current_stream(dev).synchronize()
            return outs
        base_dev = _stage_in(bases, lay, st, "ma_base", torch.float32)
        out_dev = st.buf(key, lay.total, torch.float32)
        launch(base_dev, out_dev)
        return _hand_out(out_dev, lay, shapes, [True] * len(bases), st, key, like=like)


class _Unidirectional:
    """Only client -> server is compressed; server -> client and the client's receive use the identity
    channel (quant.py:115-137,255-277,401-423,548-570)."""

    def on_server_send(self, params: Parameters) -> Tuple[CompressedParameters, float]:
        return IdentityChannel(no_compute_time=True).on_server_send(params)

    def on_client_receive(self, c_params: CompressedParameters) -> Tuple[Parameters, float]:
        return IdentityChannel(no_compute_time=True).on_client_receive(c_params)

    def broadcast_delta_(self, hidden_state: Parameters,
                         params_new: Parameters) -> Tuple[CompressedParameters, float]:
        """The server -> client direction is the identity channel, so there is nothing to encode or fuse: the
        reference's four statements (Src/ADFL/Server/qafel.py:160-161,179-180 over model.py:337-358)."""
        s_time = time.perf_counter()
        assert set(hidden_state.keys()) == set(params_new.keys())            # diff_parameters, model.py:352
        with torch.no_grad():
            update = {k: params_new[k] - hidden_state[k] for k in hidden_state}
            q_update, _ = self.on_server_send(update)
            d_update, _ = self.on_client_receive(q_update)
            assert set(hidden_state.keys()) == set(d_update.keys())          # add_parameters_inpace, model.py:340
            for k in d_update:
                hidden_state[k].mul_(1).add_(d_update[k].to(hidden_state[k].device), alpha=1)
        return q_update, time.perf_counter() - s_time


def _delta_on_device(prevs: List[torch.Tensor], news: List[torch.Tensor], dev: torch.device):
    """(new's, prev's data pointers as CPU int64 tensors) when every tensor of both lists is a contiguous
    4-byte-element tensor on the staging device (fp32: _delta_pairs saw to the dtype) — the pointer-table
    route — else None. One native call per list (adfl_torchhost.device_ptrs)."""
    th = _torchhost.get()
    ok_n, _, n_ptrs = th.device_ptrs(news, dev.index, 4)
    if not ok_n:
        return None
    ok_p, _, p_ptrs = th.device_ptrs(prevs, dev.index, 4)
    return (n_ptrs, p_ptrs) if ok_p else None


def _broadcast_groups(params_prev: Parameters, pairs, dev: torch.device):
    """broadcast_delta_'s fused entries as [names], one list per placement of params_new (on the staging device,
    on the CPU). An ndim > 1 pair (hidden, new) — fp32, of one shape and non-empty: _delta_pairs saw to that — is
    fused when the hidden tensor is the caller's own, contiguous and on the staging device, `new` is contiguous
    there or anywhere on the CPU, and the two do not share storage. Every other pair takes send_delta's encode
    and receive_add_'s update."""
    on_dev: List[str] = []
    on_cpu: List[str] = []
    for n, (h, g) in pairs.items():
        if (h is not params_prev[n] or not h.is_cuda or h.device != dev or not h.is_contiguous()
                or h.dtype != torch.float32 or g.dtype != torch.float32):
            continue
        if g.is_cuda:
            if (g.device == dev and g.is_contiguous()
                    and g.untyped_storage().data_ptr() != h.untyped_storage().data_ptr()):
                on_dev.append(n)
        elif g.device.type == "cpu":
            on_cpu.append(n)
    return [g for g in (on_dev, on_cpu) if g]


def _delta_pairs(params_prev: Parameters, params_new: Parameters, codable=None):
    """diff_parameters' view of a dict pair (Src/ADFL/model.py:350-358) without the difference of the ndim > 1
    entries: (names in params_prev's order, {name: new - prev} for the ndim <= 1 entries, and for the others
    the fp32 (prev, new) tensors to encode), raising what the reference raises on the way: the key-set
    assertion, torch's error for shapes `new - prev` cannot broadcast, and quantize's errors for an ndim > 1
    difference that would be empty or not fp32. A pair on two devices takes params_new's (plain torch would
    refuse it). codable (the stochastic channels): called as codable(name, dtype, shape) for every ndim > 1 pair
    in place of quantize's two errors — those channels encode fp16 / bf16 / fp64 differences and send an empty
    one through their zero-norm branch."""
    assert set(params_prev.keys()) == set(params_new.keys())
    names = list(params_prev.keys())
    plain: Dict[str, torch.Tensor] = {}
    pairs: Dict[str, Tuple[torch.Tensor, torch.Tensor]] = {}
    batch: List[str] = []   # ndim <= 1 pairs of one shape, dtype and device: subtracted together below
    with torch.no_grad():
        for n in names:
            a, b = params_prev[n], params_new[n]
            if a.shape == b.shape and a.ndim > 1:
                pairs[n] = (a, b)
            elif a.shape == b.shape and a.dtype == b.dtype and a.device == b.device:
                batch.append(n)
            else:
                d = b - (a if a.device == b.device else a.to(b.device))
                if a.shape != b.shape and d.ndim > 1:   # broadcastable, but not one model's two states
                    raise RuntimeError(f"send_delta: '{n}' has shape {tuple(a.shape)} in params_prev and "
                                       f"{tuple(b.shape)} in params_new")
                plain[n] = d
        if batch:   # torch's own subtraction, each result its own tensor on its own device, a few launches in all
            plain.update(zip(batch, torch._foreach_sub([params_new[n] for n in batch],
                                                       [params_prev[n] for n in batch])))
        f32 = torch.float32
        for n, (a, b) in pairs.items():   # quant.py:100-103 on the difference: its dtype is torch's promotion
            dt = a.dtype if a.dtype == b.dtype else torch.result_type(b, a)
            if codable is not None:
                codable(n, dt, b.shape)
            elif dt != f32 or b.numel() == 0:
                ops.require_quantizable(torch.empty(b.shape, dtype=dt, device="meta"))
            if a.dtype != dt or b.dtype != dt:   # e.g. fp16 - fp32: torch converts exactly, then subtracts
                pairs[n] = (a.to(dt), b.to(dt))
    return names, plain, pairs
