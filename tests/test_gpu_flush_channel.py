"""GPU: the buffered servers end to end, as INTEGRATION.md writes them: ``SLQChannel(8).receive_scaled`` makes the
buffer, ``receive_scaled_add_`` adds two more updates, then ``fedbuff_flush`` / ``FadasMoments.flush`` — for device
dicts and CPU dicts, with a bias, an int64 counter and an empty tensor present — against the reference's own
statements (Src/ADFL/Strategy/fed_buff.py:72-92, fadas.py:60-73,96-129, model.py:326-347) run by CPU torch on the
channel's own decodes.

FedBuff: bit-identical. FADAS over three rounds: the moments (and ``FadasMoments.m / v / v_hat``) bit-identical.
params_prime of the fused entries is held to the reference's statements three ways:
  * as written (``v_hat.sqrt()``): bit-identical outside the mask, the elements where the running torch's CPU sqrt
    of v_hat is not the correctly rounded root;
  * with that one call replaced by torch's own fp64 sqrt cast down, which is the correctly rounded root on every
    CPU: bit-identical on every element, no exclusions — the mask hides nothing of the flush;
  * inside the mask, the reference's value as written equals bit for bit the statements with the root moved to one
    of its two fp32 neighbours: torch's sqrt is one ulp off there, and that explains the whole difference.
test_flush_golden.py's other two conditions are about torch's CPU sqrt, not about the flush, and hold on the CPU
that generated the golden fixture but not on every CPU: there torch's sqrt is one ulp low on 0.6 % of elements; on
the EPYC 9575F hosts of the MI355X machines it is an ulp off in either direction on 16-20 %, which breaks the 2 % cap
and, at a binade edge of the step, the c = 2 ulp bound on about one element in 1,700 (the issue's own trial of
c = 2 on random data left 0-5 violations in 200,003). They are asserted where they are machine-independent
(test_flush_golden.py, on the fixture's stored mask); here the exact-neighbour condition stands in for them.
"""

import copy
import math

import numpy as np
import pytest
import torch

import flush_cases as fc

pytestmark = pytest.mark.gpu

from adfl_amd import FadasMoments, fedbuff_flush  # noqa: E402
from adfl_amd.Channel import SLQChannel  # noqa: E402
from adfl_amd.model import QuantParameter  # noqa: E402

DEVICES = ["cuda", "cpu"]
EMPTY = "empty.weight"
K, LR = 3, 0.05


def _model(seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return {"conv.weight": torch.randn(64, 3, 3, 3, generator=g) * scale,
            "fc.weight": torch.randn(10, 513, generator=g) * scale,
            "fc.bias": torch.randn(10, generator=g) * scale, "bn.num_batches_tracked": torch.tensor(seed % 7 + 1),
            "emb.weight": torch.randn(37, 33, generator=g) * scale, EMPTY: torch.zeros(0, 4)}


def _payload(ch, seed):
    """A client's update through the channel. SLQ cannot quantize an empty tensor (the reference raises,
    quant.py:100): the empty entry travels as a non-quantized ndim > 1 payload, which quant.py:110 accepts."""
    update = _model(seed, 1e-2)
    empty = update.pop(EMPTY)
    c, _ = ch.on_client_send(update)
    some = next(iter(c.params.values()))
    c.params[EMPTY] = QuantParameter(empty, ch.bits, 1, some.signs, empty.shape, empty.dtype, empty.dtype)
    return c


def _decode(ch, c):
    return ch.on_server_receive(copy.deepcopy(c))[0]


def _same(got, want, what):
    g, w = got.detach().cpu(), want.detach().cpu()
    assert g.dtype == w.dtype and g.shape == w.shape, (what, g.dtype, w.dtype, g.shape, w.shape)
    if g.dtype == torch.float32:
        assert fc.same_bits(g.reshape(-1).numpy(), w.reshape(-1).numpy()).all(), what
    else:
        assert torch.equal(g, w), what


def _same_dict(got, want, what):
    assert list(got.keys()) == list(want.keys()), what
    for k in want:
        _same(got[k], want[k], (what, k))


@pytest.mark.parametrize("device", DEVICES)
def test_fedbuff_sequence_and_flush(device):
    ch = SLQChannel(8)
    cs = [_payload(ch, 1 + i) for i in range(K)]
    fs = [fc.staleness_factor(s) for s in fc.FEDBUFF_STALENESS]
    g = {k: v.to(device) for k, v in _model(50).items()}
    g_cpu = copy.deepcopy({k: v.cpu() for k, v in g.items()})
    # the reference: fed_buff.py:72-92 over the channel's decodes
    with torch.no_grad():
        want_buf = None
        for c, f in zip(cs, fs):
            d = _decode(ch, c)
            for t in d.values():
                t.float().mul_(f)
            if want_buf is None:
                want_buf = d
            else:
                for k in d:
                    want_buf[k].mul_(1).add_(d[k], alpha=1)
        for t in want_buf.values():
            t.float().div_(K)
        want = {k: (1.0 * g_cpu[k]) + (LR * want_buf[k]) for k in want_buf}
    # the drop-in
    buf, _ = ch.receive_scaled(copy.deepcopy(cs[0]), fs[0])
    buf = {k: v.to(device) for k, v in buf.items()}
    for c, f in zip(cs[1:], fs[1:]):
        ch.receive_scaled_add_(copy.deepcopy(c), [buf], f)
    got = fedbuff_flush(buf, g, K, LR)
    assert list(got.keys()) == list(buf.keys())                   # keys in buffer's order
    _same_dict(got, want, ("fedbuff", device))
    for k, v in got.items():
        assert v.device.type == device, k
    _same_dict(g, g_cpu, "g_params modified")
    ptrs = [t.untyped_storage().data_ptr() for d in (got, g, buf) for t in d.values() if t.numel()]
    assert len(set(ptrs)) == len(ptrs)                            # every returned tensor owns its storage


class _RefFadas:
    """fadas.py's statements, as written there, on CPU tensors."""

    def __init__(self, lr):
        self.lr, self.beta_1, self.beta_2, self.eps, self.max_delay = lr, 0.9, 0.999, 1e-8, 10
        self.m, self.v, self.v_hat, self.round = {}, {}, {}, 1

    def lr_t(self, max_staleness):
        return self.lr if max_staleness <= self.max_delay else min(self.lr, self.lr / max_staleness)

    def flush(self, buffer, g_params, max_staleness):
        with torch.no_grad():
            for t in buffer.values():
                t.float().div_(K)
            if not self.m:
                for d in (self.m, self.v, self.v_hat):
                    d.update({n: torch.zeros_like(t, dtype=torch.float32) for n, t in g_params.items()})
            for k in buffer:
                self.m[k].mul_(self.beta_1).add_(buffer[k], alpha=(1 - self.beta_1))
                self.v[k].mul_(self.beta_2).addcmul_(buffer[k], buffer[k], value=(1 - self.beta_2))
                torch.maximum(self.v_hat[k], self.v[k], out=self.v_hat[k])
            bc1, bc2 = 1 - self.beta_1 ** self.round, 1 - self.beta_2 ** self.round
            step_size = self.lr_t(max_staleness) / bc1
            # _compute_model_step as written ("torch"), and with `v_hat.sqrt()` replaced by the correctly rounded
            # root (torch's own fp64 sqrt cast down: "rn") and by that root's two fp32 neighbours ("rn-1", "rn+1")
            inf = torch.tensor(math.inf)
            out = {"torch": {}, "rn": {}, "rn-1": {}, "rn+1": {}}
            for k in g_params:
                rn = self.v_hat[k].double().sqrt().float()
                roots = {"torch": self.v_hat[k].sqrt(), "rn": rn, "rn-1": torch.nextafter(rn, -inf),
                         "rn+1": torch.nextafter(rn, inf)}
                for name, root in roots.items():
                    denom = (root / math.sqrt(bc2)).add_(self.eps)
                    out[name][k] = torch.addcdiv(g_params[k], self.m[k], denom, value=step_size)
            self.round += 1
            return out


@pytest.mark.parametrize("device", DEVICES)
def test_fadas_three_rounds(device):
    ch = SLQChannel(8)
    ref, mom = _RefFadas(LR), FadasMoments()
    for r, stale in enumerate(fc.FADAS_STALENESS):
        cs = [_payload(ch, 10 * (r + 1) + i) for i in range(K)]
        g = {k: v.to(device) for k, v in _model(60 + r).items()}
        g_cpu = copy.deepcopy({k: v.cpu() for k, v in g.items()})
        # the reference's buffer: fadas.py:60-63, add_parameters_inpace(buffer, update, 1.0, 1.0, to_float=True)
        with torch.no_grad():
            want_buf = _decode(ch, cs[0])
            for c in cs[1:]:
                d = _decode(ch, c)
                for k in d:
                    want_buf[k].float().mul_(1.0).add_(d[k], alpha=1.0)
        wants = ref.flush(want_buf, g_cpu, max(stale))
        want = wants["torch"]
        # the drop-in: non-fp32 entries are left alone, as to_float=True leaves them
        buf, _ = ch.receive_scaled(copy.deepcopy(cs[0]), 1.0)
        buf = {k: v.to(device) for k, v in buf.items()}
        for c in cs[1:]:
            keep = {k: t.clone() for k, t in buf.items() if t.dtype != torch.float32}
            ch.receive_scaled_add_(copy.deepcopy(c), [buf], 1.0)
            buf.update(keep)
        got = mom.flush(buf, g, K, ref.lr_t(max(stale)), r + 1)
        assert list(got.keys()) == list(g.keys())                 # _compute_model_step walks g_params
        _same_dict(g, g_cpu, "g_params modified")
        # the moments: bit-identical, through the CPU dicts FadasMoments hands out
        for name, ours, theirs in (("m", mom.m, ref.m), ("v", mom.v, ref.v), ("v_hat", mom.v_hat, ref.v_hat)):
            for k, t in ours.items():
                assert t.device.type == "cpu"
            _same_dict(ours, theirs, (device, r, name))
        for k in want:
            o, w = got[k].detach().cpu(), want[k]
            assert got[k].device.type == device and o.dtype == w.dtype and o.shape == w.shape, (k, o.dtype, w.dtype)
            if not o.numel():
                continue
            o, w = o.reshape(-1).numpy(), w.reshape(-1).numpy()
            rn, lo, hi = (wants[x][k].reshape(-1).numpy() for x in ("rn", "rn-1", "rn+1"))
            h = ref.v_hat[k].reshape(-1)
            mask = ~fc.same_bits(h.sqrt().numpy(), h.double().sqrt().float().numpy())
            same = fc.same_bits(o, w)
            print(f"{device} r{r} {k}: torch.sqrt off on {mask.mean():.4%}, params_prime differs on "
                  f"{(~same).mean():.4%}")
            assert same[~mask].all(), (device, r, k, int((~same & ~mask).sum()))
            # inside the mask the reference's value is explained exactly by a root one ulp off
            assert (fc.same_bits(w, rn) | fc.same_bits(w, lo) | fc.same_bits(w, hi)).all(), (device, r, k)
            if k in mom._index:   # a fused entry: the correctly rounded root, on every element
                assert fc.same_bits(o, rn).all(), (device, r, k, "exact sqrt")
            elif device == "cpu":  # the reference's own statements on the same CPU
                assert same.all(), (device, r, k)
    # the fused entries' moments live on the device, in one layout, for the object's lifetime
    assert mom._buckets.is_cuda and mom._buckets.shape[0] == 3
    assert set(mom._fused) == {"conv.weight", "fc.weight", "fc.bias", "emb.weight"}


def test_fadas_moments_layout_is_fixed():
    ch = SLQChannel(8)
    mom = FadasMoments()
    g = {k: v.cuda() for k, v in _model(70).items()}
    buf = {k: v.cuda() for k, v in ch.receive_scaled(_payload(ch, 5), 1.0)[0].items()}
    mom.flush(buf, g, K, LR, 1)
    where = mom._buckets.data_ptr()
    buf = {k: v.cuda() for k, v in ch.receive_scaled(_payload(ch, 6), 1.0)[0].items()}
    mom.flush(buf, g, K, LR, 2)
    assert mom._buckets.data_ptr() == where
    bad = dict(buf)
    bad["fc.weight"] = buf["fc.weight"].double()
    with pytest.raises(ValueError, match="fused at the first flush"):
        mom.flush(bad, g, K, LR, 3)
    with pytest.raises(AssertionError):
        mom.flush({k: v for k, v in buf.items() if k != "fc.bias"}, g, K, LR, 3)
