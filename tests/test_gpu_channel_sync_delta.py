"""GPU: ``receive_mean_axpby`` — the synchronous DELTA server step, ``Simple(CommType.DELTA, sync=True)._sync_update``
(Src/ADFL/Strategy/simple.py:87-89), as one channel call.

* Against the reference executed in place (tests/golden/sync_delta.npz, made by make_golden_sync_delta.py; only its
  outputs are on this box): all five channel classes, the global parameters on the device and on the CPU; the
  stochastic channels are fed the reference's own payloads (aggregate.npz), as test_gpu_aggregate_golden.py feeds
  them to receive_mean.
* Against ``receive_mean`` followed by the reference's statement, bit for bit and key for key: a uni-directional
  class, a non-contiguous, a misaligned and a mixed-placement base, device-resident updates, and torch's sum order
  reported as not the kernels' (everything then takes the host route).
* The contract's other clauses: base and payloads unmodified, owned outputs where the base lives, the int64 counter
  back as fp32, the assertions."""

import numpy as np
import pytest
import torch

import recipes
import sync_delta_cases as sd
from golden_util import same_f32
from make_golden_aggregate import client_dict
from test_gpu_aggregate_golden import _stoch_updates, fixture as aggregate_fixture

pytestmark = pytest.mark.gpu

adfl_amd = pytest.importorskip("adfl_amd")
from adfl_amd.Channel import (CNATChannel, PackedSLQChannel, QSGDChannel, RQSGDChannel, SLQChannel,  # noqa: E402
                              UQSGDChannel, USLQChannel, _base)

DEV = torch.device("cuda", 0)
STOCH_CLS = {"qsgd": QSGDChannel, "rqsgd": RQSGDChannel, "cnat": CNATChannel}
_cache = {}


def golden():
    if "g" not in _cache:
        _cache["g"] = sd.load()
    return _cache["g"]


def updates_of(kind):
    """(channel, the updates of clients 0 .. max K - 1), made once per kind and never modified."""
    if kind not in _cache:
        if kind in STOCH_CLS:
            a, m = aggregate_fixture()
            ch = STOCH_CLS[kind](m["stoch"][kind][1])
            ups = _stoch_updates(kind, a, m, max(sd.STOCH_K))
        else:
            ch = {"slq8": SLQChannel(8), "slq4": SLQChannel(4), "packed4": PackedSLQChannel(4)}[kind]
            n = max(sd.SLQ8_K) if kind == "slq8" else max(sd.SLQ4_K)
            ups = [ch.on_client_send(client_dict(c))[0] for c in range(n)]
        _cache[kind] = (ch, ups)
    return _cache[kind]


def g_params(where):
    g = {n: torch.from_numpy(np.array(a)) for n, a in sd.g_arrays().items()}
    return {n: t.to(DEV) for n, t in g.items()} if where == "cuda" else g


def two_step(ch, updates, base, alpha, beta):
    """receive_mean, then add_parameters' statement (Src/ADFL/model.py:326-334)."""
    agg, _ = ch.receive_mean(updates)
    with torch.no_grad():
        return {n: (alpha * base[n]) + (beta * m.to(base[n].device)) for n, m in agg.items()}


def same_dicts(got, want):
    assert list(got) == list(want)
    for n in want:
        assert got[n].dtype == want[n].dtype and got[n].shape == want[n].shape and got[n].device == want[n].device, n
        assert same_f32(got[n].cpu().numpy(), want[n].cpu().numpy()), n


def check_owned(out, base):
    ptrs = set()
    for n, t in out.items():
        assert t.device == base[n].device, n
        assert t.untyped_storage().nbytes() == t.numel() * t.element_size() and t.is_contiguous(), n
        assert t.untyped_storage().data_ptr() != base[n].untyped_storage().data_ptr(), n
        ptrs.add(t.untyped_storage().data_ptr())
    assert len(ptrs) == len(out)


GOLDEN_RUNS = ([("slq8", "slq8", c) for c in sd.CASES if c[0] == "slq8"]
               + [(kind, "slq4", c) for kind in ("slq4", "packed4") for c in sd.CASES if c[0] == "slq4"]
               + [(c[0], c[0], c) for c in sd.CASES if c[0] in STOCH_CLS])


@pytest.mark.parametrize("where", ["cuda", "cpu"])
@pytest.mark.parametrize("kind,tag_ch,case", GOLDEN_RUNS,
                         ids=[f"{k}-{sd.case_tag(*c)}" for k, _, c in GOLDEN_RUNS])
def test_equals_the_executed_reference(kind, tag_ch, case, where):
    arrays, manifest = golden()
    _, k, alpha, beta = case
    ch, ups = updates_of(kind)
    base = g_params(where)
    keep = {n: t.clone() for n, t in base.items()}
    got, secs = ch.receive_mean_axpby(ups[:k], base, alpha, beta)
    assert secs > 0 and list(got) == sd.NAMES    # the first update's key order, not base's
    check_owned(got, base)
    tag = sd.case_tag(*case)
    rec = manifest["cases"][tag]
    aliased = None
    for n, t in got.items():
        assert t.dtype == torch.float32, n       # the int64 counter included
        a = t.cpu().numpy()
        if kind == "packed4" and n == "six.weight" and k > 9:
            # pack_4bit aliases client 9's out-of-range code (test_gpu_aggregate_golden.py): held to the two steps
            aliased = aliased or two_step(ch, ups[:k], base, alpha, beta)
            assert same_f32(a, aliased[n].cpu().numpy()), n
            continue
        if f"{tag}__{n}" in arrays:
            want = arrays[f"{tag}__{n}"]
            assert a.shape == want.shape and same_f32(a, want), (tag, n)
            assert np.array_equal(np.signbit(a[~np.isnan(a)]), np.signbit(want[~np.isnan(want)])), (tag, n)
        else:
            assert recipes.sha256(a) == rec["sha256"][n], (tag, n)
        assert torch.equal(base[n].view(torch.int32) if base[n].dtype == torch.float32 else base[n],
                           keep[n].view(torch.int32) if keep[n].dtype == torch.float32 else keep[n]), n


def _payload_bytes(ups):
    out = []
    for u in ups:
        for p in u.params.values():
            d = p.data
            out.append((d.int_repr() if d.is_quantized else d).clone())
    return out


@pytest.mark.parametrize("kind", ["slq8", "packed4", "rqsgd"])
@pytest.mark.parametrize("variant", ["plain", "noncontiguous", "misaligned", "mixed", "order_check_fails"])
def test_equals_receive_mean_then_the_reference_statement(kind, variant, monkeypatch):
    ch, ups = updates_of(kind)
    ups = ups[:5]
    base = g_params("cpu")
    if variant == "noncontiguous":
        wide = torch.randn(10, 66)
        wide[:, ::2] = base["fc.weight"]
        base["fc.weight"] = wide[:, ::2]
        assert not base["fc.weight"].is_contiguous()
    elif variant == "misaligned":
        buf = torch.zeros(16 * 129 + 1)
        buf[1:] = base["big.weight"].reshape(-1)
        base["big.weight"] = buf[1:].view(16, 129)
        assert base["big.weight"].data_ptr() % 16 == 4
    elif variant == "mixed":
        for n in ("conv.weight", "rag.weight", "fc.bias"):
            base[n] = base[n].to(DEV)
    elif variant == "order_check_fails":
        monkeypatch.setattr(_base, "device_mean_order_ok", lambda: False)
    before = _payload_bytes(ups)
    got, _ = ch.receive_mean_axpby(ups, base, 0.4, 0.6)
    want = two_step(ch, ups, base, 0.4, 0.6)
    same_dicts(got, want)
    check_owned(got, base)
    for a, b in zip(before, _payload_bytes(ups)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("cls,bits", [(USLQChannel, 8), (UQSGDChannel, 8)])
def test_unidirectional_class_and_device_updates(cls, bits):
    """Client-to-server is the compressed direction of a U* channel; updates encoded from device tensors stay on the
    device, the base on the device too: nothing but the biases crosses PCIe."""
    ch = cls(bits)
    torch.manual_seed(3)
    for on_dev in (False, True):
        ups = [ch.on_client_send({n: t.to(DEV) if on_dev and t.ndim > 1 else t for n, t in client_dict(c).items()})[0]
               for c in range(3)]
        for where in ("cuda", "cpu"):
            base = g_params(where)
            got, _ = ch.receive_mean_axpby(ups, base)   # alpha = beta = 1.0
            same_dicts(got, two_step(ch, ups, base, 1.0, 1.0))
            check_owned(got, base)
            assert got[sd.COUNTER_NAME].dtype == torch.float32 and base[sd.COUNTER_NAME].dtype == torch.int64


def test_assertions():
    ch, ups = updates_of("slq8")
    base = g_params("cpu")
    with pytest.raises(AssertionError):
        ch.receive_mean_axpby([], base)
    short = dict(base)
    short.pop("fc.bias")
    with pytest.raises(AssertionError):
        ch.receive_mean_axpby(ups[:2], short)
    extra = dict(base, other=torch.zeros(1))
    with pytest.raises(AssertionError):
        ch.receive_mean_axpby(ups[:2], extra)
    with pytest.raises(AssertionError):
        ch.receive_mean_axpby([{"w": torch.zeros(2, 2)}], {"w": torch.zeros(2, 2)})   # not a payload object
