"""GPU: ``broadcast_delta_(hidden_state, params_new)`` of QSGDChannel / RQSGDChannel / CNATChannel — QAFeL's
broadcast (Src/ADFL/Server/qafel.py:156-180) with the hidden-state update fused into the encode.

With the fixture's uniforms injected the channels run all three steps of tests/golden/broadcast_stoch_small.npz
(the reference's own diff_parameters, on_server_send, on_client_receive and add_parameters_inpace, the hidden
state carried from step to step): every payload field and the hidden state after every step. Under one
``torch.manual_seed`` the call equals send_delta + receive_add_ on every placement; a mixed dict fuses what the
rule allows; and a fully eligible device dict completes without the decode-and-add route. Every comparison is
exact."""

import os

import numpy as np
import pytest
import torch

import broadcast_cases as bc
import broadcast_stoch_cases as bsc
from golden_util import GOLDEN, f32_from_bits, same_f32
from test_gpu_channel_delta import _bytes

pytestmark = pytest.mark.gpu

adfl_amd = pytest.importorskip("adfl_amd")
from adfl_amd.Channel import CNATChannel, QSGDChannel, RQSGDChannel  # noqa: E402
from adfl_amd.model import QuantParameters  # noqa: E402

DEV = "cuda"
PLACEMENTS = {"device": (DEV, DEV), "g_cpu": (DEV, "cpu"), "cpu": ("cpu", "cpu"), "h_cpu_g_device": ("cpu", DEV)}
CLASSES = {"qsgd": QSGDChannel, "rqsgd": RQSGDChannel, "cnat": CNATChannel}


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "broadcast_stoch_small.npz"))


@pytest.fixture(scope="module")
def inputs():
    return bc.inputs()


def _matches(g, prefix, name, a: np.ndarray) -> bool:
    if f"{prefix}__{name}" in g.files:
        want = g[f"{prefix}__{name}"]
        return a.dtype == want.dtype and a.shape == want.shape and a.tobytes() == want.tobytes()
    return bc.sha(a) == str(g[f"{prefix}sha__{name}"])


def _to(d, dev, order=None):
    return {n: torch.from_numpy(np.array(d[n])).to(dev) for n in (order or d)}


def _clone(d):
    return {n: t.clone() for n, t in d.items()}


def _same_dict(a, b):
    assert list(a.keys()) == list(b.keys())
    for n in a:
        assert a[n].dtype == b[n].dtype and a[n].shape == b[n].shape and a[n].device == b[n].device, n
        x, y = a[n].cpu().numpy(), b[n].cpu().numpy()
        assert same_f32(x, y) if x.dtype == np.float32 else x.tobytes() == y.tobytes(), n


def _same_scalar(a, b) -> bool:
    if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
        return (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.dtype == b.dtype
                and a.shape == b.shape and _bytes(a) == _bytes(b))
    return type(a) is type(b) and (a == b or (a != a and b != b))


def assert_same_payload(got: QuantParameters, want: QuantParameters):
    """Field for field: key order, size, and per entry data, signs, scale, scale_2, bits, shape, dtype, q_dtype."""
    assert isinstance(got, QuantParameters) and isinstance(want, QuantParameters)
    assert list(got.params.keys()) == list(want.params.keys()) and got.size == want.size
    for n, a in got.params.items():
        b = want.params[n]
        assert (a.bits, tuple(a.shape), a.dtype, a.q_dtype) == (b.bits, tuple(b.shape), b.dtype, b.q_dtype), n
        assert _same_scalar(a.scale, b.scale) and _same_scalar(a.scale_2, b.scale_2), n
        for x, y in ((a.data, b.data), (a.signs, b.signs)):
            assert (x.dtype, x.shape, x.device) == (y.dtype, y.shape, y.device) and _bytes(x) == _bytes(y), n


def _unfused(ch, hidden, new):
    """What broadcast_delta_ composed before, on the caller's copies: send_delta, then receive_add_."""
    c, _ = ch.send_delta(hidden, new)
    ch.receive_add_(c, [hidden])
    return c


def _no_coded_entry(ch):
    """A receive_add_ for `ch` that fails when a coded payload entry reaches it: broadcast_delta_ hands it the
    entries its fused launches did not take (the ndim <= 1 ones always), so a coded one came back in."""
    real = ch.receive_add_

    def receive_add_(c, targets):
        assert not [n for n, p in c.params.items() if ch._fusable(p)], "the payload came back in"
        return real(c, targets)
    return receive_add_


def _scalar_matches(row, v) -> bool:
    """A [kind, bits] row of the fixture (0 Python float, 1 the zero branch's 0-dim tensor, 2 an int) against a
    payload's scale / scale_2."""
    kind, bits = int(row[0]), int(row[1])
    if kind == 2:
        return isinstance(v, int) and v == bits
    if kind == 1:
        return isinstance(v, torch.Tensor) and v.ndim == 0 and v.dtype == torch.float32 and float(v) == 0.0
    return isinstance(v, float) and same_f32(np.float32(v), f32_from_bits(bits))


@pytest.mark.parametrize("placement", ["device", "g_cpu"])
@pytest.mark.parametrize("codec,bits", bsc.RUNS, ids=[f"{c}-b{b}" for c, b in bsc.RUNS])
def test_injected_uniforms_reproduce_every_step_of_the_reference(g, inputs, codec, bits, placement, monkeypatch):
    ch = CLASSES[codec](bits)
    h_dev, g_dev = PLACEMENTS[placement]
    h0, news = inputs
    order = [str(n) for n in g["order"]]
    new_order = [str(n) for n in g["new_order"]]
    run = f"{codec}_b{bits}"
    hidden = _to(h0, h_dev, order)
    objects = {n: (id(t), t.data_ptr()) for n, t in hidden.items()}

    monkeypatch.setattr(ch, "receive_add_", _no_coded_entry(ch))
    for k, new_np in enumerate(news, 1):
        pre = f"{run}__s{k}"
        new = _to(new_np, g_dev, new_order)
        if k == bc.STEPS:   # the frozen layer: g is exactly the hidden state the run has reached
            new[bc.FROZEN] = hidden[bc.FROZEN].clone().to(g_dev)
        keep = _clone(new)
        us = bsc.uniforms(k)
        plane = torch.from_numpy(np.concatenate([us[n].reshape(-1) for n in bsc.CODED])).to(DEV)
        got = ch._quantize_delta(hidden, new, bits, uniforms=plane, update=True)
        assert isinstance(got, QuantParameters)
        assert list(got.params.keys()) == order == [str(n) for n in g[f"{pre}__order"]]
        assert got.size == int(g[f"{pre}__size"])
        for n in order:
            p = got.params[n]
            assert p.bits == bits and p.data.device.type == torch.device(g_dev).type, (k, n)
            if n in bsc.CODED:
                i = bsc.CODED.index(n)
                assert _scalar_matches(g[f"{pre}__scale"][i], p.scale), (k, n, p.scale)
                assert _scalar_matches(g[f"{pre}__scale2"][i], p.scale_2), (k, n, p.scale_2)
                assert str(p.data.dtype).replace("torch.", "") == str(g[f"{pre}__qdtype"][i]) and p.q_dtype == p.data.dtype
                assert p.dtype == torch.float32 and tuple(p.shape) == tuple(p.data.shape) == h0[n].shape, (k, n)
                assert p.signs.dtype == torch.int8 and p.signs.device == p.data.device, (k, n)
                assert _matches(g, f"{pre}__q", n, p.data.cpu().numpy().view(np.uint8)), (k, n)
                assert _matches(g, f"{pre}__signs", n, p.signs.cpu().numpy()), (k, n)
            else:
                want = g[f"{pre}__pass__{n}"]
                have = p.data.cpu().numpy()
                assert p.scale == 0 and have.dtype == want.dtype and have.tobytes() == want.tobytes(), (k, n)
            # the hidden state after the step: the same tensor objects, updated in place
            assert (id(hidden[n]), hidden[n].data_ptr()) == objects[n], (k, n)
            assert _matches(g, f"{pre}__h", n, hidden[n].cpu().numpy()), (k, n)
        assert list(new.keys()) == new_order
        for n, t in new.items():      # g unchanged
            assert _bytes(t) == _bytes(keep[n]) and t.device == keep[n].device, (k, n)


@pytest.mark.parametrize("placement", list(PLACEMENTS))
@pytest.mark.parametrize("codec,bits", bsc.RUNS, ids=[f"{c}-b{b}" for c, b in bsc.RUNS])
def test_one_seed_gives_send_delta_then_receive_add(inputs, codec, bits, placement):
    ch = CLASSES[codec](bits)
    h_dev, g_dev = PLACEMENTS[placement]
    h0, news = inputs
    hidden = _to(h0, h_dev)
    ref = _clone(hidden)
    for k, new_np in enumerate(news, 1):
        new_np = dict(new_np)
        if k == bc.STEPS:
            new_np[bc.FROZEN] = ref[bc.FROZEN].cpu().numpy()       # the frozen layer: the zero branch
        new = _to(new_np, g_dev, list(new_np)[::-1])
        keep = _clone(new)
        torch.manual_seed(1000 + k)
        want = _unfused(ch, ref, _clone(new))
        after_want = torch.get_rng_state()
        torch.manual_seed(1000 + k)
        got, seconds = ch.broadcast_delta_(hidden, new)
        assert seconds > 0 and torch.equal(torch.get_rng_state(), after_want)   # the same draws
        assert_same_payload(got, want)
        _same_dict(hidden, ref)
        _same_dict(new, keep)
    assert isinstance(got.params[bc.FROZEN].scale, torch.Tensor)


@pytest.mark.parametrize("norm", ["torch", "fp64"])
@pytest.mark.parametrize("codec", list(CLASSES))
def test_a_fully_eligible_device_dict_never_takes_the_decode_and_add_route(inputs, codec, norm, monkeypatch):
    """Both QSGD routes (the reference norm's kernel, and the decode + axpby over the resident planes under
    ADFL_STOCH_NORM=fp64), RQSGD's kernels and CNAT's decode + axpby."""
    monkeypatch.setenv("ADFL_STOCH_NORM", norm)
    ch = CLASSES[codec](8)
    h0, news = inputs
    hidden = _to(h0, DEV)
    ref = _clone(hidden)
    new = _to(news[0], DEV)
    torch.manual_seed(77)
    want = _unfused(ch, ref, _clone(new))

    monkeypatch.setattr(ch, "receive_add_", _no_coded_entry(ch))
    torch.manual_seed(77)
    got, _ = ch.broadcast_delta_(hidden, new)
    assert_same_payload(got, want)
    _same_dict(hidden, ref)


@pytest.mark.parametrize("codec", list(CLASSES))
def test_mixed_entries_fuse_what_the_rule_allows_and_route_the_rest(codec, monkeypatch):
    """One dict holding fused entries, a hidden tensor on the CPU, an fp16 pair, a non-contiguous hidden tensor, a
    pair that shares storage, a hidden view one element into its storage, and the ndim <= 1 entries."""
    ch = CLASSES[codec](8)
    rng = np.random.default_rng(9)
    mk = lambda *s: torch.from_numpy(rng.standard_normal(s, dtype=np.float32))   # noqa: E731
    shared = mk(40, 3).to(DEV)
    store = mk(1 + 21 * 5).to(DEV)
    hidden = {"fused.weight": mk(70, 33).to(DEV), "host.weight": mk(9, 9), "half.weight": mk(17, 5).half().to(DEV),
              "strided.weight": mk(33, 70).to(DEV).t(), "big.weight": mk(3, 8193).to(DEV), "shared.weight": shared,
              "offset.weight": store[1:].view(21, 5), "bias": mk(33).to(DEV), "count": torch.tensor(7, device=DEV)}
    new = {n: (t + (1e-3 * torch.randn_like(t.float())).to(t.dtype)) if t.is_floating_point() else t + 5
           for n, t in hidden.items()}
    new["shared.weight"] = shared.view(40, 3)            # the pair shares storage: g == h, by the unfused route
    new["fused.weight"] = new["fused.weight"].cpu()      # g on the CPU beside g on the device
    ref = _clone(hidden)
    ref["strided.weight"] = hidden["strided.weight"].t().clone().t()
    ref_new = _clone(new)
    ref_new["shared.weight"] = ref["shared.weight"].view(40, 3)
    torch.manual_seed(5)
    want = _unfused(ch, ref, ref_new)
    objects = {n: id(t) for n, t in hidden.items()}
    routed = []
    real = ch.receive_add_

    def spy(c, targets):
        routed.extend(n for n, p in c.params.items() if ch._fusable(p))
        return real(c, targets)
    monkeypatch.setattr(ch, "receive_add_", spy)
    torch.manual_seed(5)
    got, _ = ch.broadcast_delta_(hidden, new)
    assert_same_payload(got, want)
    _same_dict(hidden, ref)
    assert {n: id(t) for n, t in hidden.items()} == objects
    assert int(hidden["count"]) == 12
    fused = {"fused.weight", "big.weight"} | ({"offset.weight"} if codec != "cnat" else set())
    assert not fused & set(routed)                       # what the rule allows never came back in
    assert {"strided.weight", "shared.weight"} <= set(routed)


def test_errors_are_send_deltas():
    w = torch.randn(8, 8, device=DEV)
    for cls in CLASSES.values():
        ch = cls(8)
        with pytest.raises(AssertionError):                                         # diff_parameters' key-set check
            ch.broadcast_delta_({"a": w.clone()}, {"b": w.clone()})
        with pytest.raises(RuntimeError):                                           # torch's, for the subtraction
            ch.broadcast_delta_({"a": w.clone()}, {"a": torch.randn(8, 9, device=DEV)})
        with pytest.raises(RuntimeError, match="send_delta: 'a' has shape"):        # broadcastable, not one model
            ch.broadcast_delta_({"a": w.clone()}, {"a": torch.randn(1, 8, device=DEV)})
        h = {"a": w.clone(), "b": torch.ones(8, 8, dtype=torch.int32, device=DEV)}
        with pytest.raises(RuntimeError):                                           # the reference's, for integers
            ch.broadcast_delta_(h, {"a": w + 1, "b": h["b"] + 1})
        assert torch.equal(h["a"], w)                                               # nothing was updated
