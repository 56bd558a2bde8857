"""GPU: ``broadcast_delta_(hidden_state, params_new)`` — QAFeL's broadcast (Src/ADFL/Server/qafel.py:156-180).

The SLQ channels run all three steps of tests/golden/broadcast_small.npz (the reference's own diff_parameters,
SLQChannel(bits).on_server_send, on_client_receive and add_parameters_inpace, the hidden state carried from step
to step) with both dicts on the device and with g on the CPU: c_params field for field, the hidden state after
every step, the same tensor objects, an unchanged g. Every other channel is checked against the calls it
composes, on copies. Every comparison is exact."""

import os

import numpy as np
import pytest
import torch

import broadcast_cases as bc
from golden_util import GOLDEN, f32_from_bits, same_f32
from test_gpu_channel_delta import _bytes, assert_same_payload, diff_parameters

pytestmark = pytest.mark.gpu

adfl_amd = pytest.importorskip("adfl_amd")
from adfl_amd.Channel import (CNATChannel, PackedSLQChannel, QSGDChannel, RQSGDChannel, SLQChannel,  # noqa: E402
                              USLQChannel)
from adfl_amd.model import QuantParameters  # noqa: E402

DEV = "cuda"
PLACEMENTS = {"device": (DEV, DEV), "g_cpu": (DEV, "cpu"), "cpu": ("cpu", "cpu"), "h_cpu_g_device": ("cpu", DEV)}


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "broadcast_small.npz"))


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


def _unfused(ch, hidden, new):
    """What broadcast_delta_ composes, on the caller's copies: send_delta, then receive_add_."""
    c, _ = ch.send_delta(hidden, new)
    ch.receive_add_(c, [hidden])
    return c


@pytest.mark.parametrize("placement", ["device", "g_cpu"])
@pytest.mark.parametrize("bits", [8, 4])
def test_slq_channel_reproduces_every_step_of_the_reference(g, inputs, bits, placement):
    ch = SLQChannel(bits)
    h_dev, g_dev = PLACEMENTS[placement]
    h0, news = inputs
    order = [str(n) for n in g["order"]]
    new_order = [str(n) for n in g["new_order"]]
    qnames = [str(n) for n in g[f"b{bits}__qnames"]]
    hidden = _to(h0, h_dev, order)
    objects = {n: (id(t), t.data_ptr()) for n, t in hidden.items()}
    for k, new_np in enumerate(news, 1):
        pre = f"b{bits}__s{k}"
        new_np = dict(new_np)
        if k == bc.STEPS:
            new_np[bc.FROZEN] = g[f"{pre}__new__{bc.FROZEN}"]
        new = _to(new_np, g_dev, new_order)
        keep = _clone(new)
        got, seconds = ch.broadcast_delta_(hidden, new)
        assert seconds > 0 and isinstance(got, QuantParameters)
        assert list(got.params.keys()) == order == [str(n) for n in g[f"{pre}__order"]]
        assert got.size == int(g[f"{pre}__size"])
        for n in order:
            p = got.params[n]
            assert p.bits == bits and p.data.device.type == torch.device(g_dev).type, (k, n)
            if n in qnames:
                scale = f32_from_bits(int(g[f"{pre}__scale_bits"][qnames.index(n)]))
                assert isinstance(p.scale, float) and same_f32(np.float32(p.scale), scale), (k, n)
                assert p.data.dtype == torch.qint8 and p.q_dtype == torch.qint8 and p.dtype == torch.float32, (k, n)
                assert tuple(p.shape) == tuple(p.data.shape) == h0[n].shape, (k, n)
                assert p.data.q_zero_point() == 0 and (p.data.q_scale() == p.scale or scale != scale), (k, n)
                assert _matches(g, f"{pre}__q", n, p.data.cpu().int_repr().numpy()), (k, n)
            else:
                want = g[f"{pre}__pass__{n}"]
                have = p.data.cpu().numpy()
                assert p.scale == 1 and have.dtype == want.dtype and have.tobytes() == want.tobytes(), (k, n)
            # the hidden state after the step: the same tensor objects, updated in place
            assert (id(hidden[n]), hidden[n].data_ptr()) == objects[n], (k, n)
            assert _matches(g, f"{pre}__h", n, hidden[n].cpu().numpy()), (k, n)
        assert list(new.keys()) == new_order
        for n, t in new.items():      # g unchanged
            assert _bytes(t) == _bytes(keep[n]) and t.device == keep[n].device, (k, n)


@pytest.mark.parametrize("placement", list(PLACEMENTS))
@pytest.mark.parametrize("channel", ["slq8", "slq4", "packed4", "packed2"])
def test_slq_channels_equal_send_delta_then_receive_add(inputs, channel, placement):
    """Every placement, the unfused ones included (a CPU hidden state: same results by the unfused route), and
    PackedSLQChannel against its own send_delta + receive_add_."""
    ch = {"slq8": SLQChannel(8), "slq4": SLQChannel(4), "packed4": PackedSLQChannel(4),
          "packed2": PackedSLQChannel(2)}[channel]
    h_dev, g_dev = PLACEMENTS[placement]
    h0, news = inputs
    hidden = _to(h0, h_dev)
    ref = _clone(hidden)
    for k, new_np in enumerate(news, 1):
        new_np = dict(new_np)
        if k == bc.STEPS:
            new_np[bc.FROZEN] = ref[bc.FROZEN].cpu().numpy()       # the frozen layer: scale 0, codes 127
        new = _to(new_np, g_dev, list(new_np)[::-1])
        keep = _clone(new)
        want = _unfused(ch, ref, _clone(new))
        got, _ = ch.broadcast_delta_(hidden, new)
        assert_same_payload(got, want)
        _same_dict(hidden, ref)
        _same_dict(new, keep)
    if k == bc.STEPS:
        assert got.params[bc.FROZEN].scale == 0.0


def test_packed_channel_reads_the_nibbles_back_for_nan_and_frozen_tensors():
    ch = PackedSLQChannel(4)
    rng = np.random.default_rng(5)
    h = {"a.weight": rng.standard_normal((33, 31), dtype=np.float32), "b.weight": rng.standard_normal((7, 9), dtype=np.float32),
         "c.weight": rng.standard_normal((2049, 1), dtype=np.float32)}
    new = {n: (a + np.float32(1e-2)).astype(np.float32) for n, a in h.items()}
    new["a.weight"] = h["a.weight"].copy()                        # codes 127: nibbles 7 / -1 after pack_pair
    new["b.weight"][3, 3] = np.nan
    hidden = _to(h, DEV)
    ref = _clone(hidden)
    want = _unfused(ch, ref, _to(new, DEV))
    got, _ = ch.broadcast_delta_(hidden, _to(new, DEV))
    assert_same_payload(got, want)
    _same_dict(hidden, ref)
    assert bool(torch.isnan(hidden["b.weight"]).all())
    assert torch.equal(hidden["a.weight"].abs(), torch.from_numpy(h["a.weight"]).to(DEV).abs())   # h + (+-0)


@pytest.mark.parametrize("placement", ["device", "g_cpu", "cpu"])
@pytest.mark.parametrize("cls", [QSGDChannel, RQSGDChannel, CNATChannel])
def test_stochastic_channels_draw_the_stream_of_the_pair_they_compose(inputs, cls, placement):
    ch = cls(4)
    h_dev, g_dev = PLACEMENTS[placement]
    h0, news = inputs
    hidden = _to(h0, h_dev)
    ref = _clone(hidden)
    new = _to(news[0], g_dev)
    torch.manual_seed(1234)
    want = _unfused(ch, ref, _clone(new))
    torch.manual_seed(1234)
    got, _ = ch.broadcast_delta_(hidden, new)
    assert list(got.params.keys()) == list(want.params.keys()) and got.size == want.size
    for n, a in got.params.items():
        b = want.params[n]
        assert (a.bits, tuple(a.shape), a.dtype, a.q_dtype) == (b.bits, tuple(b.shape), b.dtype, b.q_dtype), n
        assert _bytes(a.data) == _bytes(b.data) and a.data.device == b.data.device, n
        assert _bytes(a.signs) == _bytes(b.signs), n
    _same_dict(hidden, ref)


def test_unidirectional_channel_runs_the_four_reference_statements(inputs):
    ch = USLQChannel(8)
    h0, news = inputs
    hidden = _to(h0, "cpu")
    ref = _clone(hidden)
    new = _to(news[0], "cpu")
    # Src/ADFL/Server/qafel.py:160-161,179-180
    update = diff_parameters(ref, new)
    q_update, _ = ch.on_server_send(update)
    d_update, _ = ch.on_client_receive(q_update)
    with torch.no_grad():
        for n in d_update:
            ref[n].mul_(1).add_(d_update[n], alpha=1)
    got, seconds = ch.broadcast_delta_(hidden, new)
    assert seconds > 0 and type(got) is type(q_update) and got.size == q_update.size
    assert list(got.params.keys()) == list(q_update.params.keys())
    for n, a in got.params.items():
        b = q_update.params[n]
        assert a.data == b.data and tuple(a.shape) == tuple(b.shape) and a.dtype == b.dtype, n
    _same_dict(hidden, ref)
    for n in hidden:   # the identity channel: h + (g - h), one rounding each
        assert torch.equal(hidden[n], torch.from_numpy(np.asarray(h0[n] + (news[0][n] - h0[n])))), n


def test_mixed_entries_fuse_what_the_rule_allows_and_route_the_rest():
    """One dict holding a fused entry, a non-contiguous hidden tensor, a hidden tensor on the CPU, a pair that
    shares storage, and the ndim <= 1 entries."""
    ch = SLQChannel(8)
    rng = np.random.default_rng(9)
    mk = lambda *s: torch.from_numpy(rng.standard_normal(s, dtype=np.float32))   # noqa: E731
    shared = mk(40, 3).to(DEV)
    hidden = {"fused.weight": mk(70, 33).to(DEV), "strided.weight": mk(33, 70).to(DEV).t(),
              "host.weight": mk(9, 9), "shared.weight": shared, "bias": mk(33).to(DEV),
              "count": torch.tensor(7, device=DEV)}
    new = {n: (t + 1e-3 * torch.randn_like(t)) if t.is_floating_point() else t + 5 for n, t in hidden.items()}
    new["shared.weight"] = shared.view(40, 3)            # the pair shares storage: g == h, by the unfused route
    assert not hidden["strided.weight"].is_contiguous()
    ref = _clone(hidden)
    ref["strided.weight"] = hidden["strided.weight"].t().clone().t()
    ref_new = _clone(new)
    ref_new["shared.weight"] = ref["shared.weight"].view(40, 3)
    want = _unfused(ch, ref, ref_new)
    objects = {n: id(t) for n, t in hidden.items()}
    got, _ = ch.broadcast_delta_(hidden, new)
    assert_same_payload(got, want)
    _same_dict(hidden, ref)
    assert {n: id(t) for n, t in hidden.items()} == objects
    assert int(hidden["count"]) == 12 and got.params["shared.weight"].scale == 0.0


def test_errors_are_send_deltas():
    ch = SLQChannel(8)
    w = torch.randn(8, 8, device=DEV)
    with pytest.raises(AssertionError):                                         # diff_parameters' key-set check
        ch.broadcast_delta_({"a": w.clone()}, {"b": w.clone()})
    with pytest.raises(RuntimeError):                                           # torch's, for the subtraction
        ch.broadcast_delta_({"a": w.clone()}, {"a": torch.randn(8, 9, device=DEV)})
    with pytest.raises(RuntimeError, match="send_delta: 'a' has shape"):        # broadcastable, not one model
        ch.broadcast_delta_({"a": w.clone()}, {"a": torch.randn(1, 8, device=DEV)})
    with pytest.raises(RuntimeError, match="Quantize only works on Float Tensor, got Double"):
        ch.broadcast_delta_({"a": w.double()}, {"a": w.double()})
    h = {"a": w.clone(), "b": w.double()}
    with pytest.raises(RuntimeError, match="Quantize only works on Float Tensor, got Double"):
        ch.broadcast_delta_(h, {"a": w + 1, "b": w.double() + 1})
    assert torch.equal(h["a"], w) and torch.equal(h["b"], w.double())           # nothing was updated
    for cls in (QSGDChannel, PackedSLQChannel):
        with pytest.raises(AssertionError):
            cls(4).broadcast_delta_({"a": w.clone()}, {"b": w.clone()})
