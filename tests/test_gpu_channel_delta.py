"""GPU: ``send_delta(prev, new)`` of the SLQ channels equals ``on_client_send(diff_parameters(prev, new))`` of the
same channel bit for bit and field for field, and both equal tests/golden/delta_small.npz (the reference's own
diff_parameters + SLQChannel(bits).on_client_send, Src/ADFL/model.py:350-358 + Src/ADFL/Channel/quant.py:61-104).
The dict pair is the fixture's (tests/golden/delta_cases.py); every comparison is exact."""

import os

import numpy as np
import pytest
import torch

import delta_cases
import slq_oracle as oracle
from golden_util import GOLDEN, f32_from_bits, same_f32

pytestmark = pytest.mark.gpu

adfl_amd = pytest.importorskip("adfl_amd")
from adfl_amd.Channel import PackedSLQChannel, SLQChannel, USLQChannel  # noqa: E402
from adfl_amd.model import QuantParameters  # noqa: E402

DEV = "cuda"
CHANNELS = {"slq8": lambda: SLQChannel(8), "slq4": lambda: SLQChannel(4), "uslq8": lambda: USLQChannel(8),
            "packed4": lambda: PackedSLQChannel(4)}
PLACEMENTS = {"device": (DEV, DEV), "cpu": ("cpu", "cpu"), "prev_device_new_cpu": (DEV, "cpu"),
              "prev_cpu_new_device": ("cpu", DEV)}


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "delta_small.npz"))


def _dicts(g, prev_dev, new_dev, new_order=False):
    order = [str(n) for n in g["order"]]
    prev = {n: torch.from_numpy(g[f"prev__{n}"].copy()).to(prev_dev) for n in order}
    new = {n: torch.from_numpy(g[f"new__{n}"].copy()).to(new_dev)
           for n in ([str(n) for n in g["new_order"]] if new_order else order)}
    return prev, new


def diff_parameters(params_a, params_b):
    """Src/ADFL/model.py:350-358 restated: b - a, in params_a's key order."""
    assert set(params_a.keys()) == set(params_b.keys())
    with torch.no_grad():
        return {k: params_b[k] - params_a[k] for k in params_a}


def _bytes(t: torch.Tensor) -> bytes:
    t = t.detach().cpu().contiguous()
    return (t.int_repr() if t.is_quantized else t).numpy().tobytes()


def assert_same_payload(got: QuantParameters, want: QuantParameters):
    """Field for field: key order, size, and per entry data (bits, dtype, shape, device, quantizer), bits,
    scale, signs, shape, dtype, q_dtype."""
    assert isinstance(got, QuantParameters) and isinstance(want, QuantParameters)
    assert list(got.params.keys()) == list(want.params.keys())
    assert got.size == want.size
    for n, a in got.params.items():
        b = want.params[n]
        assert (a.bits, tuple(a.shape), a.dtype, a.q_dtype) == (b.bits, tuple(b.shape), b.dtype, b.q_dtype), n
        assert type(a.scale) is type(b.scale) and same_f32(np.float32(a.scale), np.float32(b.scale)), n
        assert a.scale == b.scale or (a.scale != a.scale and b.scale != b.scale), n
        assert torch.equal(a.signs, b.signs) and a.signs.dtype == b.signs.dtype, n
        assert (a.data.dtype, a.data.shape, a.data.device, a.data.is_quantized) == \
               (b.data.dtype, b.data.shape, b.data.device, b.data.is_quantized), n
        if a.data.is_quantized:
            assert a.data.qscheme() == b.data.qscheme() and a.data.q_zero_point() == b.data.q_zero_point() == 0, n
            assert a.data.q_scale() == b.data.q_scale() or a.scale != a.scale, n
        assert _bytes(a.data) == _bytes(b.data), n


def assert_matches_fixture(ch, got: QuantParameters, g, new_devs):
    """The payload against the executed reference: int_repr (packed channel: pack_4bit of it), scale bits,
    passthrough values, key order, size; every entry on its params_new tensor's device."""
    bits = ch.bits
    packed = isinstance(ch, PackedSLQChannel)
    order = [str(n) for n in g["order"]]
    qnames = [str(n) for n in g[f"b{bits}__qnames"]]
    assert list(got.params.keys()) == order == [str(n) for n in g[f"b{bits}__order"]]
    size = 0
    for n in order:
        p = got.params[n]
        assert p.bits == bits and p.data.device.type == new_devs[n], n
        if n in qnames:
            q = g[f"b{bits}__q__{n}"]
            scale = f32_from_bits(int(g[f"b{bits}__scale_bits"][qnames.index(n)]))
            assert isinstance(p.scale, float) and same_f32(np.float32(p.scale), scale), n
            assert tuple(p.shape) == q.shape and p.dtype == torch.float32, n
            if packed:
                assert p.data.dtype == torch.int8 and p.q_dtype == torch.int8 and p.data.ndim == 1, n
                assert np.array_equal(p.data.cpu().numpy().view(np.uint8), oracle.pack_int4(q)), n
                size += (q.size + 1) // 2
            else:
                assert p.data.dtype == torch.qint8 and p.q_dtype == torch.qint8, n
                assert p.data.q_zero_point() == 0 and p.data.q_scale() == p.scale, n
                assert np.array_equal(p.data.cpu().int_repr().numpy(), q), n
                size += q.size
        else:
            want = g[f"pass__{n}"]
            assert p.scale == 1 and tuple(p.shape) == want.shape, n
            have = p.data.cpu().numpy()
            assert have.dtype == want.dtype and have.tobytes() == want.tobytes(), n
            size += want.nbytes
    assert got.size == size
    if not packed:
        assert got.size == int(g[f"b{bits}__size"])


def assert_decodes_to_fixture(ch, got: QuantParameters, g):
    bits = ch.bits
    dec, _ = ch.on_server_receive(got)
    qnames = [str(n) for n in g[f"b{bits}__qnames"]]
    assert list(dec.keys()) == [str(n) for n in g["order"]]
    for n, t in dec.items():
        if n in qnames:
            scale = f32_from_bits(int(g[f"b{bits}__scale_bits"][qnames.index(n)]))
            want = oracle.decode(g[f"b{bits}__q__{n}"], scale)
            assert t.dtype == torch.float32 and same_f32(t.cpu().numpy(), want), n
        else:
            assert t.cpu().numpy().tobytes() == g[f"pass__{n}"].tobytes(), n


@pytest.mark.parametrize("placement", list(PLACEMENTS))
@pytest.mark.parametrize("channel", list(CHANNELS))
def test_send_delta_equals_the_two_steps_and_the_fixture(g, channel, placement):
    ch = CHANNELS[channel]()
    prev_dev, new_dev = PLACEMENTS[placement]
    prev, new = _dicts(g, prev_dev, new_dev)
    keep = {side: {n: t.clone() for n, t in d.items()} for side, d in (("prev", prev), ("new", new))}
    got, seconds = ch.send_delta(prev, new)
    assert seconds > 0
    for side, d in (("prev", prev), ("new", new)):     # both inputs bit-unchanged
        for n, t in d.items():
            assert _bytes(t) == _bytes(keep[side][n]) and t.device == keep[side][n].device, (side, n)
    dev_type = torch.device(new_dev).type
    assert_matches_fixture(ch, got, g, {n: dev_type for n in new})
    # the two steps on one placement: plain torch refuses a difference across devices, so a mixed pair's
    # diff_parameters is taken where params_new lives
    want, _ = ch.on_client_send(diff_parameters({n: t.to(new_dev) for n, t in prev.items()}, new))
    assert_same_payload(got, want)
    assert_decodes_to_fixture(ch, got, g)


@pytest.mark.parametrize("channel", ["slq8", "packed4"])
def test_output_follows_params_prev_key_order(g, channel):
    ch = CHANNELS[channel]()
    prev, new = _dicts(g, DEV, DEV, new_order=True)
    assert list(new.keys()) != list(prev.keys())
    got, _ = ch.send_delta(prev, new)
    assert list(got.params.keys()) == list(prev.keys())
    assert_matches_fixture(ch, got, g, {n: "cuda" for n in new})
    assert_same_payload(got, ch.on_client_send(diff_parameters(prev, new))[0])


@pytest.mark.parametrize("channel", ["slq8", "packed4"])
@pytest.mark.parametrize("dev", [DEV, "cpu"])
def test_reference_errors(g, channel, dev):
    ch = CHANNELS[channel]()
    prev, new = _dicts(g, dev, dev)
    with pytest.raises(AssertionError):                       # diff_parameters' key-set assertion
        ch.send_delta(prev, {n: t for n, t in new.items() if n != "fc.bias"})
    with pytest.raises(AssertionError):
        ch.send_delta(prev, dict(new, extra=torch.zeros(2, 2, device=dev)))
    bad_prev, bad_new = dict(prev), dict(new)
    bad_prev["fc.weight"], bad_new["fc.weight"] = prev["fc.weight"].double(), new["fc.weight"].double()
    with pytest.raises(RuntimeError, match="Quantize only works on Float Tensor, got Double"):
        ch.send_delta(bad_prev, bad_new)
    with pytest.raises(RuntimeError, match="Quantize only works on Float Tensor, got Double"):
        ch.send_delta(bad_prev, new)                          # fp32 - fp64 promotes to fp64
    with pytest.raises(RuntimeError, match="Quantize only works on Float Tensor, got Double"):
        ch.on_client_send(diff_parameters(bad_prev, new))     # ... as in the two steps
    empty = torch.zeros(0, 3, device=dev)
    with pytest.raises(RuntimeError, match=r"max\(\): Expected reduction dim"):
        ch.send_delta(dict(prev, **{"fc.weight": empty}), dict(new, **{"fc.weight": empty.clone()}))
    with pytest.raises(RuntimeError, match="must match the size of tensor"):   # torch's own b - a error
        ch.send_delta(prev, dict(new, **{"fc.weight": torch.zeros(33, 16, device=dev)}))
    with pytest.raises(RuntimeError):                         # broadcastable, but not one model's two states
        ch.send_delta(prev, dict(new, **{"fc.weight": torch.zeros(1, 17, device=dev)}))
    got, _ = ch.send_delta(prev, new)                         # the channel still works after the errors
    assert_matches_fixture(ch, got, g, {n: torch.device(dev).type for n in new})


@pytest.mark.parametrize("channel", ["slq8", "slq4", "packed4"])
def test_qafel_round_with_a_device_resident_hidden_state(g, channel):
    """Src/ADFL/Server/qafel.py:160-161 then :179-180: the hidden state follows the clients' view of the global
    model. send_delta(hidden, g) + receive_add_(q, [hidden]) on the device against the reference sequence in
    torch ops on CPU copies."""
    ch = CHANNELS[channel]()
    hidden, g_params = _dicts(g, DEV, DEV)
    ref_hidden = {n: t.cpu().clone() for n, t in hidden.items()}
    ref_g = {n: t.cpu().clone() for n, t in g_params.items()}
    q_max = 2 ** (ch.bits - 1) - 1
    with torch.no_grad():
        for n, h in ref_hidden.items():
            d = ref_g[n] - h                                               # diff_parameters
            if d.ndim > 1:                                                 # quant.py:97-112
                scale = torch.max(torch.abs(d)) / q_max
                d = torch.quantize_per_tensor(d, scale, 0, dtype=torch.qint8).dequantize()
            h.mul_(1).add_(d, alpha=1)                                     # add_parameters_inpace(..., 1, 1)
    q_update, _ = ch.send_delta(hidden, g_params)
    ch.receive_add_(q_update, [hidden])
    for n, h in hidden.items():
        assert h.is_cuda and _bytes(h) == _bytes(ref_hidden[n]), n


def test_two_layouts_in_a_row_do_not_share_stale_staging(g):
    """Two calls with different layouts, device then CPU and back: each result is its own."""
    ch = SLQChannel(8)
    rng = np.random.default_rng(5)

    def pair(shapes, dev):
        new = {f"t{i}": torch.from_numpy(rng.standard_normal(s, dtype=np.float32)).to(dev)
               for i, s in enumerate(shapes)}
        prev = {n: t + 1e-3 * torch.from_numpy(rng.standard_normal(tuple(t.shape), dtype=np.float32)).to(dev)
                for n, t in new.items()}
        return prev, new

    cases = [pair([(40, 50), (3,), (1, 9000)], DEV), pair([(7, 7), (1, 70000), (5,), (64, 64)], DEV),
             pair([(40, 50), (3,), (1, 9000)], "cpu"), pair([(2, 1030), (9, 9)], DEV)]
    results = [ch.send_delta(p, n)[0] for p, n in cases]      # all sent before any is checked
    for (p, n), got in zip(cases, results):
        assert_same_payload(got, ch.on_client_send(diff_parameters(p, n))[0])
        for name, e in got.params.items():
            if e.data.is_quantized:
                x = (n[name] - p[name]).cpu().numpy()
                wq, ws = oracle.encode(x, 8)
                assert np.array_equal(e.data.cpu().int_repr().numpy(), wq) and same_f32(np.float32(e.scale), ws)
