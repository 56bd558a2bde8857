"""GPU: ``receive_add_`` of every codec family on every placement of its targets, against the reference's route —
``on_client_receive`` then ``add_parameters_inpace(t, decoded, 1, 1, False)`` (Src/ADFL/Client/pool.py:62-75,
Src/ADFL/Server/qafel.py:176-179 over Src/ADFL/model.py:337-347), the add evaluated by torch on the CPU — bit for
bit. The entries whose targets all live on the device take the codec's fused decode + axpby in place with alpha =
beta = 1; CPU targets, mixed placements and the targets the rule declines (a view 4 bytes off 16-byte alignment, a
non-contiguous one, an fp64 one) take the reference's route itself.

The weights are (1, n) for n around the 8192-element chunk: a tail shorter than 4 elements (1, 3, 5), the chunk
boundary from both sides (8191, 8192, 8193) and a third chunk (16385). A (1, n) tensor is contiguous whatever its
strides, so the non-contiguous target is the small (33, 65) matrix."""

import copy

import pytest
import torch

from test_gpu_channel_apply import same_dict

pytestmark = pytest.mark.gpu

from adfl_amd.Channel import (CNATChannel, PackedQSGDChannel, PackedRQSGDChannel, PackedSLQChannel,  # noqa: E402
                              QSGDChannel, RQSGDChannel, SLQChannel)

CHANNELS = {"slq8": lambda: SLQChannel(8), "slq4": lambda: SLQChannel(4), "packed_slq4": lambda: PackedSLQChannel(4),
            "qsgd8": lambda: QSGDChannel(8), "rqsgd8": lambda: RQSGDChannel(8), "cnat8": lambda: CNATChannel(8),
            "packed_qsgd8": lambda: PackedQSGDChannel(8), "packed_rqsgd4": lambda: PackedRQSGDChannel(4)}
SIZES = [1, 3, 5, 8191, 8192, 8193, 16385]
SKEWED, STRIDED, DOUBLE = "w8193.weight", "mat.weight", "w8191.weight"
K = 2


def _model(seed, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    m = {f"w{n}.weight": torch.randn(1, n, generator=g) for n in SIZES}
    m.update({"mat.weight": torch.randn(33, 65, generator=g), "zero.weight": torch.randn(4, 9, generator=g),
              "fc.bias": torch.randn(10, generator=g), "bn.num_batches_tracked": torch.tensor(7)})
    return {k: v.to(device) for k, v in m.items()}


_cache = {}


def payloads(name):
    """Two CPU payloads per channel, as they arrive from a client: encoded once, handed out as deep copies (the
    passthrough entries alias the payload's own tensors)."""
    if name not in _cache:
        ch = CHANNELS[name]()
        made = []
        for i in range(2):
            update = {k: v * 10.0 ** (-2 - i) if v.is_floating_point() else v for k, v in _model(1 + i).items()}
            update["zero.weight"] = torch.zeros(4, 9)
            torch.manual_seed(11 + i)   # the stochastic encodes' seed
            made.append(ch.on_client_send(update)[0])
        _cache[name] = made
    return [copy.deepcopy(c) for c in _cache[name]]


def _raw(t):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu()
        if t.is_quantized:
            return (t.q_scale(), t.int_repr().numpy().tobytes())
        return (str(t.dtype), tuple(t.shape), t.numpy().tobytes())
    return t


def _snapshot(c):
    return {n: tuple(_raw(getattr(p, f, None)) for f in ("data", "signs", "scale", "scale_2", "shape", "bits"))
            for n, p in c.params.items()}


def _expected(ch, c, targets):
    """The reference's route on CPU copies of `targets`."""
    want = [copy.deepcopy({k: v.cpu() for k, v in t.items()}) for t in targets]
    decoded, _ = ch.on_client_receive(copy.deepcopy(c))
    with torch.no_grad():
        for t in want:
            for k, d in decoded.items():
                t[k].mul_(1).add_(d.cpu(), alpha=1)
    return want


def _check_call(ch, c, targets, what, bystander=None):
    """One receive_add_ call: the targets against the reference's route; the payload, the target tensors' identity
    and the bystander model unmodified."""
    want = _expected(ch, c, targets)
    before = _snapshot(c)
    objects = [{k: (id(v), v.data_ptr(), v.dtype, v.device, v.stride()) for k, v in t.items()} for t in targets]
    aside = copy.deepcopy(bystander)
    assert ch.receive_add_(c, targets) >= 0
    for t, w, o in zip(targets, want, objects):
        same_dict(t, w, what)
        assert {k: (id(v), v.data_ptr(), v.dtype, v.device, v.stride()) for k, v in t.items()} == o, what
    assert _snapshot(c) == before, (what, "payload modified")
    if bystander is not None:
        same_dict(bystander, aside, (what, "bystander modified"))


def _skew(t):
    """A copy of `t` as a view one element (4 bytes) into its storage, and that storage."""
    store = torch.full((t.numel() + 1,), 123.0, device=t.device)
    view = store[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4
    return view, store


@pytest.mark.parametrize("placement", [("cuda", "cuda"), ("cpu", "cpu"), ("cuda", "cpu")],
                         ids=["device", "cpu", "one_each"])
@pytest.mark.parametrize("name", list(CHANNELS))
def test_receive_add_matches_reference_route(name, placement):
    ch = CHANNELS[name]()
    c = payloads(name)[0]
    targets = [_model(20 + i, dev) for i, dev in enumerate(placement)]
    _check_call(ch, c, targets, (name, placement), bystander=_model(30, "cuda"))


@pytest.mark.parametrize("name", list(CHANNELS))
def test_declined_targets_take_the_reference_route(name):
    """A device model whose one weight is a view misaligned by 4 bytes, one non-contiguous and one fp64, beside a
    plain device model: those entries leave the fused launch, the others stay in it."""
    ch = CHANNELS[name]()
    c = payloads(name)[0]
    odd = _model(40, "cuda")
    odd[SKEWED], store = _skew(odd[SKEWED])
    odd[STRIDED] = odd[STRIDED].t().contiguous().t()
    assert not odd[STRIDED].is_contiguous()
    odd[DOUBLE] = odd[DOUBLE].double()
    _check_call(ch, c, [odd, _model(41, "cuda")], (name, "declined"))
    assert float(store[0]) == 123.0   # the element in front of the misaligned view


@pytest.mark.parametrize("name", list(CHANNELS))
def test_special_values_in_the_targets(name):
    """-0.0, inf and NaN at fixed positions of every weight (same_dict compares the NaN positions separately)."""
    ch = CHANNELS[name]()
    c = payloads(name)[0]
    targets = [_model(50 + i, "cuda") for i in range(K)]
    for t in targets:
        for k, v in t.items():
            if v.ndim > 1:
                flat = v.view(-1)
                n = flat.numel()
                flat[0] = -0.0
                if n >= 3:
                    flat[n // 2] = float("inf")
                    flat[n - 1] = float("nan")
                if n > 8192:
                    flat[8192] = float("-inf")
    _check_call(ch, c, targets, (name, "specials"))


@pytest.mark.parametrize("name", list(CHANNELS))
def test_back_to_back_calls_with_different_cpu_payloads(name):
    """The second call's staging must not rewrite what the first call's copies still read."""
    ch = CHANNELS[name]()
    c1, c2 = payloads(name)
    targets = [_model(60 + i, "cuda") for i in range(K)]
    want = _expected(ch, c1, targets)
    want = _expected(ch, c2, want)
    snaps = [_snapshot(c1), _snapshot(c2)]
    ch.receive_add_(c1, targets)
    ch.receive_add_(c2, targets)
    for t, w in zip(targets, want):
        same_dict(t, w, (name, "back to back"))
    assert [_snapshot(c1), _snapshot(c2)] == snaps

