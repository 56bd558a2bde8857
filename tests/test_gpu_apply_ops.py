"""GPU: torch.ops.adfl_apply.slq_decode_axpby_batched, slq_decode_axpby_batched_int4 and stoch_decode_axpby_batched —
the asynchronous server's update step over flat buckets as traceable custom ops: each through
torch.library.opcheck (schema, fake implementation, AOT dispatch), equal to decode then torch's own
(alpha * base) + (beta * decoded) bit for bit, and one decode-and-apply function under torch.compile
(aot_eager, fullgraph) equal to eager."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import adfl_amd  # noqa: E402,F401  registers torch.ops.adfl.*

DEV = torch.device("cuda", 0)
A = torch.ops.adfl
AP = torch.ops.adfl_apply
ALPHA, BETA = 1 - 0.6 * 2 ** -0.5, 0.6 * 2 ** -0.5


def _bucket(seed, sizes, gap):
    """Flat fp32 buffer with tensors at even offsets separated by `gap` elements."""
    rng = np.random.default_rng(seed)
    offsets, pos = [], 0
    for n in sizes:
        offsets.append(pos)
        pos += n + n % 2 + gap
    flat = np.zeros(pos, np.float32)
    for o, n in zip(offsets, sizes):
        flat[o:o + n] = rng.standard_normal(n, dtype=np.float32) * np.float32(1e-2)
    return (torch.from_numpy(flat).to(DEV), torch.tensor(offsets, dtype=torch.int64),
            torch.tensor(sizes, dtype=torch.int64))


def _same(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _owned(off, siz, n):
    m = torch.zeros(n, dtype=torch.bool)
    for o, s in zip(off.tolist(), siz.tolist()):
        m[o:o + s] = True
    return m.to(DEV)


@pytest.mark.parametrize("gap", [0, 2])
def test_slq_ops_equal_decode_then_torch(gap):
    x, off, siz = _bucket(4, [3, 4097, 900, 8192], gap)
    base = torch.randn(x.numel(), device=DEV)
    own = _owned(off, siz, x.numel())
    q, s = A.slq_encode_batched(x, off, siz, 8)
    got = AP.slq_decode_axpby_batched(q, s, base, off, siz, ALPHA, BETA)
    want = (ALPHA * base) + (BETA * A.slq_decode_batched(q, s, off, siz))
    assert got.dtype == torch.float32 and got.shape == base.shape
    assert _same(got[own], want[own]) and not got[~own].any()   # positions no tensor owns are zero
    p, s4 = A.slq_encode_batched_int4(x, off, siz, 4)
    got4 = AP.slq_decode_axpby_batched_int4(p, s4, base, off, siz, ALPHA, BETA)
    want4 = (ALPHA * base) + (BETA * A.slq_decode_batched_int4(p, s4, off, siz, x.numel()))
    assert _same(got4[own], want4[own]) and not got4[~own].any()
    torch.library.opcheck(AP.slq_decode_axpby_batched, (q, s, base, off, siz, ALPHA, BETA))
    torch.library.opcheck(AP.slq_decode_axpby_batched_int4, (p, s4, base, off, siz, ALPHA, BETA))


@pytest.mark.parametrize("codec", ["qsgd", "rqsgd", "cnat"])
def test_stoch_op_equals_decode_then_torch(codec):
    x, off, siz = _bucket(6, [3, 4097, 900, 8192], 3)
    base = torch.randn(x.numel(), device=DEV)
    own = _owned(off, siz, x.numel())
    lv, sg, nr, mn = A.stoch_encode_batched(x, off, siz, codec, 8, 99, 0)
    got = AP.stoch_decode_axpby_batched(lv, sg, nr, mn, base, off, siz, codec, 8, ALPHA, BETA)
    want = (ALPHA * base) + (BETA * A.stoch_decode_batched(lv, sg, nr, mn, off, siz, codec, 8))
    assert _same(got[own], want[own]) and not got[~own].any()
    torch.library.opcheck(AP.stoch_decode_axpby_batched, (lv, sg, nr, mn, base, off, siz, codec, 8, ALPHA, BETA))


def test_decode_and_apply_under_torch_compile():
    """One function that encodes a client's update, then applies it to the server's bucket through each fused op,
    traced by torch.compile (fullgraph: every op through its fake implementation at trace time, the HIP kernels
    at run time), equals eager bit for bit."""
    x, off, siz = _bucket(9, [4096, 80, 8192], 0)
    base = torch.randn(x.numel(), device=DEV)

    def step(x, base):
        q, s = torch.ops.adfl.slq_encode_batched(x, off, siz, 8)
        g = torch.ops.adfl_apply.slq_decode_axpby_batched(q, s, base, off, siz, ALPHA, BETA)
        p, s4 = torch.ops.adfl.slq_encode_batched_int4(x, off, siz, 4)
        g = torch.ops.adfl_apply.slq_decode_axpby_batched_int4(p, s4, g, off, siz, 1.0, 1.0)
        e = torch.ops.adfl.stoch_encode_batched(x, off, siz, "rqsgd", 8, 99, 0)
        return torch.ops.adfl_apply.stoch_decode_axpby_batched(*e, g, off, siz, "rqsgd", 8, 0.4, 0.6)

    eager = step(x, base)
    compiled = torch.compile(step, backend="aot_eager", fullgraph=True)(x, base)
    assert _same(eager, compiled)
