"""GPU: the fused decode-mean + axpby entries (adfl_slq_dequantize_mean_axpby_batched, its int4 form and
adfl_stoch_dequantize_mean_axpby_batched; the synchronous DELTA server step, Src/ADFL/Strategy/simple.py:87-89)
through ops / stoch and the three torch.ops.adfl_apply ops, held to what they fuse: the existing
*_dequantize_mean_batched output copied to the host and combined by the reference's statement
(alpha * g) + (beta * mean) in CPU torch. Every element is compared as its 32 bits; a NaN must meet a NaN (the
CPU and the GPU do not give a generated NaN the same sign bit).

Shapes: the aggregate fixture's ten tensor sizes (SEQ, ILP4 and INNER columns), plus one tensor of 2 * 8192 + 37
elements (chunk boundaries and heads), in a compact layout (tensors at odd offsets) and a 64-aligned one. Bases and
outputs as separate tensors (compact layout: the slot's phase differs from the tensor's, the 4-byte route), as
bucket + offset tables (the 16-byte route where the layout is aligned) and in place."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import adfl_amd  # noqa: E402,F401  registers the ops
from adfl_amd import ops, stoch  # noqa: E402

DEV = torch.device("cuda", 0)
AP = torch.ops.adfl_apply
F32 = np.float32
SMALL = [432, 330, 35, 6, 1, 3, 9, 2064, 1313, 1024]
BIG = SMALL + [2 * 8192 + 37]
CODECS = ["slq8", "int4", "qsgd", "rqsgd", "cnat"]
PAIRS = [(1.0, 1.0), (0.4, 0.6)]


def same_bits(got, want):
    got, want = np.asarray(got, F32).reshape(-1), np.asarray(want, F32).reshape(-1)
    ng, nw = np.isnan(got), np.isnan(want)
    return np.array_equal(ng, nw) and np.array_equal(got[~ng].view(np.uint32), want[~nw].view(np.uint32))


class Rows:
    """K bucket payloads of one codec drawn directly as bytes, the existing mean over them and the fused launch.
    Tensor 0's first column decodes to -0 in every row; with `special`, row 0 has a zero scale / norm for tensor
    1, row k-1 a NaN one for tensor 2 and an inf one for tensor 3."""

    def __init__(self, codec, sizes, align, k, special=True, seed=0, lay=None):
        self.codec, self.k = codec, k
        if codec == "int4" and align == 1:
            align = 2
        self.lay = lay = lay if lay is not None else ops.BucketLayout(sizes, align=align)
        rng = np.random.default_rng(seed * 1000 + k * 10 + align)
        row = (lay.total + 15) // 16 * 16
        t = len(sizes)
        sc = (rng.random((k, t), dtype=F32) + F32(0.5)) * F32(1e-3)
        o0 = int(lay.offsets[0])
        if codec in ("slq8", "int4"):
            sc[:, 0] = -sc[:, 0]   # code 0 under a negative scale: -0
        if special:
            sc[0, 1] = 0.0
            sc[k - 1, 2] = np.nan
            sc[k - 1, 3] = np.inf
        self.scales = torch.from_numpy(sc).to(DEV)
        self.mins = None
        if codec == "slq8":
            q = rng.integers(-127, 128, size=(k, row), dtype=np.int8)
            q[:, o0] = 0
            self.q = torch.from_numpy(q).to(DEV)
        elif codec == "int4":
            p = rng.integers(0, 256, size=(k, row), dtype=np.uint8)   # a row holds 2 * row nibbles >= the layout
            p[:, o0 // 2] = (p[:, o0 // 2] & 0x0F) | 0x80             # high nibble 8: code 0 for the even element
            self.q = torch.from_numpy(p).to(DEV)
        else:
            if codec == "cnat":
                lv = rng.integers(-20, 1, size=(k, row), dtype=np.int8).view(np.uint8)
            else:
                lv = rng.integers(0, 256, size=(k, row), dtype=np.uint8)
            sg = (rng.integers(0, 2, size=(k, row), dtype=np.int8) * 2 - 1).astype(np.int8)
            if codec != "cnat":
                lv[:, o0], sg[:, o0] = 0, -1   # level 0, sign -1: -0
            self.q = torch.from_numpy(lv).to(DEV)
            self.signs = torch.from_numpy(sg).to(DEV)
            if codec == "rqsgd":
                self.mins = torch.from_numpy((rng.random((k, t), dtype=F32) - F32(0.5)) * F32(1e-3)).to(DEV)

    def mean(self):
        """The existing entry's bucket, on the host."""
        if self.codec in ("slq8", "int4"):
            m = ops.dequantize_mean_batched(self.q, self.scales, self.lay, packed=self.codec == "int4")
        else:
            m = stoch.dequantize_mean_batched(self.codec, self.q, self.signs, self.scales, self.lay, 8,
                                              mins=self.mins, out=torch.zeros(self.lay.total, device=DEV))
        return m.cpu()

    def fused(self, bases, outs, alpha, beta):
        if self.codec in ("slq8", "int4"):
            ops.dequantize_mean_axpby_batched(self.q, self.scales, self.lay, bases, outs, alpha, beta,
                                              packed=self.codec == "int4")
        else:
            stoch.dequantize_mean_axpby_batched(self.codec, self.q, self.signs, self.scales, self.mins, self.lay, 8,
                                                bases, outs, alpha, beta)


def draw_g(lay, seed):
    """The global parameters, one host tensor per layout tensor: -0.0 against the all -0 column, a denormal, an inf."""
    rng = np.random.default_rng(seed)
    g = [torch.from_numpy(rng.standard_normal(int(n), dtype=F32) * F32(1e-2)) for n in lay.sizes]
    g[0][0] = -0.0
    g[0][1] = 1e-41
    g[0][2] = float("inf")
    g[7][33] = float("-inf")
    return g


def check(rows, pairs=PAIRS):
    lay = rows.lay
    m = rows.mean()
    g = draw_g(lay, rows.k)
    spans = list(zip(lay.offsets.tolist(), lay.sizes.tolist()))
    for alpha, beta in pairs:
        with torch.no_grad():
            want = [((alpha * gt) + (beta * m[o:o + n])).numpy() for gt, (o, n) in zip(g, spans)]
        tag = (rows.codec, rows.k, alpha, beta)
        # separate tensors, out of place
        bases = [t.to(DEV) for t in g]
        outs = [torch.full_like(b, 7.0) for b in bases]
        rows.fused(bases, outs, alpha, beta)
        # in place
        inpl = [b.clone() for b in bases]
        rows.fused(inpl, inpl, alpha, beta)
        # bucket + offset tables; positions no tensor owns stay as they are
        bb = torch.full((lay.total,), 3.0, device=DEV)
        for gt, (o, n) in zip(g, spans):
            bb[o:o + n] = gt.to(DEV)
        ob = torch.full((lay.total,), 7.0, device=DEV)
        rows.fused(bb, ob, alpha, beta)
        torch.cuda.synchronize()
        own = np.zeros(lay.total, bool)
        obn = ob.cpu().numpy()
        for t, (o, n) in enumerate(spans):
            own[o:o + n] = True
            assert same_bits(outs[t].cpu().numpy(), want[t]), ("tensors",) + tag + (t, n)
            assert same_bits(inpl[t].cpu().numpy(), want[t]), ("in place",) + tag + (t, n)
            assert same_bits(obn[o:o + n], want[t]), ("bucket",) + tag + (t, n)
            assert same_bits(bases[t].cpu().numpy(), g[t].numpy()), ("base modified",) + tag + (t, n)
        assert (obn[~own] == 7.0).all(), ("unowned positions written",) + tag


@pytest.mark.parametrize("align", [1, 64])
@pytest.mark.parametrize("k", [1, 2, 5, 16, 17])
@pytest.mark.parametrize("codec", CODECS)
def test_fused_equals_mean_then_reference_statement(codec, k, align):
    check(Rows(codec, BIG, align, k))


@pytest.mark.parametrize("codec", CODECS)
def test_deep_form_at_k_257(codec):
    """K >= 256 takes the DEEP cascade (levels 2-3); the small shapes only."""
    check(Rows(codec, SMALL, 1, 257, special=False), pairs=PAIRS[:1])


def test_g_minus_zero_against_an_all_minus_zero_column():
    """Every row decodes tensor 0's first element to -0; the sum starts from +0, so the mean is +0 and
    1 * -0.0 + 1 * +0 is +0: the fused output's sign bit is clear."""
    for codec in ("slq8", "qsgd"):
        rows = Rows(codec, SMALL, 1, 5)
        assert rows.mean()[int(rows.lay.offsets[0])].view(torch.int32).item() == 0
        base = [t.to(DEV) for t in draw_g(rows.lay, 1)]
        out = [torch.empty_like(b) for b in base]
        rows.fused(base, out, 1.0, 1.0)
        assert out[0][:1].view(torch.int32).item() == 0


@pytest.mark.parametrize("gap", [0, 2])
def test_custom_ops_equal_the_two_steps_and_pass_opcheck(gap):
    """Caller-placed tensors at even offsets `gap` apart, K = 5 rows, a flat base bucket in, a new one out."""
    alpha, beta = 0.4, 0.6
    sizes = [3, 4097, 900, 8192]
    offsets, pos = [], 0
    for n in sizes:
        offsets.append(pos)
        pos += n + n % 2 + gap
    off, siz = torch.tensor(offsets, dtype=torch.int64), torch.tensor(sizes, dtype=torch.int64)
    base = torch.randn(pos, device=DEV)
    for codec in ("slq8", "int4", "rqsgd"):
        rows = Rows(codec, sizes, 2, 5, special=False, lay=ops.layout_for(off, siz))
        if codec == "rqsgd":
            args = (rows.q, rows.signs, rows.scales, rows.mins, base, off, siz, codec, 8, alpha, beta)
            op = AP.stoch_decode_mean_axpby_batched
        else:
            args = (rows.q, rows.scales, base, off, siz, alpha, beta)
            op = AP.slq_decode_mean_axpby_batched_int4 if codec == "int4" else AP.slq_decode_mean_axpby_batched
        got = op(*args).cpu()
        assert got.dtype == torch.float32 and got.shape == base.shape
        m, own = rows.mean(), np.zeros(pos, bool)
        for o, n in zip(offsets, sizes):
            with torch.no_grad():
                want = (alpha * base[o:o + n].cpu()) + (beta * m[o:o + n])
            assert same_bits(got[o:o + n].numpy(), want.numpy()), (codec, gap, n)
            own[o:o + n] = True
        assert not got.numpy()[~own].any()   # positions no tensor owns are zero
        torch.library.opcheck(op, args)


def test_odd_int4_offsets_are_refused_before_anything_is_launched():
    """The chunk table lives on the device, so the int4 C entry cannot see an odd tensor offset: the op that
    builds the table refuses the layout."""
    lay = ops.BucketLayout([3, 5], align=1)   # the second tensor at offset 3
    q = torch.zeros((2, 16), dtype=torch.uint8, device=DEV)
    sc = torch.ones((2, 2), device=DEV)
    g = [torch.zeros(3, device=DEV), torch.zeros(5, device=DEV)]
    with pytest.raises(ValueError):
        ops.dequantize_mean_axpby_batched(q, sc, lay, g, g, 1.0, 1.0, packed=True)
