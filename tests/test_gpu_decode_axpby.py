"""GPU: the fused decode + axpby / scale kernels (adfl_slq_dequantize_axpby_batched, its int4 form and
adfl_stoch_dequantize_axpby_batched) through ops / stoch, against the three-rounding restatement computed on the
host in numpy fp32 from the decode's own values: out = fp32(fp32(af * y) + fp32(bf * d)), SCALE out = fp32(bf * d)
— what torch computes for add_parameters (Src/ADFL/model.py:326-334) and FedBuff's mul_ (fed_buff.py:72-80).
Compared as uint32 bits, NaNs by position."""

import numpy as np
import pytest
import torch

import slq_oracle as oracle

pytestmark = pytest.mark.gpu

from adfl_amd import ops, stoch  # noqa: E402

DEV = torch.device("cuda", 0)
F32 = np.float32
CODECS = ["slq8", "int4", "qsgd", "rqsgd", "cnat"]
SHAPES = [([1, 3, 5, 8192, 8193, 70001], 3), ([64] * 300, 2), ([7, 1, 8191, 8195, 13, 40000, 2], 1)]
PAIRS = [(1.0, 1.0), (0.4, 0.6), (1 - 0.6 * 2 ** -0.5, 0.6 * 2 ** -0.5), (1.0, 3 ** -0.5), (0.0, 1.0), (1.0, 0.0)]
CASES = [(c, s, k, a) for c in CODECS for s, k in SHAPES for a in (64, 1, 2) if not (c == "int4" and a == 1)]


class Payload:
    """One bucket payload of a codec, its decode (host numpy, per tensor) and the fused launch over it."""

    def __init__(self, codec, lay, flat=None, planes=None):
        self.codec, self.lay = codec, lay
        if planes is not None:
            self.p = planes
        elif codec == "slq8":
            self.p = ops.encode_batched(flat, lay, 8)
        elif codec == "int4":
            self.p = ops.encode_batched_int4(flat, lay, 4)
        elif codec == "qsgd":
            self.p = stoch.qsgd_encode_batched(flat, lay, 8, seed=5, counter=0)
        elif codec == "rqsgd":
            self.p = stoch.rqsgd_encode_batched(flat, lay, 8, seed=5, counter=0)
        else:
            self.p = stoch.cnat_encode_batched(flat, lay, 8, seed=5, counter=0)

    def decoded(self):
        p, lay = self.p, self.lay
        if self.codec == "slq8":   # the oracle's decode; every other codec: the existing decode op's output
            q, s = p[0].cpu().numpy(), p[1].cpu().numpy()
            return [oracle.np_decode(q[o:o + n], s[t]) for t, (o, n) in enumerate(zip(lay.offsets, lay.sizes))]
        if self.codec == "int4":
            d = ops.decode_batched_int4(p[0], p[1], lay)
        elif self.codec == "qsgd":
            d = stoch.qsgd_decode_batched(p[0], p[1], p[2], lay, 8)
        elif self.codec == "rqsgd":
            d = stoch.rqsgd_decode_batched(p[0], p[1], p[2], p[3], lay, 8)
        else:
            d = stoch.cnat_decode_batched(p[0], p[1], p[2], lay)
        d = d.cpu().numpy()
        return [d[o:o + n].copy() for o, n in zip(lay.offsets, lay.sizes)]

    def apply(self, bases, outs, alpha, beta):
        p, lay = self.p, self.lay
        if self.codec in ("slq8", "int4"):
            ops.dequantize_axpby_batched(p[0], p[1], lay, bases, outs, alpha, beta, packed=self.codec == "int4")
        else:
            stoch.dequantize_axpby_batched(self.codec, p[0], p[1], p[2], lay, 8, bases, outs, alpha, beta,
                                           mins=p[3] if self.codec == "rqsgd" else None)


def same_bits(got, want):
    got, want = np.asarray(got, F32).reshape(-1), np.asarray(want, F32).reshape(-1)
    ng, nw = np.isnan(got), np.isnan(want)
    return np.array_equal(ng, nw) and np.array_equal(got[~ng].view(np.uint32), want[~nw].view(np.uint32))


def np_axpby(y, d, alpha, beta):
    with np.errstate(all="ignore"):
        return ((F32(alpha) * y).astype(F32) + (F32(beta) * d).astype(F32)).astype(F32)


def np_scale(d, beta):
    with np.errstate(all="ignore"):
        return (F32(beta) * d).astype(F32)


def bucket_of(lay, parts):
    flat = np.zeros(lay.total, F32)
    for o, x in zip(lay.offsets, parts):
        flat[o:o + x.size] = x
    return flat


def check_all_modes(pl, bases_np, pairs):
    """Out of place, in place and SCALE for every coefficient pair; bases_np: K lists of T host arrays."""
    lay, dec = pl.lay, pl.decoded()
    k = len(bases_np)
    for alpha, beta in pairs:
        bases = [[torch.from_numpy(b).to(DEV) for b in model] for model in bases_np]
        outs = [[torch.full((int(n),), 7.0, device=DEV) for n in lay.sizes] for _ in range(k)]
        pl.apply(bases, outs, alpha, beta)
        scaled = [[torch.full((int(n),), 7.0, device=DEV) for n in lay.sizes] for _ in range(k)]
        pl.apply(None, scaled, alpha, beta)
        inplace = [[b.clone() for b in model] for model in bases]
        pl.apply(inplace, inplace, alpha, beta)
        torch.cuda.synchronize()
        for m in range(k):
            for t, d in enumerate(dec):
                y = bases_np[m][t]
                want = np_axpby(y, d, alpha, beta)
                tag = (pl.codec, alpha, beta, m, t, d.size)
                assert same_bits(outs[m][t].cpu().numpy(), want), ("out of place",) + tag
                assert same_bits(inplace[m][t].cpu().numpy(), want), ("in place",) + tag
                assert same_bits(scaled[m][t].cpu().numpy(), np_scale(d, beta)), ("scale",) + tag
                assert same_bits(bases[m][t].cpu().numpy(), y), ("base modified",) + tag
    if k == 1:   # two flat buckets, pointer t = bucket + offset t (the channels' host route): any alignment
        alpha, beta = pairs[1]
        base = torch.from_numpy(bucket_of(lay, bases_np[0])).to(DEV)
        out = torch.full((lay.total,), 7.0, device=DEV)
        pl.apply(base, out, alpha, beta)
        got = out.cpu().numpy()
        for t, (o, n, d) in enumerate(zip(lay.offsets, lay.sizes, dec)):
            assert same_bits(got[o:o + n], np_axpby(bases_np[0][t], d, alpha, beta)), ("flat", pl.codec, t)


@pytest.mark.parametrize("codec,sizes,k,align", CASES,
                         ids=[f"{c}-{len(s)}t-k{k}-a{a}" for c, s, k, a in CASES])
def test_axpby_scale_and_inplace_match_the_three_roundings(codec, sizes, k, align):
    """Aligned buckets (16-byte path), compact ones (align 1 / 2: offsets with every residue mod 4, the
    element-wise path), one-element tensors, chunk boundaries (8192, 8193), many small tensors, K targets."""
    rng = np.random.default_rng(len(sizes) * 10 + k + align)
    lay = ops.BucketLayout(sizes, align=align)
    xs = [rng.standard_normal(n, dtype=F32) * F32(1e-2) for n in sizes]
    pl = Payload(codec, lay, torch.from_numpy(bucket_of(lay, xs)).to(DEV))
    bases = [[rng.standard_normal(n, dtype=F32) for n in sizes] for _ in range(k)]
    check_all_modes(pl, bases, PAIRS)


@pytest.mark.parametrize("codec", CODECS)
def test_special_values(codec):
    """An all-zero tensor (scale / norm 0), a tensor holding NaN, one holding +-inf, one of magnitude about 1e-38
    (with beta 0.5 the products are subnormal: kept, not flushed), over a base holding +-inf, NaN, -0.0 and
    denormals. No shortcut for a zero coefficient: 0 * inf and 0 * NaN are NaN."""
    rng = np.random.default_rng(3)
    sizes = [40, 37, 33, 64, 8200]
    xs = [rng.standard_normal(n, dtype=F32) for n in sizes]
    xs[0][:] = 0.0
    xs[1][5] = np.nan
    xs[2][3], xs[2][17] = np.inf, -np.inf
    xs[3] *= F32(4e-39)   # max |x| about 1e-38: every decoded value times 0.5 is below the smallest normal
    lay = ops.BucketLayout(sizes)
    pl = Payload(codec, lay, torch.from_numpy(bucket_of(lay, xs)).to(DEV))
    bases = [[rng.standard_normal(n, dtype=F32) for n in sizes]]
    for b in bases[0]:
        b[0], b[1], b[2], b[3] = np.inf, -np.inf, np.nan, -0.0
        b[4], b[5] = F32(1e-45), F32(-3e-39)
    check_all_modes(pl, bases, PAIRS + [(1.0, 0.5), (0.5, 0.5)])
    sub = np_scale(pl.decoded()[3], 0.5)
    if codec not in ("qsgd", "cnat"):   # their L2 norm of 1e-38 data underflows to 0: the zero branch instead
        assert np.any((np.abs(sub) > 0) & (np.abs(sub) < F32(1.1754944e-38))), "the case must produce subnormals"


@pytest.mark.parametrize("codec", CODECS)
def test_scale_keeps_the_sign_of_zero_axpby_over_zeros_does_not(codec):
    """SCALE is not AXPBY over a zero base: a decode of -0.0 stays -0.0 under fp32(bf * d), while
    fp32(+0.0 + -0.0) is +0.0. The two differ in the sign of zero and nowhere else."""
    n = 4099
    lay = ops.BucketLayout([n])
    rng = np.random.default_rng(8)
    neg = rng.random(lay.total) < 0.5
    one = torch.ones(1, device=DEV)
    zero = torch.zeros(1, device=DEV)
    if codec == "slq8":     # scale 0: fp32(0 * q) is -0.0 for q < 0
        q = torch.from_numpy(np.where(neg, -5, 9).astype(np.int8)).to(DEV)
        planes = (q, zero)
    elif codec == "int4":   # nibbles 3 (code -5) and 12 (code 4), scale 0
        codes = np.where(neg, 3, 12).astype(np.uint8)
        codes = np.concatenate([codes, np.zeros(lay.total % 2, np.uint8)])
        planes = (torch.from_numpy((codes[0::2] << 4 | codes[1::2]).astype(np.uint8)).to(DEV), zero)
    else:                   # level 0 (CNAT: exponent -128 under a tiny norm) with sign -1
        lv = torch.full((lay.total,), -128 if codec == "cnat" else 0, dtype=torch.int8, device=DEV)
        sg = torch.from_numpy(np.where(neg, -1, 1).astype(np.int8)).to(DEV)
        norm = torch.full((1,), 1e-30, device=DEV) if codec == "cnat" else one
        planes = (lv.view(torch.uint8) if codec != "cnat" else lv, sg, norm, zero)
    pl = Payload(codec, lay, planes=planes)
    d = pl.decoded()[0]
    assert np.all(d == 0) and np.signbit(d).any() and not np.signbit(d).all()
    scaled, summed = torch.full((n,), 7.0, device=DEV), torch.full((n,), 7.0, device=DEV)
    pl.apply(None, [[scaled]], 1.0, 0.5)
    pl.apply([[torch.zeros(n, device=DEV)]], [[summed]], 1.0, 0.5)
    a, b = scaled.cpu().numpy().view(np.uint32), summed.cpu().numpy().view(np.uint32)
    assert np.array_equal(a, np_scale(d, 0.5).view(np.uint32))
    assert np.all(b == 0)
    assert np.all((a ^ b) & 0x7fffffff == 0) and np.array_equal(a != b, np.signbit(d))


def test_rejects_bad_targets():
    lay = ops.BucketLayout([10, 20])
    q = torch.zeros(lay.total, dtype=torch.int8, device=DEV)
    s = torch.ones(2, device=DEV)
    good = [torch.zeros(10, device=DEV), torch.zeros(20, device=DEV)]
    short = [good[0], torch.zeros(21, device=DEV)]
    skew = [good[0], torch.zeros(21, device=DEV)[1:]]
    for bad in (short, skew):
        with pytest.raises(ValueError, match="16-byte aligned fp32"):
            ops.dequantize_axpby_batched(q, s, lay, [good], [bad], 1.0, 1.0)
        with pytest.raises(ValueError, match="16-byte aligned fp32"):
            ops.dequantize_axpby_batched(q, s, lay, [bad], [good], 1.0, 1.0)
        with pytest.raises(ValueError, match="16-byte aligned fp32"):
            stoch.dequantize_axpby_batched("qsgd", q.view(torch.uint8), q, s, lay, 8, None, [bad], 1.0, 1.0)
    with pytest.raises(ValueError):
        ops.dequantize_axpby_batched(q, s, lay, [good, good], [good], 1.0, 1.0)          # 2 bases, 1 output
    with pytest.raises(ValueError):
        ops.dequantize_axpby_batched(q, s, lay, None, [[good[0].double(), good[1]]], 1.0, 1.0)   # not fp32
    with pytest.raises(ValueError):
        ops.dequantize_axpby_batched(q, s, lay, None, torch.zeros(lay.total - 1, device=DEV), 1.0, 1.0)
    with pytest.raises(ValueError):
        ops.dequantize_axpby_batched(q, s, ops.BucketLayout([10, 20], align=1), None, [good], 1.0, 1.0, packed=True)
