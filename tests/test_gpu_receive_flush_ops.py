"""GPU: the fused decode + accumulate + flush entries (the buffered servers' K-th client update; csrc/slq_codec.hip
k_dequantize_flush_batched, csrc/stoch_codec.hip k_stoch_dequantize_flush) through ops / stoch and the six custom
ops, bit for bit against

* the numpy restatement: the oracle's decode of the stored bytes (slq_oracle / stoch_oracle), u = fp32(factor * d),
  B = fp32(buf + u) (B = u without a buffer), then flush_cases' fedbuff_flush / fadas_flush;
* the two-call route on the device: dequantize_axpby_batched in place on a copy of the buffer (SCALE without one),
  then flush.fedbuff_flush_batched / fadas_flush_batched — `out` and all three moments.

NaN positions must agree; a NaN's sign and payload are not compared (flush_cases.same_bits).

Tensor lengths 1, 3, 4, 5, 8191, 8192, 8193, 2 * 8192 + 3 (below a float4, the tails of 1-3 elements, one chunk
exactly, one element over, more than two chunks, odd sizes for int4's pad nibble) and four short tensors that carry
the special scales / norms (0, denormal, inf, NaN). Layouts: 64-aligned (the 16-byte path), compact (align 1, offsets
of every residue mod 4; int4: align 2, even offsets — the element path) and pointer tables to separate tensors with
buf / g / out / one moment of four tensors viewed 4 bytes into their storage (those chunks alone go element by
element). K = 1 without a buffer, 3 and 7; lr = 0.05; factor = 6 ** -0.5 (FADAS: 1)."""

import numpy as np
import pytest
import torch

import flush_cases as fc
import slq_oracle
import stoch_oracle

pytestmark = pytest.mark.gpu

import adfl_amd  # noqa: E402,F401
from adfl_amd import flush, ops, stoch  # noqa: E402

DEV = torch.device("cuda", 0)
AP = torch.ops.adfl_apply
F32 = np.float32
CODECS = ["slq8", "int4", "qsgd", "rqsgd", "cnat"]
LAYOUTS = ["aligned", "compact", "pointers"]
SIZES = [1, 3, 4, 5, 8191, 8192, 8193, 2 * 8192 + 3, 64, 68, 72, 77]
# scale (SLQ) / norm (stochastic) per tensor; the last four: 0, a denormal, inf, NaN
SCALES = [0.0, 1e-3, 1e-40, np.inf, 3e-4, 2e-4, 1e-4, 5e-4, 0.0, 3e-41, np.inf, np.nan]
NORMS = [0.0, 1.5, 1e-40, np.inf, 0.7, 2.0, 0.3, 1.1, 0.0, 3e-41, np.inf, np.nan]
MINS = [1e-3] * len(SIZES)
LR = 0.05
FACTOR = 6 ** -0.5
KS = [1, 3, 7]           # K = 1: no buffer
BUF_SPECIAL = [-0.0, np.inf, -np.inf, np.nan, 1e-41, 0.0]
MISALIGNED = {"buf": 8193, "g": 8192, "out": 2 * 8192 + 3, "m": 8191}   # operand -> the tensor viewed 4 bytes in
_memo = {}


class Payload:
    """One hand-made bucket payload of a codec in `lay`: its device planes, the oracle's decode per tensor, the
    fused launches and the existing decode + axpby over it."""

    def __init__(self, codec, lay, seed):
        self.codec, self.lay = codec, lay
        rng = np.random.default_rng(seed)
        self.dec = []
        nt = len(SIZES)
        if codec in ("slq8", "int4"):
            nbytes = lay.total if codec == "slq8" else (lay.total + 1) // 2
            plane = np.zeros(nbytes, np.uint8)
            for t, (o, n) in enumerate(zip(lay.offsets.tolist(), SIZES)):
                q = rng.integers(-128, 128, n, dtype=np.int64).astype(np.int8)
                q[0], q[-1] = -128, 127                                   # the extreme codes, first and last element
                if codec == "slq8":
                    plane[o:o + n] = q.view(np.uint8)
                    self.dec.append(slq_oracle.np_decode(q, F32(SCALES[t])))
                else:   # any int8 through pack_4bit: out-of-range codes alias, an odd tensor ends in a pad nibble
                    packed = slq_oracle.np_pack_int4(q)
                    plane[o // 2:o // 2 + packed.size] = packed
                    self.dec.append(slq_oracle.np_decode(slq_oracle.np_unpack_int4(packed, n), F32(SCALES[t])))
            self.planes = (torch.from_numpy(plane).to(DEV), torch.tensor(SCALES, dtype=torch.float32, device=DEV))
        else:
            lv, sg = np.zeros(lay.total, np.uint8), np.zeros(lay.total, np.int8)
            for t, (o, n) in enumerate(zip(lay.offsets.tolist(), SIZES)):
                lo = -128 if codec == "cnat" else 0
                l = rng.integers(lo, lo + 256, n, dtype=np.int64)
                l[0], l[-1] = lo, lo + 255
                if n > 8:
                    l[3:6] = 0                                           # level 0: RQSGD's minimum branch, QSGD's -0.0
                s = rng.choice(np.array([-1, 1], np.int8), n)
                if codec == "cnat":
                    l8 = l.astype(np.int8)
                    lv[o:o + n], sg[o:o + n] = l8.view(np.uint8), s
                    self.dec.append(stoch_oracle.cnat_dequantize(l8, s, F32(NORMS[t])))
                else:
                    l8 = l.astype(np.uint8)
                    lv[o:o + n], sg[o:o + n] = l8, s
                    if codec == "qsgd":
                        self.dec.append(stoch_oracle.qsgd_dequantize(l8, s, 255, F32(NORMS[t])))
                    else:
                        self.dec.append(stoch_oracle.rqsgd_dequantize(l8, s, 255, F32(NORMS[t]), F32(MINS[t])))
            self.planes = (torch.from_numpy(lv).to(DEV), torch.from_numpy(sg).to(DEV),
                           torch.tensor(NORMS, dtype=torch.float32, device=DEV),
                           torch.tensor(MINS, dtype=torch.float32, device=DEV))
        assert len(self.dec) == nt and all(d.dtype == np.float32 for d in self.dec)

    @property
    def _mins(self):
        return self.planes[3] if self.codec == "rqsgd" else None

    def fedbuff(self, buf, g, out, K, factor, lr):
        p, lay = self.planes, self.lay
        if self.codec in ("slq8", "int4"):
            ops.dequantize_fedbuff_flush_batched(p[0], p[1], lay, buf, g, out, K, factor, lr,
                                                 packed=self.codec == "int4")
        else:
            stoch.dequantize_fedbuff_flush_batched(self.codec, p[0], p[1], p[2], lay, 8, buf, g, out, K, factor, lr,
                                                   mins=self._mins)

    def fadas(self, buf, g, m, v, h, out, K, sc):
        p, lay = self.planes, self.lay
        if self.codec in ("slq8", "int4"):
            ops.dequantize_fadas_flush_batched(p[0], p[1], lay, buf, g, m, v, h, out, K, sc,
                                               packed=self.codec == "int4")
        else:
            stoch.dequantize_fadas_flush_batched(self.codec, p[0], p[1], p[2], lay, 8, buf, g, m, v, h, out, K, sc,
                                                 mins=self._mins)

    def axpby(self, bases, outs, alpha, beta):
        p, lay = self.planes, self.lay
        if self.codec in ("slq8", "int4"):
            ops.dequantize_axpby_batched(p[0], p[1], lay, bases, outs, alpha, beta, packed=self.codec == "int4")
        else:
            stoch.dequantize_axpby_batched(self.codec, p[0], p[1], p[2], lay, 8, bases, outs, alpha, beta,
                                           mins=self._mins)


def _layout(codec, kind):
    if kind == "compact":
        return ops.BucketLayout(SIZES, align=2 if codec == "int4" else 1)
    return ops.BucketLayout(SIZES, align=64)


def _payload(codec, kind):
    key = (codec, "compact" if kind == "compact" else "aligned")
    if key not in _memo:
        _memo[key] = Payload(codec, _layout(codec, kind), 31 + CODECS.index(codec))
    return _memo[key]


def _operands(seed):
    """Per tensor: buf, g, m, v, v_hat (numpy fp32), the special buffer values in bodies and tails."""
    if ("ops", seed) in _memo:
        return _memo[("ops", seed)]
    rng = np.random.default_rng(seed)
    out = []
    for n in SIZES:
        buf = rng.standard_normal(n, dtype=np.float32) * F32(1e-2)
        g = rng.standard_normal(n, dtype=np.float32)
        m = rng.standard_normal(n, dtype=np.float32) * F32(1e-3)
        v = np.abs(rng.standard_normal(n, dtype=np.float32)) * F32(1e-5)
        h = v * (1 + rng.random(n, dtype=np.float32))
        for at in (40, 8186, n - 3):           # a body group, across the first chunk's end, the tensor's tail
            for j, x in enumerate(BUF_SPECIAL):
                if 0 <= at + j < n:
                    buf[at + j] = x
        if n == 3:
            buf[:] = BUF_SPECIAL[:3]
        out.append((buf, g, m, v, h))
    _memo[("ops", seed)] = out
    return out


def _place(arrays, lay):
    flat = np.zeros(lay.total, np.float32)
    for a, o in zip(arrays, lay.offsets.tolist()):
        flat[o:o + a.size] = a
    return torch.from_numpy(flat).to(DEV)


def _take(bucket, lay):
    host = bucket.cpu().numpy()
    return [host[o:o + n] for o, n in zip(lay.offsets.tolist(), lay.sizes.tolist())]


def _skewed(a):
    """A device copy of `a` viewed one element into its storage: 4-byte aligned only."""
    store = torch.zeros(a.size + 1, device=DEV)
    store[1:].copy_(torch.from_numpy(a))
    assert store[1:].data_ptr() % 16 == 4
    return store[1:]


def _sides(data, lay, kind, with_buf):
    """([buf or None, g, m, v, v_hat, out] for the launch, read-back function)."""
    cols = list(zip(*data))
    if kind != "pointers":
        sides = [_place(c, lay) for c in cols] + [torch.full((lay.total,), 7.0, device=DEV)]
        read = lambda s: _take(s, lay)   # noqa: E731
    else:
        sides = [[torch.from_numpy(a.copy()).to(DEV) for a in c] for c in cols]
        sides.append([torch.full((n,), 7.0, device=DEV) for n in SIZES])
        for name, col in (("buf", 0), ("g", 1), ("m", 2), ("out", 5)):
            t = SIZES.index(MISALIGNED[name])
            sides[col][t] = _skewed(np.full(SIZES[t], 7.0, np.float32) if name == "out" else cols[col][t])
        read = lambda s: [x.cpu().numpy() for x in s]   # noqa: E731
    if not with_buf:
        sides[0] = None
    return sides, read


def _accumulated(pl, data, with_buf, factor):
    """The restatement's full buffer per tensor: B = fp32(buf + fp32(factor * d)), or fp32(factor * d)."""
    out = []
    with np.errstate(all="ignore"):
        for d, (buf, *_rest) in zip(pl.dec, data):
            u = (F32(factor) * d).astype(np.float32)
            out.append((buf + u).astype(np.float32) if with_buf else u)
    return out


def _two_call_buffer(pl, data, with_buf, factor):
    """Today's first call on aligned copies: the updated buffer as T device tensors."""
    if with_buf:
        bufs = [torch.from_numpy(b.copy()).to(DEV) for b, *_ in data]
        pl.axpby([bufs], [bufs], 1.0, factor)
    else:
        bufs = [torch.full((n,), 7.0, device=DEV) for n in SIZES]
        pl.axpby(None, [bufs], 1.0, factor)
    return bufs


def _assert_same(got, want, what):
    ok = fc.same_bits(got, want)
    assert ok.all(), (what, int((~ok).sum()), np.nonzero(~ok)[0][:8], np.asarray(got)[~ok][:4],
                      np.asarray(want)[~ok][:4])


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("kind", LAYOUTS)
@pytest.mark.parametrize("codec", CODECS)
def test_fedbuff_receive_flush_bit_for_bit(codec, kind, K):
    pl, data, with_buf = _payload(codec, kind), _operands(51), K > 1
    sides, read = _sides(data, pl.lay, kind, with_buf)
    buf, g, out = sides[0], sides[1], sides[5]
    pl.fedbuff(buf, g, out, K, FACTOR, LR)
    # today's two calls, on aligned copies
    full = _two_call_buffer(pl, data, with_buf, FACTOR)
    out2 = [torch.full((n,), 7.0, device=DEV) for n in SIZES]
    flush.fedbuff_flush_batched(full, [torch.from_numpy(x[1].copy()).to(DEV) for x in data], out2, ops.BucketLayout(SIZES),
                                K, LR)
    torch.cuda.synchronize()
    B = _accumulated(pl, data, with_buf, FACTOR)
    got = read(out)
    for t, n in enumerate(SIZES):
        tag = (codec, kind, K, n)
        _assert_same(got[t], fc.fedbuff_flush(B[t], data[t][1], K, LR), ("restatement",) + tag)
        _assert_same(got[t], out2[t].cpu().numpy(), ("two calls",) + tag)
    if with_buf:                                    # the buffer is read, never written; g likewise
        for t, b_now in enumerate(read(buf)):
            _assert_same(b_now, data[t][0], ("buf written", codec, kind, SIZES[t]))
    for t, g_now in enumerate(read(g)):
        _assert_same(g_now, data[t][1], ("g written", codec, kind, SIZES[t]))
    if kind != "pointers":                          # pads between tensors are never written
        own = np.zeros(pl.lay.total, bool)
        for o, n in zip(pl.lay.offsets.tolist(), SIZES):
            own[o:o + n] = True
        assert (out.cpu().numpy()[~own] == 7.0).all()
    # the placed values do what they are there for
    t = SIZES.index(8192)
    if with_buf:
        assert np.isnan(B[t][40 + 3]) and np.isinf(B[t][40 + 1])
    zero = SIZES.index(64)                          # scale / norm 0
    if codec in ("qsgd", "rqsgd", "cnat"):
        assert not pl.dec[zero].any() and not np.signbit(pl.dec[zero]).any()        # +0 where the norm is 0
    else:
        assert not pl.dec[zero].any() and np.signbit(pl.dec[zero]).any()            # fp32(0 * q) keeps q's sign


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("kind", LAYOUTS)
@pytest.mark.parametrize("codec", CODECS)
def test_fadas_receive_flush_bit_for_bit(codec, kind, K):
    pl, data, with_buf = _payload(codec, kind), _operands(52), K > 1
    rnd = 1 if K == 3 else 1000
    sc = fc.fadas_scalars(fc.BETA_1, fc.BETA_2, fc.EPS, LR, rnd)
    sides, read = _sides(data, pl.lay, kind, with_buf)
    pl.fadas(*sides, K, sc)
    full = _two_call_buffer(pl, data, with_buf, 1.0)
    two = [[torch.from_numpy(x[c].copy()).to(DEV) for x in data] for c in (1, 2, 3, 4)]
    two.append([torch.full((n,), 7.0, device=DEV) for n in SIZES])
    flush.fadas_flush_batched(full, *two, ops.BucketLayout(SIZES), K, sc)
    torch.cuda.synchronize()
    B = _accumulated(pl, data, with_buf, 1.0)
    got = {k: read(sides[i]) for k, i in (("m", 2), ("v", 3), ("v_hat", 4), ("out", 5))}
    ref2 = {k: [x.cpu().numpy() for x in two[i]] for k, i in (("m", 1), ("v", 2), ("v_hat", 3), ("out", 4))}
    for t, (_, g, m, v, h) in enumerate(data):
        want = fc.fadas_flush(B[t], g, m, v, h, K, sc)
        for key in ("m", "v", "v_hat", "out"):
            tag = (codec, kind, K, SIZES[t], key)
            _assert_same(got[key][t], want[key], ("restatement",) + tag)
            _assert_same(got[key][t], ref2[key][t], ("two calls",) + tag)
    if with_buf:
        for t, b_now in enumerate(read(sides[0])):
            _assert_same(b_now, data[t][0], ("buf written", codec, kind, SIZES[t]))


# ---------------------------------------------------------------------------------------------------------
# the six custom ops over flat buckets
# ---------------------------------------------------------------------------------------------------------
def _flat(kind_codec):
    pl = _payload(kind_codec, "aligned")
    lay, data = pl.lay, _operands(53)
    cols = [_place(c, lay) for c in zip(*data)]
    return pl, lay, cols, torch.from_numpy(lay.offsets.copy()), torch.from_numpy(lay.sizes.copy())


def _op_args(codec, pl):
    if codec in ("slq8", "int4"):
        return (pl.planes[0].view(torch.int8) if codec == "slq8" else pl.planes[0], pl.planes[1]), ()
    return tuple(pl.planes), (codec, 8)


def _ops_of(codec):
    if codec == "slq8":
        return AP.slq_dequantize_fedbuff_flush_batched, AP.slq_dequantize_fadas_flush_batched
    if codec == "int4":
        return AP.slq_dequantize_fedbuff_flush_batched_int4, AP.slq_dequantize_fadas_flush_batched_int4
    return AP.stoch_dequantize_fedbuff_flush_batched, AP.stoch_dequantize_fadas_flush_batched


@pytest.mark.parametrize("codec", ["slq8", "int4", "rqsgd"])
def test_custom_ops_equal_the_ops_calls_and_pass_opcheck(codec):
    pl, lay, (buf, g, m, v, h), off, siz = _flat(codec)
    head, tail = _op_args(codec, pl)
    fed, fad = _ops_of(codec)
    own = np.zeros(lay.total, bool)
    for o, n in zip(lay.offsets.tolist(), SIZES):
        own[o:o + n] = True
    sc = fc.fadas_scalars(fc.BETA_1, fc.BETA_2, fc.EPS, LR, 3)
    for b in (buf, None):
        K = 3 if b is not None else 1
        got = fed(*head, b, g, off, siz, *tail, K, FACTOR, LR).cpu().numpy()
        want = torch.full((lay.total,), 7.0, device=DEV)
        pl.fedbuff(b, g, want, K, FACTOR, LR)
        _assert_same(got[own], want.cpu().numpy()[own], ("fedbuff op", codec, K))
        assert not got[~own].any()                                    # positions no tensor owns are zero
        mom = [x.clone() for x in (m, v, h)]
        mom2 = [x.clone() for x in (m, v, h)]
        got = fad(*head, b, g, *mom, off, siz, *tail, K, *sc).cpu().numpy()
        want = torch.full((lay.total,), 7.0, device=DEV)
        pl.fadas(b, g, *mom2, want, K, sc)
        _assert_same(got[own], want.cpu().numpy()[own], ("fadas op", codec, K))
        assert not got[~own].any()
        for a, c, before in zip(mom, mom2, (m, v, h)):
            assert torch.equal(a.view(torch.int32), c.view(torch.int32))          # mutated in place, identically
            assert not torch.equal(a.view(torch.int32), before.view(torch.int32))
    # opcheck compares an eager run with a traced one by value, so it gets a payload and operands without NaN
    x = torch.randn(lay.total, device=DEV) * 1e-2
    if codec == "slq8":
        head = ops.encode_batched(x, lay, 8)
    elif codec == "int4":
        head = ops.encode_batched_int4(x, lay, 4)
    else:
        head = stoch.rqsgd_encode_batched(x, lay, 8, seed=5, counter=0)
    buf = torch.randn(lay.total, device=DEV) * 1e-2
    torch.library.opcheck(fed, (*head, buf, g, off, siz, *tail, 3, FACTOR, LR))
    torch.library.opcheck(fed, (*head, None, g, off, siz, *tail, 1, FACTOR, LR))
    torch.library.opcheck(fad, (*head, buf, g, m.clone(), v.clone(), h.clone(), off, siz, *tail, 3, *sc))


def test_functional_op_under_torch_compile():
    """One server step — encode a client's update, then FedBuff's K-th update through the fused op — traced by
    torch.compile (fullgraph: the fake implementations at trace time, the HIP kernels at run time) equals eager."""
    sizes = [4096, 80, 8192]
    off, siz = torch.tensor([0, 4096, 4224]), torch.tensor(sizes)
    x = torch.randn(4224 + 8192, device=DEV) * 1e-2
    buf, g = torch.randn_like(x) * 1e-2, torch.randn_like(x)

    def step(x, buf, g):
        q, s = torch.ops.adfl.slq_encode_batched(x, off, siz, 8)
        return torch.ops.adfl_apply.slq_dequantize_fedbuff_flush_batched(q, s, buf, g, off, siz, 3, FACTOR, LR)

    eager = step(x, buf, g)
    compiled = torch.compile(step, backend="aot_eager", fullgraph=True)(x, buf, g)
    assert torch.equal(eager.view(torch.int32), compiled.view(torch.int32))
    q, s = torch.ops.adfl.slq_encode_batched(x, off, siz, 8)
    d = torch.ops.adfl.slq_decode_batched(q, s, off, siz)
    # the reference's statements (fed_buff.py:72-92) by CPU torch on the decode
    d, b, gg = d.cpu(), buf.cpu(), g.cpu()
    d.mul_(FACTOR)
    b.mul_(1).add_(d, alpha=1)
    b.div_(3)
    want = (1.0 * gg) + (LR * b)
    own = torch.zeros(x.numel(), dtype=torch.bool)
    for o, n in zip(off.tolist(), sizes):
        own[o:o + n] = True
    assert torch.equal(eager.cpu()[own].view(torch.int32), want[own].view(torch.int32))


def test_argument_checks_raise_before_launching():
    lay = ops.BucketLayout([8, 8])
    ok = torch.zeros(lay.total, device=DEV)
    q = torch.zeros(lay.total, dtype=torch.int8, device=DEV)
    s = torch.ones(2, device=DEV)
    sc = fc.fadas_scalars(fc.BETA_1, fc.BETA_2, fc.EPS, LR, 1)
    with pytest.raises(ValueError, match="max_buffer_size"):
        ops.dequantize_fedbuff_flush_batched(q, s, lay, ok, ok.clone(), ok.clone(), 0, 1.0, LR)
    with pytest.raises(ValueError, match="required"):
        ops.dequantize_fedbuff_flush_batched(q, s, lay, ok, None, ok.clone(), 3, 1.0, LR)
    with pytest.raises(ValueError, match="bucket"):
        ops.dequantize_fedbuff_flush_batched(q, s, lay, ok, ok[:8], ok.clone(), 3, 1.0, LR)
    with pytest.raises(ValueError, match="fp32"):
        ops.dequantize_fadas_flush_batched(q, s, lay, ok, ok.clone(), ok.double(), ok.clone(), ok.clone(), ok.clone(),
                                           3, sc)
    with pytest.raises(ValueError, match="payload"):
        ops.dequantize_fedbuff_flush_batched(q[:8], s, lay, ok, ok.clone(), ok.clone(), 3, 1.0, LR)
    with pytest.raises(ValueError, match="seven"):
        ops.dequantize_fadas_flush_batched(q, s, lay, None, ok, ok.clone(), ok.clone(), ok.clone(), ok.clone(), 1, sc[:6])
    with pytest.raises(ValueError):
        ops.dequantize_fedbuff_flush_batched(q, s, ops.BucketLayout([7, 8], align=1), None, ok, ok.clone(), 1, 1.0, LR,
                                             packed=True)                              # int4 needs even offsets
    with pytest.raises(ValueError, match="codec"):
        stoch.dequantize_fedbuff_flush_batched("slq", q.view(torch.uint8), q, s, lay, 8, ok, ok.clone(), ok.clone(), 3,
                                               1.0, LR)
    with pytest.raises(ValueError, match="mins"):
        stoch.dequantize_fedbuff_flush_batched("rqsgd", q.view(torch.uint8), q, s, lay, 8, ok, ok.clone(), ok.clone(),
                                               3, 1.0, LR)
    with pytest.raises(ValueError, match="bits"):
        stoch.dequantize_fadas_flush_batched("qsgd", q.view(torch.uint8), q, s, lay, 17, ok, ok.clone(), ok.clone(),
                                             ok.clone(), ok.clone(), ok.clone(), 3, sc)
