"""GPU: adfl_fedbuff_flush_batched / adfl_fadas_flush_batched (csrc/server_flush.hip) through adfl_amd.flush and
the two custom ops, against the numpy restatement (flush_cases.py) bit for bit on every element, the in-place m,
v and v_hat included. NaN positions must agree; a NaN's sign and payload are not compared (IEEE 754 leaves them to
the implementation, and x86, gfx950 and torch's own vector and scalar paths differ).

Tensor lengths 1, 3, 4, 5, 8191, 8192, 8193 and 16,387 in one bucket: below a float4, the tails of 1-3 elements,
one chunk exactly, one element over, more than two chunks. Layouts: 64-aligned (16-byte path), compact align=1
(element path, tensors at odd offsets), and pointer tables to separate tensors with one source a view one element
into its storage (that tensor alone goes element by element). Special values sit in bodies and in tails.
"""

import numpy as np
import pytest
import torch

import flush_cases as fc

pytestmark = pytest.mark.gpu

import adfl_amd  # noqa: E402,F401
from adfl_amd import flush, ops  # noqa: E402

DEV = torch.device("cuda", 0)
AP = torch.ops.adfl_apply
SIZES = [1, 3, 4, 5, 8191, 8192, 8193, 16387]
LR = 0.05


# (buf, m, v, v_hat)
SPECIAL = [
    (0.0, 0.0, 0.0, 0.0),            # v_hat' = 0 with m' = 0: den = eps, out = g + 0 / eps
    (0.0, 0.5, 0.0, 0.0),            # v_hat' = 0 with m' != 0: a large step over den = eps
    (np.nan, 0.1, 1e-6, 1e-6),       # NaN in buf
    (1e-2, 0.1, 1e-6, np.nan),       # NaN in v_hat with a finite v
    (np.inf, 0.1, 1e-6, 1e-6),       # inf in buf: inf / inf in the step
    (-0.0, -0.0, 0.0, 0.0),          # -0.0
    (1e-41, 1e-42, 1e-44, 1e-43),    # denormals in every stream
    (-1e-39, 3e-40, 0.0, 2e-45),     # the square root of a denormal
]
BODY = 40        # a 16-byte group boundary: SPECIAL sits at [40, 48) of every tensor that long


def _data(seed):
    """Per tensor: buf, g, m, v, v_hat (numpy, fp32) with the special values placed in bodies and tails."""
    rng = np.random.default_rng(seed)
    out = []
    for n in SIZES:
        buf = rng.standard_normal(n, dtype=np.float32) * np.float32(1e-2)
        g = rng.standard_normal(n, dtype=np.float32)
        m = rng.standard_normal(n, dtype=np.float32) * np.float32(1e-3)
        v = np.abs(rng.standard_normal(n, dtype=np.float32)) * np.float32(1e-5)
        h = v * (1 + rng.random(n, dtype=np.float32))

        def put(at, rows):
            for j, row in enumerate(rows):
                if 0 <= at + j < n:
                    buf[at + j], m[at + j], v[at + j], h[at + j] = row

        if n >= 8191:
            put(BODY, SPECIAL)
            put(8184, SPECIAL)                                   # the end of the first chunk, and past it
            put(n - 3, [SPECIAL[1], SPECIAL[2], SPECIAL[6]])     # the tensor's last elements (a chunk's tail)
        elif n == 5:
            put(4, [SPECIAL[2]])                                 # the one-element tail after one group
        elif n == 3:
            put(0, [SPECIAL[0], SPECIAL[5], SPECIAL[6]])         # tail only
        out.append((buf, g, m, v, h))
    return out


def _place(arrays, lay, shift=0):
    """One flat device bucket in `lay` (zeros between tensors)."""
    flat = np.zeros(lay.total + shift, np.float32)
    for a, o in zip(arrays, lay.offsets.tolist()):
        flat[shift + o:shift + o + a.size] = a
    return torch.from_numpy(flat).to(DEV)


def _take(bucket, lay):
    host = bucket.cpu().numpy()
    return [host[o:o + n] for o, n in zip(lay.offsets.tolist(), lay.sizes.tolist())]


def _assert_same(got, want, what):
    ok = fc.same_bits(got, want)
    assert ok.all(), (what, int((~ok).sum()), np.nonzero(~ok)[0][:8], got[~ok][:4], want[~ok][:4])


def _sides(data, layout_kind):
    """(layout, [buf, g, m, v, v_hat, out] sides for the launch, read-back function)."""
    cols = list(zip(*data))
    if layout_kind in ("aligned", "compact"):
        lay = ops.BucketLayout(SIZES, align=64 if layout_kind == "aligned" else 1)
        sides = [_place(c, lay) for c in cols] + [torch.full((lay.total,), 7.0, device=DEV)]
        return lay, sides, lambda s: _take(s, lay)
    lay = ops.BucketLayout(SIZES)
    sides = [[torch.from_numpy(a.copy()).to(DEV) for a in c] for c in cols]
    sides.append([torch.full((n,), 7.0, device=DEV) for n in SIZES])
    # one source a view one element into its storage: 4-byte aligned only
    t = SIZES.index(8193)
    store = torch.zeros(SIZES[t] + 1, device=DEV)
    store[1:].copy_(sides[0][t])
    sides[0][t] = store[1:]
    assert sides[0][t].data_ptr() % 16 == 4
    return lay, sides, lambda s: [x.cpu().numpy() for x in s]


LAYOUTS = ["aligned", "compact", "pointers"]


@pytest.mark.parametrize("K", [1, 3, 10])
@pytest.mark.parametrize("layout_kind", LAYOUTS)
def test_fedbuff_flush_bit_for_bit(layout_kind, K):
    data = _data(11)
    lay, sides, read = _sides(data, layout_kind)
    buf, g, out = sides[0], sides[1], sides[5]
    flush.fedbuff_flush_batched(buf, g, out, lay, K, LR)
    torch.cuda.synchronize()
    for t, (got, (b, gg, *_)) in enumerate(zip(read(out), data)):
        _assert_same(got, fc.fedbuff_flush(b, gg, K, LR), (layout_kind, K, SIZES[t]))
    for t, (b_now, g_now) in enumerate(zip(read(buf), read(g))):   # inputs untouched (no averaged write-back)
        _assert_same(b_now, data[t][0], "buf")
        _assert_same(g_now, data[t][1], "g")
    if layout_kind != "pointers":   # pads between tensors are never written
        own = np.zeros(lay.total, bool)
        for o, n in zip(lay.offsets.tolist(), lay.sizes.tolist()):
            own[o:o + n] = True
        assert (out.cpu().numpy()[~own] == 7.0).all()


@pytest.mark.parametrize("rnd", [1, 1000])
@pytest.mark.parametrize("K", [1, 3, 10])
@pytest.mark.parametrize("layout_kind", LAYOUTS)
def test_fadas_flush_bit_for_bit(layout_kind, K, rnd):
    data = _data(12)
    lay, sides, read = _sides(data, layout_kind)
    sc = fc.fadas_scalars(fc.BETA_1, fc.BETA_2, fc.EPS, LR, rnd)
    assert tuple(sc) == tuple(flush.fadas_scalars(fc.BETA_1, fc.BETA_2, fc.EPS, LR, rnd))
    flush.fadas_flush_batched(*sides, lay, K, sc)
    torch.cuda.synchronize()
    got = {k: read(sides[i]) for k, i in (("m", 2), ("v", 3), ("v_hat", 4), ("out", 5))}
    for t, (b, g, m, v, h) in enumerate(data):
        want = fc.fadas_flush(b, g, m, v, h, K, sc)
        for key in ("m", "v", "v_hat", "out"):
            _assert_same(got[key][t], want[key], (layout_kind, K, rnd, SIZES[t], key))
    # the placed values do what they are there for
    t, B = SIZES.index(8191), BODY
    want = fc.fadas_flush(*data[t], K, sc)
    assert want["den"][B] == np.float32(fc.EPS) and want["out"][B] == data[t][1][B]           # 0 / eps
    assert want["den"][B + 1] == np.float32(fc.EPS) and want["out"][B + 1] != data[t][1][B + 1]
    assert np.isnan(want["out"][[B + 2, B + 3, B + 4]]).all()
    assert np.isnan(want["v_hat"][B + 3]) and not np.isnan(want["v"][B + 3])
    assert np.signbit(want["m"][B + 5]) and want["m"][B + 5] == 0                             # -0.0 kept
    assert 0 < abs(want["m"][B + 6]) < 1.2e-38 and 0 < want["den"][B + 7]                     # denormals kept


def test_fadas_two_rounds_feed_in_place_moments():
    """Two flushes over the same moment buckets: the second call reads what the first wrote."""
    data = _data(13)
    lay = ops.BucketLayout(SIZES)
    cols = list(zip(*data))
    m, v, h = (_place(c, lay) for c in cols[2:])
    ref = [(mm, vv, hh) for _, _, mm, vv, hh in data]
    for rnd in (1, 2):
        rng = np.random.default_rng(100 + rnd)
        bufs = [rng.standard_normal(n, dtype=np.float32) * np.float32(1e-2) for n in SIZES]
        gs = [rng.standard_normal(n, dtype=np.float32) for n in SIZES]
        sc = fc.fadas_scalars(fc.BETA_1, fc.BETA_2, fc.EPS, LR, rnd)
        out = torch.empty(lay.total, device=DEV)
        flush.fadas_flush_batched(_place(bufs, lay), _place(gs, lay), m, v, h, out, lay, 3, sc)
        torch.cuda.synchronize()
        want = [fc.fadas_flush(b, g, *mom, 3, sc) for b, g, mom in zip(bufs, gs, ref)]
        ref = [(w["m"], w["v"], w["v_hat"]) for w in want]
        for key, bucket in (("m", m), ("v", v), ("v_hat", h), ("out", out)):
            for t, got in enumerate(_take(bucket, lay)):
                _assert_same(got, want[t][key], (rnd, key, SIZES[t]))


def _flat_case(seed, gap):
    """A caller-placed layout for the custom ops: tensors `gap` elements apart, not in offset order."""
    sizes = [4097, 3, 900, 8192]
    offsets, pos = [], 0
    for n in sizes:
        offsets.append(pos)
        pos += n + gap
    order = [2, 0, 3, 1]
    sizes, offsets = [sizes[i] for i in order], [offsets[i] for i in order]
    rng = np.random.default_rng(seed)
    cols = [rng.standard_normal(pos, dtype=np.float32) * np.float32(s) for s in (1e-2, 1.0, 1e-3)]
    v = np.abs(rng.standard_normal(pos, dtype=np.float32)) * np.float32(1e-5)
    cols += [v, v * np.float32(1.5)]
    own = np.zeros(pos, bool)
    for o, n in zip(offsets, sizes):
        own[o:o + n] = True
    return cols, torch.tensor(offsets), torch.tensor(sizes), own


@pytest.mark.parametrize("gap", [0, 5])
def test_custom_ops_equal_the_restatement(gap):
    (buf, g, m, v, h), off, siz, own = _flat_case(21, gap)
    d = [torch.from_numpy(a.copy()).to(DEV) for a in (buf, g, m, v, h)]
    got = AP.fedbuff_flush_batched(d[0], d[1], off, siz, 3, LR).cpu().numpy()
    _assert_same(got[own], fc.fedbuff_flush(buf, g, 3, LR)[own], "fedbuff op")
    assert not got[~own].any()                                    # positions no tensor owns are zero
    sc = fc.fadas_scalars(fc.BETA_1, fc.BETA_2, fc.EPS, LR / 25, 7)
    out = AP.fadas_flush_batched(*d, off, siz, 3, *sc).cpu().numpy()
    want = fc.fadas_flush(buf, g, m, v, h, 3, sc)
    _assert_same(out[own], want["out"][own], "fadas op")
    assert not out[~own].any()
    for key, t, before in (("m", d[2], m), ("v", d[3], v), ("v_hat", d[4], h)):
        now = t.cpu().numpy()
        _assert_same(now[own], want[key][own], key)               # mutated in place ...
        _assert_same(now[~own], before[~own], key)                # ... and only where a tensor lives


def test_custom_ops_opcheck():
    (buf, g, m, v, h), off, siz, _ = _flat_case(22, 3)
    d = [torch.from_numpy(a.copy()).to(DEV) for a in (buf, g, m, v, h)]
    sc = fc.fadas_scalars(fc.BETA_1, fc.BETA_2, fc.EPS, LR, 2)
    torch.library.opcheck(AP.fedbuff_flush_batched, (d[0], d[1], off, siz, 3, LR))
    torch.library.opcheck(AP.fadas_flush_batched, (*d, off, siz, 3, *sc))


def test_argument_checks_raise_before_launching():
    lay = ops.BucketLayout([8, 8])
    ok = torch.zeros(lay.total, device=DEV)
    with pytest.raises(ValueError, match="max_buffer_size"):
        flush.fedbuff_flush_batched(ok, ok.clone(), ok.clone(), lay, 0, LR)
    with pytest.raises(ValueError, match="bucket"):
        flush.fedbuff_flush_batched(ok, ok[:8], ok.clone(), lay, 3, LR)          # too small for the layout
    with pytest.raises(ValueError, match="fp32"):
        flush.fedbuff_flush_batched(ok, ok.double(), ok.clone(), lay, 3, LR)
    with pytest.raises(ValueError, match="tensors"):
        flush.fedbuff_flush_batched([ok[:8]], [ok[:8]], [ok[:8]], lay, 3, LR)    # one tensor for a layout of two
