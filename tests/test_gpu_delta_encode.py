"""GPU: the delta encode (adfl_amd.ops.encode_delta_batched / _int4 and torch.ops.adfl.slq_encode_delta_batched
/ _int4) against the oracle on numpy's fp32 ``new - prev`` and against ops.encode_batched / _int4 of the
device-computed difference. Every comparison is exact (NaN positions, not NaN payload bits).

Reference: diff_parameters (Src/ADFL/model.py:350-358) then the per-tensor encode (Src/ADFL/Channel/quant.py:
74-104; Src/ADFL/compression.py:35-48 for the packed payload). Shapes: tests/golden/delta_cases.py."""

import functools

import numpy as np
import pytest
import torch

import delta_cases
import slq_oracle as oracle
from golden_util import same_f32

pytestmark = pytest.mark.gpu

DEV = "cuda"
A = torch.ops.adfl
R = delta_cases.R
SENTINEL = 0x5A

# how the two sources reach the kernels, and the payload layout's alignment (int8, int4)
FORMS = {
    "separate": (64, 64),      # separately allocated tensors, 64-aligned payload: the 16-byte path
    "flat": (1, 2),            # two flat compact buckets, compact payload: the 16-byte path past each head
    "offset1": (64, 64),       # views starting 1 element into their storage: the element-wise path
    "prev_offset1": (64, 64),  # `new` aligned, `prev` not: element-wise, and the absmax pass's too
}
VALUES = ["noise", "equal", "nan_head", "nan_body", "nan_tail", "inf_inf", "inf_fin", "denormal", "negzero"]


@functools.lru_cache(maxsize=None)
def _pair(sizes, kind):
    """One (new, prev) pair of fp32 arrays per tensor; computed once per (sizes, kind), shared, never modified."""
    news, prevs = [], []
    for t, n in enumerate(sizes):
        rng = np.random.default_rng(1000 * t + n)
        b = rng.standard_normal(n, dtype=np.float32)
        a = (b + np.float32(1e-3) * rng.standard_normal(n, dtype=np.float32)).astype(np.float32)
        pos = {"nan_head": 0, "nan_body": n // 2, "nan_tail": n - 1}.get(kind, (n * 2) // 3)
        if kind == "equal":
            a = b.copy()
        elif kind.startswith("nan"):
            b[pos] = np.nan                       # in `new` only
        elif kind == "inf_inf":
            a[pos] = b[pos] = np.inf              # +inf - +inf = NaN
        elif kind == "inf_fin":
            b[pos] = np.inf
        elif kind == "denormal":                  # a cancellation that leaves a denormal maximum
            a = np.full(n, 2.0 ** -126, dtype=np.float32)
            k = rng.integers(-(1 << 20), 1 << 20, size=n)
            b = (a.view(np.uint32).astype(np.int64) + k).astype(np.uint32).view(np.float32)
        elif kind == "negzero":
            a[::3] = 0.0
            b[::3] = -0.0                         # -0.0 - 0.0 = -0.0
            a[1::3] = b[1::3]                     # +0.0
        news.append(b)
        prevs.append(a)
    return tuple(news), tuple(prevs)


@functools.lru_cache(maxsize=None)
def _expected(sizes, kind, bits):
    """The oracle on numpy's fp32 difference: per tensor (int8 payload, packed payload, scale)."""
    news, prevs = _pair(sizes, kind)
    out = []
    with np.errstate(all="ignore"):
        for b, a in zip(news, prevs):
            x = b - a
            assert x.dtype == np.float32
            q, s = oracle.encode(x, bits)
            out.append((q, oracle.pack_int4(q) if bits <= 4 else None, s))
    return out


def _layout(sizes, form, int4):
    from adfl_amd import ops
    return ops.BucketLayout(list(sizes), align=FORMS[form][1 if int4 else 0])


def _offset1(arrs):
    out = []
    for a in arrs:
        store = torch.empty(a.size + 1, dtype=torch.float32, device=DEV)
        v = store[1:]
        v.copy_(torch.from_numpy(a))
        assert v.data_ptr() % 16 == 4
        out.append(v)
    return out


def _flat(arrs, lay):
    flat = torch.zeros(lay.total, dtype=torch.float32, device=DEV)
    for a, o in zip(arrs, lay.offsets.tolist()):
        flat[o:o + a.size].copy_(torch.from_numpy(a))
    return flat


def _sources(sizes, kind, form, lay):
    news, prevs = _pair(sizes, kind)
    sep = lambda arrs: [torch.from_numpy(a).to(DEV) for a in arrs]   # noqa: E731
    if form == "separate":
        return sep(news), sep(prevs)
    if form == "flat":
        return _flat(news, lay), _flat(prevs, lay)
    if form == "offset1":
        return _offset1(news), _offset1(prevs)
    return sep(news), _offset1(prevs)


def _check(sizes, kind, form, bits, int4):
    """Encode through adfl_amd.ops into caller-supplied, sentinel-filled outputs; compare with the oracle and
    with the two-step route on the device; check in-place filling and untouched pads."""
    from adfl_amd import ops
    lay = _layout(sizes, form, int4)
    new, prev = _sources(sizes, kind, form, lay)
    nbytes = (lay.total + 1) // 2 if int4 else lay.total
    out = torch.full((nbytes,), SENTINEL, dtype=torch.uint8 if int4 else torch.int8, device=DEV)
    scales = torch.full((lay.ntensors,), -1.0, dtype=torch.float32, device=DEV)
    partials = torch.full((lay.nchunks,), -1, dtype=torch.int32, device=DEV)
    if int4:
        got, gs = ops.encode_delta_batched_int4(new, prev, lay, bits, packed=out, scales=scales, partials=partials)
    else:
        got, gs = ops.encode_delta_batched(new, prev, lay, bits, q=out, scales=scales, partials=partials)
    assert got.data_ptr() == out.data_ptr() and gs.data_ptr() == scales.data_ptr()   # filled in place
    news, prevs = _pair(sizes, kind)
    # the two-step route: the device's own new - prev in a bucket, then the existing bucketed encode
    diff = _flat(news, lay) - _flat(prevs, lay)
    if int4:
        two, ts = ops.encode_batched_int4(diff, lay, bits)
    else:
        two, ts = ops.encode_batched(diff, lay, bits)
    got_h, two_h = got.cpu().numpy().view(np.uint8), two.cpu().numpy().view(np.uint8)
    gs_h, ts_h = gs.cpu().numpy(), ts.cpu().numpy()
    owned = np.zeros(nbytes, dtype=bool)
    for t, ((q, packed, s), o, n) in enumerate(zip(_expected(sizes, kind, bits), lay.offsets.tolist(), sizes)):
        lo, hi = (o // 2, o // 2 + (n + 1) // 2) if int4 else (o, o + n)
        want = packed if int4 else q.view(np.uint8)
        where = (kind, form, bits, t, n)
        assert np.array_equal(got_h[lo:hi], want), where
        assert np.array_equal(got_h[lo:hi], two_h[lo:hi]), where
        assert same_f32(gs_h[t], s) and same_f32(gs_h[t], ts_h[t]), where
        if int4 and n % 2:
            assert got_h[hi - 1] & 0xF == 8, where        # an odd tensor's pad is a zero code
        owned[lo:hi] = True
    assert (got_h[~owned] == SENTINEL).all(), (kind, form, bits)   # an aligned bucket's pads are untouched
    # the two passes fill the caller's partials (magnitude bits: never -1); the resident form leaves them
    two_pass = lay.max_tensor_chunks > delta_cases.DELTA_RESIDENT_CHUNKS
    assert bool((partials.cpu().numpy() != -1).all()) == two_pass
    assert bool((partials.cpu().numpy() == -1).all()) == (not two_pass)
    return lay


@pytest.mark.parametrize("int4", [False, True], ids=["int8", "int4"])
@pytest.mark.parametrize("n", delta_cases.ALL_SIZES)
def test_one_tensor_buckets(n, int4):
    for form in FORMS:
        lay = _check((n,), "noise", form, 4 if int4 else 8, int4)
        assert (lay.nwork == 1) == (n <= R)     # R + 1 takes the two passes


@pytest.mark.parametrize("int4", [False, True], ids=["int8", "int4"])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("sizes", [tuple(delta_cases.RESIDENT_SIZES), tuple(delta_cases.ALL_SIZES)],
                         ids=["resident", "twopass"])
def test_buckets_every_bit_width(sizes, form, int4):
    for bits in ((4, 2) if int4 else (8, 4, 2)):
        lay = _check(sizes, "noise", form, bits, int4)
    assert (lay.nwork > 0) == (max(sizes) <= R)


@pytest.mark.parametrize("int4", [False, True], ids=["int8", "int4"])
@pytest.mark.parametrize("kind", VALUES[1:])
@pytest.mark.parametrize("sizes", [tuple(delta_cases.RESIDENT_SIZES), tuple(delta_cases.ALL_SIZES)],
                         ids=["resident", "twopass"])
def test_special_values(sizes, kind, int4):
    for form in ("separate", "offset1"):    # the 16-byte path and the element-wise path
        _check(sizes, kind, form, 4 if int4 else 8, int4)


def test_equal_inputs_give_scale_zero_and_payload_127():
    from adfl_amd import ops
    sizes = tuple(delta_cases.ALL_SIZES)
    lay = _layout(sizes, "separate", False)
    new, prev = _sources(sizes, "equal", "separate", lay)
    q, s = ops.encode_delta_batched(new, prev, lay, 8)
    assert (s.cpu().numpy() == 0).all()
    qh = q.cpu().numpy()
    for o, n in zip(lay.offsets.tolist(), sizes):
        assert (qh[o:o + n] == 127).all()      # 0 * inf = NaN -> 127, as the oracle gives
        assert (oracle.encode(np.zeros(n, np.float32), 8)[0] == 127).all()


def test_inputs_are_not_modified_and_bad_arguments_raise():
    from adfl_amd import _lib, ops
    sizes = (1025, 33)
    lay = _layout(sizes, "separate", False)
    new, prev = _sources(sizes, "noise", "separate", lay)
    keep = [t.clone() for t in new + prev]
    ops.encode_delta_batched(new, prev, lay, 8)
    ops.encode_delta_batched_int4(new, prev, lay, 4)
    for t, k in zip(new + prev, keep):
        assert torch.equal(t.view(torch.int32), k.view(torch.int32))
    with pytest.raises(ValueError, match="tensors for a layout"):
        ops.encode_delta_batched(new[:1], prev, lay, 8)
    with pytest.raises(ValueError, match="elements"):
        ops.encode_delta_batched(new, [prev[0], prev[1][:-1]], lay, 8)
    with pytest.raises(ValueError, match="device tensor"):
        ops.encode_delta_batched(new, [p.cpu() for p in prev], lay, 8)
    with pytest.raises(RuntimeError, match="Quantize only works on Float Tensor, got Double"):
        ops.encode_delta_batched(new, [p.double() for p in prev], lay, 8)
    with pytest.raises(ValueError, match="smaller than the layout"):
        ops.encode_delta_batched(torch.zeros(10, device=DEV), torch.zeros(lay.total, device=DEV), lay, 8)
    with pytest.raises(ValueError, match="even"):
        ops.encode_delta_batched_int4(new, prev, ops.BucketLayout(list(sizes), align=1), 4)
    for bits in (0, 9):
        with pytest.raises(_lib.AdflError, match="invalid argument"):
            ops.encode_delta_batched(new, prev, lay, bits)
    with pytest.raises(_lib.AdflError, match="invalid argument"):
        ops.encode_delta_batched_int4(new, prev, lay, 5)


def _op_inputs(gap):
    """Two flat buffers with caller-placed tensors (one gap of `gap` elements, out of order)."""
    sizes = [902, 4098, 33]   # even offsets: the int4 op takes the same layout
    offs = [4098 + gap, 0, 4098 + gap + 902]
    off, siz = torch.tensor(offs), torch.tensor(sizes)
    total = offs[2] + sizes[2]
    rng = np.random.default_rng(77)
    new = rng.standard_normal(total, dtype=np.float32)
    prev = (new + np.float32(1e-3) * rng.standard_normal(total, dtype=np.float32)).astype(np.float32)
    return new, prev, off, siz


@pytest.mark.parametrize("gap", [0, 2])
def test_custom_ops_match_the_oracle(gap):
    new, prev, off, siz = _op_inputs(gap)
    n_d, p_d = torch.from_numpy(new).to(DEV), torch.from_numpy(prev).to(DEV)
    q, s = A.slq_encode_delta_batched(n_d, p_d, off, siz, 8)
    p4, s4 = A.slq_encode_delta_batched_int4(n_d, p_d, off, siz, 4)
    assert q.shape == (new.size,) and q.dtype == torch.int8 and s.shape == (3,)
    assert p4.shape == ((new.size + 1) // 2,) and p4.dtype == torch.uint8
    qh, ph = q.cpu().numpy(), p4.cpu().numpy()
    want_q, want_p = np.zeros_like(qh), np.zeros_like(ph)   # positions no tensor owns are zero
    for t, (o, n) in enumerate(zip(off.tolist(), siz.tolist())):
        x = new[o:o + n] - prev[o:o + n]
        wq, ws = oracle.encode(x, 8)
        want_q[o:o + n] = wq
        assert same_f32(s[t].item(), ws)
        w4, ws4 = oracle.encode(x, 4)
        want_p[o // 2:o // 2 + (n + 1) // 2] = oracle.pack_int4(w4)
        assert same_f32(s4[t].item(), ws4)
    assert np.array_equal(qh, want_q) and np.array_equal(ph, want_p)
    # the two-step ops on the device's own difference
    q2, s2 = A.slq_encode_batched(n_d - p_d, off, siz, 8)
    assert torch.equal(q, q2) and torch.equal(s.view(torch.int32), s2.view(torch.int32))


def test_opcheck_and_compile():
    new, prev, off, siz = _op_inputs(2)
    n_d, p_d = torch.from_numpy(new).to(DEV), torch.from_numpy(prev).to(DEV)
    torch.library.opcheck(A.slq_encode_delta_batched, (n_d, p_d, off, siz, 8))
    torch.library.opcheck(A.slq_encode_delta_batched_int4, (n_d, p_d, off, siz, 4))

    def pipeline(n, p):
        q, s = torch.ops.adfl.slq_encode_delta_batched(n, p, off, siz, 8)
        return torch.ops.adfl.slq_decode_batched(q, s, off, siz)

    eager = pipeline(n_d, p_d)
    compiled = torch.compile(pipeline, backend="aot_eager", fullgraph=True)(n_d, p_d)
    assert torch.equal(eager.view(torch.int32), compiled.view(torch.int32))
    want = np.zeros(new.size, np.float32)
    for o, n in zip(off.tolist(), siz.tolist()):
        q, s = oracle.encode(new[o:o + n] - prev[o:o + n], 8)
        want[o:o + n] = oracle.decode(q, s)
    assert same_f32(eager.cpu().numpy(), want)
