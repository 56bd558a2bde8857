"""GPU: the broadcast kernels (adfl_amd.ops.encode_delta_update_batched / _int4 and
torch.ops.adfl_apply.slq_encode_delta_update_batched / _int4) against the two calls they fuse, on copies of the
inputs: the payload and scales of ops.encode_delta_batched / _int4, and the hidden state that
ops.dequantize_add_batched (int4: ops.decode_batched_int4, then torch's add) leaves. Every comparison is bit for
bit and nothing is excluded (NaN positions are compared, NaN payload bits are not).

Reference: Src/ADFL/Server/qafel.py:156-180. Shapes: tests/golden/delta_cases.py."""

import functools

import numpy as np
import pytest
import torch

import delta_cases
from golden_util import same_f32

pytestmark = pytest.mark.gpu

DEV = "cuda"
AP = torch.ops.adfl_apply
R = delta_cases.R
SENTINEL = 0x5A
F_SENTINEL = np.float32(-12345.5)

# how g and h reach the kernels, and the payload layout's alignment (int8, int4)
FORMS = {
    "aligned": (64, 64),         # two flat 64-aligned buckets: the 16-byte path; pads hold sentinels
    "compact": (1, 2),           # two flat compact buckets: the 16-byte path past each head
    "separate": (64, 64),        # separately allocated tensors through pointer tables
    "offset1": (64, 64),         # views starting 1 element into their storage: the element-wise path
    "hidden_offset1": (64, 64),  # g aligned, h not: element-wise, and the absmax pass's too
}
SPECIALS = [f"{v}_{p}" for v in ("nan", "pinf", "ninf", "negzero", "denormal") for p in ("head", "body", "tail")]
VALUES = ["noise", "equal", "denormal_all"] + SPECIALS


@functools.lru_cache(maxsize=None)
def _pair(sizes, kind):
    """One (g, h) pair of fp32 arrays per tensor; computed once per (sizes, kind), shared, never modified."""
    gs, hs = [], []
    for t, n in enumerate(sizes):
        rng = np.random.default_rng(1000 * t + n)
        h = rng.standard_normal(n, dtype=np.float32)
        g = (h + np.float32(1e-3) * rng.standard_normal(n, dtype=np.float32)).astype(np.float32)
        what, _, where = kind.partition("_")
        pos = {"head": 0, "body": n // 2, "tail": n - 1}.get(where, 0)
        if kind == "equal":                       # the frozen layer; a -0.0 in h follows IEEE
            h[0] = -0.0
            g = h.copy()
        elif kind == "denormal_all":              # a cancellation that leaves a denormal maximum
            h = np.full(n, 2.0 ** -126, dtype=np.float32)
            k = rng.integers(-(1 << 20), 1 << 20, size=n)
            g = (h.view(np.uint32).astype(np.int64) + k).astype(np.uint32).view(np.float32)
        elif what == "nan":                       # in g for even tensors, in h for odd ones
            (g if t % 2 == 0 else h)[pos] = np.nan
        elif what in ("pinf", "ninf"):
            (g if t % 2 == 0 else h)[pos] = np.inf if what == "pinf" else -np.inf
        elif what == "negzero":
            h[pos] = -0.0
            g[pos] = -0.0
        elif what == "denormal":
            h[pos] = np.float32(1e-40)
            g[pos] = np.float32(-3e-40)
        gs.append(g)
        hs.append(h)
    return tuple(gs), tuple(hs)


def _dev(arrs):
    return [torch.from_numpy(a).to(DEV) for a in arrs]


@functools.lru_cache(maxsize=None)
def _reference(sizes, kind, bits, int4):
    """The unfused route on copies, once per case: per tensor (payload bytes, scale bits, h' array)."""
    from adfl_amd import ops
    lay = ops.BucketLayout(list(sizes), align=64)
    gs, hs = _pair(sizes, kind)
    g, h = _dev(gs), _dev(hs)
    if int4:
        p, s = ops.encode_delta_batched_int4(g, h, lay, bits)
        dec = ops.decode_batched_int4(p, s, lay)
        h2 = [ht + dec[o:o + n] for ht, o, n in zip(h, lay.offsets.tolist(), sizes)]   # one fp32 add
        payload = p.cpu().numpy()
        pay = [payload[o // 2:o // 2 + (n + 1) // 2] for o, n in zip(lay.offsets.tolist(), sizes)]
    else:
        q, s = ops.encode_delta_batched(g, h, lay, bits)
        ops.dequantize_add_batched(q, s, lay, [h])
        h2 = h
        payload = q.cpu().numpy().view(np.uint8)
        pay = [payload[o:o + n] for o, n in zip(lay.offsets.tolist(), sizes)]
    return pay, s.cpu().numpy(), [t.cpu().numpy() for t in h2]


def _guarded(arrs, lead):
    """Every array as a view `lead` elements into its own storage, sentinels before and after it."""
    stores, views = [], []
    for a in arrs:
        store = torch.full((a.size + lead + 1,), float(F_SENTINEL), dtype=torch.float32, device=DEV)
        v = store[lead:lead + a.size]
        v.copy_(torch.from_numpy(a))
        assert v.data_ptr() % 16 == (4 * lead) % 16
        stores.append(store)
        views.append(v)
    return stores, views


def _flat(arrs, lay):
    flat = torch.full((lay.total,), float(F_SENTINEL), dtype=torch.float32, device=DEV)
    for a, o in zip(arrs, lay.offsets.tolist()):
        flat[o:o + a.size].copy_(torch.from_numpy(a))
    return flat


def _check(sizes, kind, form, bits, int4):
    from adfl_amd import ops
    lay = ops.BucketLayout(list(sizes), align=FORMS[form][1 if int4 else 0])
    gs, hs = _pair(sizes, kind)
    offs = lay.offsets.tolist()
    if form in ("aligned", "compact"):
        g_arg, h_arg = _flat(gs, lay), _flat(hs, lay)
        g_all, h_all = [g_arg], [h_arg]
        g_t = [g_arg[o:o + n] for o, n in zip(offs, sizes)]
        h_t = [h_arg[o:o + n] for o, n in zip(offs, sizes)]
    else:
        g_all, g_t = _guarded(gs, 1 if form == "offset1" else 4)
        h_all, h_t = _guarded(hs, 4 if form == "separate" else 1)
        g_arg, h_arg = g_t, h_t
    h_ptrs = [t.data_ptr() for t in h_t]
    nbytes = (lay.total + 1) // 2 if int4 else lay.total
    out = torch.full((nbytes,), SENTINEL, dtype=torch.uint8 if int4 else torch.int8, device=DEV)
    scales = torch.full((lay.ntensors,), -1.0, dtype=torch.float32, device=DEV)
    partials = torch.full((lay.nchunks,), -1, dtype=torch.int32, device=DEV)
    if int4:
        got, gsc = ops.encode_delta_update_batched_int4(g_arg, h_arg, lay, bits, packed=out, scales=scales,
                                                        partials=partials)
    else:
        got, gsc = ops.encode_delta_update_batched(g_arg, h_arg, lay, bits, q=out, scales=scales, partials=partials)
    assert got.data_ptr() == out.data_ptr() and gsc.data_ptr() == scales.data_ptr()   # filled in place
    assert [t.data_ptr() for t in h_t] == h_ptrs
    pay, want_s, want_h = _reference(sizes, kind, bits, int4)
    got_h, gs_h = got.cpu().numpy().view(np.uint8), gsc.cpu().numpy()
    owned = np.zeros(nbytes, dtype=bool)
    for t, (o, n) in enumerate(zip(offs, sizes)):
        where = (kind, form, bits, t, n)
        lo, hi = (o // 2, o // 2 + (n + 1) // 2) if int4 else (o, o + n)
        assert np.array_equal(got_h[lo:hi], pay[t]), where
        assert same_f32(gs_h[t], want_s[t]), where
        assert same_f32(h_t[t].cpu().numpy(), want_h[t]), where
        assert np.array_equal(g_t[t].cpu().numpy().view(np.uint32), gs[t].view(np.uint32)), where   # g unchanged
        owned[lo:hi] = True
    assert (got_h[~owned] == SENTINEL).all(), (kind, form, bits)       # the payload bucket's pads are untouched
    # whatever surrounds the tensors (bucket pads, the guards around separate tensors) is as it was
    for whole, parts in ((g_all, g_t), (h_all, h_t)):
        for store in whole:
            mine = torch.zeros(store.numel(), dtype=torch.bool, device=DEV)
            for v in parts:
                if v.untyped_storage().data_ptr() == store.untyped_storage().data_ptr():
                    mine[v.storage_offset():v.storage_offset() + v.numel()] = True
            assert bool((store[~mine] == float(F_SENTINEL)).all()), (kind, form, bits)
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
    for form in ("aligned", "offset1"):    # the 16-byte path and the element-wise path
        _check(sizes, kind, form, 4 if int4 else 8, int4)


@pytest.mark.parametrize("int4", [False, True], ids=["int8", "int4"])
def test_resident_forms_are_forced_onto_the_two_passes_with_the_same_result(int4, monkeypatch):
    monkeypatch.setenv("ADFL_SLQ_ENCODE", "twopass")
    _check(tuple(delta_cases.RESIDENT_SIZES), "noise", "aligned", 4 if int4 else 8, int4)
    _check(tuple(delta_cases.RESIDENT_SIZES), "equal", "offset1", 4 if int4 else 8, int4)


def test_equal_inputs_leave_the_hidden_state_and_special_values_poison_it():
    from adfl_amd import ops
    sizes = tuple(delta_cases.ALL_SIZES)
    lay = ops.BucketLayout(list(sizes))
    gs, hs = _pair(sizes, "equal")
    h = _dev(hs)
    q, s = ops.encode_delta_update_batched(_dev(gs), h, lay, 8)
    assert (s.cpu().numpy().view(np.uint32) == 0).all()                # scale +0, codes 127, d = +0
    for t, (ht, a) in enumerate(zip(h, hs)):
        got = ht.cpu().numpy()
        assert np.array_equal(got[1:].view(np.uint32), a[1:].view(np.uint32))
        assert got[0].view(np.uint32) == 0                             # -0.0 + (+0.0) = +0.0
    gs, hs = _pair(sizes, "nan_body")
    h = _dev(hs)
    ops.encode_delta_update_batched(_dev(gs), h, lay, 8)
    assert all(bool(torch.isnan(t).all()) for t in h)                  # the tensor's whole hidden state
    gs, hs = _pair(sizes, "pinf_tail")
    h = _dev(hs)
    _, s = ops.encode_delta_update_batched(_dev(gs), h, lay, 8)
    assert bool(torch.isinf(s).all())
    for t in h:   # inf * 0 = NaN on the finite elements; the inf element itself: code 127, inf * 127 = inf
        assert int(torch.isnan(t).sum()) == t.numel() - 1 and bool(torch.isinf(t[-1]))


def test_a_work_entry_above_the_resident_bound_gets_a_nan_scale_and_touches_nothing():
    from adfl_amd import _lib, ops
    lay = ops.BucketLayout([R + 1])
    assert lay.nwork == 0
    g = torch.randn(R + 1, device=DEV)
    h = torch.randn(R + 1, device=DEV)
    keep = h.clone()
    tabs = [torch.tensor([t.data_ptr()], dtype=torch.int64, device=DEV) for t in (g, h)]
    work = torch.zeros(1, dtype=torch.int32, device=DEV)
    for fn, dt in ((_lib.load().adfl_slq_encode_delta_update_batched_work, torch.int8),
                   (_lib.load().adfl_slq_encode_delta_update_batched_int4_work, torch.uint8)):
        out = torch.full((lay.total,), SENTINEL, dtype=dt, device=DEV)
        scales = torch.zeros(1, device=DEV)
        partials = torch.zeros(lay.nchunks, dtype=torch.int32, device=DEV)
        _lib.check(fn(tabs[0].data_ptr(), tabs[1].data_ptr(), lay.device_chunks(g.device).data_ptr(), lay.nchunks,
                      work.data_ptr(), 1, 4, out.data_ptr(), scales.data_ptr(), partials.data_ptr(),
                      torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert bool(torch.isnan(scales).all()) and bool((out == SENTINEL).all())
        assert torch.equal(h.view(torch.int32), keep.view(torch.int32))


def test_bad_arguments_raise():
    from adfl_amd import _lib, ops
    sizes = (1025, 33)
    lay = ops.BucketLayout(list(sizes))
    gs, hs = _pair(sizes, "noise")
    g, h = _dev(gs), _dev(hs)
    with pytest.raises(ValueError, match="tensors for a layout"):
        ops.encode_delta_update_batched(g[:1], h, lay, 8)
    with pytest.raises(ValueError, match="fp32 device tensor"):
        ops.encode_delta_update_batched(g, [t.cpu() for t in h], lay, 8)
    with pytest.raises(ValueError, match="fp32 device tensor"):
        ops.encode_delta_update_batched(g, [t.double() for t in h], lay, 8)
    with pytest.raises(ValueError, match="contiguous"):
        ops.encode_delta_update_batched(g, [h[0], torch.zeros(33, 2, device=DEV)[:, 0]], lay, 8)
    with pytest.raises(ValueError, match="contiguous fp32 device buffer"):
        ops.encode_delta_update_batched(torch.zeros(lay.total, device=DEV),
                                        torch.zeros(2 * lay.total, device=DEV)[::2], lay, 8)
    with pytest.raises(ValueError, match="even"):
        ops.encode_delta_update_batched_int4(g, h, ops.BucketLayout(list(sizes), align=1), 4)
    for bits in (0, 9):
        with pytest.raises(_lib.AdflError, match="invalid argument"):
            ops.encode_delta_update_batched(g, h, lay, bits)
    with pytest.raises(_lib.AdflError, match="invalid argument"):
        ops.encode_delta_update_batched_int4(g, h, lay, 5)
    for t, a in zip(h, hs):    # nothing was launched
        assert np.array_equal(t.cpu().numpy().view(np.uint32), a.view(np.uint32))


def _op_inputs(gap):
    """Two flat buffers with caller-placed tensors (one gap of `gap` elements, out of order)."""
    sizes = [902, 4098, 33]   # even offsets: the int4 op takes the same layout
    offs = [4098 + gap, 0, 4098 + gap + 902]
    off, siz = torch.tensor(offs), torch.tensor(sizes)
    total = offs[2] + sizes[2]
    rng = np.random.default_rng(78)
    hidden = rng.standard_normal(total, dtype=np.float32)
    new = (hidden + np.float32(1e-3) * rng.standard_normal(total, dtype=np.float32)).astype(np.float32)
    return new, hidden, off, siz


@pytest.mark.parametrize("gap", [0, 2])
def test_custom_ops_match_the_two_calls(gap):
    from adfl_amd import ops
    new, hidden, off, siz = _op_inputs(gap)
    lay = ops.layout_for(off, siz)
    for int4 in (False, True):
        n_d, h_d = torch.from_numpy(new).to(DEV), torch.from_numpy(hidden).to(DEV)
        h_ref = torch.from_numpy(hidden).to(DEV)
        if int4:
            got, s = AP.slq_encode_delta_update_batched_int4(n_d, h_d, off, siz, 4)
            want, ws = torch.ops.adfl.slq_encode_delta_batched_int4(n_d, h_ref, off, siz, 4)
            dec = ops.decode_batched_int4(want, ws, lay)
            for o, n in zip(off.tolist(), siz.tolist()):
                h_ref[o:o + n] += dec[o:o + n]
        else:
            got, s = AP.slq_encode_delta_update_batched(n_d, h_d, off, siz, 8)
            want, ws = torch.ops.adfl.slq_encode_delta_batched(n_d, h_ref, off, siz, 8)
            dec = ops.decode_batched(want, ws, lay)
            for o, n in zip(off.tolist(), siz.tolist()):
                h_ref[o:o + n] += dec[o:o + n]
        assert got.dtype == want.dtype and torch.equal(got, want)       # positions no tensor owns are zero
        assert torch.equal(s.view(torch.int32), ws.view(torch.int32))
        assert torch.equal(h_d.view(torch.int32), h_ref.view(torch.int32))   # the gap of hidden is untouched
        assert np.array_equal(n_d.cpu().numpy().view(np.uint32), new.view(np.uint32))


def test_opcheck():
    new, hidden, off, siz = _op_inputs(2)
    n_d, h_d = torch.from_numpy(new).to(DEV), torch.from_numpy(hidden).to(DEV)
    torch.library.opcheck(AP.slq_encode_delta_update_batched, (n_d, h_d, off, siz, 8))
    torch.library.opcheck(AP.slq_encode_delta_update_batched_int4, (n_d, h_d, off, siz, 4))
