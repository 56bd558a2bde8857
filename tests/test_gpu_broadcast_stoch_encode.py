"""GPU: the stochastic broadcast ops — stoch.rqsgd_encode_delta_update_batched (two passes and one launch) and
stoch.qsgd_quantize_update_batched — against the existing ops composed on separate buffers: the delta encode
(rqsgd_encode_delta_batched; bucket_diff + reference_norms + qsgd_quantize_batched), then the codec's decode, then
an fp32 add. Planes, norms and mins byte for byte; the hidden state bit for bit, NaN by position."""

import numpy as np
import pytest
import torch

import delta_cases
from golden_util import same_f32

pytestmark = pytest.mark.gpu

adfl_amd = pytest.importorskip("adfl_amd")
from adfl_amd import _lib, ops, stoch  # noqa: E402

DEV = "cuda"
R = delta_cases.R
HEAD_SIZES = [3, 2, 4, 5, 7]   # for the 4-element head; in this order the compact offsets take every phase mod 4
SIZES = {"all": HEAD_SIZES + delta_cases.ALL_SIZES,            # the largest is R + 1: forces the two passes
         "res": HEAD_SIZES + delta_cases.RESIDENT_SIZES,       # every tensor within the resident bound: one launch
         "mid": [3 * delta_cases.CHUNK_ELEMS + 6]}
GUARD = 0x5A
F_GUARD = 12345.0
U1 = float(np.nextafter(np.float32(1), np.float32(0)))


def _compact(sizes):
    return ops.BucketLayout(sizes, align=1)


def _sources(sizes, seed, special=None):
    """(news, hiddens) as lists of numpy arrays, hidden = new + small noise with a -0 in front; `special(i, h, g)`
    edits a pair in place."""
    rng = np.random.default_rng(seed)
    news, hiddens = [], []
    for i, n in enumerate(sizes):
        g = rng.standard_normal(n, dtype=np.float32)
        h = (g + np.float32(1e-2) * rng.standard_normal(n, dtype=np.float32)).astype(np.float32)
        h[0] = np.float32(-0.0)
        if special is not None:
            special(i, h, g)
        news.append(g)
        hiddens.append(h)
    return news, hiddens


@pytest.fixture(scope="module")
def base():
    return {k: _sources(s, 1 + i) for i, (k, s) in enumerate(SIZES.items())}


def _dev(arrays, offset=0):
    """Separately allocated device tensors, each inside a guarded storage, `offset` elements past a 16-byte
    boundary (offset 1: the element-wise / 4-byte path). Returns (views, storages)."""
    views, stores = [], []
    for a in arrays:
        store = torch.full((a.size + 8,), F_GUARD, dtype=torch.float32, device=DEV)
        v = store[4 + offset:4 + offset + a.size]
        v.copy_(torch.from_numpy(a))
        views.append(v)
        stores.append(store)
    return views, stores


def _assert_hidden(h_views, h_stores, want, offset=0):
    torch.cuda.synchronize()
    for t, (v, s, w) in enumerate(zip(h_views, h_stores, want)):
        assert same_f32(v.cpu().numpy(), w.cpu().numpy()), t
        s = s.cpu().numpy()
        assert (s[:4 + offset] == F_GUARD).all() and (s[4 + offset + v.numel():] == F_GUARD).all(), t


def _guarded(lay, extra=64):
    lv = torch.full((lay.total + extra,), GUARD, dtype=torch.uint8, device=DEV)
    sg = torch.full((lay.total + extra,), GUARD, dtype=torch.int8, device=DEV)
    return lv, sg


def _assert_guard(lay, lv, sg):
    owned = np.zeros(lv.numel(), dtype=bool)
    for o, n in zip(lay.offsets.tolist(), lay.sizes.tolist()):
        owned[o:o + n] = True
    assert (lv.cpu().numpy()[~owned] == GUARD).all() and (sg.cpu().numpy()[~owned] == GUARD).all()


def _same_planes(lay, got, want):
    for a, b in zip(got, want):
        if a.dtype == torch.float32:
            assert same_f32(a.cpu().numpy(), b.cpu().numpy())
        else:
            a, b = a.cpu().numpy(), b.cpu().numpy()
            for t, (o, n) in enumerate(zip(lay.offsets.tolist(), lay.sizes.tolist())):
                assert np.array_equal(a[o:o + n], b[o:o + n]), t


def _rqsgd_composed(news, hiddens, lay, bits, **kw):
    """The existing ops on separate buffers: (levels, signs, norms, mins), [h + decode per tensor]."""
    g, _ = _dev(news)
    h, _ = _dev(hiddens)
    lv, sg, nr, mn = stoch.rqsgd_encode_delta_batched(g, h, lay, bits, resident=False, **kw)
    d = stoch.rqsgd_decode_batched(lv, sg, nr, mn, lay, bits)
    return (lv, sg, nr, mn), [x + d[o:o + n] for x, o, n in zip(h, lay.offsets.tolist(), lay.sizes.tolist())]


def _rqsgd_check(news, hiddens, lay, bits, offset=0, forms=(None, False), **kw):
    """Both forms of the fused op against the composition; guards around planes and hidden tensors."""
    want_planes, want_h = _rqsgd_composed(news, hiddens, lay, bits, **kw)
    outs = []
    for resident in forms:
        g, _ = _dev(news)
        h, stores = _dev(hiddens, offset)
        keep_g = [x.clone() for x in g]
        lv, sg = _guarded(lay)
        out = stoch.rqsgd_encode_delta_update_batched(g, h, lay, bits, levels=lv, signs=sg, resident=resident, **kw)
        _assert_hidden(h, stores, want_h, offset)
        _assert_guard(lay, lv, sg)
        _same_planes(lay, out, want_planes)
        assert all(torch.equal(a, b) or same_f32(a.cpu().numpy(), b.cpu().numpy()) for a, b in zip(g, keep_g))
        outs.append(out)
    return outs


def _qsgd_composed(news, hiddens, comp, bits, **kw):
    g, _ = _dev(news)
    h, _ = _dev(hiddens)
    diff = ops.bucket_diff(g, h, comp)
    norms = stoch.torch_norms(diff, comp)
    lv, sg = stoch.qsgd_quantize_batched(diff, comp, bits, norms, **kw)
    d = stoch.qsgd_decode_batched(lv, sg, norms, comp, bits)
    return (lv, sg), norms, [x + d[o:o + n] for x, o, n in zip(h, comp.offsets.tolist(), comp.sizes.tolist())]


def _qsgd_check(news, hiddens, comp, bits, offset=0, **kw):
    want_planes, norms, want_h = _qsgd_composed(news, hiddens, comp, bits, **kw)
    g, _ = _dev(news)
    h, stores = _dev(hiddens, offset)
    diff = ops.bucket_diff(g, h, comp)
    keep = diff.clone()
    lv, sg = _guarded(comp)
    out = stoch.qsgd_quantize_update_batched(diff, comp, bits, norms, h, levels=lv, signs=sg, **kw)
    _assert_hidden(h, stores, want_h, offset)
    _assert_guard(comp, lv, sg)
    _same_planes(comp, out, want_planes)
    assert same_f32(diff.cpu().numpy(), keep.cpu().numpy())       # the difference bucket is read only
    return norms, h


def _uniform_plane(kind, n):
    return {"random": lambda: torch.from_numpy(np.random.default_rng(3).random(n, dtype=np.float32)),
            "zeros": lambda: torch.zeros(n), "ones": lambda: torch.full((n,), U1)}[kind]().to(DEV)


def test_the_size_lists_cover_every_phase_and_both_forms():
    for which in ("all", "res"):
        comp, al = _compact(SIZES[which]), ops.BucketLayout(SIZES[which])
        assert set(((comp.offsets - al.offsets) % 4).tolist()) == {0, 1, 2, 3}
        assert set((comp.offsets % 4).tolist()) == {0, 1, 2, 3}
    assert ops.BucketLayout(SIZES["all"]).nwork == 0 and max(SIZES["all"]) == R + 1
    assert ops.BucketLayout(SIZES["res"]).nwork == len(SIZES["res"])
    assert ops.BucketLayout(SIZES["mid"]).nwork == 1 and ops.BucketLayout(SIZES["mid"]).nchunks == 4


@pytest.mark.parametrize("which", list(SIZES))
@pytest.mark.parametrize("bits", [8, 4, 2, 9])
def test_rqsgd_aligned_planes_with_ushift_philox(base, which, bits):
    news, hiddens = base[which]
    comp, lay = _compact(SIZES[which]), ops.BucketLayout(SIZES[which])
    _rqsgd_check(news, hiddens, lay, bits, ushift=comp.offsets - lay.offsets, seed=0x1234567, counter=77)


@pytest.mark.parametrize("which", list(SIZES))
@pytest.mark.parametrize("uniforms", ["random", "zeros", "ones"])
def test_rqsgd_injected_uniforms_with_and_without_ushift(base, which, uniforms):
    news, hiddens = base[which]
    comp, lay = _compact(SIZES[which]), ops.BucketLayout(SIZES[which])
    u = _uniform_plane(uniforms, comp.total)
    _rqsgd_check(news, hiddens, lay, 4, ushift=comp.offsets - lay.offsets, uniforms=u)
    _rqsgd_check(news, hiddens, comp, 8, uniforms=u)      # compact planes: every chunk has a head


@pytest.mark.parametrize("which", list(SIZES))
def test_rqsgd_compact_planes_philox(base, which):
    news, hiddens = base[which]
    _rqsgd_check(news, hiddens, _compact(SIZES[which]), 8, seed=99, counter=5)


@pytest.mark.parametrize("which", list(SIZES))
def test_rqsgd_hidden_one_element_into_its_storage_goes_element_wise(base, which):
    news, hiddens = base[which]
    comp, lay = _compact(SIZES[which]), ops.BucketLayout(SIZES[which])
    _rqsgd_check(news, hiddens, lay, 8, offset=1, ushift=comp.offsets - lay.offsets, seed=7, counter=1)


def test_rqsgd_flat_buckets(base):
    news, hiddens = base["res"]
    comp = _compact(SIZES["res"])
    want_planes, want_h = _rqsgd_composed(news, hiddens, comp, 8, seed=3, counter=9)
    g = torch.from_numpy(np.concatenate(news)).to(DEV)
    h = torch.from_numpy(np.concatenate(hiddens)).to(DEV)
    out = stoch.rqsgd_encode_delta_update_batched(g, h, comp, 8, seed=3, counter=9)
    _same_planes(comp, out, want_planes)
    assert same_f32(h.cpu().numpy(), torch.cat(want_h).cpu().numpy())


@pytest.mark.parametrize("which", list(SIZES))
@pytest.mark.parametrize("bits", [8, 4, 2, 9])
def test_qsgd_quantize_update_philox(base, which, bits):
    news, hiddens = base[which]
    _qsgd_check(news, hiddens, _compact(SIZES[which]), bits, seed=0x7654321, counter=13)


@pytest.mark.parametrize("which", list(SIZES))
@pytest.mark.parametrize("uniforms", ["random", "zeros", "ones"])
def test_qsgd_quantize_update_injected_uniforms(base, which, uniforms):
    news, hiddens = base[which]
    comp = _compact(SIZES[which])
    _qsgd_check(news, hiddens, comp, 8, uniforms=_uniform_plane(uniforms, comp.total))


@pytest.mark.parametrize("which", list(SIZES))
@pytest.mark.parametrize("layout", ["compact", "aligned"])
def test_qsgd_hidden_phases_take_the_4_byte_path(base, which, layout):
    """In the compact bucket most slots differ in phase from their (aligned) hidden tensors; one element into the
    storage, the aligned bucket's do too. The same bits either way."""
    news, hiddens = base[which]
    lay = _compact(SIZES[which]) if layout == "compact" else ops.BucketLayout(SIZES[which])
    _qsgd_check(news, hiddens, lay, 8, offset=1, seed=5, counter=2)
    _qsgd_check(news, hiddens, lay, 4, offset=0, seed=5, counter=2)


# one tensor per path: inside the head, a few groups, under a chunk, several chunks, and the largest the form takes
SPECIAL_SIZES = {"twopass": [5, 7, 4099, 3 * delta_cases.CHUNK_ELEMS + 6, R + 1],
                 "resident": [5, 7, 4099, 3 * delta_cases.CHUNK_ELEMS + 6, R]}
POSITIONS = {"head": lambda n: 1, "body": lambda n: n // 2, "tail": lambda n: n - 2}


def _special(kind, where):
    def edit(i, h, g):
        n = h.size
        k = min(max(POSITIONS[where](n), 0), n - 1)
        if kind == "zero":          # the whole tensor's difference is zero: the norm == 0 fill
            g[:] = h
        elif kind == "inf_minus_inf":
            h[k] = g[k] = np.float32(np.inf)
        elif kind == "nan":
            (h if i % 2 else g)[k] = np.float32(np.nan)
        elif kind == "denormal":    # denormal differences: the norm is below the fast division's range
            g[:] = np.float32(1e-39) * np.arange(n, dtype=np.float32) % np.float32(7e-39)
            h[:] = 0
            h[0] = np.float32(-0.0)
            h[k] = g[k] - np.float32(1e-45)
    return edit


@pytest.mark.parametrize("form", list(SPECIAL_SIZES))
@pytest.mark.parametrize("where", list(POSITIONS))
@pytest.mark.parametrize("kind", ["zero", "inf_minus_inf", "nan", "denormal"])
def test_special_differences_in_head_body_and_tail(kind, where, form):
    sizes = SPECIAL_SIZES[form]
    news, hiddens = _sources(sizes, 11, _special(kind, where))
    comp, lay = _compact(sizes), ops.BucketLayout(sizes)
    assert (lay.nwork > 0) == (form == "resident")
    ushift = comp.offsets - lay.offsets
    for offset in (0, 1):   # the vector path, then the element-wise one on the same values
        outs = _rqsgd_check(news, hiddens, lay, 8, offset=offset, ushift=ushift, seed=5, counter=3)
        norms, h = _qsgd_check(news, hiddens, comp, 8, offset=offset, seed=5, counter=3)
        for nr in (outs[0][2], norms):
            nr = nr.cpu()
            if kind == "zero":
                assert (nr == 0).all()
            if kind in ("inf_minus_inf", "nan"):
                assert torch.isnan(nr).all()
    if kind == "zero":      # h unchanged, except that -0 becomes +0
        for t, want in zip(h, hiddens):
            got = t.cpu().numpy()
            assert np.array_equal(got, want) and not np.signbit(got[0]) and np.signbit(want[0])
            assert same_f32(got[1:], want[1:])
    if kind in ("inf_minus_inf", "nan"):
        assert all(bool(torch.isnan(t).all()) for t in h)


def test_a_nan_norm_poisons_exactly_that_tensor(base):
    news, hiddens = base["res"]
    news = [g.copy() for g in news]
    bad = 9
    news[bad][news[bad].size // 2] = np.float32(np.nan)
    comp, lay = _compact(SIZES["res"]), ops.BucketLayout(SIZES["res"])
    for check, L in ((_rqsgd_check, lay), (_qsgd_check, comp)):
        g, _ = _dev(news)
        h, _ = _dev(hiddens)
        if check is _rqsgd_check:
            stoch.rqsgd_encode_delta_update_batched(g, h, L, 8, seed=1, counter=1)
        else:
            diff = ops.bucket_diff(g, h, L)
            stoch.qsgd_quantize_update_batched(diff, L, 8, stoch.torch_norms(diff, L), h, seed=1, counter=1)
        for t, x in enumerate(h):
            assert bool(torch.isnan(x).all()) if t == bad else not bool(torch.isnan(x).any()), t


def test_a_work_entry_above_the_resident_bound_gets_nan_norm_and_min_and_touches_nothing():
    lay = ops.BucketLayout([R + 1])
    assert lay.nwork == 0
    g = torch.randn(R + 1, device=DEV)
    h = torch.randn(R + 1, device=DEV)
    keep = h.clone()
    tabs = [torch.tensor([t.data_ptr()], dtype=torch.int64, device=DEV) for t in (g, h)]
    work = torch.zeros(1, dtype=torch.int32, device=DEV)
    lv, sg = _guarded(lay, 0)
    norms, mins = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    ws = stoch.workspace(lay, g.device)
    _lib.check(_lib.load().adfl_rqsgd_encode_delta_update_batched_work(
        tabs[0].data_ptr(), tabs[1].data_ptr(), lay.device_chunks(g.device).data_ptr(), lay.nchunks, work.data_ptr(),
        1, 8, None, None, 1, 2, ws.data_ptr(), ws.numel(), lv.data_ptr(), sg.data_ptr(), norms.data_ptr(),
        mins.data_ptr(), ops._stream(g.device)))
    torch.cuda.synchronize()
    assert bool(torch.isnan(norms).all()) and bool(torch.isnan(mins).all())
    assert bool((lv == GUARD).all()) and bool((sg == GUARD).all()) and torch.equal(h, keep)


def test_value_errors(base):
    news, hiddens = base["res"]
    g, _ = _dev(news)
    h, _ = _dev(hiddens)
    lay, comp = ops.BucketLayout(SIZES["res"]), _compact(SIZES["res"])
    enc = stoch.rqsgd_encode_delta_update_batched
    with pytest.raises(ValueError):
        enc([t.cpu() for t in g], h, lay, 8)                              # wrong device
    with pytest.raises(ValueError):
        enc(g, [t.cpu() for t in h], lay, 8)
    with pytest.raises(ValueError):
        enc(g, [t.double() for t in h], lay, 8)                           # dtype
    with pytest.raises(ValueError):
        enc(g[:-1], h[:-1], lay, 8)                                       # count
    with pytest.raises(ValueError):
        enc(g, h[:-1] + [h[-1][:-1]], lay, 8)                             # size
    with pytest.raises(ValueError):
        enc(g, h[:-1] + [torch.zeros(2 * h[-1].numel(), device=DEV)[::2]], lay, 8)   # not contiguous
    with pytest.raises(ValueError):
        enc(torch.cat(g), torch.cat(h)[:-1], comp, 8)                     # flat buffer smaller than the layout
    with pytest.raises(ValueError):
        enc(g, h, lay, 8, ushift=np.full(lay.ntensors, -1, dtype=np.int64))   # g + ushift below 0
    with pytest.raises(ValueError):
        enc(g, h, lay, 8, uniforms=torch.zeros(8, device=DEV))            # uniforms too short
    diff = ops.bucket_diff(g, h, comp)
    norms = stoch.torch_norms(diff, comp)
    qup = stoch.qsgd_quantize_update_batched
    with pytest.raises(ValueError):
        qup(diff.double(), comp, 8, norms, h)
    with pytest.raises(ValueError):
        qup(diff, comp, 8, norms, [t.cpu() for t in h])
    with pytest.raises(ValueError):
        qup(diff, comp, 8, norms, [t.double() for t in h])
    with pytest.raises(ValueError):
        qup(diff, comp, 8, norms, h[:-1])
    with pytest.raises(ValueError):
        qup(diff, comp, 8, norms, h[:-1] + [h[-1][:-1]])
    with pytest.raises(ValueError):
        qup(diff[:-1], comp, 8, norms, h)
    keep = [t.clone() for t in h]
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(h, keep))                # nothing was launched
    out = enc(g, h, lay, 8, ushift=comp.offsets - lay.offsets)            # still works afterwards
    assert out[0].numel() == lay.total


@pytest.mark.parametrize("codec", ["qsgd", "rqsgd", "cnat"])
def test_custom_op_against_the_python_entries(base, codec):
    news, hiddens = base["res"]
    comp = _compact(SIZES["res"])
    new_flat = torch.from_numpy(np.concatenate(news)).to(DEV)
    h_np = np.concatenate(hiddens)
    off, siz = torch.from_numpy(comp.offsets.copy()), torch.from_numpy(comp.sizes.copy())
    hidden = torch.from_numpy(h_np).to(DEV)
    got = torch.ops.adfl_apply.stoch_encode_delta_update_batched(new_flat, hidden, off, siz, codec, 8, 42, 6)
    h0 = torch.from_numpy(h_np).to(DEV)
    if codec == "rqsgd":
        want = stoch.rqsgd_encode_delta_batched(new_flat, h0, comp, 8, seed=42, counter=6)
        d = stoch.rqsgd_decode_batched(*want, comp, 8)
    elif codec == "qsgd":
        diff = ops.bucket_diff(new_flat, h0, comp)
        norms = stoch.torch_norms(diff, comp)
        want = stoch.qsgd_quantize_batched(diff, comp, 8, norms, seed=42, counter=6) + (norms, torch.zeros_like(norms))
        d = stoch.qsgd_decode_batched(want[0], want[1], norms, comp, 8)
    else:
        diff = ops.bucket_diff(new_flat, h0, comp)
        want = stoch.cnat_encode_batched(diff, comp, 8, seed=42, counter=6)
        want = want + (torch.zeros_like(want[2]),)
        d = stoch.cnat_decode_batched(want[0], want[1], want[2], comp)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape
        assert same_f32(a.cpu().numpy(), b.cpu().numpy()) if a.dtype == torch.float32 else torch.equal(a, b)
    assert same_f32(hidden.cpu().numpy(), (h0 + d).cpu().numpy())


def test_custom_op_opcheck(base):
    news, hiddens = base["res"]
    sizes = SIZES["res"][:6]
    comp = _compact(sizes)
    new_flat = torch.from_numpy(np.concatenate(news[:6])).to(DEV)
    hidden = torch.from_numpy(np.concatenate(hiddens[:6])).to(DEV)
    off, siz = torch.from_numpy(comp.offsets.copy()), torch.from_numpy(comp.sizes.copy())
    for codec in ("qsgd", "rqsgd", "cnat"):
        torch.library.opcheck(torch.ops.adfl_apply.stoch_encode_delta_update_batched,
                              (new_flat, hidden.clone(), off, siz, codec, 8, 1, 2))
    with pytest.raises(ValueError):
        torch.ops.adfl_apply.stoch_encode_delta_update_batched(new_flat.double(), hidden, off, siz, "rqsgd", 8, 1, 2)
    with pytest.raises(ValueError):
        torch.ops.adfl_apply.stoch_encode_delta_update_batched(new_flat, hidden.double(), off, siz, "rqsgd", 8, 1, 2)
    with pytest.raises(ValueError):
        torch.ops.adfl_apply.stoch_encode_delta_update_batched(new_flat, hidden, off, siz, "slq", 8, 1, 2)
