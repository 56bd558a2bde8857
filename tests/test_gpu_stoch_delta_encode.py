"""GPU: the two-source RQSGD encode (stoch.rqsgd_encode_delta_batched) against rqsgd_encode_batched on the
materialised difference in the compact layout, bucket_diff against torch.sub, and the custom op. Every
comparison is exact (bytes; fp32 by bits with NaN by position)."""

import numpy as np
import pytest
import torch

import delta_cases
from golden_util import same_f32

pytestmark = pytest.mark.gpu

adfl_amd = pytest.importorskip("adfl_amd")
from adfl_amd import ops, stoch  # noqa: E402

DEV = "cuda"
HEAD_SIZES = [3, 2, 4, 5, 7]   # for the 4-element head; in this order the compact offsets take every phase mod 4
SIZES = HEAD_SIZES + delta_cases.ALL_SIZES            # the largest is R + 1 = 65,537: forces the two passes
RES_SIZES = HEAD_SIZES + delta_cases.RESIDENT_SIZES   # every tensor within the resident bound
GUARD = 0x5A
U1 = float(np.nextafter(np.float32(1), np.float32(0)))


def _compact(sizes):
    return ops.BucketLayout(sizes, align=1)


def test_the_size_list_covers_every_ushift_phase_and_the_two_pass_bound():
    for sizes in (SIZES, RES_SIZES):
        comp, al = _compact(sizes), ops.BucketLayout(sizes)
        assert set(((comp.offsets - al.offsets) % 4).tolist()) == {0, 1, 2, 3}
    assert _compact(SIZES).nwork == 0 and max(SIZES) == delta_cases.R + 1      # no resident work list
    assert _compact(RES_SIZES).nwork == len(RES_SIZES)


def _sources(sizes, seed, special=None):
    """(news, prevs) lists of separately allocated device tensors, prev = new + small noise; `special(i, a, b)`
    edits a numpy pair in place."""
    rng = np.random.default_rng(seed)
    news, prevs = [], []
    for i, n in enumerate(sizes):
        b = rng.standard_normal(n, dtype=np.float32)
        a = (b + np.float32(1e-2) * rng.standard_normal(n, dtype=np.float32)).astype(np.float32)
        if special is not None:
            special(i, a, b)
        news.append(torch.from_numpy(b).to(DEV))
        prevs.append(torch.from_numpy(a).to(DEV))
    return news, prevs


@pytest.fixture(scope="module")
def base():
    return {"all": _sources(SIZES, 1), "res": _sources(RES_SIZES, 2)}


def _reference(news, prevs, sizes, bits, **kw):
    """rqsgd_encode_batched over torch's own difference gathered into the compact bucket."""
    comp = _compact(sizes)
    diff = torch.cat([b - a for a, b in zip(prevs, news)])
    lv, sg, nr, mn = stoch.rqsgd_encode_batched(diff, comp, bits, **kw)
    return comp, lv, sg, nr, mn


def _assert_planes(lay, comp, lv, sg, nr, mn, ref):
    _, rlv, rsg, rnr, rmn = ref
    torch.cuda.synchronize()
    assert same_f32(nr.cpu().numpy(), rnr.cpu().numpy()) and same_f32(mn.cpu().numpy(), rmn.cpu().numpy())
    lv, sg, rlv, rsg = (t.cpu().numpy() for t in (lv, sg, rlv, rsg))
    for t, (o, c, n) in enumerate(zip(lay.offsets.tolist(), comp.offsets.tolist(), lay.sizes.tolist())):
        assert np.array_equal(lv[o:o + n], rlv[c:c + n]), t
        assert np.array_equal(sg[o:o + n], rsg[c:c + n]), t


def _guarded(lay, extra=64):
    lv = torch.full((lay.total + extra,), GUARD, dtype=torch.uint8, device=DEV)
    sg = torch.full((lay.total + extra,), GUARD, dtype=torch.int8, device=DEV)
    return lv, sg


def _assert_guard(lay, lv, sg):
    owned = np.zeros(lv.numel(), dtype=bool)
    for o, n in zip(lay.offsets.tolist(), lay.sizes.tolist()):
        owned[o:o + n] = True
    assert (lv.cpu().numpy()[~owned] == GUARD).all() and (sg.cpu().numpy()[~owned] == GUARD).all()


@pytest.mark.parametrize("which", ["all", "res"])
@pytest.mark.parametrize("bits", [8, 4, 2, 9])
def test_pointer_tables_aligned_planes_and_ushift_philox(base, which, bits):
    sizes = SIZES if which == "all" else RES_SIZES
    news, prevs = base[which]
    comp, lay = _compact(sizes), ops.BucketLayout(sizes)
    ushift = comp.offsets - lay.offsets
    ref = _reference(news, prevs, sizes, bits, seed=0x1234567, counter=77)
    assert (lay.nwork > 0) == (which == "res")
    # resident=None against resident=False byte-equal; pads and bytes past lay.total untouched
    out = _encode_both_forms(news, prevs, lay, bits, ushift=ushift, seed=0x1234567, counter=77)
    _assert_planes(lay, comp, *out, ref)


@pytest.mark.parametrize("which", ["all", "res"])
@pytest.mark.parametrize("uniforms", ["philox", "random", "zeros", "ones"])
def test_two_compact_buckets_no_ushift(base, which, uniforms):
    sizes = SIZES if which == "all" else RES_SIZES
    news, prevs = base[which]
    comp = _compact(sizes)
    new_flat, prev_flat = torch.cat(news), torch.cat(prevs)
    kw = {"seed": 99, "counter": 5}
    if uniforms != "philox":
        u = {"random": lambda: torch.from_numpy(np.random.default_rng(3).random(comp.total, dtype=np.float32)),
             "zeros": lambda: torch.zeros(comp.total), "ones": lambda: torch.full((comp.total,), U1)}[uniforms]()
        kw = {"uniforms": u.to(DEV)}
    ref = _reference(news, prevs, sizes, 8, **kw)
    lv, sg = _guarded(comp)
    out = stoch.rqsgd_encode_delta_batched(new_flat, prev_flat, comp, 8, levels=lv, signs=sg, **kw)
    _assert_planes(comp, comp, *out, ref)
    _assert_guard(comp, lv, sg)


def _lists(which):
    """(sizes, whether the layout has a resident work list): "res" launches k_rqsgd_encode_delta_resident by
    default, "all" (one tensor of R + 1) the two passes."""
    sizes = SIZES if which == "all" else RES_SIZES
    lay = ops.BucketLayout(sizes)
    assert (lay.nwork > 0) == (which == "res")
    return sizes, lay


def _encode_both_forms(news, prevs, lay, bits, **kw):
    """The encode as the layout picks its form (resident=None) and forced to the two passes (resident=False), into
    guarded planes: byte-equal, pads untouched. Returns the first."""
    outs = []
    for resident in (None, False):
        lv, sg = _guarded(lay)
        outs.append(stoch.rqsgd_encode_delta_batched(news, prevs, lay, bits, levels=lv, signs=sg, resident=resident,
                                                     **kw))
        _assert_guard(lay, lv, sg)
    torch.cuda.synchronize()
    (lv, sg, nr, mn), (lv2, sg2, nr2, mn2) = outs
    assert torch.equal(lv, lv2) and torch.equal(sg, sg2)
    assert same_f32(nr.cpu().numpy(), nr2.cpu().numpy()) and same_f32(mn.cpu().numpy(), mn2.cpu().numpy())
    return outs[0]


@pytest.mark.parametrize("which", ["all", "res"])
@pytest.mark.parametrize("uniforms", ["random", "zeros", "ones"])
def test_injected_uniforms_with_ushift(base, which, uniforms):
    """Injected uniforms are indexed by the shifted (compact) index, whatever the shift's phase (a tensor whose
    shift is not a multiple of 4 goes element-wise, in the resident kernel too)."""
    sizes, lay = _lists(which)
    news, prevs = base[which]
    comp = _compact(sizes)
    u = {"random": lambda: torch.from_numpy(np.random.default_rng(4).random(comp.total, dtype=np.float32)),
         "zeros": lambda: torch.zeros(comp.total), "ones": lambda: torch.full((comp.total,), U1)}[uniforms]().to(DEV)
    ref = _reference(news, prevs, sizes, 4, uniforms=u)
    out = _encode_both_forms(news, prevs, lay, 4, ushift=comp.offsets - lay.offsets, uniforms=u)
    _assert_planes(lay, comp, *out, ref)


def _one_element_in(tensors):
    out = []
    for a in tensors:
        store = torch.empty(a.numel() + 1, dtype=torch.float32, device=DEV)
        store[1:].copy_(a)
        out.append(store[1:])
    return out


@pytest.mark.parametrize("which", ["all", "res"])
def test_a_prev_view_one_element_into_its_storage_goes_element_wise(base, which):
    sizes, lay = _lists(which)
    news, prevs = base[which]
    shifted = _one_element_in(prevs)
    assert all((a.data_ptr() - b.data_ptr()) % 16 for a, b in zip(shifted, news))
    comp = _compact(sizes)
    ref = _reference(news, prevs, sizes, 8, seed=7, counter=1)
    out = _encode_both_forms(news, shifted, lay, 8, ushift=comp.offsets - lay.offsets, seed=7, counter=1)
    _assert_planes(lay, comp, *out, ref)


# one tensor per path: inside the head, a few groups, under a chunk, several chunks, and the largest the form takes
SPECIAL_SIZES = {"twopass": [5, 7, 4099, 3 * delta_cases.CHUNK_ELEMS + 6, delta_cases.R + 1],
                 "resident": [5, 7, 4099, 3 * delta_cases.CHUNK_ELEMS + 6, delta_cases.R]}
POSITIONS = {"head": lambda n: 1, "body": lambda n: n // 2, "tail": lambda n: n - 2}


def _special(kind, where):
    def edit(i, a, b):
        n = a.size
        k = min(max(POSITIONS[where](n), 0), n - 1)
        if kind == "zero":          # the whole tensor's difference is zero: the norm == 0 fill
            a[:] = b
        elif kind == "inf_minus_inf":
            a[k] = b[k] = np.float32(np.inf)
        elif kind == "nan":
            (a if i % 2 else b)[k] = np.float32(np.nan)
        elif kind == "denormal":    # denormal differences: the norm is below the fast division's range
            b[:] = np.float32(1e-39) * np.arange(n, dtype=np.float32) % np.float32(7e-39)
            a[:] = 0
            a[k] = b[k] - np.float32(1e-45)
    return edit


@pytest.mark.parametrize("form", list(SPECIAL_SIZES))
@pytest.mark.parametrize("where", list(POSITIONS))
@pytest.mark.parametrize("kind", ["zero", "inf_minus_inf", "nan", "denormal"])
def test_special_differences_in_head_body_and_tail(kind, where, form):
    sizes = SPECIAL_SIZES[form]
    news, prevs = _sources(sizes, 11, _special(kind, where))
    comp, lay = _compact(sizes), ops.BucketLayout(sizes)
    assert (lay.nwork > 0) == (comp.nwork > 0) == (form == "resident")
    ref = _reference(news, prevs, sizes, 8, seed=5, counter=3)
    if kind == "zero":
        assert (ref[3].cpu() == 0).all()
    if kind in ("inf_minus_inf", "nan"):
        assert torch.isnan(ref[3].cpu()).all() and torch.isnan(ref[4].cpu()).all()
    ushift = comp.offsets - lay.offsets
    out = _encode_both_forms(news, prevs, lay, 8, ushift=ushift, seed=5, counter=3)
    _assert_planes(lay, comp, *out, ref)
    if kind == "zero":
        for o, n in zip(lay.offsets.tolist(), lay.sizes.tolist()):
            assert (out[0][o:o + n] == 0).all() and (out[1][o:o + n] == 1).all()
    # the same sources as two compact buckets: every chunk has a head now
    out = _encode_both_forms(torch.cat(news), torch.cat(prevs), comp, 8, seed=5, counter=3)
    _assert_planes(comp, comp, *out, ref)
    # ... and with `prev` one element into its storage: the element-wise branches on the same special values
    out = _encode_both_forms(news, _one_element_in(prevs), lay, 8, ushift=ushift, seed=5, counter=3)
    _assert_planes(lay, comp, *out, ref)


@pytest.mark.parametrize("aligned", [True, False])
def test_bucket_diff_equals_torch_sub(base, aligned):
    news, prevs = base["all"]
    prevs_in = [t.clone() for t in prevs] if aligned else _one_element_in(prevs)   # the fixture stays as it is
    news = [t.clone() for t in news]
    news[3][1] = float("inf")
    prevs_in[3][1] = float("inf")
    news[8][0] = float("nan")
    for lay in (ops.BucketLayout(SIZES), _compact(SIZES)):
        out = torch.full((lay.total + 8,), 123.0, dtype=torch.float32, device=DEV)
        got = ops.bucket_diff(news, prevs_in, lay, out=out)
        assert got.data_ptr() == out.data_ptr()
        torch.cuda.synchronize()
        owned = np.zeros(out.numel(), dtype=bool)
        g = out.cpu().numpy()
        for o, n, a, b in zip(lay.offsets.tolist(), lay.sizes.tolist(), prevs_in, news):
            assert same_f32(g[o:o + n], (b - a).cpu().numpy())
            owned[o:o + n] = True
        assert (g[~owned] == 123.0).all()
    comp = _compact(SIZES)
    flat = ops.bucket_diff(torch.cat(news), torch.cat(prevs_in), comp)     # two flat buckets
    assert same_f32(flat.cpu().numpy(), (torch.cat(news) - torch.cat(prevs_in)).cpu().numpy())


@pytest.mark.parametrize("codec", ["qsgd", "rqsgd", "cnat"])
def test_custom_op_against_the_python_entries(base, codec):
    news, prevs = base["res"]
    comp = _compact(RES_SIZES)
    new_flat, prev_flat = torch.cat(news), torch.cat(prevs)
    off, siz = torch.from_numpy(comp.offsets.copy()), torch.from_numpy(comp.sizes.copy())
    got = torch.ops.adfl.stoch_encode_delta_batched(new_flat, prev_flat, off, siz, codec, 8, 42, 6)
    want = torch.ops.adfl.stoch_encode_batched(new_flat - prev_flat, off, siz, codec, 8, 42, 6)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape
        assert same_f32(a.cpu().numpy(), b.cpu().numpy()) if a.dtype == torch.float32 else torch.equal(a, b)
    if codec == "rqsgd":
        lv, sg, nr, mn = stoch.rqsgd_encode_delta_batched(new_flat, prev_flat, comp, 8, seed=42, counter=6)
        assert torch.equal(got[0], lv) and torch.equal(got[1], sg)


def test_custom_op_opcheck_and_compile(base):
    news, prevs = base["res"]
    sizes = RES_SIZES[:6]
    comp = _compact(sizes)
    new_flat, prev_flat = torch.cat(news[:6]), torch.cat(prevs[:6])
    off, siz = torch.from_numpy(comp.offsets.copy()), torch.from_numpy(comp.sizes.copy())
    for codec in ("qsgd", "rqsgd", "cnat"):
        torch.library.opcheck(torch.ops.adfl.stoch_encode_delta_batched,
                              (new_flat, prev_flat, off, siz, codec, 8, 1, 2))

    def f(a, b):
        lv, sg, nr, mn = torch.ops.adfl.stoch_encode_delta_batched(a, b, off, siz, "rqsgd", 8, 1, 2)
        return torch.ops.adfl.stoch_decode_batched(lv, sg, nr, mn, off, siz, "rqsgd", 8)

    got = torch.compile(f, backend="aot_eager", fullgraph=True)(new_flat, prev_flat)
    assert same_f32(got.cpu().numpy(), f(new_flat, prev_flat).cpu().numpy())
    with pytest.raises(ValueError):
        torch.ops.adfl.stoch_encode_delta_batched(new_flat.double(), prev_flat.double(), off, siz, "rqsgd", 8, 1, 2)
    with pytest.raises(ValueError):
        torch.ops.adfl.stoch_encode_delta_batched(new_flat, prev_flat, off, siz, "slq", 8, 1, 2)


def test_value_errors(base):
    news, prevs = base["res"]
    lay = ops.BucketLayout(RES_SIZES)
    comp = _compact(RES_SIZES)
    enc = stoch.rqsgd_encode_delta_batched
    with pytest.raises(ValueError):
        enc([t.cpu() for t in news], prevs, lay, 8)                       # wrong device
    with pytest.raises(ValueError):
        enc(news, [t.cpu() for t in prevs], lay, 8)
    with pytest.raises(ValueError):
        enc([t.double() for t in news], prevs, lay, 8)                    # dtype
    with pytest.raises(ValueError):
        enc(torch.cat(news).half(), torch.cat(prevs).half(), comp, 8)
    with pytest.raises(ValueError):
        enc(news[:-1], prevs[:-1], lay, 8)                                # count
    with pytest.raises(ValueError):
        enc(news, prevs[:-1] + [prevs[-1][:-1]], lay, 8)                  # size
    with pytest.raises(ValueError):
        enc(torch.cat(news)[:-1], torch.cat(prevs), comp, 8)              # flat buffer smaller than the layout
    with pytest.raises(ValueError):
        enc(news, prevs, lay, 8, ushift=np.full(lay.ntensors, -1, dtype=np.int64))   # first index below 0
    with pytest.raises(ValueError):
        enc(news, prevs, lay, 8, ushift=np.zeros(3, dtype=np.int64))
    with pytest.raises(ValueError):
        enc(news, prevs, lay, 8, uniforms=torch.zeros(8, device=DEV))     # uniforms too short
    with pytest.raises(ValueError):
        ops.bucket_diff(news[:-1], prevs[:-1], lay)
    out = enc(news, prevs, lay, 8, ushift=comp.offsets - lay.offsets)     # still works afterwards
    assert out[0].numel() == lay.total
