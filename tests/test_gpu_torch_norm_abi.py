"""GPU: adfl_torch_norms / adfl_torch_norms_work (include/adfl_stoch.h) at the C ABI itself, where
stoch.reference_norms never goes: the entry with no first-chunk list, explicit `kinds` hints (exact, 0, single
bits that do not name every tensor, invalid values), caller-owned scratch that holds anything at all, outputs
given one at a time, and the edges of the count arguments.

Every expected value is torch.linalg.vector_norm of the tensor on this box's CPU, compared bit for bit (NaN
matches NaN). Outputs are pre-filled with -1.0, which no norm is, so a slot no kernel wrote shows. A tensor that
a single-bit hint does not name must hold a quiet NaN (the behaviour include/adfl_stoch.h states for `kinds`).
Layouts are built from the library's own short-tensor bound B = adfl_torch_norm_short_max_dt(dtype): all short
(up to B), all long (from B + 1) and both mixed orders — the smallest sizes that reach every launch branch.
"""

import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from adfl_amd import _lib, ops, stoch  # noqa: E402

DEV = torch.device("cuda", 0)
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "f64": torch.float64}
IDS = {"f32": _lib.DTYPE_F32, "bf16": _lib.DTYPE_BF16, "f16": _lib.DTYPE_F16, "f64": _lib.DTYPE_F64}
SHORT, LONG = 1, 2          # ADFL_TORCH_NORM_SHORT / ADFL_TORCH_NORM_LONG
E_ARG = -1                  # ADFL_E_ARG
THREADS = 8                 # fp16's at::parallel_for split (the other dtypes do not use it)
SENTINEL = -1.0
LAYOUTS = ["all_short", "all_long", "mixed", "mixed_rev"]


def _data(kind: str, n: int, rng, dtype) -> torch.Tensor:
    """test_gpu_torch_norm_dt._data's "grad" and "ints" (ints: ties); that file covers the data variety."""
    x = rng.standard_normal(n) * 1e-3 if kind == "grad" else np.trunc(rng.standard_normal(n) * 20)
    return torch.from_numpy(x).to(dtype)


def _torch_norm(x: torch.Tensor, threads: int) -> float:
    old = torch.get_num_threads()
    torch.set_num_threads(threads)
    try:
        return torch.linalg.vector_norm(x).item()
    finally:
        torch.set_num_threads(old)


def _same(a: float, b: float) -> bool:
    return (np.isnan(a) and np.isnan(b)) or np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64)


def _bound(dt: str) -> int:
    return int(_lib.load().adfl_torch_norm_short_max_dt(IDS[dt]))


def _sizes(dt: str, layout: str):
    B = _bound(dt)
    if layout == "all_short":
        return [1, 7, 4097, 45663, B - 3, B]
    if layout == "all_long":
        return [B + 1, B + 8199, 2 * B + 5]
    mixed = [B + 1, 3, B, 2 * B + 5, 65, B + 8199, 4097]  # long first, short last
    return mixed if layout == "mixed" else mixed[::-1]


def _exact_kinds(dt: str, sizes) -> int:
    B = _bound(dt)
    return (SHORT if min(sizes) <= B else 0) | (LONG if max(sizes) > B else 0)


@functools.lru_cache(maxsize=None)
def _case(dt: str, layout, data: str):
    """(tensors, torch's norms) of one (dtype, layout, data): computed once per module, never modified. layout is
    a name of LAYOUTS or a tuple of sizes."""
    sizes = _sizes(dt, layout) if isinstance(layout, str) else list(layout)
    seed = [list(DTYPES).index(dt), len(sizes), sizes[0] % 1000, sizes[-1] % 1000, int(data == "ints")]
    rng = np.random.default_rng(seed)
    xs = [_data(data, n, rng, DTYPES[dt]) for n in sizes]
    want = np.array([_torch_norm(x, THREADS) for x in xs], np.float64)
    return xs, want


def _bucket(xs, align, dtype):
    lay = ops.BucketLayout([x.numel() for x in xs], align=align)
    flat = torch.zeros(lay.total, dtype=dtype)
    for x, o in zip(xs, lay.offsets):
        flat[o:o + x.numel()] = x
    return lay, flat.to(DEV)


def _need(lay) -> int:
    return int(_lib.load().adfl_torch_norm_scratch_bytes(lay.nchunks, lay.ntensors))


def _call(dt, lay, flat, *, kinds, use_list, scratch=None, out64=True, out32=True, extra=0, threads=THREADS):
    """One call of adfl_torch_norms (use_list False: NULL list) or adfl_torch_norms_work (the layout's device
    list) straight through the library: (status, norms64 or None, norms32 or None) as numpy arrays of
    ntensors + extra slots, every slot pre-filled with the sentinel; read back after a device synchronize."""
    L = _lib.load()
    need = _need(lay)
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=DEV)
    assert scratch.numel() >= need and scratch.data_ptr() % 256 == 0
    nt = lay.ntensors
    o64 = torch.full((nt + extra,), SENTINEL, dtype=torch.float64, device=DEV) if out64 else None
    o32 = torch.full((nt + extra,), SENTINEL, dtype=torch.float32, device=DEV) if out32 else None
    p64 = o64.data_ptr() if out64 else None
    p32 = o32.data_ptr() if out32 else None
    chunks = lay.device_chunks(DEV).data_ptr()
    stream = torch.cuda.current_stream(DEV).cuda_stream
    if use_list:
        st = L.adfl_torch_norms_work(IDS[dt], flat.data_ptr(), chunks, lay.nchunks, lay.device_tfirst(DEV).data_ptr(), nt,
                                     kinds, threads, scratch.data_ptr(), need, p64, p32, stream)
    else:
        st = L.adfl_torch_norms(IDS[dt], flat.data_ptr(), chunks, lay.nchunks, nt, kinds, threads, scratch.data_ptr(),
                                need, p64, p32, stream)
    torch.cuda.synchronize()
    return st, (o64.cpu().numpy() if out64 else None), (o32.cpu().numpy() if out32 else None)


def _check(tag, want, g64, g32, named=None):
    """Every named tensor (default: all) holds torch's value in the outputs given; every other one a NaN."""
    for i, w in enumerate(want):
        if named is not None and not named[i]:
            w = float("nan")
        if g64 is not None:
            assert _same(float(g64[i]), float(w)), (tag, "norms64", i, float(g64[i]), float(w))
        if g32 is not None:
            assert _same(float(g32[i]), float(np.float32(w))), (tag, "norms32", i, float(g32[i]), float(np.float32(w)))


# 1. the entry with no list (k_tn_tfirst builds it in scratch), 2. the entry with the caller's list
@pytest.mark.parametrize("data", ["grad", "ints"])
@pytest.mark.parametrize("align", [1, 64])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dt", list(DTYPES))
def test_torch_norms_no_list_entry(dt, layout, align, data):
    xs, want = _case(dt, layout, data)
    lay, flat = _bucket(xs, align, DTYPES[dt])
    exact = _exact_kinds(dt, lay.sizes)
    for kinds in (exact, 0):
        st, g64, g32 = _call(dt, lay, flat, kinds=kinds, use_list=False)
        assert st == 0, (dt, layout, kinds, st)
        _check((dt, layout, align, data, kinds), want, g64, g32)
    st, g64, _ = _call(dt, lay, flat, kinds=exact, use_list=False, out32=False)
    assert st == 0
    _check((dt, layout, align, data, "norms64 only"), want, g64, None)
    st, _, g32 = _call(dt, lay, flat, kinds=exact, use_list=False, out64=False)
    assert st == 0
    _check((dt, layout, align, data, "norms32 only"), want, None, g32)


@pytest.mark.parametrize("data", ["grad", "ints"])
@pytest.mark.parametrize("align", [1, 64])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dt", list(DTYPES))
def test_torch_norms_list_entry_agrees(dt, layout, align, data):
    xs, want = _case(dt, layout, data)
    lay, flat = _bucket(xs, align, DTYPES[dt])
    st, g64, g32 = _call(dt, lay, flat, kinds=0, use_list=True)
    assert st == 0
    _check((dt, layout, align, data, "list"), want, g64, g32)
    st, g64, _ = _call(dt, lay, flat, kinds=0, use_list=True, out32=False)
    assert st == 0
    _check((dt, layout, align, data, "list, norms64 only"), want, g64, None)
    st, _, g32 = _call(dt, lay, flat, kinds=0, use_list=True, out64=False)
    assert st == 0
    _check((dt, layout, align, data, "list, norms32 only"), want, None, g32)


# 3. a hint never drops a tensor: the ones it names get torch's value, the others a quiet NaN, none is unwritten
HINTS = [("all_short", LONG), ("all_long", SHORT), ("mixed", SHORT), ("mixed", LONG), ("mixed_rev", SHORT),
         ("mixed_rev", LONG)]


def _check_hint(tag, dt, lay, flat, want, kinds, use_list):
    st, g64, g32 = _call(dt, lay, flat, kinds=kinds, use_list=use_list)
    print(tag, "status", st, "norms64", g64.tolist(), "norms32", g32.tolist())
    assert st == 0, (tag, st)
    assert not (g64 == SENTINEL).any() and not (g32 == SENTINEL).any(), (tag, "a slot was never written", g64, g32)
    B = _bound(dt)
    named = [(n <= B and kinds & SHORT) or (n > B and kinds & LONG) for n in lay.sizes]
    _check(tag, want, g64, g32, named)


@pytest.mark.parametrize("use_list", [False, True])
@pytest.mark.parametrize("layout,kinds", HINTS)
@pytest.mark.parametrize("dt", list(DTYPES))
def test_torch_norms_hint_never_drops_a_tensor(dt, layout, kinds, use_list):
    xs, want = _case(dt, layout, "grad")
    lay, flat = _bucket(xs, 1, DTYPES[dt])
    _check_hint((dt, layout, kinds, use_list), dt, lay, flat, want, kinds, use_list)


@pytest.mark.parametrize("use_list", [False, True])
def test_torch_norms_hint_sized_by_the_old_bound(use_list):
    """A caller that still sizes fp32's `kinds` by adfl_torch_norm_short_max() (2^16, the fp16 / fp64 bound) names
    tensors of (2^16, 2^19] long; they are short: NaN for each, never a stale slot."""
    old = int(_lib.load().adfl_torch_norm_short_max())
    sizes = (70_000, 300_000, 524_288)
    assert old < min(sizes) and max(sizes) <= _bound("f32")
    xs, want = _case("f32", sizes, "grad")
    lay, flat = _bucket(xs, 1, torch.float32)
    kinds = (SHORT if min(sizes) <= old else 0) | (LONG if max(sizes) > old else 0)
    assert kinds == LONG
    _check_hint(("f32", "old bound", use_list), "f32", lay, flat, want, kinds, use_list)


# 4. invalid hints
@pytest.mark.parametrize("kinds", [4, 8, 7, -1])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_torch_norms_rejects_invalid_hints(dt, kinds):
    xs, _ = _case(dt, (7, 4097, 45663), "grad")
    lay, flat = _bucket(xs, 1, DTYPES[dt])
    for use_list in (False, True):
        st, g64, g32 = _call(dt, lay, flat, kinds=kinds, use_list=use_list)  # (synchronizes before reading)
        print(dt, kinds, use_list, "status", st, g64.tolist(), g32.tolist())
        assert st == E_ARG, (dt, kinds, use_list, st)
        assert (g64 == SENTINEL).all() and (g32 == SENTINEL).all(), (dt, kinds, use_list, g64, g32)


# 5. d_scratch needs no initialisation
@pytest.mark.parametrize("dt", list(DTYPES))
def test_torch_norms_scratch_needs_no_initialisation(dt):
    xs, want = _case(dt, "mixed", "grad")
    lay, flat = _bucket(xs, 1, DTYPES[dt])
    need = _need(lay)
    buf = torch.empty(need + 512, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 256 == 0
    canary = torch.from_numpy(np.random.default_rng(77).integers(0, 256, 512, dtype=np.uint8))
    kinds = _exact_kinds(dt, lay.sizes)

    def run(tag):
        buf[need:] = canary.to(DEV)
        st, g64, g32 = _call(dt, lay, flat, kinds=kinds, use_list=False, scratch=buf, extra=2)
        assert st == 0, (dt, tag, st)
        _check((dt, tag), want, g64, g32)
        assert (g64[-2:] == SENTINEL).all() and (g32[-2:] == SENTINEL).all(), (dt, tag, "wrote past ntensors")
        assert torch.equal(buf[need:].cpu(), canary), (dt, tag, "wrote past the scratch size")

    buf[:need] = 0
    run("zeros")
    buf[:need] = 0xFF  # NaN doubles, -1 ints
    run("ones")
    g = torch.Generator().manual_seed(1234)
    buf[:need] = torch.randint(0, 256, (need,), dtype=torch.uint8, generator=g).to(DEV)
    run("random")
    xs2, want2 = _case(dt, "all_long", "grad")  # then what another layout's run leaves behind
    lay2, flat2 = _bucket(xs2, 1, DTYPES[dt])
    assert _need(lay2) <= need
    st, g64, g32 = _call(dt, lay2, flat2, kinds=LONG, use_list=False, scratch=buf)
    assert st == 0
    _check((dt, "all_long into the shared scratch"), want2, g64, g32)
    run("after all_long")


# 6. edges of the count arguments
@pytest.mark.parametrize("dt", list(DTYPES))
def test_torch_norms_every_tensor_one_chunk(dt):
    sizes = (1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 4097, 8191, 8192)
    xs, want = _case(dt, sizes, "ints")
    for align in (1, 64):
        lay, flat = _bucket(xs, align, DTYPES[dt])
        assert lay.ntensors == lay.nchunks
        for kinds in (SHORT, 0):
            for use_list in (False, True):
                st, g64, g32 = _call(dt, lay, flat, kinds=kinds, use_list=use_list)
                assert st == 0
                _check((dt, align, kinds, use_list), want, g64, g32)


@pytest.mark.parametrize("long_", [False, True])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_torch_norms_one_tensor(dt, long_):
    n = _bound(dt) + 8199 if long_ else 45663
    xs, want = _case(dt, (n,), "grad")
    lay, flat = _bucket(xs, 1, DTYPES[dt])
    assert lay.ntensors == 1
    for kinds in (LONG if long_ else SHORT, 0):
        for use_list in (False, True):
            st, g64, g32 = _call(dt, lay, flat, kinds=kinds, use_list=use_list)
            assert st == 0
            _check((dt, n, kinds, use_list), want, g64, g32)


# 7. the Python wrapper
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("threads", [0, -3])
def test_reference_norms_rejects_threads_below_one(dt, threads):
    lay = ops.BucketLayout([100], align=1)
    x = torch.zeros(100, dtype=DTYPES[dt], device=DEV)
    with pytest.raises(ValueError, match="threads"):
        stoch.reference_norms(x, lay, threads=threads)
