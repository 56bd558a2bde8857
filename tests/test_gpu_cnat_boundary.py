"""GPU: every CNAT route, in fp32 / fp16 / bf16 / fp64, over the band tensors of tests/cnat_boundary_cases.py, against
the executed reference's recorded bytes and decoded floats (tests/golden/cnat_boundary.npz). Every comparison is
exact: bytes as bytes, fp32 by bit pattern with NaN by position. Only the Philox-drawn uniforms have no recorded
counterpart: there the oracles (pinned to the fixture by tests/test_cnat_boundary_golden.py) stand in.

The tensors place v = R(|x| + eps) on every power of two of every dtype, on each edge of the band in which
fl(log2 v) is an integer and on both sides of it, with u on prob and one grid step to either side. For fp32 the
same elements come three times: `inside` the fast form's flag window (every wave takes the exact form), `outside`
it (the fast form decides alone, up to 64 ulps from the power of two) and `mixed`. The compact layouts put every
tensor at each offset residue mod the vector width, so the same elements move between vector groups and chunk heads
/ tails; a 65,537-element filler in the fp32 bucket forces the multi-launch kernels.
"""

import json

import numpy as np
import pytest
import torch

import boundary_cases as bc
import cnat_boundary_cases as cb
import stoch_dt_oracle as do
import stoch_oracle as so
from golden_util import f32_from_bits

pytestmark = pytest.mark.gpu

import adfl_amd  # noqa: E402,F401
from adfl_amd import ops, stoch  # noqa: E402
from adfl_amd.Channel import CNATChannel  # noqa: E402

DEV = torch.device("cuda", 0)
F32 = np.float32
FILLER_N = 65537          # one element over the resident bound: the layout has no work list
RESIDENT_MAX = 65536      # a tensor of up to 8 chunks fits the one-launch form
SEED, COUNTER = 0x5EEDC4A7, 13
TDT = {cb.F32N: torch.float32, cb.F16N: torch.float16, cb.BF16N: torch.bfloat16, cb.F64N: torch.float64}
VEC = {cb.F32N: 4, cb.F16N: 8, cb.BF16N: 8, cb.F64N: 2}    # elements per 16-byte vector

with open(cb.MANIFEST) as _f:
    MAN = json.load(_f)
ENC = {(c["dtype"], c["tensor"], c["bits"]): c for c in MAN["encode"]}
_fix = {}


def fixture():
    if "g" not in _fix:
        _fix["g"] = np.load(cb.FIXTURE)
        r = np.random.default_rng(78)
        _fix["filler"] = r.standard_normal(FILLER_N, dtype=np.float32)
        _fix["filler_u"] = r.random(FILLER_N, dtype=np.float32)
    return _fix["g"]


def scale_of(rec) -> float:
    return float(np.array([rec["scale"]["f64_bits"]], dtype=np.uint64).view(np.float64)[0])


class Want:
    """A tensor with the reference's recorded output at one bit width, in the tensor's order."""

    def __init__(self, dtn, name, bits):
        g = fixture()
        self.t = t = cb.tensor(dtn, name)
        self.dtn, self.bits = dtn, bits
        rec = ENC[(dtn, name, bits)]
        src = "mixed" if t.src is not None else name      # inside / outside: mixed's elements, mixed's record
        assert cb.tensor(dtn, src).digest() == MAN["tensors"][dtn][src]["inputs_sha256"]
        self.e, self.signs = cb.recorded(g, dtn, name, bits)
        self.scale = scale_of(rec)
        self.tag = cb.case_name(dtn, name, bits)


def to_torch(raw, dtn):
    raw = np.ascontiguousarray(raw).reshape(-1)
    if raw.dtype == np.uint16:
        return torch.from_numpy(raw.view(np.int16).copy()).view(TDT[dtn])
    return torch.from_numpy(raw.copy())


def dev(a, dtn=cb.F32N):
    return to_torch(a, dtn).to(DEV)


def same_float(a: float, b: float) -> bool:
    return a == b or (np.isnan(a) and np.isnan(b))


def assert_bytes(want, ex, sg, route, where="", lo=0, hi=None):
    """Exponent and sign bytes of one copy (or the piece [lo, hi) of one) against the reference's."""
    t = want.t
    ex, sg = np.asarray(ex).view(np.int8), np.asarray(sg).view(np.int8)
    we, ws = want.e[lo:hi], want.signs[lo:hi]
    bad = cb.first_diffs(ex, we)
    assert bad.size == 0, (f"{want.tag} {route} {where}: exponents differ at",
                           [(t.describe(lo + int(i)), f"got {ex[i]} want {we[i]}") for i in bad])
    bad = cb.first_diffs(sg, ws)
    assert bad.size == 0, (f"{want.tag} {route} {where}: signs differ at", [t.describe(lo + int(i)) for i in bad])


def oracle_bytes(dtn, raw_x, bits, raw_u):
    e, s = cb.quantize(raw_x, dtn, bits, raw_u)
    return e.view(np.int8), s


class Bucket:
    """Copies of one tensor (and its uniforms) in a bucket of its dtype: aligned (one copy), or compact with small
    separators that put the copies at offsets of every residue mod the vector width. A copy longer than the
    resident bound goes in as two tensors (CNAT's bytes are element-wise), so that an fp32 layout keeps its work
    list; `filler` appends the 65,537-element tensor, which takes it away. pieces: (tensor index, lo, hi) of every
    piece of a copy; the other tensors are checked against the oracle."""

    def __init__(self, t, compact, filler=False, split=True):
        dtn, n, v = t.dtn, t.n, VEC[t.dtn]
        fixture()
        rt = cb.raw_type(dtn)
        parts, us, self.pieces, firsts = [], [], [], []
        cuts = [0, n] if n <= RESIDENT_MAX or not split else [0, n // 2 + 1, n]
        r = np.random.default_rng(n)
        ncopy = v if compact else 1
        sep = (1 - n) % v or v
        for j in range(ncopy):
            firsts.append(len(parts))
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                self.pieces.append((len(parts), lo, hi))
                parts.append(t.x[lo:hi])
                us.append(t.u[lo:hi])
            if j < ncopy - 1:
                parts.append(cb.from_compute(r.standard_normal(sep).astype(cb.ctype(dtn)), dtn).astype(rt))
                us.append(cb.from_compute((r.integers(0, 256, sep) / 256.0).astype(cb.ctype(dtn)), dtn).astype(rt))
        if filler:
            parts.append(_fix["filler"])
            us.append(_fix["filler_u"])
        self.dtn, self.parts, self.us = dtn, parts, us
        self.lay = lay = ops.BucketLayout([p.size for p in parts], align=1 if compact else 64)
        if compact:
            assert sorted(int(lay.offsets[i]) % v for i in firsts) == list(range(v))
        x, u = np.zeros(lay.total, rt), np.zeros(lay.total, rt)
        for o, p, uu in zip(lay.offsets.tolist(), parts, us):
            x[o:o + p.size], u[o:o + p.size] = p, uu
        self.x, self.u = dev(x, dtn), dev(u, dtn)

    def slices(self, plane):
        a = plane.cpu().numpy()
        return [a[o:o + n] for o, n in zip(self.lay.offsets.tolist(), self.lay.sizes.tolist())]

    def check(self, want, ex, sg, route):
        torch.cuda.synchronize()
        exs, sgs = self.slices(ex), self.slices(sg)
        piece = {i: (lo, hi) for i, lo, hi in self.pieces}
        for i, (p, uu) in enumerate(zip(self.parts, self.us)):
            where = f"tensor {i} at offset {int(self.lay.offsets[i])}"
            if i in piece:
                assert_bytes(want, exs[i], sgs[i], route, where, *piece[i])
            else:
                e, s = oracle_bytes(self.dtn, p, want.bits, uu)
                assert np.array_equal(exs[i].view(np.int8), e) and np.array_equal(sgs[i], s), (route, where)


# ------------------------------------------------------------------------------------------------
# fp32 encode
# ------------------------------------------------------------------------------------------------
F32_CASES = [c for c in cb.ENC_CASES if c[0] == cb.F32N]
F32_IDS = [cb.case_name(*c) for c in F32_CASES]
DT_CASES = [c for c in cb.ENC_CASES if c[0] != cb.F32N]
DT_IDS = [cb.case_name(*c) for c in DT_CASES]
ALL_IDS = [cb.case_name(*c) for c in cb.ENC_CASES]
BATCHED_ROUTES = [(compact, filler) for compact in (False, True) for filler in (False, True)]


@pytest.mark.parametrize("compact,filler", BATCHED_ROUTES,
                         ids=[f"{'compact' if c else 'aligned'}-{'multilaunch' if f else 'resident'}"
                              for c, f in BATCHED_ROUTES])
@pytest.mark.parametrize("dtn,name,bits", F32_CASES, ids=F32_IDS)
def test_cnat_encode_batched_injected_uniforms(dtn, name, bits, compact, filler):
    """One launch (the layout's resident work list) and the multi-launch kernels (no work list: lay.nwork == 0)."""
    want = Want(dtn, name, bits)
    b = Bucket(want.t, compact, filler)
    assert (b.lay.nwork == 0) == filler                     # which form the encode runs
    ex, sg, _ = stoch.cnat_encode_batched(b.x, b.lay, bits, uniforms=b.u)
    b.check(want, ex, sg, f"cnat_encode_batched nwork={b.lay.nwork}")


F32_TENSORS = [(cb.F32N, n) for n in cb.TENSOR_NAMES[cb.F32N]]


@pytest.mark.parametrize("dtn,name", F32_TENSORS, ids=[n for _, n in F32_TENSORS])
def test_cnat_encode_batched_with_the_references_norm(dtn, name):
    """torch_norm=True on the whole tensor: the bytes again, and the norm is the recorded scale (inf for the band
    tensors, whose squares overflow; NaN for `special`)."""
    want = Want(dtn, name, 8)
    b = Bucket(want.t, False, split=False)
    ex, sg, nr = stoch.cnat_encode_batched(b.x, b.lay, 8, uniforms=b.u, torch_norm=True)
    b.check(want, ex, sg, "cnat_encode_batched torch_norm")
    got = float(nr.cpu().numpy()[0])
    assert same_float(got, float(F32(want.scale))), (want.tag, got, want.scale)


@pytest.mark.parametrize("dtn,name,bits", cb.ENC_CASES, ids=ALL_IDS)
def test_channel_end_to_end(dtn, name, bits):
    """CNATChannel(bits) with the reference's constructor on the tensor in its dtype, only the uniforms injected:
    exponents, signs and the scale are the reference's."""
    want = Want(dtn, name, bits)
    t = want.t
    ch = CNATChannel(bits)
    qp = ch._quantize_params({"w": to_torch(t.x, dtn).reshape(1, -1)}, bits, uniforms=dev(t.u, dtn))
    p = qp.params["w"]
    assert p.data.dtype == torch.int8 and p.signs.dtype == torch.int8 and tuple(p.data.shape) == (1, t.n)
    assert_bytes(want, p.data.numpy().reshape(-1), p.signs.numpy().reshape(-1), "CNATChannel._quantize_params")
    assert isinstance(p.scale, float) and same_float(p.scale, want.scale), (want.tag, p.scale, want.scale)


@pytest.mark.parametrize("dtn,name,bits", F32_CASES, ids=F32_IDS)
def test_channel_delta_route(dtn, name, bits):
    """send_delta's encode with new = x, prev = +0: the difference x - 0 is x bit for bit (-0 stays -0)."""
    want = Want(dtn, name, bits)
    t = want.t
    x = dev(t.x).reshape(1, -1)
    qp = CNATChannel(bits)._quantize_delta({"w": torch.zeros_like(x)}, {"w": x}, bits, uniforms=dev(t.u))
    p = qp.params["w"]
    ex, sg = p.data.cpu().numpy().reshape(-1), p.signs.cpu().numpy().reshape(-1)
    assert_bytes(want, ex, sg, "CNATChannel._quantize_delta")
    assert isinstance(p.scale, float) and same_float(p.scale, want.scale), (want.tag, p.scale, want.scale)


@pytest.mark.parametrize("dtn,name", F32_TENSORS, ids=[n for _, n in F32_TENSORS])
def test_cnat_encode_batched_seeded(dtn, name):
    """Philox uniforms (SEED, COUNTER): only the x side of each band is placed; against so.cnat_quantize on
    so.philox_uniforms, resident (a long tensor goes in as two) and multi-launch."""
    t = cb.tensor(dtn, name)
    b = Bucket(t, False)
    assert b.lay.nwork > 0
    for bits in (8, 9):
        for resident in (None, False):
            ex, sg, _ = stoch.cnat_encode_batched(b.x, b.lay, bits, seed=SEED, counter=COUNTER, resident=resident)
            torch.cuda.synchronize()
            exs, sgs = b.slices(ex), b.slices(sg)
            for i, lo, hi in b.pieces:
                o = int(b.lay.offsets[i])
                e, s = so.cnat_quantize(t.x[lo:hi], bits, 1.0, so.philox_uniforms(hi - lo, SEED, COUNTER, o))
                bad = cb.first_diffs(exs[i], e)
                assert bad.size == 0, (f"{dtn} {name} b{bits} seeded resident={resident}: exponents differ at",
                                       [(t.describe(lo + int(j)), f"got {exs[i][j]} want {e[j]}") for j in bad])
                assert np.array_equal(sgs[i], s)


# ------------------------------------------------------------------------------------------------
# fp16 / bf16 / fp64 encode
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compact", [False, True], ids=["aligned", "compact"])
@pytest.mark.parametrize("dtn,name,bits", DT_CASES, ids=DT_IDS)
def test_dt_quantize_and_encode_batched_injected_uniforms(dtn, name, bits, compact):
    """quantize_batched_dt with the recorded norm and encode_batched_dt (the read-once kernel) over one bucket;
    compact: a copy at every offset residue mod the vector width (scalar head, whole vectors, tail)."""
    want = Want(dtn, name, bits)
    b = Bucket(want.t, compact, split=False)
    own = {i for i, _, _ in b.pieces}
    norms = [want.scale if i in own else 1.0 for i in range(len(b.parts))]
    norms = torch.tensor(norms, dtype=torch.float64, device=DEV)
    ex, sg = stoch.quantize_batched_dt("cnat", b.x, b.lay, bits, norms, uniforms=b.u)
    b.check(want, ex, sg, "quantize_batched_dt")
    ex, sg, _, _ = stoch.encode_batched_dt("cnat", b.x, b.lay, bits, uniforms=b.u)
    b.check(want, ex, sg, "encode_batched_dt")


DT_TENSORS = [(dtn, n) for dtn in cb.DTYPES[1:] for n in cb.TENSOR_NAMES[dtn] if n != "sub"]


@pytest.mark.parametrize("dtn,name", DT_TENSORS, ids=[f"{d}-{n}" for d, n in DT_TENSORS])
def test_dt_encode_batched_seeded(dtn, name):
    t = cb.tensor(dtn, name)
    lay = ops.BucketLayout([t.n], align=1)
    u = do.philox_uniforms_dt(cb.DT[dtn], t.n, SEED, COUNTER)
    for bits in (8, 9):
        ex, sg, _, _ = stoch.encode_batched_dt("cnat", dev(t.x, dtn), lay, bits, seed=SEED, counter=COUNTER)
        torch.cuda.synchronize()
        ex, sg = ex.cpu().numpy(), sg.cpu().numpy()
        e, s = oracle_bytes(dtn, t.x, bits, u)
        bad = cb.first_diffs(ex, e)
        assert bad.size == 0, (f"{dtn} {name} b{bits} seeded: exponents differ at",
                               [(t.describe(int(j)), f"got {ex[j]} want {e[j]}") for j in bad])
        assert np.array_equal(sg, s)


# ------------------------------------------------------------------------------------------------
# decode
# ------------------------------------------------------------------------------------------------
DEC_TILE = 3              # 2304 elements: two 1024-element wave tiles and a dword remainder ...
DEC_TAIL = 7              # ... then a ragged tail: edge elements
DEC = {d["norm_id"]: d for d in MAN["decode"]}
DEC_EXPS = bc.DEC_LEVELS.view(np.int8)


class DecodeBucket:
    """[the case's tensor, a tensor with norm 0, one with a NaN norm, the case's tensor again] packed back to back:
    with 2311 elements each the two copies sit at offsets 0 and 6933 (residues 0 and 1 mod 4), beside the
    per-tensor branches (norm == 0, NaN)."""

    def __init__(self, nid):
        rec = DEC[nid]
        norm = f32_from_bits(rec["norm_bits"])
        ex = np.concatenate([np.tile(DEC_EXPS, DEC_TILE), DEC_EXPS[-DEC_TAIL:]])
        sg = np.concatenate([np.tile(bc.DEC_SIGNS, DEC_TILE), bc.DEC_SIGNS[-DEC_TAIL:]])
        self.ex1, self.sg1, n = ex, sg, ex.size
        self.lay = lay = ops.BucketLayout([n] * 4, align=1)
        assert [int(o) % 4 for o in lay.offsets] == [0, 3, 2, 1]
        self.norms = np.array([norm, 0.0, np.nan, norm], F32)
        one = fixture()[rec["name"] + "__deq"]                       # the reference's output
        ref = np.concatenate([np.tile(one, DEC_TILE), one[-DEC_TAIL:]])
        self.want = [ref, so.cnat_dequantize(ex, sg, F32(0)), so.cnat_dequantize(ex, sg, F32(np.nan)), ref]
        assert not self.want[1].any() and np.isnan(self.want[2]).all()
        self.ex, self.sg = dev(np.tile(ex, 4)), dev(np.tile(sg, 4))
        self.tag = f"cnat decode norm={nid}"

    def check(self, outs, route, want=None):
        torch.cuda.synchronize()
        for t, (got, w) in enumerate(zip(outs, want or self.want)):
            got = got.cpu().numpy()
            bad = cb.first_diffs(got, w)
            assert bad.size == 0, (f"{self.tag} {route} tensor {t} at offset {int(self.lay.offsets[t])} (norm "
                                   f"{self.norms[t]!r}): differs at",
                                   [(f"exponent byte {int(self.ex1[i])} sign {int(self.sg1[i])}", got[i], w[i])
                                    for i in bad])

    def split(self, out):
        return [out[o:o + n] for o, n in zip(self.lay.offsets.tolist(), self.lay.sizes.tolist())]


@pytest.mark.parametrize("nid", list(cb.DEC_NORMS))
def test_cnat_decode_batched_of_every_exponent_byte(nid):
    b = DecodeBucket(nid)
    out = stoch.cnat_decode_batched(b.ex, b.sg, dev(b.norms), b.lay)
    b.check(b.split(out), "cnat_decode_batched")


@pytest.mark.parametrize("nid", list(cb.DEC_NORMS))
def test_dequantize_axpby_scale_mode_keeps_the_decodes_bits(nid):
    """SCALE mode with beta = 1: fp32(1 * d) is d, so the output bits are the decode's."""
    b = DecodeBucket(nid)
    outs = [torch.full((int(n),), 7.0, device=DEV) for n in b.lay.sizes]
    stoch.dequantize_axpby_batched("cnat", b.ex, b.sg, dev(b.norms), b.lay, 8, None, [outs], 0.0, 1.0)
    b.check(outs, "dequantize_axpby_batched SCALE beta=1")


@pytest.mark.parametrize("nid", list(cb.DEC_NORMS))
def test_dequantize_mean_of_one_client_keeps_the_decodes_bits(nid):
    """K = 1 against the reference's recorded simple_aggregate of that one decode: the decode's floats, except that
    the sum's start from +0 turns a -0 decode into +0 (tests/test_cnat_boundary_golden.py reads that off the
    record)."""
    b = DecodeBucket(nid)
    row = -(-b.lay.total // 16) * 16
    ex, sg = torch.zeros(1, row, dtype=torch.int8, device=DEV), torch.ones(1, row, dtype=torch.int8, device=DEV)
    ex[0, :b.lay.total], sg[0, :b.lay.total] = b.ex, b.sg
    out = stoch.dequantize_mean_batched("cnat", ex, sg, dev(b.norms).reshape(1, -1), b.lay, 8)
    one = fixture()[DEC[nid]["name"] + "__mean"]
    ref = np.concatenate([np.tile(one, DEC_TILE), one[-DEC_TAIL:]])
    with np.errstate(invalid="ignore"):
        want = [ref, F32(0) + b.want[1], F32(0) + b.want[2], ref]
    b.check(b.split(out), "dequantize_mean_batched K=1", want)
