"""GPU: every QSGD / RQSGD fp32 route over the boundary tensors of tests/boundary_cases.py, against the executed
reference's recorded bytes and decoded floats (tests/golden/stoch_boundary.npz). Every comparison is exact: bytes as
bytes, fp32 by bit pattern with NaN by position. Only the Philox-drawn uniforms of the straddling path have no
recorded counterpart: there the oracle (pinned to the fixture by tests/test_stoch_boundary_golden.py) stands in.

The tensors place inputs where the fast form of the level rule and of the decode (csrc/stoch_device.h: a
per-tensor reciprocal with one correction step, valid inside [2^-60, 2^60]) can differ from the exact form: scaled
on an integer and one ulp to either side, u == prob and its neighbours, the window's edges, waves in which only
some lanes flag, levels that wrap through the u8 conversion, and quotients that are denormal ties. The compact
layouts put every tensor at each offset residue mod 4, so the same elements move between 4-element groups (fast
form) and chunk heads / tails (exact form); a 65,537-element filler in the bucket forces the multi-launch kernels.
"""

import json

import numpy as np
import pytest
import torch

import boundary_cases as bc
import stoch_oracle as so
from golden_util import f32_from_bits, same_f32

pytestmark = pytest.mark.gpu

import adfl_amd  # noqa: E402,F401
from adfl_amd import ops, stoch  # noqa: E402

DEV = torch.device("cuda", 0)
F32 = np.float32
FILLER_N = 65537          # one element over the resident bound: the layout has no work list
SEED, COUNTER = 0x5EEDB0DA, 11

with open(bc.MANIFEST) as _f:
    MAN = json.load(_f)
ENC = {(c["bits"], c["norm_id"]): c for c in MAN["encode"]}
DEC = {(c["bits"], c["norm_id"]): c for c in MAN["decode"]}
_fix = {}


def fixture():
    if "g" not in _fix:
        _fix["g"] = np.load(bc.FIXTURE)
        r = np.random.default_rng(77)
        _fix["filler"] = r.standard_normal(FILLER_N, dtype=np.float32)
        _fix["filler_u"] = r.random(FILLER_N, dtype=np.float32)
    return _fix["g"]


class Want:
    """An encode case with the reference's recorded output in the tensor's order."""

    def __init__(self, bits, nid):
        g = fixture()
        self.case = c = bc.encode_case(bits, nid)
        rec = ENC[(bits, nid)]
        assert bc.digest_inputs(c) == rec["inputs_sha256"]
        self.q, self.signs = c.shuffle(g[rec["name"] + "__q"]), c.shuffle(g[rec["name"] + "__signs"])
        self.deq = c.shuffle(g[rec["name"] + "__deq"])
        self.norm, self.min = f32_from_bits(rec["norm_bits"]), f32_from_bits(rec["min_bits"])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def assert_bytes(want, lv, sg, route, where=""):
    """Level and sign bytes of one copy of the case's tensor against the reference's."""
    c = want.case
    lv, sg = np.asarray(lv).view(np.uint8), np.asarray(sg).view(np.int8)
    bad = bc.first_diffs(lv, want.q)
    assert bad.size == 0, (f"b{c.bits} {c.nid} {route} {where}: levels differ at",
                           [(c.describe(int(i)), f"got {lv[i]} want {want.q[i]}") for i in bad])
    bad = bc.first_diffs(sg, want.signs)
    assert bad.size == 0, (f"b{c.bits} {c.nid} {route} {where}: signs differ at", [c.describe(int(i)) for i in bad])


def assert_scales(want, nr, mn, route):
    c = want.case
    assert same_f32(nr, want.norm) and same_f32(mn, want.min), (f"b{c.bits} {c.nid} {route}", nr, mn)


class Bucket:
    """Copies of one case's tensor (and its uniforms) in a bucket: aligned (one copy), or compact with small
    separators that put the four copies at offsets of every residue mod 4; `filler` appends the 65,537-element
    tensor. others: the tensors that are not copies (checked against the oracle)."""

    def __init__(self, case, compact, filler):
        n = case.n
        fixture()
        parts, us, self.copies = [], [], []
        if compact:
            sep = (1 - n) % 4 or 4
            r = np.random.default_rng(n)
            for j in range(4):
                self.copies.append(len(parts))
                parts.append(case.x)
                us.append(case.u)
                if j < 3:
                    parts.append(r.standard_normal(sep, dtype=np.float32))
                    us.append(r.random(sep, dtype=np.float32))
        else:
            self.copies.append(0)
            parts.append(case.x)
            us.append(case.u)
        if filler:
            parts.append(_fix["filler"])
            us.append(_fix["filler_u"])
        self.parts, self.us = parts, us
        self.lay = lay = ops.BucketLayout([p.size for p in parts], align=1 if compact else 64)
        if compact:
            assert sorted(int(lay.offsets[t]) % 4 for t in self.copies) == [0, 1, 2, 3]
        assert (lay.nwork == 0) == filler                     # which form an encode with a work list runs
        x, u = np.zeros(lay.total, F32), np.zeros(lay.total, F32)
        for o, p, uu in zip(lay.offsets.tolist(), parts, us):
            x[o:o + p.size], u[o:o + p.size] = p, uu
        self.x, self.u = dev(x), dev(u)

    def slices(self, plane):
        a = plane.cpu().numpy()
        return [a[o:o + n] for o, n in zip(self.lay.offsets.tolist(), self.lay.sizes.tolist())]

    def check(self, want, lv, sg, route, nr=None, mn=None):
        torch.cuda.synchronize()
        lvs, sgs = self.slices(lv), self.slices(sg)
        nr = None if nr is None else nr.cpu().numpy()
        mn = None if mn is None else mn.cpu().numpy()
        for t, (p, uu) in enumerate(zip(self.parts, self.us)):
            where = f"tensor {t} at offset {int(self.lay.offsets[t])}"
            if t in self.copies:
                assert_bytes(want, lvs[t], sgs[t], route, where)
                if nr is not None:
                    assert_scales(want, nr[t], mn[t], route)
            else:
                q, s = so.qsgd_quantize(p, want.case.s, so.linf_norm(p), uu)
                assert np.array_equal(lvs[t], q) and np.array_equal(sgs[t], s), (route, where)


ENC_IDS = [f"b{b}-{n}" for b, n in bc.ENC_CASES]
BATCHED_ROUTES = [(compact, filler) for compact in (False, True) for filler in (False, True)]


@pytest.mark.parametrize("compact,filler", BATCHED_ROUTES,
                         ids=[f"{'compact' if c else 'aligned'}-{'twopass' if f else 'resident'}"
                              for c, f in BATCHED_ROUTES])
@pytest.mark.parametrize("bits,nid", bc.ENC_CASES, ids=ENC_IDS)
def test_rqsgd_encode_batched_injected_uniforms(bits, nid, compact, filler):
    """One launch (the layout's resident work list) and the three launches (no work list: lay.nwork == 0)."""
    want = Want(bits, nid)
    b = Bucket(want.case, compact, filler)
    lv, sg, nr, mn = stoch.rqsgd_encode_batched(b.x, b.lay, bits, uniforms=b.u)
    b.check(want, lv, sg, f"rqsgd_encode_batched nwork={b.lay.nwork}", nr, mn)


@pytest.mark.parametrize("compact", [False, True], ids=["aligned", "compact"])
@pytest.mark.parametrize("bits,nid", bc.ENC_CASES, ids=ENC_IDS)
def test_qsgd_quantize_batched_with_the_fixture_norm(bits, nid, compact):
    """The level rule is QSGD's too: with the reference's norm injected the bytes are the RQSGD fixture's."""
    want = Want(bits, nid)
    b = Bucket(want.case, compact, False)
    norms = np.array([want.norm if t in b.copies else so.linf_norm(p) for t, p in enumerate(b.parts)], F32)
    lv, sg = stoch.qsgd_quantize_batched(b.x, b.lay, bits, dev(norms), uniforms=b.u)
    b.check(want, lv, sg, "qsgd_quantize_batched")


def _one_element_in(a):
    store = torch.empty(a.numel() + 1, dtype=torch.float32, device=DEV)
    store[1:].copy_(a)
    return store[1:]


@pytest.mark.parametrize("route", ["new=x,prev=+0", "new=+0,prev=-x", "prev-view"])
@pytest.mark.parametrize("bits,nid", bc.ENC_CASES, ids=ENC_IDS)
def test_rqsgd_encode_delta_batched_injected_uniforms(bits, nid, route):
    """Both differences are exact (x - 0 and 0 - (-x); a -0 element becomes +0 in the second, with the same bytes).
    `prev-view`: prev one element into its storage, the element-wise path. Both forms: resident=None (one launch:
    the layout has a work list) and resident=False (two passes)."""
    want = Want(bits, nid)
    c = want.case
    lay = ops.BucketLayout([c.n])
    assert lay.nwork == 1
    x, zero, u = dev(c.x), torch.zeros(c.n, device=DEV), dev(c.u)
    new, prev = ([x], [zero]) if route != "new=+0,prev=-x" else ([zero], [dev(-c.x)])
    if route == "prev-view":
        prev = [_one_element_in(prev[0])]
        assert (prev[0].data_ptr() - new[0].data_ptr()) % 16
    for resident in (None, False):
        lv, sg, nr, mn = stoch.rqsgd_encode_delta_batched(new, prev, lay, bits, uniforms=u, resident=resident)
        torch.cuda.synchronize()
        name = f"rqsgd_encode_delta_batched {route} resident={resident}"
        assert_bytes(want, lv.cpu().numpy()[:c.n], sg.cpu().numpy()[:c.n], name)
        assert_scales(want, nr.cpu().numpy()[0], mn.cpu().numpy()[0], name)


@pytest.mark.parametrize("bits,nid", bc.ENC_CASES, ids=ENC_IDS)
def test_philox_uniforms_at_every_ushift_phase(bits, nid):
    """The straddling path takes Philox uniforms only, so here only the x side of each boundary is placed: the
    uniforms are whatever the stream (SEED, COUNTER) gives. Four copies in a 64-aligned layout with ushift 0, 1, 2, 3
    (phase 0 is quantize_regs, 1..3 quantize_regs_straddle), both forms of the delta encode, and the seeded
    rqsgd_encode_batched on the same bucket; against so.qsgd_quantize on so.philox_uniforms of the shifted
    indices."""
    want = Want(bits, nid)
    c = want.case
    lay = ops.BucketLayout([c.n] * 4)
    assert lay.nwork == 4
    ushift = np.arange(4, dtype=np.int64)
    x, zero = dev(c.x), torch.zeros(c.n, device=DEV)
    exp = [so.qsgd_quantize(c.x, c.s, want.norm, so.philox_uniforms(c.n, SEED, COUNTER, int(o + sh)))
           for o, sh in zip(lay.offsets.tolist(), [0, 1, 2, 3])]
    for resident in (None, False):
        lv, sg, nr, mn = stoch.rqsgd_encode_delta_batched([x] * 4, [zero] * 4, lay, bits, ushift=ushift, seed=SEED,
                                                          counter=COUNTER, resident=resident)
        torch.cuda.synchronize()
        lv, sg = lv.cpu().numpy(), sg.cpu().numpy()
        for t, o in enumerate(lay.offsets.tolist()):
            bad = bc.first_diffs(lv[o:o + c.n], exp[t][0])
            assert bad.size == 0, (f"b{bits} {nid} delta phase {t} resident={resident}",
                                   [(c.describe(int(i)), f"got {lv[o + i]} want {exp[t][0][i]}") for i in bad])
            assert np.array_equal(sg[o:o + c.n], exp[t][1]), (t, resident)
            assert_scales(want, nr.cpu().numpy()[t], mn.cpu().numpy()[t], "delta philox")
    flat = torch.zeros(lay.total, device=DEV)
    for o in lay.offsets.tolist():
        flat[o:o + c.n] = x
    for resident in (None, False):
        lv, sg, nr, mn = stoch.rqsgd_encode_batched(flat, lay, bits, seed=SEED, counter=COUNTER, resident=resident)
        torch.cuda.synchronize()
        lv = lv.cpu().numpy()
        for t, o in enumerate(lay.offsets.tolist()):
            q, _ = so.qsgd_quantize(c.x, c.s, want.norm, so.philox_uniforms(c.n, SEED, COUNTER, int(o)))
            bad = bc.first_diffs(lv[o:o + c.n], q)
            assert bad.size == 0, (f"b{bits} {nid} seeded rqsgd_encode_batched tensor {t} resident={resident}",
                                   [(c.describe(int(i)), f"got {lv[o + i]} want {q[i]}") for i in bad])


@pytest.mark.parametrize("bits,nid", bc.ENC_CASES, ids=ENC_IDS)
def test_rqsgd_decode_of_the_recorded_payload(bits, nid):
    """The reference's own payload of every encode case (level s + 1 wrapped to byte 0 and decoded as min * sign
    among them) decodes to the reference's floats, at a bucket offset that is a multiple of 4 and at one that is
    not."""
    want = Want(bits, nid)
    n = want.case.n
    lay = ops.BucketLayout([n, (1 - n) % 4 or 4, n], align=1)
    assert [int(o) % 4 for o in lay.offsets[[0, 2]]] == [0, 1]
    lv, sg = np.zeros(lay.total, np.uint8), np.ones(lay.total, np.int8)
    for o in lay.offsets[[0, 2]].tolist():
        lv[o:o + n], sg[o:o + n] = want.q, want.signs
    norms, mins = np.full(3, want.norm, F32), np.full(3, want.min, F32)
    out = stoch.rqsgd_decode_batched(dev(lv), dev(sg), dev(norms), dev(mins), lay, bits)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    for o in lay.offsets[[0, 2]].tolist():
        bad = bc.first_diffs(out[o:o + n], want.deq)
        assert bad.size == 0, (f"b{bits} {nid} rqsgd_decode_batched at offset {o}: differs at",
                               [(want.case.describe(int(i)), out[o + i], want.deq[i]) for i in bad])


# ------------------------------------------------------------------------------------------------
# decode
# ------------------------------------------------------------------------------------------------
DEC_TILE = 3              # 2304 elements: two 1024-element wave tiles and a dword remainder ...
DEC_TAIL = 7              # ... then a ragged tail: edge elements
DEC_IDS = [f"b{b}-{n}" for b, n in bc.DEC_CASES]
DEC_KINDS = [("qsgd", None), ("rqsgd", "normal"), ("rqsgd", "denormal")]


class DecodeBucket:
    """[the case's tensor, a tensor with norm 0, one with a NaN norm, the case's tensor again] packed back to back:
    with 2311 elements each the two copies sit at offsets 0 and 6933 (residues 0 and 1 mod 4), and the per-tensor
    branches (norm == 0, NaN) sit beside tensors that take the fast form."""

    def __init__(self, bits, nid, codec, mid):
        rec, self.s = DEC[(bits, nid)], 2 ** bits - 1
        self.bits, self.codec = bits, codec
        norm = f32_from_bits(rec["norm_bits"])
        mn = bc.DEC_MINS[mid] if mid else F32(0)
        lv = np.concatenate([np.tile(bc.DEC_LEVELS, DEC_TILE), bc.DEC_LEVELS[-DEC_TAIL:]])
        sg = np.concatenate([np.tile(bc.DEC_SIGNS, DEC_TILE), bc.DEC_SIGNS[-DEC_TAIL:]])
        n = lv.size
        self.lay = lay = ops.BucketLayout([n] * 4, align=1)
        assert [int(o) % 4 for o in lay.offsets] == [0, 3, 2, 1]
        self.norms = np.array([norm, 0.0, np.nan, norm], F32)
        self.mins = np.array([mn, mn, mn, mn], F32)
        one = fixture()[rec["name"] + ("__qsgd" if codec == "qsgd" else f"__rqsgd_{mid}")]   # the reference's output
        ref = np.concatenate([np.tile(one, DEC_TILE), one[-DEC_TAIL:]])
        # beside it: norm 0 decodes to zeros; a NaN norm to NaN (RQSGD: except level 0, which is min * sign)
        self.want = [ref, self._oracle(lv, sg, F32(0), mn), self._oracle(lv, sg, F32(np.nan), mn), ref]
        assert not self.want[1].any() and np.isnan(self.want[2][(lv != 0) | (codec == "qsgd")]).all()
        self.lv, self.sg = dev(np.tile(lv, 4)), dev(np.tile(sg, 4))
        self.tag = f"b{bits} {nid} {codec} min={mid}"

    def _oracle(self, lv, sg, norm, mn):
        if self.codec == "qsgd":
            return so.qsgd_dequantize(lv, sg, self.s, norm)
        return so.rqsgd_dequantize(lv, sg, self.s, norm, mn)

    def check(self, outs, route):
        torch.cuda.synchronize()
        for t, (got, want) in enumerate(zip(outs, self.want)):
            got = got.cpu().numpy()
            bad = bc.first_diffs(got, want)
            assert bad.size == 0, (f"{self.tag} {route} tensor {t} at offset {int(self.lay.offsets[t])} (norm "
                                   f"{self.norms[t]!r}): differs at", [(int(i), got[i], want[i]) for i in bad])


@pytest.mark.parametrize("codec,mid", DEC_KINDS, ids=["qsgd", "rqsgd-min-normal", "rqsgd-min-denormal"])
@pytest.mark.parametrize("bits,nid", bc.DEC_CASES, ids=DEC_IDS)
def test_decode_batched_of_every_level_byte(bits, nid, codec, mid):
    b = DecodeBucket(bits, nid, codec, mid)
    norms, mins = dev(b.norms), dev(b.mins)
    if codec == "qsgd":
        out = stoch.qsgd_decode_batched(b.lv, b.sg, norms, b.lay, bits)
    else:
        out = stoch.rqsgd_decode_batched(b.lv, b.sg, norms, mins, b.lay, bits)
    b.check([out[o:o + n] for o, n in zip(b.lay.offsets.tolist(), b.lay.sizes.tolist())], "decode_batched")


@pytest.mark.parametrize("codec,mid", DEC_KINDS, ids=["qsgd", "rqsgd-min-normal", "rqsgd-min-denormal"])
@pytest.mark.parametrize("bits,nid", bc.DEC_CASES, ids=DEC_IDS)
def test_dequantize_axpby_scale_mode_keeps_the_decodes_bits(bits, nid, codec, mid):
    """SCALE mode with beta = 1: fp32(1 * d) is d, so the output bits are the decode's. The copy at bucket offset
    0 takes decode4 (fast form), the one at offset 6933 decode_exact."""
    b = DecodeBucket(bits, nid, codec, mid)
    outs = [torch.full((int(n),), 7.0, device=DEV) for n in b.lay.sizes]
    stoch.dequantize_axpby_batched(codec, b.lv, b.sg, dev(b.norms), b.lay, bits, None, [outs], 0.0, 1.0,
                                   mins=dev(b.mins) if codec == "rqsgd" else None)
    b.check(outs, "dequantize_axpby_batched SCALE beta=1")
