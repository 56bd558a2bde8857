"""CPU: the oracle (oracle/stoch_oracle.py) reproduces the executed reference on the boundary tensors of
tests/boundary_cases.py — every level and sign byte, the norm and the minimum factor, and every bit of every
decoded tensor (tests/golden/stoch_boundary.npz + stoch_boundary_manifest.json, made by
tests/golden/make_golden_stoch_boundary.py) — and the placed elements do what they were placed for, read off the
reference's own recorded bytes. Every comparison is exact."""

import json
import os

import numpy as np
import pytest

import boundary_cases as bc
import stoch_oracle as so
from golden_util import f32_from_bits, same_f32


@pytest.fixture(scope="module")
def g():
    return np.load(bc.FIXTURE)


with open(bc.MANIFEST) as _f:
    MAN = json.load(_f)
ENC = {(c["bits"], c["norm_id"]): c for c in MAN["encode"]}
DEC = {(c["bits"], c["norm_id"]): c for c in MAN["decode"]}
ENC_IDS = [f"b{b}-{n}" for b, n in bc.ENC_CASES]
DEC_IDS = [f"b{b}-{n}" for b, n in bc.DEC_CASES]


def recorded(g, case):
    """The reference's level and sign bytes of an encode case, in the tensor's (shuffled) order."""
    rec = ENC[(case.bits, case.nid)]
    return case.shuffle(g[rec["name"] + "__q"]), case.shuffle(g[rec["name"] + "__signs"]), rec


def test_fixture_is_small_and_lists_every_case(g):
    assert os.path.getsize(bc.FIXTURE) <= 256 * 1024
    assert list(ENC) == bc.ENC_CASES and list(DEC) == bc.DEC_CASES
    names = [f"{c['name']}__{k}" for c in MAN["encode"] for k in ("q", "signs", "deq")]
    names += [f"{c['name']}__{k}" for c in MAN["decode"] for k in ("qsgd", "rqsgd_normal", "rqsgd_denormal")]
    assert sorted(g.files) == sorted(names)
    for c in MAN["decode"]:
        assert c["min_bits"] == {mid: int(bc.bits_of(mn)) for mid, mn in bc.DEC_MINS.items()}


@pytest.mark.parametrize("bits,nid", bc.ENC_CASES, ids=ENC_IDS)
def test_inputs_are_the_ones_the_reference_ran_on(bits, nid):
    case = bc.encode_case(bits, nid)
    rec = ENC[(bits, nid)]
    assert case.n == rec["n"] and bc.digest_inputs(case) == rec["inputs_sha256"]
    assert int(bc.bits_of(case.norm)) == rec["norm_bits"]


@pytest.mark.parametrize("bits,nid", bc.ENC_CASES, ids=ENC_IDS)
def test_oracle_encode_and_decode_equal_the_reference(g, bits, nid):
    case = bc.encode_case(bits, nid)
    q_ref, s_ref, rec = recorded(g, case)
    norm, mn = f32_from_bits(rec["norm_bits"]), f32_from_bits(rec["min_bits"])
    assert same_f32(so.linf_norm(case.x), norm) and same_f32(so.lminf_norm(case.x), mn)
    q, signs = so.qsgd_quantize(case.x, case.s, norm, case.u)
    bad = bc.first_diffs(q, q_ref)
    assert bad.size == 0, [(case.describe(i), int(q[i]), int(q_ref[i])) for i in bad]
    assert np.array_equal(signs, s_ref)
    d, d_ref = so.rqsgd_dequantize(q_ref, s_ref, case.s, norm, mn), case.shuffle(g[rec["name"] + "__deq"])
    bad = bc.first_diffs(d, d_ref)
    assert bad.size == 0, [(case.describe(i), d[i], d_ref[i]) for i in bad]


@pytest.mark.parametrize("bits,nid", bc.DEC_CASES, ids=DEC_IDS)
def test_oracle_decode_of_every_level_byte_equals_the_reference(g, bits, nid):
    rec, s = DEC[(bits, nid)], 2 ** bits - 1
    norm = f32_from_bits(rec["norm_bits"])
    assert same_f32(norm, bc.DEC_NORMS[nid])
    outs = {"qsgd": so.qsgd_dequantize(bc.DEC_LEVELS, bc.DEC_SIGNS, s, norm)}
    for mid, mn in bc.DEC_MINS.items():
        outs[f"rqsgd_{mid}"] = so.rqsgd_dequantize(bc.DEC_LEVELS, bc.DEC_SIGNS, s, norm, mn)
    for key, got in outs.items():
        want = g[f"{rec['name']}__{key}"]
        bad = bc.first_diffs(got, want)
        assert bad.size == 0, (key, [(int(bc.DEC_LEVELS[i]), int(bc.DEC_SIGNS[i]), got[i], want[i]) for i in bad])


def test_decode_cases_reach_inf_nan_and_denormal_outputs(g):
    """The decode norms do what they are there for, read off the reference's recorded outputs."""
    d = g["dec_b8_inf_above_200__qsgd"]
    zero_sign = bc.DEC_SIGNS == 0
    assert np.isinf(d[~zero_sign]).any() and np.isfinite(d[~zero_sign]).any()
    assert np.isnan(d[zero_sign]).any() and (d[zero_sign] == 0).any()          # inf * sign 0 = NaN
    d = g["dec_b8_denormal__qsgd"]
    assert ((d != 0) & (np.abs(d) < np.float32(2.0 ** -126))).any()
    assert not g["dec_b8_zero__qsgd"].any() and not g["dec_b8_zero__rqsgd_normal"].any()
    d = g["dec_b8_nan__rqsgd_denormal"]                    # a NaN norm: NaN except level 0, which is min * sign
    assert np.isnan(d[bc.DEC_LEVELS != 0]).all() and not np.isnan(d[bc.DEC_LEVELS == 0]).any()


@pytest.mark.parametrize("bits", bc.ENC_BITS)
def test_anchor_above_s_wraps_through_u8(g, bits):
    """RN(RN(s * norm) / norm) > s: with u = 0 the element with |x| == norm gets level s + 1 — byte 0 at 8 bits
    (decoded as min * sign by RQSGD), 16 at 4 bits. Against the `< s` norm the floor is s - 1 and u = 0 rounds up
    to s."""
    case = bc.encode_case(bits, "gt_s")
    q_ref, s_ref, rec = recorded(g, case)
    a = case.anchor
    assert case.kind[a] == bc.K_ANCHOR and case.x[a] == case.norm and s_ref[a] == 1
    assert int(q_ref[a]) == (case.s + 1) & 0xFF
    if bits == 8:
        assert q_ref[a] == 0
        mn = f32_from_bits(rec["min_bits"])
        d = case.shuffle(g[rec["name"] + "__deq"])
        assert same_f32(d[a], np.float32(mn) * np.float32(s_ref[a]))
    if bits == 4:
        assert q_ref[a] == 16
    low = bc.encode_case(bits, "lt_s")
    q_low, _, _ = recorded(g, low)
    assert np.floor(bc.scaled_of(low.norm, low.s, low.norm)) == low.s - 1
    assert int(q_low[low.anchor]) == low.s & 0xFF


@pytest.mark.parametrize("bits,nid", bc.ENC_CASES, ids=ENC_IDS)
def test_the_strict_less_than_on_the_references_bytes(g, bits, nid):
    """u == prob rounds down, nextafter(prob, 0) rounds up, and u = 0 rounds up exactly where prob > 0 — each read
    off the reference's recorded bytes against the restated floor."""
    case = bc.encode_case(bits, nid)
    q_ref, _, _ = recorded(g, case)
    sc = bc.scaled_of(np.abs(case.x), case.s, case.norm)
    lo = np.floor(sc)
    down, up = so.to_u8(lo), so.to_u8(lo + np.float32(1))
    eq, below, above, zero = (case.var == v for v in (bc.V_EQ, bc.V_BELOW, bc.V_ABOVE, bc.V_ZERO))
    assert eq.any() and below.any()
    assert np.array_equal(q_ref[eq], down[eq])
    assert np.array_equal(q_ref[below], up[below])
    assert np.array_equal(q_ref[above], down[above])
    assert np.array_equal(q_ref[zero], np.where(sc - lo > 0, up, down)[zero])
    assert (zero & (sc == lo) & (case.kind == bc.K_CROSS)).any()           # u = 0 against prob = 0


def test_tie_elements_round_to_even_in_the_reference(g):
    """The denormal-quotient ties: the reference's division rounds them to even, which the level bytes of the
    u == prob / one-ulp-below variants show (0 / 1 against the even neighbour)."""
    case = bc.encode_case(2, "tie")
    q_ref, _, _ = recorded(g, case)
    tie = case.kind == bc.K_TIE
    sc = bc.scaled_of(np.abs(case.x[tie]), case.s, case.norm)
    units = sc.astype(np.float64) * 2.0 ** 149
    assert tie.sum() >= 16 and (units % 2 == 0).all() and (units > 0).all()
    var = case.var[tie]
    assert (q_ref[tie][var == bc.V_EQ] == 0).all() and (q_ref[tie][var == bc.V_BELOW] == 1).all()
    assert bc.fast_form_flags(case.x[tie], case.s, case.norm).all()
