"""CPU: the stochastic-codec oracle on numpy's ``new - prev`` against the executed reference's DELTA send
(tests/golden/delta_stoch_small.npz: diff_parameters + on_client_send + on_server_receive of QSGD / RQSGD / CNAT
at bits 8 and 4 with recorded uniforms). Every byte, scale record and decoded bit must match: this pins the
fixture the GPU channel test compares send_delta with, and the claim that numpy's fp32 subtraction is the
difference the reference encodes."""

import numpy as np
import pytest

from golden_util import bits_of, same_f32

import delta_stoch_fixture as fx
import stoch_oracle as so

CASES = [(p, c, b) for p in fx.PAIRS for c, b in fx.RUNS]


@pytest.mark.parametrize("pname,codec,bits", CASES, ids=[f"{p}-{c}-b{b}" for p, c, b in CASES])
def test_oracle_on_numpy_difference_reproduces_the_fixture(pname, codec, bits):
    prev, new = fx.pair(pname)
    rec = fx.run(pname, codec, bits)
    assert rec["order"] == list(prev.keys())                      # diff_parameters iterates params_prev
    assert rec["coded"] == [n for n in prev if prev[n].ndim > 1]
    levels = 2 ** bits - 1
    size = 0
    for n in rec["order"]:
        with np.errstate(invalid="ignore"):
            x = new[n] - prev[n]
        if n not in rec["coded"]:
            got = fx.arr(pname, codec, bits, "pass", n)
            assert got.dtype == x.dtype and got.shape == x.shape
            assert np.array_equal(got, x) if x.dtype != np.float32 else same_f32(got, x)
            size += x.nbytes
            continue
        assert x.dtype == np.float32
        u = fx.uniforms(pname, n)
        norm = so.linf_norm(x) if codec == "rqsgd" else so.torch_l2_norm(x)
        g_norm, g_tensor, _ = fx.scale_value(rec["scale"][n])
        assert np.isnan(norm) == np.isnan(g_norm) and (np.isnan(norm) or bits_of(norm) == bits_of(g_norm)), n
        assert g_tensor == (norm == 0)                              # the zero branch keeps the 0-dim tensor
        g_min, _, g_min_int = fx.scale_value(rec["scale_2"][n])
        if codec == "rqsgd" and norm != 0:
            mn = so.lminf_norm(x)
            assert np.isnan(mn) == np.isnan(g_min) and (np.isnan(mn) or bits_of(mn) == bits_of(g_min)), n
        else:
            assert g_min_int and g_min == 0
        if codec == "cnat":
            q, s = so.cnat_quantize(x, bits, norm, u)
        else:
            q, s = so.qsgd_quantize(x, levels, norm, u)
        q_ref, s_ref, d_ref = (fx.arr(pname, codec, bits, k, n) for k in ("q", "signs", "deq"))
        assert str(q.dtype) == rec["q_dtype"][n]
        np.testing.assert_array_equal(q.view(np.uint8), q_ref)
        np.testing.assert_array_equal(s, s_ref)
        if codec == "cnat":
            d = so.cnat_dequantize(q_ref.view(np.int8) if rec["q_dtype"][n] == "int8" else q_ref, s_ref, norm)
        elif codec == "qsgd":
            d = so.qsgd_dequantize(q_ref, s_ref, levels, norm)
        else:
            d = so.rqsgd_dequantize(q_ref, s_ref, levels, norm, g_min)
        assert same_f32(d, d_ref), n
        size += x.size
    assert size == rec["size"]


def test_the_zero_and_nan_pairs_are_what_they_claim():
    prev, new = fx.pair("zero")
    for n in ("z.a", "z.b"):
        assert np.array_equal(prev[n].view(np.uint32), new[n].view(np.uint32))
        for codec, bits in fx.RUNS:
            rec = fx.run("zero", codec, bits)
            assert rec["scale"][n] == {"tensor": True, "bits": 0} and rec["q_dtype"][n] == "uint8"
            assert not fx.arr("zero", codec, bits, "q", n).any()
            assert (fx.arr("zero", codec, bits, "signs", n) == 1).all()
    prev, new = fx.pair("nan")
    with np.errstate(invalid="ignore"):
        d = new["n.a"] - prev["n.a"]
    assert np.isinf(prev["n.a"][2, 3]) and np.isnan(d[2, 3]) and np.isinf(d[4, 6])
    assert np.isnan(new["n.b"]).sum() == 1
