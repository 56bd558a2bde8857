"""CPU: the numpy three-rounding restatement of the asynchronous server's update step against the executed
reference (tests/golden/apply_small.npz, make_golden_apply.py): from the reference's own payloads, decoded by the
oracles, it reproduces every output the reference's FedAsync / add_parameters / FedBuff computed, bit for bit
(the fixture keeps a SHA-256 per output tensor and the ndim <= 1 entries in full). This pins the arithmetic the
kernels implement — fp32(fp32(af * y) + fp32(bf * d)) and fp32(bf * d), af / bf the coefficients rounded to fp32
first — and the fixture the GPU channel test compares with."""

import numpy as np
import pytest

import apply_cases as ac
import apply_fixture as fx


def test_inputs_regenerate_to_the_fixture_digests():
    _, m = ac.fixture()
    assert m["strategies"], "the fixture was made with the reference's own FedAsync / FedBuff classes"
    assert m["order"] == [n for n, _, _ in ac.DICT_SHAPES]
    assert {n: ac.digest(a) for n, a in ac.update().items()} == m["update"]
    assert {n: ac.digest(a) for n, a in ac.base().items()} == m["base"]


@pytest.mark.parametrize("run", list(ac.RUNS))
def test_oracle_decode_is_the_reference_decode(run):
    _, m = ac.fixture()
    want = m["runs"][run]["results"]["decoded"]
    got = fx.decoded(run)
    assert list(got) == m["order"]
    for n, d in got.items():
        assert ac.digest(d) == want[n], (run, n)


@pytest.mark.parametrize("run", list(ac.RUNS))
def test_coefficients_are_the_strategies(run):
    for s in ac.FEDASYNC_STALENESS:
        a_t = ac.FEDASYNC_ALPHA * ac.poly(s)
        assert fx.coef(run, f"fedasync_{s}") == [1 - a_t, a_t]
    for k, s in enumerate(ac.FEDBUFF_STALENESS, 1):
        assert fx.coef(run, f"fedbuff_{k}") == [ac.poly(s)]


@pytest.mark.parametrize("run", list(ac.RUNS))
def test_three_roundings_reproduce_add_parameters(run):
    z, m = ac.fixture()
    res = m["runs"][run]["results"]
    base, dec = ac.base(), fx.decoded(run)
    cases = [(f"fedasync_{s}", *fx.coef(run, f"fedasync_{s}")) for s in ac.FEDASYNC_STALENESS]
    cases.append(("pair_1_1", 1.0, 1.0))
    for case, alpha, beta in cases:
        for n in m["order"]:
            if dec[n].dtype == np.float32:
                got = fx.np_axpby(base[n], dec[n], alpha, beta)
            else:   # the int64 counter: torch promotes int64 * Python float to fp32
                got = fx.np_axpby(base[n].astype(np.float32), dec[n].astype(np.float32), alpha, beta)
            assert ac.digest(got) == res[case][n], (run, case, n)
            if got.ndim <= 1:
                assert np.array_equal(z[f"{run}__{case}__{n}"], got) and z[f"{run}__{case}__{n}"].dtype == got.dtype


@pytest.mark.parametrize("run", list(ac.RUNS))
def test_three_roundings_reproduce_the_fedbuff_buffer(run):
    """Update 1 scaled becomes the buffer; updates 2 and 3 are scaled, then added: fp32(buf + fp32(f * d)). The
    int64 counter is never scaled (`.float()` copies it) and adds exactly."""
    z, m = ac.fixture()
    res = m["runs"][run]["results"]
    dec = fx.decoded(run)
    buf = None
    for k, s in enumerate(ac.FEDBUFF_STALENESS, 1):
        (f,) = fx.coef(run, f"fedbuff_{k}")
        upd = {n: fx.np_scale(d, f) if d.dtype == np.float32 else d.copy() for n, d in dec.items()}
        if buf is None:
            buf = upd
        else:
            buf = {n: fx.np_axpby(buf[n], upd[n], 1.0, 1.0) if upd[n].dtype == np.float32 else buf[n] + upd[n]
                   for n in buf}
        for n in m["order"]:
            assert ac.digest(buf[n]) == res[f"fedbuff_{k}"][n], (run, k, n)
            if buf[n].ndim <= 1:
                assert np.array_equal(z[f"{run}__fedbuff_{k}__{n}"], buf[n])


def test_a_contracted_product_would_not_reproduce_it():
    """The finding behind the three separate operations: forming fp32(af * y + fp32(bf * d)) with the first product
    unrounded (an FMA) changes a large share of random elements, so these digests detect contraction."""
    run, n = "slq_b8", "emb.weight"
    alpha, beta = fx.coef(run, "fedasync_1")
    y, d = ac.base()[n], fx.oracle_decode(run, n)
    b = (np.float32(beta) * d).astype(np.float32)
    fma = (np.float64(np.float32(alpha)) * y.astype(np.float64) + b.astype(np.float64)).astype(np.float32)
    differ = np.count_nonzero(fma.view(np.uint32) != fx.np_axpby(y, d, alpha, beta).view(np.uint32))
    assert differ > 0.05 * y.size
