"""CPU: QAFeL's broadcast through QSGD / RQSGD / CNAT as the executed reference computes it. The numpy
restatement (tests/broadcast_stoch_ref.py: stoch_oracle's quantize of fp32(g - h) under the recorded uniforms, its
dequantize of those bytes, then fp32(h + d)) reproduces every step of tests/golden/broadcast_stoch_small.npz — the
reference's diff_parameters, on_server_send, on_client_receive and add_parameters_inpace, three broadcasts in a
row, so a 1-ulp slip in h' would change the next step's difference — bit for bit."""

import os

import numpy as np
import pytest

import broadcast_cases as bc
import broadcast_stoch_cases as bsc
import broadcast_stoch_ref as br
import delta_cases
from golden_util import GOLDEN, bits_of

PATH = os.path.join(GOLDEN, "broadcast_stoch_small.npz")


def same_bytes(a, b) -> bool:
    a, b = np.atleast_1d(np.asarray(a)), np.atleast_1d(np.asarray(b))
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def matches(g, prefix: str, name: str, a: np.ndarray) -> bool:
    """a against prefix__<name>, or its SHA-256 against prefixsha__<name>."""
    if f"{prefix}__{name}" in g.files:
        return same_bytes(a, g[f"{prefix}__{name}"])
    return bc.sha(a) == str(g[f"{prefix}sha__{name}"])


def scale_matches(row, value, zero_branch: bool) -> bool:
    """A [kind, bits] row of the fixture against an fp32 value (None: the untouched int 0)."""
    kind, bits = int(row[0]), int(row[1])
    if value is None:
        return kind == 2 and bits == 0
    if zero_branch:
        return kind == 1 and bits == 0
    v = np.float32(value)
    return kind == 0 and (bits_of(v) == bits or (np.isnan(v) and np.isnan(np.array([bits], np.uint32).view(np.float32)[0])))


@pytest.fixture(scope="module")
def g():
    return np.load(PATH)


@pytest.fixture(scope="module")
def inputs():
    return bc.inputs()


def test_fixture_is_small_holds_data_only_and_names_its_runs(g):
    assert os.path.getsize(PATH) <= 256 * 1024
    order = [str(n) for n in g["order"]]
    assert order == [name for name, _, _ in delta_cases.DICT_SHAPES]
    assert [str(n) for n in g["new_order"]] == order[::-1]
    assert [str(n) for n in g["coded"]] == bsc.CODED
    for codec, bits in bsc.RUNS:
        for k in range(1, bc.STEPS + 1):
            assert f"{codec}_b{bits}__s{k}__order" in g.files
    for f in g.files:
        assert g[f].dtype.kind in "iufUS", f         # numbers and names


def test_uniform_recipe_is_deterministic_and_differs_per_step():
    a, b, c = bsc.uniforms(1), bsc.uniforms(1), bsc.uniforms(2)
    for n in bsc.CODED:
        assert a[n].dtype == np.float32 and a[n].min() >= 0 and a[n].max() < 1
        assert same_bytes(a[n], b[n]) and not same_bytes(a[n], c[n])


@pytest.mark.parametrize("codec,bits", bsc.RUNS, ids=[f"{c}-b{b}" for c, b in bsc.RUNS])
def test_restatement_reproduces_every_step_of_the_reference(g, inputs, codec, bits):
    h0, news = inputs
    order = [str(n) for n in g["order"]]
    run = f"{codec}_b{bits}"
    hidden = {n: h0[n].copy() for n in order}
    for k, new in enumerate(news, 1):
        pre = f"{run}__s{k}"
        assert [str(n) for n in g[f"{pre}__order"]] == order          # diff_parameters iterates hidden_state
        assert int(g[f"{pre}__rand_calls"]) == len(bsc.CODED) - (k == bc.STEPS)   # none on the zero branch
        us = bsc.uniforms(k)
        size = 0
        for name in order:
            gn = hidden[name].copy() if (k == bc.STEPS and name == bc.FROZEN) else new[name]
            if name in bsc.CODED:
                i = bsc.CODED.index(name)
                q, s, norm, mn, h2 = br.step(hidden[name], gn, codec, bits, us[name])
                assert str(q.dtype) == str(g[f"{pre}__qdtype"][i]), (k, name)
                assert matches(g, f"{pre}__q", name, q.view(np.uint8)), (k, name)
                assert matches(g, f"{pre}__signs", name, s), (k, name)
                assert scale_matches(g[f"{pre}__scale"][i], norm, norm == 0), (k, name)
                assert scale_matches(g[f"{pre}__scale2"][i], mn if codec == "rqsgd" and norm != 0 else None,
                                     False), (k, name)
                size += q.size
            else:
                d = gn - hidden[name]
                assert same_bytes(d, g[f"{pre}__pass__{name}"]), (k, name)
                h2 = hidden[name] + d
                size += d.nbytes
            assert h2.dtype == hidden[name].dtype
            assert matches(g, f"{pre}__h", name, h2), (k, name)
            hidden[name] = h2
        assert size == int(g[f"{pre}__size"])
    i = bsc.CODED.index(bc.FROZEN)                                   # the frozen layer: zero branch, h + 0
    assert g[f"{run}__s3__scale"][i].tolist() == [1, 0] and str(g[f"{run}__s3__qdtype"][i]) == "uint8"
    assert not g[f"{run}__s3__q__{bc.FROZEN}"].any() and (g[f"{run}__s3__signs__{bc.FROZEN}"] == 1).all()
    assert same_bytes(g[f"{run}__s3__h__{bc.FROZEN}"], g[f"{run}__s2__h__{bc.FROZEN}"])


@pytest.mark.parametrize("codec", ["qsgd", "rqsgd", "cnat"])
def test_zero_norm_adds_plus_zero_and_a_nan_norm_poisons_the_tensor(codec):
    h = np.array([[-0.0, 1.5, -2.0], [0.0, 3.0, -0.0]], dtype=np.float32)
    u = np.full(h.shape, 0.5, dtype=np.float32)
    q, s, norm, mn, h2 = br.step(h, h.copy(), codec, 8, u)
    assert norm == 0 and not q.any() and (s == 1).all()
    assert same_bytes(h2, np.where(h == 0, np.float32(0.0), h).astype(np.float32))   # -0 becomes +0, the rest stays
    assert not np.signbit(h2[0, 0]) and not np.signbit(h2[1, 2])
    gn = h.copy()
    gn[0, 1] = np.nan
    q, s, norm, mn, h2 = br.step(h, gn, codec, 8, u)
    assert np.isnan(norm) and np.isnan(h2).all()
