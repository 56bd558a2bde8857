"""CPU: "fp32 subtract, then SLQ" is what the executed reference computes for a DELTA send. The oracle
(oracle/slq_oracle.py) applied to numpy's fp32 ``new - prev`` reproduces every payload and scale of
tests/golden/delta_small.npz (the reference's own diff_parameters + SLQChannel(bits).on_client_send), and
the passthrough entries are ``new - prev`` in their own dtype."""

import os

import numpy as np
import pytest

import delta_cases
import slq_oracle as so
from golden_util import GOLDEN, bits_of

PATH = os.path.join(GOLDEN, "delta_small.npz")


def same_bytes(a, b) -> bool:
    a, b = np.atleast_1d(np.asarray(a)), np.atleast_1d(np.asarray(b))
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def g():
    return np.load(PATH)


def test_fixture_is_small_and_holds_the_listed_dict_pair(g):
    assert os.path.getsize(PATH) <= 256 * 1024
    order = [str(n) for n in g["order"]]
    assert order == [name for name, _, _ in delta_cases.DICT_SHAPES]
    assert sorted(str(n) for n in g["new_order"]) == sorted(order) and [str(n) for n in g["new_order"]] != order
    for name, shape, dt in delta_cases.DICT_SHAPES:
        for side in ("prev", "new"):
            a = g[f"{side}__{name}"]
            assert a.shape == tuple(shape) and a.dtype == dt, (side, name)
    # the recipe in delta_cases reproduces the stored inputs bit for bit
    prev, new = delta_cases.dict_pair()
    for name in order:
        assert same_bytes(prev[name], g[f"prev__{name}"]) and same_bytes(new[name], g[f"new__{name}"]), name
    assert g["new__big.weight"].size == delta_cases.R + 1


@pytest.mark.parametrize("bits", [8, 4])
def test_oracle_on_numpy_difference_reproduces_the_reference(g, bits):
    order = [str(n) for n in g["order"]]
    assert [str(n) for n in g[f"b{bits}__order"]] == order          # diff_parameters iterates params_prev
    qnames = [str(n) for n in g[f"b{bits}__qnames"]]
    assert qnames == [n for n in order if g[f"prev__{n}"].ndim > 1]
    size = 0
    for k, name in enumerate(qnames):
        x = g[f"new__{name}"] - g[f"prev__{name}"]
        assert x.dtype == np.float32
        for enc in (so.encode, so.np_encode):
            q, scale = enc(x, bits)
            assert np.array_equal(q, g[f"b{bits}__q__{name}"]), (name, enc.__name__)
            assert bits_of(scale) == int(g[f"b{bits}__scale_bits"][k]), (name, enc.__name__)
        size += x.size
    for name in order:
        if name not in qnames:
            size += g[f"pass__{name}"].nbytes
    assert size == int(g[f"b{bits}__size"])


def test_passthrough_entries_are_the_difference_in_their_own_dtype(g):
    names = [str(n) for n in g["order"] if g[f"prev__{n}"].ndim <= 1]
    assert names == ["conv.bias", "bn.num_batches_tracked", "fc.bias"]
    for name in names:
        want = g[f"new__{name}"] - g[f"prev__{name}"]
        got = g[f"pass__{name}"]
        assert got.dtype == want.dtype == g[f"prev__{name}"].dtype and got.shape == want.shape
        assert same_bytes(got, want)
    assert g["pass__bn.num_batches_tracked"].dtype == np.int64 and int(g["pass__bn.num_batches_tracked"]) == 5
