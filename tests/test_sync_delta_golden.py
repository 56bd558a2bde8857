"""CPU: tests/golden/sync_delta.npz (the reference's Simple(CommType.DELTA, sync=True) executed over the aggregate
fixture's client updates, tests/golden/make_golden_sync_delta.py) against the formula the fused kernels implement.

For every stored case the mean is the one tests/golden/aggregate.npz already pins (the reference's
simple_aggregate of its own decodes); fp32 (alpha * g) + (beta * mean) in numpy with three separate roundings must
equal the new fixture bit for bit (NaNs compare as NaN): full arrays where they are stored, and the SHA-256 of the
fp32 bytes for every (channel, K, tensor). That ties the new fixture to the existing one and to
out = fp32(fp32(alpha * g) + fp32(beta * m))."""

import os

import numpy as np
import pytest

import recipes
import sync_delta_cases as sd
from golden_util import same_f32

GOLDEN = os.path.dirname(sd.FIXTURE)


@pytest.fixture(scope="module")
def fx():
    arrays, manifest = sd.load()
    return arrays, manifest, np.load(os.path.join(GOLDEN, "aggregate.npz")), sd.g_arrays()


def test_fixture_size_and_g_recipe(fx):
    _, manifest, _, g = fx
    assert os.path.getsize(sd.FIXTURE) + os.path.getsize(sd.MANIFEST) <= sd.MAX_BYTES
    assert manifest["g"]["order"] == list(g) and set(g) == set(sd.NAMES) and list(g) != sd.NAMES
    for n, a in g.items():
        assert recipes.sha256(a) == manifest["g"]["sha256"][n], n
    assert g[sd.COUNTER_NAME].dtype == np.int64
    bits = {(n, i): b for n, i, b in sd.G_SPECIAL}
    for (n, i), b in bits.items():
        assert int(g[n].reshape(-1).view(np.uint32)[i]) == b
    assert [tuple(manifest["cases"][sd.case_tag(*c)][f] for f in ("channel", "k", "alpha", "beta"))
            for c in sd.CASES] == sd.CASES
    assert len(manifest["cases"]) == len(sd.CASES)


@pytest.mark.parametrize("case", sd.CASES, ids=[sd.case_tag(*c) for c in sd.CASES])
def test_fixture_is_the_three_roundings_over_the_pinned_mean(fx, case):
    arrays, manifest, agg, g = fx
    ch, k, alpha, beta = case
    tag = sd.case_tag(*case)
    rec = manifest["cases"][tag]
    assert list(rec["sha256"]) == sd.NAMES          # the first update's key order
    for n in sd.NAMES:
        want = sd.axpby(g[n], agg[f"{ch}__k{k}__{n}"], alpha, beta)
        assert rec["dtypes"][n] == "float32", n     # the int64 counter included: true division, then 1.0 * int64
        full = f"{tag}__{n}" in arrays
        assert full == (n in rec["full"]) and (full or want.size > sd.FULL_MAX), n
        if full:
            got = arrays[f"{tag}__{n}"]
            assert got.dtype == np.float32 and got.shape == want.shape and same_f32(got, want), n
            assert recipes.sha256(got) == rec["sha256"][n], n
        if not np.isnan(want).any():   # a NaN's payload is the producing CPU's; such tensors are stored in full
            assert recipes.sha256(want) == rec["sha256"][n], n
        else:
            assert full, n
