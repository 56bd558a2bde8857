"""CPU: the numpy restatement of the fused decode + accumulate + flush (what the GPU tests hold the kernels to)
against the executed reference, tests/golden/receive_flush_small.npz: the reference's own channels' payloads of six
seeded updates, fed decoded to its own ``FedBuff(3, 0.05, True)``, ``FADAS(3, 0.05)`` (two flushes) and
``FedBuff(1, 0.05, True)`` (golden/make_golden_receive_flush.py).

The restatement is the oracle's decode of the stored payload (receive_flush_cases.decoded), then the fused entries'
arithmetic through flush_cases: u = fp32(factor * d), B = fp32(buf + u) (B = u without a buffer), then fedbuff_flush /
fadas_flush.

FedBuff's params_prime and FADAS's m, v and v_hat: bit for bit (SHA-256 of every tensor, the ndim <= 1 ones element
by element). FADAS's params_prime: ``flush_cases.explained_by_sqrt`` on every stored element — the reference's value
equals, bit for bit, the restatement with the square root at the correctly rounded value or one of its two fp32
neighbours, the exact and machine-independent set of values torch's faithfully rounded CPU sqrt allows. No tolerance
and no cap."""

import numpy as np
import pytest
import torch

import flush_cases as fc
import receive_flush_cases as rc

RUNS = list(rc.RUNS)


def _check_exact(run, tag, got, digests, z):
    for n, a in got.items():
        assert fc.digest(a) == digests[n], (run, tag, n)
        key = f"{run}__{tag}__{n}"
        if key in z.files:
            assert fc.same_bits(a, z[key]).all(), key


def _accumulate(buf, d, factor):
    """The fused entries' arithmetic up to the full buffer: B = fp32(buf + fp32(factor * d)), or fp32(factor * d)."""
    with np.errstate(all="ignore"):
        u = (np.float32(factor) * np.asarray(d, np.float32)).astype(np.float32)
        return u if buf is None else (buf + u).astype(np.float32)


def test_fixture_is_the_prescribed_run():
    z, man = rc.fixture()
    assert man["order"] == rc.ORDER and list(man["runs"]) == RUNS
    for j in range(len(rc.UPDATES)):
        assert {n: fc.digest(a) for n, a in rc.update(j).items()} == man["inputs"][f"u{j}"]
    assert {n: fc.digest(a) for n, a in rc.fedbuff_g().items()} == man["inputs"]["fedbuff_g"]
    import os
    assert os.path.getsize(rc.FIXTURE) <= rc.MAX_BYTES
    for run in RUNS:
        rec = man["runs"][run]
        assert len(rec["payloads"]) == len(rc.UPDATES) and [f["round"] for f in rec["fadas"]] == [1, 2]
        for r, f in enumerate(rec["fadas"]):
            assert {n: fc.digest(a) for n, a in rc.fadas_g(r).items()} == man["inputs"][f"fadas_g{r}"]
            assert f["max_staleness"] == max(rc.FADAS_STALENESS[r])
            assert float.fromhex(f["lr_t"]) == fc.delay_lr(rc.LR, max(rc.FADAS_STALENESS[r]))
        assert float.fromhex(rec["fadas"][1]["lr_t"]) == rc.LR / 25          # the delay correction fires once
        full = [k for k in z.files if k.startswith(f"{run}__fadas_r0__params_prime__")]
        assert len(full) == (len(rc.ORDER) if run in rc.FULL_PRIME else len(rc.ORDER) - len(rc.CODED))


@pytest.mark.parametrize("run", RUNS)
def test_fedbuff_params_prime_bit_for_bit(run):
    """The first K - 1 updates as receive_scaled / receive_scaled_add_ leave the buffer, the K-th through the fused
    arithmetic."""
    z, man = rc.fixture()
    g = rc.fedbuff_g()
    decs = [rc.decoded(run, j) for j in rc.FEDBUFF_UPDATES]
    fs = [fc.staleness_factor(s) for s in rc.FEDBUFF_STALENESS]
    got = {}
    for n in fc.FLOAT_NAMES:
        buf = None
        for d, f in zip(decs[:-1], fs[:-1]):
            buf = _accumulate(buf, d[n], f)
        got[n] = fc.fedbuff_flush(_accumulate(buf, decs[-1][n], fs[-1]), g[n], rc.K, rc.LR)
        assert fc.same_bits(got[n], fc.fedbuff_flush(fc.fedbuff_buffer([d[n] for d in decs], rc.FEDBUFF_STALENESS), g[n],
                                                     rc.K, rc.LR)).all()
    rec = man["runs"][run]["fedbuff"]
    _check_exact(run, "fedbuff__params_prime", got, rec["params_prime"], z)
    # the int64 counter: `.float()` copies it, so the buffer keeps the summed counters; add_parameters promotes
    n = "bn.num_batches_tracked"
    want = (1.0 * torch.tensor(int(g[n]))) + (rc.LR * torch.tensor(sum(int(d[n]) for d in decs)))
    assert rec["dtypes"][n] == "torch.float32" and z[f"{run}__fedbuff__params_prime__{n}"] == want.numpy()


@pytest.mark.parametrize("run", RUNS)
def test_fedbuff_without_a_buffer_bit_for_bit(run):
    """FedBuff(1): the first update is also the last; B = fp32(factor * d), factor = (1 + 0) ** -0.5."""
    z, man = rc.fixture()
    g = rc.fedbuff_g()
    d = rc.decoded(run, rc.FEDBUFF1_UPDATE)
    f = fc.staleness_factor(rc.FEDBUFF1_STALENESS)
    got = {n: fc.fedbuff_flush(_accumulate(None, d[n], f), g[n], 1, rc.LR) for n in fc.FLOAT_NAMES}
    _check_exact(run, "fedbuff1__params_prime", got, man["runs"][run]["fedbuff1"]["params_prime"], z)


@pytest.mark.parametrize("run", RUNS)
def test_fadas_two_rounds(run):
    z, man = rc.fixture()
    mom = {n: (np.zeros(s, np.float32),) * 3 for n, s, _ in fc.DICT_SHAPES if n in fc.FLOAT_NAMES}
    checked = 0
    for r, (js, stale) in enumerate(zip(rc.FADAS_UPDATES, rc.FADAS_STALENESS)):
        rec = man["runs"][run]["fadas"][r]
        g = rc.fadas_g(r)
        decs = [rc.decoded(run, j) for j in js]
        sc = fc.fadas_scalars(fc.BETA_1, fc.BETA_2, fc.EPS, fc.delay_lr(rc.LR, max(stale)), r + 1)
        full = {}
        for n in fc.FLOAT_NAMES:
            buf = None
            for d in decs[:-1]:
                buf = _accumulate(buf, d[n], 1.0)
            full[n] = _accumulate(buf, decs[-1][n], 1.0)
            assert fc.same_bits(full[n], fc.fadas_buffer([d[n] for d in decs])).all()
        res = {n: fc.fadas_flush(full[n], g[n], *mom[n], rc.K, sc) for n in fc.FLOAT_NAMES}
        before, mom = mom, {n: (x["m"], x["v"], x["v_hat"]) for n, x in res.items()}
        for key in ("m", "v", "v_hat"):
            _check_exact(run, f"fadas_r{r}__{key}", {n: x[key] for n, x in res.items()}, rec[key], z)
        for n in fc.FLOAT_NAMES:
            key = f"{run}__fadas_r{r}__params_prime__{n}"
            if key not in z.files:
                continue
            ok = fc.explained_by_sqrt(z[key], full[n], g[n], *before[n], rc.K, sc)
            assert ok.all(), (run, r, n, int((~ok).sum()))
            assert fc.digest(z[key]) == rec["params_prime"][n]
            checked += z[key].size
    # every stored element: the whole dict for the two full runs, the bias for the others
    floats = sum(int(np.prod(s)) for n, s, _ in fc.DICT_SHAPES if n in fc.FLOAT_NAMES)
    assert checked == 2 * (floats if run in rc.FULL_PRIME else 10)
