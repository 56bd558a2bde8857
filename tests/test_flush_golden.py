"""CPU: the numpy restatement of the buffered servers' flush (flush_cases.py — what the GPU tests hold the kernels
to) against the executed reference, tests/golden/flush_small.npz: its own ``FedBuff(3, 0.05, True)`` and
``FADAS(3, 0.05)`` over seeded updates fed to ``produce_update`` (golden/make_golden_flush.py).

FedBuff's params_prime and FADAS's averaged buffer, m, v and v_hat over three flushes: bit for bit (SHA-256 of
every tensor, and the small ones element by element).

FADAS's params_prime cannot be: torch's CPU fp32 sqrt is not correctly rounded, and the restatement (like the
kernel) uses the correctly rounded one. How often torch misses belongs to the CPU it runs on: one ulp low on 0.6 %
of uniform inputs on the Xeon that generated the fixture, one ulp off in either direction on 20 % on an EPYC 9575F.
A mask formed with the running torch therefore says nothing about the stored params_prime on another machine, so
the generator stores its own: mask = the elements where the generating torch's ``sqrt`` of the new v_hat differs
from fp32(sqrt(fp64)) (``fadas_r<r>__sqrt_off__<name>``). The rule, on every machine:
  * outside the mask the restatement equals the reference bit for bit;
  * the mask covers at most 2 % of a tensor (flush_cases.MASK_CAP);
  * inside it |out - ref| <= c * ulp(|step * m' / den|) + ulp(|out|), c = flush_cases.MASK_C = 2: the generator
    measured the largest (|out - ref| - ulp(|out|)) / ulp(|step * m' / den|) of this fixture at 0.938 (11 of 24,267
    elements differ at all, none outside the mask); doubled, because the one-ulp denominator error passes through
    one division and one addition, that is 1.876, rounded up to 2;
  * and, stricter than the bound, every element of the reference equals bit for bit the restatement with the root
    at the correctly rounded value or one of its two neighbours (flush_cases.explained_by_sqrt).
"""

import numpy as np
import torch

import flush_cases as fc


def _inputs_pinned(tag, d, manifest):
    for n, a in d.items():
        assert fc.digest(a) == manifest["inputs"][tag][n], (tag, n)


def _check_exact(tag, got, digests, z):
    for n, a in got.items():
        assert fc.digest(a) == digests[n], (tag, n)
        key = f"{tag}__{n}"
        if key in z.files:
            assert fc.same_bits(a, z[key]).all(), key


def test_fixture_is_the_prescribed_run():
    z, man = fc.fixture()
    assert man["order"] == [n for n, _, _ in fc.DICT_SHAPES]
    assert [r["round"] for r in man["fadas"]] == [1, 2, 3]
    assert [r["max_staleness"] for r in man["fadas"]] == [max(s) for s in fc.FADAS_STALENESS]
    assert max(fc.FADAS_STALENESS[1]) > fc.MAX_DELAY            # the delay correction fires once
    for r, rec in enumerate(man["fadas"]):
        assert float.fromhex(rec["lr_t"]) == fc.delay_lr(fc.LR, max(fc.FADAS_STALENESS[r]))
    assert float.fromhex(man["fadas"][1]["lr_t"]) == fc.LR / 25
    # the tolerance's basis, as the generator measured it
    assert man["measured"]["outside_mask"] == 0 and 2 * man["measured"]["worst_c"] <= fc.MASK_C


def test_exact_fma_restatement():
    """fma32 is one rounding of the exact a * b + c: against Python's exact rational arithmetic on values chosen so
    that the separately rounded form and the fp64-rounded form both differ from it."""
    from fractions import Fraction
    rng = np.random.default_rng(5)
    a = rng.standard_normal(4000, dtype=np.float32)
    b = rng.standard_normal(4000, dtype=np.float32)
    c = (-(a.astype(np.float64) * b.astype(np.float64))).astype(np.float32) * np.float32(1 + 2 ** -12)  # cancellation
    c[::3] = rng.standard_normal(c[::3].size, dtype=np.float32) * np.float32(1e-3)
    a[:4], b[:4], c[:4] = [1 + 2 ** -23] * 4, [1 + 2 ** -23] * 4, [2 ** -60, -2 ** -60, 0.0, 1e-45]
    got = fc.fma32(a, b, c)
    for i in range(a.size):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        # float(Fraction) is correctly rounded to fp64; the rational itself rounds to fp32 through one comparison
        lo = np.float32(float(exact))
        cands = sorted({lo, np.nextafter(lo, np.float32(np.inf)), np.nextafter(lo, np.float32(-np.inf))}, key=float)
        dist = [abs(Fraction(float(x)) - exact) for x in cands]
        best = min(dist)
        winners = [x for x, d in zip(cands, dist) if d == best]
        want = winners[0] if len(winners) == 1 else next(x for x in winners if (x.view(np.uint32) & 1) == 0)
        assert got[i].view(np.uint32) == np.float32(want).view(np.uint32), (i, a[i], b[i], c[i], got[i], want)
    sep = (a * b) + c
    assert (sep.view(np.uint32) != got.view(np.uint32)).any()   # the data does tell an FMA from mul + add


def test_fedbuff_params_prime_bit_for_bit():
    z, man = fc.fixture()
    g = fc.g_params("fedbuff", 0)
    ups = [fc.update("fedbuff", 0, k) for k in range(fc.K)]
    _inputs_pinned("fedbuff_g0", g, man)
    for k, u in enumerate(ups):
        _inputs_pinned(f"fedbuff_u0_{k}", u, man)
    got = {n: fc.fedbuff_flush(fc.fedbuff_buffer([u[n] for u in ups], fc.FEDBUFF_STALENESS), g[n], fc.K, fc.LR)
           for n in fc.FLOAT_NAMES}
    _check_exact("fedbuff__params_prime", got, man["fedbuff"]["params_prime"], z)
    # the int64 counter: `.float()` copies it, so the buffer keeps the summed counters; add_parameters promotes
    n = "bn.num_batches_tracked"
    want = (1.0 * torch.tensor(int(g[n]))) + (fc.LR * torch.tensor(sum(int(u[n]) for u in ups)))
    assert man["fedbuff"]["dtypes"][n] == "torch.float32" and z[f"fedbuff__params_prime__{n}"] == want.numpy()


def _stored_mask(z, r, n, shape):
    """Where the generating torch's sqrt of the new v_hat was not the correctly rounded fp32 root."""
    bits = np.unpackbits(z[f"fadas_r{r}__sqrt_off__{n}"])[:int(np.prod(shape))]
    return bits.astype(bool).reshape(shape)


def test_fadas_three_rounds():
    z, man = fc.fixture()
    mom = {n: (np.zeros(s, np.float32),) * 3 for n, s, _ in fc.DICT_SHAPES if n in fc.FLOAT_NAMES}
    for r, stale in enumerate(fc.FADAS_STALENESS):
        rec = man["fadas"][r]
        g = fc.g_params("fadas", r)
        ups = [fc.update("fadas", r, k) for k in range(fc.K)]
        _inputs_pinned(f"fadas_g{r}", g, man)
        sc = fc.fadas_scalars(fc.BETA_1, fc.BETA_2, fc.EPS, fc.delay_lr(fc.LR, max(stale)), r + 1)
        res = {n: fc.fadas_flush(fc.fadas_buffer([u[n] for u in ups]), g[n], *mom[n], fc.K, sc)
               for n in fc.FLOAT_NAMES}
        before, mom = mom, {n: (x["m"], x["v"], x["v_hat"]) for n, x in res.items()}
        for key, field in (("b", "buffer"), ("m", "m"), ("v", "v"), ("v_hat", "v_hat")):
            _check_exact(f"fadas_r{r}__{field}", {n: x[key] for n, x in res.items()}, rec[field], z)
        for n, x in res.items():
            ref = z[f"fadas_r{r}__params_prime__{n}"]
            mask = _stored_mask(z, r, n, ref.shape)
            same = fc.same_bits(x["out"], ref)
            close = fc.masked_close(x["out"], ref, x["upd"])
            print(f"fadas r{r} {n}: mask {mask.mean():.4%}, differs {(~same).mean():.4%}, "
                  f"outside the bound {(~close).sum()}")
            assert mask.mean() <= fc.MASK_CAP, (r, n, mask.mean())
            assert same[~mask].all(), (r, n, int((~same & ~mask).sum()))
            assert close[mask].all(), (r, n)
            assert fc.explained_by_sqrt(ref, fc.fadas_buffer([u[n] for u in ups]), g[n], *before[n], fc.K, sc).all()


def test_restatement_special_values():
    """The formulas at the values the GPU tests place: den = eps when v_hat' = 0, NaN and inf propagate as in
    torch's own statements (positions; NaN payloads are not compared), -0.0 and denormals are kept."""
    sc = fc.fadas_scalars(fc.BETA_1, fc.BETA_2, fc.EPS, fc.LR, 1)
    buf = np.array([0.0, -0.0, np.nan, np.inf, 1e-41, 3e-3, 0.0], np.float32)
    g = np.ones(7, np.float32)
    m = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.5], np.float32)
    v = np.zeros(7, np.float32)
    h = np.array([0.0, 0.0, 0.0, 0.0, 0.0, np.nan, 0.0], np.float32)
    res = fc.fadas_flush(buf, g, m, v, h, 3, sc)
    tb, tm, tv, th = (torch.from_numpy(x.copy()) for x in (buf, m, v, h))
    tb.div_(3)
    tm.mul_(fc.BETA_1).add_(tb, alpha=1 - fc.BETA_1)
    tv.mul_(fc.BETA_2).addcmul_(tb, tb, value=1 - fc.BETA_2)
    torch.maximum(th, tv, out=th)
    for key, t in (("b", tb), ("m", tm), ("v", tv), ("v_hat", th)):
        assert fc.same_bits(res[key], t.numpy()).all(), key
    assert res["den"][0] == np.float32(fc.EPS) and res["den"][6] == np.float32(fc.EPS)
    assert res["out"][0] == 1.0 and 2e7 < res["out"][6] < 3e7          # 0 / eps and (0.5 * 0.45) / eps
    assert np.isnan(res["out"][[2, 3, 5]]).all() and np.isnan(res["v_hat"][5]) and not np.isnan(res["v"][5])
    assert np.signbit(res["b"][1]) and res["m"][4] != 0                # -0.0 / 3, a denormal average times 0.1
