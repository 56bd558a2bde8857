"""Generate tests/golden/flush_small.npz: the buffered servers' flush, pinned to the reference's own output.

Run in the build container (the reference tree exists only there), on the CPU:

    python tests/golden/make_golden_flush.py

Every expected value is produced by EXECUTING the reference's own strategy classes in place — ``FedBuff(3, 0.05,
True)`` and ``FADAS(3, 0.05)`` (``Src/ADFL/Strategy/fed_buff.py``, ``fadas.py``; they import only ``ADFL.model`` and
``.base``), through ``ref_loader`` and a bare ``ADFL.Strategy`` package registered here — over the seeded fp32
update dicts of flush_cases.py fed straight to ``produce_update``:

  fedbuff          one flush of three updates with staleness 0, 2, 5
  fadas_r0..r2     three flushes of three updates each, so the moments carry over; the second has a staleness
                   of 25 > max_delay = 10, so ``_apply_delay_correction`` fires

Data only. Inputs are regenerated from the seeds and are not stored (the manifest pins their digests). Stored
per flush: ``params_prime`` in full (FADAS's cannot be compared by digest: torch's CPU sqrt is one ulp low on
some inputs), with the elements where this torch's ``sqrt`` of the new v_hat is not the correctly rounded root
as packed bits (``fadas_r<r>__sqrt_off__<name>``: that property belongs to the torch and the CPU that generated
the file, so the test reads it from here); the ndim <= 1 entries of FADAS's averaged buffer, m, v and v_hat in full and a SHA-256 of every
entry (``flush_cases.digest``) in the manifest (a JSON string in the array ``manifest``), with the scalars the
strategy used. The generator also reports what the test's tolerance rests on: how many elements of params_prime
differ from the restatement, whether all of them lie where torch.sqrt differs from the correctly rounded root,
and the largest such difference in units of ulp(|step * m / den|).
"""

import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import flush_cases as fc  # noqa: E402
from ref_loader import REF_SRC, load_reference  # noqa: E402

MAX_BYTES = 400 * 1000


def load_strategies():
    pkg = types.ModuleType("ADFL.Strategy")
    pkg.__path__ = [os.path.join(REF_SRC, "Strategy")]
    sys.modules["ADFL.Strategy"] = pkg
    mods = {}
    for name in ("base", "fed_buff", "fadas"):
        full = f"ADFL.Strategy.{name}"
        spec = importlib.util.spec_from_file_location(full, os.path.join(REF_SRC, "Strategy", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[full] = mod
        spec.loader.exec_module(mod)
        mods[name] = mod
    return mods["base"].AggregationInfo, mods["fed_buff"].FedBuff, mods["fadas"].FADAS


def tensors(d):
    return {n: torch.from_numpy(np.array(a)) for n, a in d.items()}


def arrays_of(d):
    return {n: t.detach().numpy().copy() for n, t in d.items()}


def main():
    torch.set_num_threads(8)
    load_reference()
    info, fed_buff, fadas = load_strategies()
    print("torch", torch.__version__)
    arrays = {}
    manifest = {"torch": torch.__version__, "generator": "tests/golden/make_golden_flush.py",
                "order": [n for n, _, _ in fc.DICT_SHAPES], "inputs": {}, "fedbuff": {}, "fadas": []}

    def pin_inputs(tag, d):
        manifest["inputs"][tag] = {n: fc.digest(a) for n, a in d.items()}

    def store(tag, d, full):
        for n, a in d.items():
            if full or a.ndim <= 1:
                arrays[f"{tag}__{n}"] = a
        return {n: fc.digest(a) for n, a in d.items()}

    # FedBuff: one flush
    strat = fed_buff(fc.K, fc.LR, True)
    g_np = fc.g_params("fedbuff", 0)
    pin_inputs("fedbuff_g0", g_np)
    g = tensors(g_np)
    out = None
    for k, s in enumerate(fc.FEDBUFF_STALENESS):
        u_np = fc.update("fedbuff", 0, k)
        pin_inputs(f"fedbuff_u0_{k}", u_np)
        out = strat.produce_update(info(g, [tensors(u_np)], s))
        assert (out is g) == (k < fc.K - 1)
    manifest["fedbuff"] = {"params_prime": store("fedbuff__params_prime", arrays_of(out), True),
                           "dtypes": {n: str(t.dtype) for n, t in out.items()}}
    for n, a in g_np.items():   # the strategy left g_params alone
        assert fc.digest(g[n].numpy()) == fc.digest(a), n

    # FADAS: three flushes, the moments carried over
    # the reference's FADAS does not define Strategy's abstract on_client_finish, so the class cannot be
    # instantiated as it stands; the subclass adds that one no-op and nothing else
    strat = type("FADAS", (fadas,), {"on_client_finish": lambda self, client_id: None})(fc.K, fc.LR)
    worst, n_diff, n_all, outside = 0.0, 0, 0, 0
    mom = {n: [np.zeros(s, np.float32)] * 3 for n, s, _ in fc.DICT_SHAPES if n in fc.FLOAT_NAMES}
    for r, stale in enumerate(fc.FADAS_STALENESS):
        g_np = fc.g_params("fadas", r)
        pin_inputs(f"fadas_g{r}", g_np)
        g = tensors(g_np)
        rnd, first, ups = strat.round, None, []
        for k, s in enumerate(stale):
            u_np = fc.update("fadas", r, k)
            pin_inputs(f"fadas_u{r}_{k}", u_np)
            u = tensors(u_np)
            ups.append(u_np)
            first = first or dict(u)     # the first update's tensors become the buffer (averaged in place, dict cleared)
            if k == fc.K - 1:
                lr_t = strat.lr if max(stale) <= strat.max_delay else min(strat.lr, strat.lr / max(stale))
            out = strat.produce_update(info(g, [u], s))
        assert strat.round == rnd + 1 and out is not g
        rec = {"round": rnd, "lr_t": float(lr_t).hex(), "max_staleness": max(stale),
               "buffer": store(f"fadas_r{r}__buffer", arrays_of(first), False),
               "m": store(f"fadas_r{r}__m", arrays_of(strat.m), False),
               "v": store(f"fadas_r{r}__v", arrays_of(strat.v), False),
               "v_hat": store(f"fadas_r{r}__v_hat", arrays_of(strat.v_hat), False),
               "params_prime": store(f"fadas_r{r}__params_prime", arrays_of(out), True),
               "dtypes": {n: str(t.dtype) for n, t in out.items()}}
        manifest["fadas"].append(rec)
        # what the tolerance of tests/test_flush_golden.py rests on
        sc = fc.fadas_scalars(fc.BETA_1, fc.BETA_2, fc.EPS, fc.delay_lr(fc.LR, max(stale)), rnd)
        for n in fc.FLOAT_NAMES:
            before = mom[n]
            res = fc.fadas_flush(fc.fadas_buffer([u[n] for u in ups]), g_np[n], *before, fc.K, sc)
            mom[n] = [res["m"], res["v"], res["v_hat"]]
            for key, ref in (("b", first[n]), ("m", strat.m[n]), ("v", strat.v[n]), ("v_hat", strat.v_hat[n])):
                assert fc.same_bits(res[key], ref.numpy()).all(), (r, n, key)
            ref = out[n].numpy()
            h = res["v_hat"]
            mask = torch.sqrt(torch.from_numpy(h)).numpy() != np.sqrt(h.astype(np.float64)).astype(np.float32)
            arrays[f"fadas_r{r}__sqrt_off__{n}"] = np.packbits(mask.reshape(-1))
            diff = ~fc.same_bits(res["out"], ref)
            assert fc.explained_by_sqrt(ref, fc.fadas_buffer([u[n] for u in ups]), g_np[n], *before, fc.K, sc).all()
            outside += int((diff & ~mask).sum())
            n_diff += int(diff.sum())
            n_all += diff.size
            if diff.any():
                d = np.abs(res["out"].astype(np.float64) - ref.astype(np.float64)) - fc.ulp(res["out"])
                worst = max(worst, float((d[diff] / fc.ulp(res["upd"])[diff]).max()))
            print(f"  fadas r{r} {n}: sqrt mask {mask.mean():.4%}, params_prime differs on {diff.mean():.4%}")
        for n, a in g_np.items():
            assert fc.digest(g[n].numpy()) == fc.digest(a), n
    print(f"params_prime: {n_diff} of {n_all} elements differ from the restatement, {outside} outside the sqrt "
          f"mask; largest (|diff| - ulp(|out|)) / ulp(|upd|) = {worst:.3f}")
    manifest["measured"] = {"differ": n_diff, "elements": n_all, "outside_mask": outside, "worst_c": worst}
    arrays["manifest"] = np.array(json.dumps(manifest))
    np.savez_compressed(fc.FIXTURE, **arrays)
    size = os.path.getsize(fc.FIXTURE)
    print(f"wrote {fc.FIXTURE}: {size} bytes, {len(arrays)} arrays")
    assert size <= MAX_BYTES, f"{size} bytes: the fixture must stay within {MAX_BYTES}"


if __name__ == "__main__":
    main()
