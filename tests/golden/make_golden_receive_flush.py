"""Generate tests/golden/receive_flush_small.npz: the buffered servers' K-th client update from the payload on, pinned
to the reference's own output.

Run in the build container (the reference tree exists only there), on the CPU:

    python tests/golden/make_golden_receive_flush.py

Every expected value is produced by EXECUTING the reference in place: ``ref_loader`` for the channels and
``model.py``, and — through a bare ``ADFL.Strategy`` package registered here, ref_loader.py itself unchanged — its own
``FedBuff`` and ``FADAS`` classes (``Src/ADFL/Strategy/fed_buff.py``, ``fadas.py``). For each run of
receive_flush_cases.RUNS (SLQChannel(8), SLQChannel(4), QSGDChannel(8), RQSGDChannel(8), CNATChannel(8)):

  payloads   ``on_client_send`` of the six updates of receive_flush_cases.UPDATES (flush_cases.update; the
             stochastic codecs' uniforms are torch's, seeded: decoding needs none)
  decoded    ``on_server_receive`` of a fresh copy of a payload, every time a strategy is fed (as a transported
             update is)
  fedbuff    ``FedBuff(3, 0.05, True)``: updates 0-2 with staleness 0, 2, 5; the third produce_update flushes
  fadas_r0/1 ``FADAS(3, 0.05)``: updates 0-2, then 3-5, so the moments carry over; the second flush has a staleness
             of 25 > max_delay = 10
  fedbuff1   ``FedBuff(1, 0.05, True)``: update 0 alone — no buffer, the first update is also the last

Data only. Stored: the coded entries' payloads (``<run>__u<j>__q__<name>``, ``__signs__``), the ndim <= 1 entries of
every result in full, FADAS's ``params_prime`` in full for the slq_b8 and qsgd_b8 runs, and a manifest (a JSON string
in the array ``manifest``) with the scales, lr_t, and flush_cases.digest of the inputs and of every result tensor.
"""

import copy
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
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))

import flush_cases as fc  # noqa: E402
import receive_flush_cases as rc  # noqa: E402
from make_golden_stoch import scale_record  # noqa: E402
from ref_loader import REF_SRC, load_reference  # noqa: E402


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
    ref = load_reference()
    info, fed_buff, fadas = load_strategies()
    # the reference's FADAS does not define Strategy's abstract on_client_finish, so the class cannot be instantiated
    # as it stands; the subclass adds that one no-op and nothing else (make_golden_flush.py)
    fadas = type("FADAS", (fadas,), {"on_client_finish": lambda self, client_id: None})
    print("torch", torch.__version__)
    arrays = {}
    manifest = {"torch": torch.__version__, "generator": "tests/golden/make_golden_receive_flush.py",
                "order": rc.ORDER, "inputs": {}, "runs": {}}
    ups = [rc.update(j) for j in range(len(rc.UPDATES))]
    for j, u in enumerate(ups):
        manifest["inputs"][f"u{j}"] = {n: fc.digest(a) for n, a in u.items()}
    manifest["inputs"]["fedbuff_g"] = {n: fc.digest(a) for n, a in rc.fedbuff_g().items()}
    for r in range(len(rc.FADAS_UPDATES)):
        manifest["inputs"][f"fadas_g{r}"] = {n: fc.digest(a) for n, a in rc.fadas_g(r).items()}

    for run, (cls, bits) in rc.RUNS.items():
        ch = getattr(ref.quant, cls)(bits)
        rec = {"bits": bits, "payloads": [], "fadas": []}
        payloads = []
        for j, u in enumerate(ups):
            torch.manual_seed(31000 + 10 * bits + j)
            qp, _ = ch.on_client_send(tensors(u))
            prec = {"scale": {}, "scale_2": {}, "q_dtype": {}}
            for n, p in qp.params.items():
                if n not in rc.CODED:   # passthrough: the update's own entry
                    assert fc.digest(p.data.numpy()) == fc.digest(u[n]), (run, j, n)
                    continue
                if p.data.is_quantized:
                    arrays[f"{run}__u{j}__q__{n}"] = p.data.int_repr().numpy().copy()
                    prec["scale"][n] = {"f64_bits": int(np.array([p.data.q_scale()], np.float64).view(np.uint64)[0])}
                    assert p.data.q_zero_point() == 0
                else:
                    arrays[f"{run}__u{j}__q__{n}"] = p.data.numpy().view(np.uint8).copy()
                    arrays[f"{run}__u{j}__signs__{n}"] = p.signs.numpy().copy()
                    prec["scale"][n] = scale_record(p.scale)
                    prec["scale_2"][n] = scale_record(p.scale_2)
                prec["q_dtype"][n] = str(p.data.dtype).replace("torch.", "")
            rec["payloads"].append(prec)
            payloads.append(qp)

        def fresh(j):   # a transported update: its own payload objects, decoded again
            return ch.on_server_receive(copy.deepcopy(payloads[j]))[0]

        def store(tag, d, full):
            for n, a in d.items():
                if full or a.ndim <= 1:
                    arrays[f"{run}__{tag}__{n}"] = a
            return {n: fc.digest(a) for n, a in d.items()}

        # FedBuff(3, 0.05, True): one flush
        strat = fed_buff(rc.K, rc.LR, True)
        g_np = rc.fedbuff_g()
        g = tensors(g_np)
        for k, (j, s) in enumerate(zip(rc.FEDBUFF_UPDATES, rc.FEDBUFF_STALENESS)):
            out = strat.produce_update(info(g, [fresh(j)], s))
            assert (out is g) == (k < rc.K - 1)
        rec["fedbuff"] = {"params_prime": store("fedbuff__params_prime", arrays_of(out), False),
                          "dtypes": {n: str(t.dtype) for n, t in out.items()}}
        # FedBuff(1, 0.05, True): no buffer
        strat = fed_buff(1, rc.LR, True)
        out = strat.produce_update(info(g, [fresh(rc.FEDBUFF1_UPDATE)], rc.FEDBUFF1_STALENESS))
        assert out is not g
        rec["fedbuff1"] = {"params_prime": store("fedbuff1__params_prime", arrays_of(out), False)}
        for n, a in g_np.items():   # the strategies left g_params alone
            assert fc.digest(g[n].numpy()) == fc.digest(a), n

        # FADAS(3, 0.05): two flushes, the moments carried over
        strat = fadas(rc.K, rc.LR)
        for r, (js, stale) in enumerate(zip(rc.FADAS_UPDATES, rc.FADAS_STALENESS)):
            g_np = rc.fadas_g(r)
            g = tensors(g_np)
            rnd = strat.round
            for j, s in zip(js, stale):
                out = strat.produce_update(info(g, [fresh(j)], s))
            assert strat.round == rnd + 1 and out is not g
            lr_t = strat.lr if max(stale) <= strat.max_delay else min(strat.lr, strat.lr / max(stale))
            rec["fadas"].append({
                "round": rnd, "lr_t": float(lr_t).hex(), "max_staleness": max(stale),
                "m": store(f"fadas_r{r}__m", arrays_of(strat.m), False),
                "v": store(f"fadas_r{r}__v", arrays_of(strat.v), False),
                "v_hat": store(f"fadas_r{r}__v_hat", arrays_of(strat.v_hat), False),
                "params_prime": store(f"fadas_r{r}__params_prime", arrays_of(out), run in rc.FULL_PRIME),
                "dtypes": {n: str(t.dtype) for n, t in out.items()}})
            for n, a in g_np.items():
                assert fc.digest(g[n].numpy()) == fc.digest(a), n
        manifest["runs"][run] = rec
        print(f"  {run}: {len(payloads)} payloads, fedbuff, fedbuff1, {len(rec['fadas'])} fadas flushes")
    arrays["manifest"] = np.array(json.dumps(manifest))
    np.savez_compressed(rc.FIXTURE, **arrays)
    size = os.path.getsize(rc.FIXTURE)
    print(f"wrote {rc.FIXTURE}: {size} bytes, {len(arrays)} arrays")
    assert size <= rc.MAX_BYTES, f"{size} bytes: the fixture must stay within {rc.MAX_BYTES}"


if __name__ == "__main__":
    main()
