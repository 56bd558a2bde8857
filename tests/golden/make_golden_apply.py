"""Generate tests/golden/apply_small.npz: the asynchronous server's update step, pinned to the reference's own
output.

Run in the build container (the reference tree exists only there), on the CPU:

    python tests/golden/make_golden_apply.py

Every expected value is produced by EXECUTING the reference in place: ``ref_loader`` for the channels and
``model.py``, and — through a bare ``ADFL.Strategy`` package registered here, ref_loader.py itself unchanged —
its own ``FedAsync`` and ``FedBuff`` classes (``Src/ADFL/Strategy/fed_async.py``, ``fed_buff.py``; they import
only ``ADFL.model`` and ``.base``). For each run of apply_cases.RUNS (SLQChannel(8), SLQChannel(4), QSGDChannel(8),
RQSGDChannel(8), CNATChannel(8)) over apply_cases.update():

  payload     ``on_client_send``'s own payload (the stochastic codecs' uniforms are torch's, seeded: decoding
              needs none)
  decoded     ``on_server_receive`` of it
  fedasync_s  ``FedAsync(POLY, alpha=0.6).produce_update`` on (base, decoded, staleness s), s = 0, 1, 3, 7:
              add_parameters(base, decoded, 1 - a_t, a_t)
  pair_1_1    add_parameters(base, decoded, 1.0, 1.0) (Strategy/simple.py:100)
  fedbuff_k   ``FedBuff(10, 1.0, True)``'s buffer after its k-th produce_update, k = 1, 2, 3, with staleness
              0, 2, 5, every update a fresh copy of the payload decoded again (as a transported update is)

Data only. Stored: the payloads (``<run>__q__<name>``, ``__signs__``, ``__pass__``), the small entries of every
result in full (``<run>__<case>__<name>`` for the ndim <= 1 entries), and a manifest (a JSON string in the
array ``manifest``) with the scales, the coefficients the strategies used, and apply_cases.digest of every
tensor: inputs, decoded tensors and results.
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

import apply_cases as ac  # noqa: E402
from make_golden_stoch import scale_record  # noqa: E402
from ref_loader import REF_SRC, load_reference  # noqa: E402

MAX_BYTES = 200 * 1000


def load_strategies():
    """The reference's FedAsync / FedBuff / AggregationInfo, executed where they lie (None if they do not
    import under the stubs)."""
    try:
        pkg = types.ModuleType("ADFL.Strategy")
        pkg.__path__ = [os.path.join(REF_SRC, "Strategy")]
        sys.modules["ADFL.Strategy"] = pkg
        mods = {}
        for name in ("base", "fed_async", "fed_buff"):
            full = f"ADFL.Strategy.{name}"
            spec = importlib.util.spec_from_file_location(full, os.path.join(REF_SRC, "Strategy", name + ".py"))
            mod = importlib.util.module_from_spec(spec)
            sys.modules[full] = mod
            spec.loader.exec_module(mod)
            mods[name] = mod
        return mods["base"].AggregationInfo, mods["fed_async"].FedAsync, mods["fed_buff"].FedBuff
    except Exception as e:  # noqa: BLE001
        print("strategies do not import under the stubs:", repr(e))
        return None


def tensors(d):
    return {n: torch.from_numpy(np.array(a)) for n, a in d.items()}


def main():
    torch.set_num_threads(8)
    ref = load_reference()
    strategies = load_strategies()
    print("torch", torch.__version__, "| strategies:", "reference classes" if strategies else "model.py statements")
    upd_np, base_np = ac.update(), ac.base()
    arrays = {}
    manifest = {"torch": torch.__version__, "generator": "tests/golden/make_golden_apply.py",
                "strategies": bool(strategies), "order": [n for n, _, _ in ac.DICT_SHAPES],
                "update": {n: ac.digest(a) for n, a in upd_np.items()},
                "base": {n: ac.digest(a) for n, a in base_np.items()}, "runs": {}}

    def record(run, case, params, rec):
        rec[case] = {n: ac.digest(t.numpy()) for n, t in params.items()}
        for n, t in params.items():
            if t.ndim <= 1:
                arrays[f"{run}__{case}__{n}"] = t.numpy().copy()

    for run, (cls, bits) in ac.RUNS.items():
        ch = getattr(ref.quant, cls)(bits)
        torch.manual_seed(20240 + bits)
        qp, _ = ch.on_client_send(tensors(upd_np))
        rec = {"bits": bits, "scale": {}, "scale_2": {}, "q_dtype": {}, "results": {}, "coef": {}}
        for n, p in qp.params.items():
            if n not in ac.CODED:
                arrays[f"{run}__pass__{n}"] = p.data.numpy().copy()
                continue
            if p.data.is_quantized:
                arrays[f"{run}__q__{n}"] = p.data.int_repr().numpy().copy()
                rec["scale"][n] = {"f64_bits": int(np.array([p.data.q_scale()], np.float64).view(np.uint64)[0])}
                assert p.data.q_zero_point() == 0
            else:
                arrays[f"{run}__q__{n}"] = p.data.numpy().view(np.uint8).copy()
                arrays[f"{run}__signs__{n}"] = p.signs.numpy().copy()
                rec["scale"][n] = scale_record(p.scale)
                rec["scale_2"][n] = scale_record(p.scale_2)
            rec["q_dtype"][n] = str(p.data.dtype).replace("torch.", "")

        def fresh():   # a transported update: its own payload objects, decoded again
            return ch.on_server_receive(copy.deepcopy(qp))[0]

        res = rec["results"]
        record(run, "decoded", fresh(), res)
        base = tensors(base_np)
        for s in ac.FEDASYNC_STALENESS:
            if strategies:
                info, fed_async, _ = strategies
                strat = fed_async(fed_async.Method.POLY, alpha=ac.FEDASYNC_ALPHA)
                out = strat.produce_update(info(base, [fresh()], s))
                a_t = strat.alpha * strat._poly(s)
            else:
                a_t = ac.FEDASYNC_ALPHA * ac.poly(s)
                out = ref.model.add_parameters(base, fresh(), (1 - a_t), a_t)
            rec["coef"][f"fedasync_{s}"] = [float(1 - a_t).hex(), float(a_t).hex()]
            record(run, f"fedasync_{s}", out, res)
        record(run, "pair_1_1", ref.model.add_parameters(base, fresh(), 1.0, 1.0), res)
        if strategies:
            info, _, fed_buff = strategies
            strat = fed_buff(10, 1.0, True)
        buffer = None
        for k, s in enumerate(ac.FEDBUFF_STALENESS, 1):
            d = fresh()
            if strategies:
                assert strat.produce_update(info(base, [d], s)) is base   # no flush before 10 updates
                buffer, f = strat.buffer, strat._staleness_factor(s)
            else:
                f = ac.poly(s)
                for t in d.values():
                    t.float().mul_(f)
                if buffer is None:
                    buffer = d
                else:
                    ref.model.add_parameters_inpace(buffer, d, 1, 1, to_float=False)
            rec["coef"][f"fedbuff_{k}"] = [float(f).hex()]
            record(run, f"fedbuff_{k}", buffer, res)
        for n, a in base_np.items():   # the strategies left g_params alone
            assert ac.digest(base[n].numpy()) == ac.digest(a), n
        manifest["runs"][run] = rec
    arrays["manifest"] = np.array(json.dumps(manifest))
    np.savez_compressed(ac.FIXTURE, **arrays)
    size = os.path.getsize(ac.FIXTURE)
    print(f"wrote {ac.FIXTURE}: {size} bytes, {len(arrays)} arrays")
    assert size <= MAX_BYTES, f"{size} bytes: the fixture must stay within {MAX_BYTES}"


if __name__ == "__main__":
    main()
