"""Generate tests/golden/sync_delta.npz + sync_delta_manifest.json: the synchronous DELTA server step, pinned to
the reference's own output.

Run in the build container (the reference tree exists only there), on the CPU:

    python tests/golden/make_golden_sync_delta.py

Every expected value is produced by EXECUTING the reference in place: its channels (``ref_loader``) encode and
decode make_golden_aggregate.py's client updates exactly as that generator does (the stochastic channels under
``torch.manual_seed(7000 + client)``, so their payloads are the ones aggregate.npz stores; this is asserted), and
the reference's ``Simple(CommType.DELTA, True)`` (``Src/ADFL/Strategy/simple.py``, loaded through a bare
``ADFL.Strategy`` package as make_golden_flush.py loads the buffered strategies) turns the seeded global dict g of
sync_delta_cases.py and the first K decodes into the new global parameters. The strategy's constructor and
``produce_update`` run without ray, so every (1.0, 1.0) case goes through
``produce_update(AggregationInfo(g, decoded[:K], 0))``, not ``_sync_update`` directly. The two (0.4, 0.6) cases
execute ``add_parameters(g, simple_aggregate(decoded[:5]), 0.4, 0.6)`` (``Src/ADFL/model.py``) directly.

Data only. g is regenerated from its recipe (the manifest pins its SHA-256 values). Stored per case: every tensor
of at most FULL_MAX elements in full (all tensors for FULL_CASES), and the SHA-256 of every tensor's bytes in the
manifest, with the dtypes and the torch version.
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

import recipes  # noqa: E402
import sync_delta_cases as sd  # noqa: E402
from make_golden_aggregate import SHAPES, STOCH, client_dict  # noqa: E402
from ref_loader import REF_SRC, load_reference  # noqa: E402


def load_simple():
    pkg = types.ModuleType("ADFL.Strategy")
    pkg.__path__ = [os.path.join(REF_SRC, "Strategy")]
    sys.modules["ADFL.Strategy"] = pkg
    mods = {}
    for name in ("base", "simple"):
        full = f"ADFL.Strategy.{name}"
        spec = importlib.util.spec_from_file_location(full, os.path.join(REF_SRC, "Strategy", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[full] = mod
        spec.loader.exec_module(mod)
        mods[name] = mod
    return mods["base"].AggregationInfo, mods["base"].CommType, mods["simple"].Simple


def main():
    torch.set_num_threads(8)
    ref = load_reference()
    info, comm, simple = load_simple()
    agg = np.load(os.path.join(HERE, "aggregate.npz"))
    g_np = sd.g_arrays()
    manifest = {"torch": torch.__version__, "generator": "tests/golden/make_golden_sync_delta.py",
                "via": "Simple(CommType.DELTA, True).produce_update(AggregationInfo(g, decoded[:K], 0))",
                "g": {"seed": sd.G_SEED, "mult": sd.G_MULT, "counter": sd.COUNTER,
                      "special": [[n, i, b] for n, i, b in sd.G_SPECIAL], "order": list(g_np),
                      "sha256": {n: recipes.sha256(a) for n, a in g_np.items()}},
                "cases": {}}
    nclients = max(sd.SLQ8_K)
    clients = [client_dict(c) for c in range(nclients)]
    decoded = {}
    for bits in (8, 4):
        ch = ref.quant.SLQChannel(bits=bits)
        decoded[f"slq{bits}"] = [ch.on_server_receive(ch.on_client_send(clients[c])[0])[0] for c in range(nclients)]
    for codec, (cls, bits) in STOCH.items():
        ch = getattr(ref.quant, cls)(bits)
        decoded[codec] = []
        for c in range(max(sd.STOCH_K)):
            torch.manual_seed(7000 + c)
            qp, _ = ch.on_client_send(clients[c])
            for n in SHAPES:   # the payloads aggregate.npz stores
                assert np.array_equal(qp.params[n].data.numpy().view(np.uint8), agg[f"{codec}__c{c}__{n}__q"]), (codec, c, n)
                assert np.array_equal(qp.params[n].signs.numpy(), agg[f"{codec}__c{c}__{n}__signs"]), (codec, c, n)
            decoded[codec].append(ch.on_server_receive(qp)[0])

    arrays = {}
    for ch_tag, k, alpha, beta in sd.CASES:
        g = {n: torch.from_numpy(np.array(a)) for n, a in g_np.items()}
        ups = decoded[ch_tag][:k]
        if (alpha, beta) == (1.0, 1.0):
            strat = simple(comm.DELTA, True)
            out = strat.produce_update(info(g, ups, 0))
            assert strat.get_round() == 1
        else:
            out = ref.model.add_parameters(g, ref.model.simple_aggregate(ups), alpha, beta)
        assert list(out) == list(ups[0])   # the first update's key order
        for n, a in g_np.items():          # g left alone
            assert recipes.sha256(g[n].numpy()) == recipes.sha256(a), n
        tag = sd.case_tag(ch_tag, k, alpha, beta)
        rec = {"k": k, "alpha": alpha, "beta": beta, "channel": ch_tag, "sha256": {}, "dtypes": {}, "full": []}
        for n, t in out.items():
            a = t.numpy()
            rec["sha256"][n] = recipes.sha256(a)
            rec["dtypes"][n] = str(a.dtype)
            if (ch_tag, k, alpha, beta) in sd.FULL_CASES or a.size <= sd.FULL_MAX:
                arrays[f"{tag}__{n}"] = a
                rec["full"].append(n)
        manifest["cases"][tag] = rec
    np.savez_compressed(sd.FIXTURE, **arrays)
    with open(sd.MANIFEST, "w") as f:
        json.dump(manifest, f, indent=1)
    size = os.path.getsize(sd.FIXTURE) + os.path.getsize(sd.MANIFEST)
    print(f"torch {torch.__version__}: {len(arrays)} arrays, {len(manifest['cases'])} cases, {size} bytes")
    assert size <= sd.MAX_BYTES, f"{size} bytes: the fixture must stay within {sd.MAX_BYTES}"


if __name__ == "__main__":
    main()
