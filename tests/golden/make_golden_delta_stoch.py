"""Generate tests/golden/delta_stoch_small.npz + delta_stoch_manifest.json: the send side of a DELTA round
through the stochastic channels, pinned to the reference's own output.

Run in the build container (the reference tree exists only there), on the CPU:

    python tests/golden/make_golden_delta_stoch.py

Every expected value is produced by EXECUTING the reference in place through ``ref_loader``: its own
``diff_parameters(prev, new)`` (``Src/ADFL/model.py:350-358``) followed by ``on_client_send`` and
``on_server_receive`` of QSGDChannel / RQSGDChannel / CNATChannel (``Src/ADFL/Channel/quant.py:140-570``) at bits
8 and 4, with ``torch.rand_like`` replaced, for the duration of the call, by recorded uniforms (one plane per
ndim > 1 tensor, shared by all six runs: the patching of make_golden_stoch.py). Three dict pairs:

  main   delta_cases.dict_pair() — prev / new are those of delta_small.npz and are not stored again
  zero   (5, 7) and (3, 3) with new == prev bit for bit: the norm == 0 branch
  nan    (5, 7) whose difference holds inf - inf, and (3, 3) with a NaN in `new`

Data only — uniforms, inputs of the two small pairs and expected outputs; no reference source is stored.

Arrays in the .npz (``<pair>`` main / zero / nan, ``<run>`` e.g. qsgd_b8, ``<name>`` a dict key):
  u__<pair>__<name>                the uniforms of an ndim > 1 tensor
  prev__<pair>__<name>, new__...   inputs of the zero / nan pairs
  <pair>__<run>__q__<name>         level / exponent bytes (uint8 view), __signs__, __deq__ (decoded floats)
  <pair>__<run>__pass__<name>      the ndim <= 1 entries the reference passes through
The manifest holds, per pair and run: key order, the coded names, scale / scale_2 records (make_golden_stoch.py's
scale_record format), q dtypes, size and the number of rand_like calls.
"""

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import delta_cases  # noqa: E402
from make_golden_stoch import CODECS, scale_record  # noqa: E402
from ref_loader import load_reference  # noqa: E402

OUT = os.path.join(HERE, "delta_stoch_small.npz")
MANIFEST = os.path.join(HERE, "delta_stoch_manifest.json")
MAX_BYTES = 1000 * 1000
BITS = (8, 4)


def small_pairs():
    """The zero and nan pairs as (prev, new) dicts of numpy arrays."""
    rng = np.random.default_rng(77)
    a = rng.standard_normal((5, 7), dtype=np.float32)
    b = rng.standard_normal((3, 3), dtype=np.float32)
    a[1, 2], b[0, 0] = 0.0, -0.0
    bias = rng.standard_normal(4, dtype=np.float32)
    zero = ({"z.a": a.copy(), "z.b": b.copy(), "z.bias": bias.copy()},
            {"z.a": a.copy(), "z.b": b.copy(), "z.bias": (bias + np.float32(0.5)).astype(np.float32)})
    pa = rng.standard_normal((5, 7), dtype=np.float32)
    na = (pa + np.float32(1e-2) * rng.standard_normal((5, 7), dtype=np.float32)).astype(np.float32)
    pa[2, 3] = na[2, 3] = np.float32(np.inf)          # inf - inf
    pa[4, 6], na[4, 6] = np.float32(-np.inf), np.float32(1.0)   # a +inf difference beside it
    pb = rng.standard_normal((3, 3), dtype=np.float32)
    nb = (pb + np.float32(1e-2)).astype(np.float32)
    nb[1, 1] = np.float32(np.nan)
    nan = ({"n.a": pa, "n.b": pb}, {"n.a": na, "n.b": nb})
    return {"zero": zero, "nan": nan}


def run(ref, codec: str, bits: int, prev, new, planes):
    ch = getattr(ref.quant, CODECS[codec])(bits)
    by_shape = {tuple(u.shape): torch.from_numpy(u.copy()) for u in planes.values()}
    assert len(by_shape) == len(planes), "one uniform plane per shape"
    calls = []
    orig = torch.rand_like

    def fake_rand_like(p, *a, **k):
        assert p.dtype == torch.float32
        calls.append(1)
        return by_shape[tuple(p.shape)].clone()

    diff = ref.model.diff_parameters(prev, new)
    torch.rand_like = fake_rand_like
    try:
        qp, _ = ch.on_client_send(diff)
    finally:
        torch.rand_like = orig
    dec, _ = ch.on_server_receive(qp)
    return qp, dec, len(calls)


def main():
    torch.set_num_threads(8)
    ref = load_reference()
    print("torch", torch.__version__)
    main_prev, main_new = delta_cases.dict_pair()
    order = [name for name, _, _ in delta_cases.DICT_SHAPES]
    pairs = {"main": ({n: main_prev[n] for n in order}, {n: main_new[n] for n in order[::-1]})}
    pairs.update(small_pairs())
    arrays, manifest = {}, {"torch": torch.__version__, "generator": "tests/golden/make_golden_delta_stoch.py",
                            "pairs": {}}
    for pi, (pname, (prev_np, new_np)) in enumerate(pairs.items()):
        planes = {}
        for k, (n, a) in enumerate(prev_np.items()):
            if a.ndim > 1:
                u = np.random.default_rng(5000 + 100 * pi + k).random(a.size, dtype=np.float32)
                if a.size > 4096:   # the two large tensors: a 2^-12 grid, so the plane compresses
                    u = (np.floor(u * np.float32(4096)) * np.float32(2.0 ** -12)).astype(np.float32)
                planes[n] = u.reshape(a.shape)
                arrays[f"u__{pname}__{n}"] = planes[n]
        if pname != "main":
            for n in prev_np:
                arrays[f"prev__{pname}__{n}"] = prev_np[n]
                arrays[f"new__{pname}__{n}"] = new_np[n]
        prev = {n: torch.from_numpy(np.array(a)) for n, a in prev_np.items()}
        new = {n: torch.from_numpy(np.array(a)) for n, a in new_np.items()}
        runs = {}
        for codec in CODECS:
            for bits in BITS:
                rname = f"{codec}_b{bits}"
                qp, dec, ncalls = run(ref, codec, bits, prev, new, planes)
                names = list(qp.params.keys())
                coded = [n for n in names if prev[n].ndim > 1]
                rec = {"order": names, "coded": coded, "size": int(qp.size), "rand_calls": ncalls, "scale": {},
                       "scale_2": {}, "q_dtype": {}}
                for n in names:
                    p = qp.params[n]
                    assert p.bits == bits
                    if n in coded:
                        arrays[f"{pname}__{rname}__q__{n}"] = p.data.numpy().view(np.uint8)
                        arrays[f"{pname}__{rname}__signs__{n}"] = p.signs.numpy()
                        arrays[f"{pname}__{rname}__deq__{n}"] = dec[n].numpy()
                        rec["scale"][n] = scale_record(p.scale)
                        rec["scale_2"][n] = scale_record(p.scale_2)
                        rec["q_dtype"][n] = str(p.data.dtype).replace("torch.", "")
                    else:
                        assert p.scale == 0 and p.scale_2 == 0
                        arrays[f"{pname}__{rname}__pass__{n}"] = p.data.numpy()
                runs[rname] = rec
        manifest["pairs"][pname] = {"prev_order": list(prev_np.keys()), "new_order": list(new_np.keys()), "runs": runs}
    np.savez_compressed(OUT, **arrays)
    with open(MANIFEST, "w") as f:
        json.dump(manifest, f, indent=1)
    size = os.path.getsize(OUT)
    print(f"wrote {OUT}: {size} bytes, {len(arrays)} arrays")
    assert size <= MAX_BYTES, f"{size} bytes: the fixture must stay within {MAX_BYTES}"


if __name__ == "__main__":
    main()
