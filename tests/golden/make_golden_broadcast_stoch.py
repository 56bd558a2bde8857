"""Generate tests/golden/broadcast_stoch_small.npz: QAFeL's broadcast through the stochastic channels, pinned to
the reference's own output.

Run in the build container (the reference tree exists only there), on the CPU:

    python tests/golden/make_golden_broadcast_stoch.py

Every expected value is produced by EXECUTING the reference in place through ``ref_loader``: the four statements
of ``Src/ADFL/Server/qafel.py:156-180`` with the reference's own QSGDChannel / RQSGDChannel / CNATChannel at bits
8 and 4,

    update   = diff_parameters(hidden_state, g_params)
    q_update = channel.on_server_send(update)
    d_update = channel.on_client_receive(q_update)
    add_parameters_inpace(hidden_state, d_update, 1, 1, False)

three times in a row, the hidden state carried from one broadcast to the next, with ``torch.rand_like`` replaced,
for the duration of on_server_send, by recorded uniforms (make_golden_delta_stoch.py's patching). The inputs are
``broadcast_cases.inputs()`` (broadcast_small.npz pins them) and the uniforms ``broadcast_stoch_cases.uniforms``;
in step 3 ``fc.weight`` of g is exactly the hidden state the run has reached (a frozen layer: the norm == 0
branch, h + 0). Data only — expected outputs; no reference source is stored, and neither are the inputs or the
uniforms (seeded recipes reproduce them).

The file has to stay within 256 KiB, so arrays of more than ``broadcast_cases.SHA_ABOVE`` elements are stored as
the SHA-256 of their bytes.

Arrays in the .npz (``<run>`` e.g. qsgd_b8, k the step 1..3, ``<name>`` a dict key; ``X`` / ``Xsha`` is the array
or its SHA-256):
  order, new_order, coded            hidden_state's key order / the order g is built in / the ndim > 1 keys
  <run>__s<k>__order                 the keys of the reference's QuantParameters, in its order
  <run>__s<k>__q__<name> / __qsha__  level / exponent bytes (uint8 view); __signs__ / __signssha__ the sign bytes
  <run>__s<k>__qdtype                the payloads' dtypes, in coded order
  <run>__s<k>__scale, __scale2       per coded key [kind, fp32 bits]: kind 0 a Python float, 1 the 0-dim tensor of
                                     the zero branch, 2 an int (the value itself in the second column)
  <run>__s<k>__size, __rand_calls    QuantParameters.size, the number of rand_like calls
  <run>__s<k>__pass__<name>          the ndim <= 1 entries the reference passes through
  <run>__s<k>__h__<name> / __hsha__  the hidden state after step k
"""

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import broadcast_cases as bc  # noqa: E402
import broadcast_stoch_cases as bsc  # noqa: E402
import delta_cases  # noqa: E402
from make_golden_stoch import CODECS, scale_record  # noqa: E402
from ref_loader import load_reference  # noqa: E402

OUT = os.path.join(HERE, "broadcast_stoch_small.npz")
MAX_BYTES = 256 * 1024


def put(arrays: dict, prefix: str, name: str, a: np.ndarray) -> None:
    """prefix__<name> = a, or prefixsha__<name> = its SHA-256 when a is large."""
    if a.size > bc.SHA_ABOVE:
        arrays[f"{prefix}sha__{name}"] = np.array(bc.sha(a))
    else:
        arrays[f"{prefix}__{name}"] = a.copy()


def scale_row(v):
    rec = scale_record(v)
    if "int" in rec:
        return [2, rec["int"]]
    return [1 if rec.get("tensor") else 0, rec["bits"]]


def send_with(channel, update, planes):
    """channel.on_server_send(update) with rand_like answering from `planes` (one per shape)."""
    by_shape = {tuple(u.shape): torch.from_numpy(u.copy()) for u in planes.values()}
    assert len(by_shape) == len(planes), "one uniform plane per shape"
    calls = []
    orig = torch.rand_like

    def fake_rand_like(p, *a, **k):
        assert p.dtype == torch.float32
        calls.append(1)
        return by_shape[tuple(p.shape)].clone()

    torch.rand_like = fake_rand_like
    try:
        q_update, _ = channel.on_server_send(update)
    finally:
        torch.rand_like = orig
    return q_update, len(calls)


def main():
    torch.set_num_threads(8)
    ref = load_reference()
    print("torch", torch.__version__)
    h0, news = bc.inputs()
    order = [name for name, _, _ in delta_cases.DICT_SHAPES]
    new_order = order[::-1]
    arrays = {"order": np.array(order), "new_order": np.array(new_order), "coded": np.array(bsc.CODED)}
    for codec, bits in bsc.RUNS:
        run = f"{codec}_b{bits}"
        channel = getattr(ref.quant, CODECS[codec])(bits)
        hidden = {n: torch.from_numpy(h0[n].copy()) for n in order}
        for k, g_np in enumerate(news, 1):
            pre = f"{run}__s{k}"
            g = {n: torch.from_numpy(g_np[n].copy()) for n in new_order}
            if k == bc.STEPS:   # the frozen layer: g is exactly the hidden state
                g[bc.FROZEN] = hidden[bc.FROZEN].clone()
            update = ref.model.diff_parameters(hidden, g)
            q_update, ncalls = send_with(channel, update, bsc.uniforms(k))
            d_update, _ = channel.on_client_receive(q_update)
            ref.model.add_parameters_inpace(hidden, d_update, 1, 1, False)
            names = list(q_update.params.keys())
            arrays[f"{pre}__order"] = np.array(names)
            arrays[f"{pre}__size"] = np.array(q_update.size, dtype=np.int64)
            arrays[f"{pre}__rand_calls"] = np.array(ncalls, dtype=np.int64)
            arrays[f"{pre}__scale"] = np.array([scale_row(q_update.params[n].scale) for n in bsc.CODED], dtype=np.int64)
            arrays[f"{pre}__scale2"] = np.array([scale_row(q_update.params[n].scale_2) for n in bsc.CODED],
                                                dtype=np.int64)
            arrays[f"{pre}__qdtype"] = np.array([str(q_update.params[n].data.dtype).replace("torch.", "")
                                                 for n in bsc.CODED])
            for n in names:
                p = q_update.params[n]
                assert p.bits == bits
                if n in bsc.CODED:
                    put(arrays, f"{pre}__q", n, p.data.numpy().view(np.uint8))
                    put(arrays, f"{pre}__signs", n, p.signs.numpy())
                else:
                    assert p.scale == 0 and p.scale_2 == 0
                    arrays[f"{pre}__pass__{n}"] = p.data.numpy().copy()
                put(arrays, f"{pre}__h", n, hidden[n].numpy())
            if k == bc.STEPS:
                assert arrays[f"{pre}__scale"][bsc.CODED.index(bc.FROZEN)].tolist() == [1, 0], "the frozen norm is 0"
    np.savez_compressed(OUT, **arrays)
    size = os.path.getsize(OUT)
    print(f"wrote {OUT}: {size} bytes, {len(arrays)} arrays")
    assert size <= MAX_BYTES, f"{size} bytes: the fixture must stay within {MAX_BYTES}"


if __name__ == "__main__":
    main()
