"""Generate tests/golden/broadcast_small.npz: QAFeL's broadcast, pinned to the reference's own output.

Run in the build container (the reference tree exists only there), on the CPU:

    python tests/golden/make_golden_broadcast.py

Every expected value is produced by EXECUTING the reference in place through ``ref_loader``: the four statements
of ``Src/ADFL/Server/qafel.py:156-180`` with the reference's own ``SLQChannel(bits)``, for bits 8 and 4,

    update   = diff_parameters(hidden_state, g_params)
    q_update = channel.on_server_send(update)
    d_update = channel.on_client_receive(q_update)
    add_parameters_inpace(hidden_state, d_update, 1, 1, False)

three times in a row, the hidden state carried from one broadcast to the next. The inputs are
``broadcast_cases.inputs()``: step 1 is ``delta_cases.dict_pair()`` (hidden = prev, g = new); steps 2 and 3 move
g again; in step 3 ``fc.weight`` of g is exactly the hidden state (a frozen layer: scale 0, codes 127, h + 0).
Data only — inputs and expected outputs; no reference source is stored.

The file has to stay within 256 KiB, so arrays of more than ``broadcast_cases.SHA_ABOVE`` elements are stored as
the SHA-256 of their bytes (as manifest.json does for large cases), except the payloads of step 1 and of
``col.weight``: the inputs (the recipe reproduces them), the hidden states, and ``big.weight``'s payloads of
steps 2 and 3.

Arrays in the .npz (``<name>`` is a dict key, k the step 1..3; ``X`` / ``Xsha`` is the array or its SHA-256):
  order, new_order                  the keys in hidden_state's order / the order g is built in (another one)
  h0__<name> / h0sha__<name>        the hidden state before step 1
  s<k>__new__<name> / s<k>__newsha__<name>   g of step k (step 3's fc.weight depends on bits:
                                    b<bits>__s3__new__fc.weight)
  b<bits>__qnames                   the quantized (ndim > 1) keys
  b<bits>__s<k>__order              the keys of the reference's QuantParameters, in its order
  b<bits>__s<k>__q__<name> / __qsha__   int_repr of every quantized payload
  b<bits>__s<k>__scale_bits         uint32 bits of their fp32 scales, in qnames order
  b<bits>__s<k>__size               QuantParameters.size
  b<bits>__s<k>__pass__<name>       the ndim <= 1 entries the reference passes through
  b<bits>__s<k>__h__<name> / __hsha__   the hidden state after step k
"""

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import broadcast_cases as bc  # noqa: E402
import delta_cases  # noqa: E402
from ref_loader import load_reference  # noqa: E402

OUT = os.path.join(HERE, "broadcast_small.npz")
MAX_BYTES = 256 * 1024
PAYLOAD_KEPT = "col.weight"   # the large tensor whose payloads are stored at every step


def scale_bits(scale) -> int:
    """The reference's scale is a Python float holding an exact fp32 value (quant.py:100-104)."""
    s32 = np.float32(scale)
    assert (np.isnan(scale) and np.isnan(s32)) or float(s32) == float(scale), scale
    return int(np.array([s32], dtype=np.float32).view(np.uint32)[0])


def put(arrays: dict, prefix: str, name: str, a: np.ndarray, keep: bool = False) -> None:
    """prefix__<name> = a, or prefixsha__<name> = its SHA-256 when a is large (and not `keep`)."""
    if a.size > bc.SHA_ABOVE and not keep:
        arrays[f"{prefix}sha__{name}"] = np.array(bc.sha(a))
    else:
        arrays[f"{prefix}__{name}"] = a.copy()


def main():
    torch.set_num_threads(8)
    ref = load_reference()
    print("torch", torch.__version__, "engine", torch.backends.quantized.engine)
    h0, news = bc.inputs()
    order = [name for name, _, _ in delta_cases.DICT_SHAPES]
    new_order = order[::-1]
    arrays = {"order": np.array(order), "new_order": np.array(new_order)}
    for n in order:
        put(arrays, "h0", n, h0[n])
        for k, g in enumerate(news, 1):
            if not (k == bc.STEPS and n == bc.FROZEN):
                put(arrays, f"s{k}__new", n, g[n])
    for bits in (8, 4):
        channel = ref.quant.SLQChannel(bits=bits)
        hidden = {n: torch.from_numpy(h0[n].copy()) for n in order}
        for k, g_np in enumerate(news, 1):
            g = {n: torch.from_numpy(g_np[n].copy()) for n in new_order}
            if k == bc.STEPS:   # the frozen layer: g is exactly the hidden state
                g[bc.FROZEN] = hidden[bc.FROZEN].clone()
                arrays[f"b{bits}__s{k}__new__{bc.FROZEN}"] = g[bc.FROZEN].numpy().copy()
            update = ref.model.diff_parameters(hidden, g)
            q_update, _ = channel.on_server_send(update)
            d_update, _ = channel.on_client_receive(q_update)
            ref.model.add_parameters_inpace(hidden, d_update, 1, 1, False)
            names = list(q_update.params.keys())
            qnames = [n for n in names if q_update.params[n].data.ndim > 1]
            arrays[f"b{bits}__qnames"] = np.array(qnames)
            arrays[f"b{bits}__s{k}__order"] = np.array(names)
            arrays[f"b{bits}__s{k}__scale_bits"] = np.array([scale_bits(q_update.params[n].scale) for n in qnames],
                                                            dtype=np.uint32)
            arrays[f"b{bits}__s{k}__size"] = np.array(q_update.size, dtype=np.int64)
            for n in names:
                p = q_update.params[n]
                assert p.bits == bits
                if n in qnames:
                    assert p.data.dtype == torch.qint8 and p.data.q_zero_point() == 0
                    put(arrays, f"b{bits}__s{k}__q", n, p.data.int_repr().numpy(), keep=k == 1 or n == PAYLOAD_KEPT)
                else:
                    assert p.scale == 1
                    arrays[f"b{bits}__s{k}__pass__{n}"] = p.data.numpy().copy()
                put(arrays, f"b{bits}__s{k}__h", n, hidden[n].numpy())
            if k == bc.STEPS:
                assert arrays[f"b{bits}__s{k}__scale_bits"][qnames.index(bc.FROZEN)] == 0, "the frozen scale is +0"
    np.savez_compressed(OUT, **arrays)
    size = os.path.getsize(OUT)
    print(f"wrote {OUT}: {size} bytes, {len(arrays)} arrays")
    assert size <= MAX_BYTES, f"{size} bytes: the fixture must stay within {MAX_BYTES}"


if __name__ == "__main__":
    main()
