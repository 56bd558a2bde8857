"""Generate tests/golden/delta_small.npz: the send side of a DELTA round, pinned to the reference's own output.

Run in the build container (the reference tree exists only there), on the CPU:

    python tests/golden/make_golden_delta.py

Every expected value is produced by EXECUTING the reference in place through ``ref_loader``: its own
``diff_parameters(prev, new)`` (``Src/ADFL/model.py:350-358``) followed by ``SLQChannel(bits).on_client_send``
(``Src/ADFL/Channel/quant.py:61-104``), for bits 8 and 4, on the one small dict pair of ``delta_cases.dict_pair``.
Data only — inputs and expected outputs; no reference source is stored.

Arrays in the .npz (``<name>`` is a dict key):
  order                  the keys in params_prev's order (what diff_parameters iterates)
  new_order              the order params_new is built in (another one: the output must follow prev)
  prev__<name>, new__<name>   both inputs
  b<bits>__order         the keys of the reference's QuantParameters, in its order
  b<bits>__qnames        the quantized (ndim > 1) keys
  b<bits>__q__<name>     int_repr of every quantized payload
  b<bits>__scale_bits    uint32 bits of their fp32 scales, in b<bits>__qnames order
  b<bits>__size          QuantParameters.size
  pass__<name>           the ndim <= 1 entries the reference passes through (new - prev in their own dtype)
"""

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import delta_cases  # noqa: E402
from ref_loader import load_reference  # noqa: E402

OUT = os.path.join(HERE, "delta_small.npz")
MAX_BYTES = 256 * 1024


def scale_bits(scale) -> int:
    """The reference's scale is a Python float holding an exact fp32 value (quant.py:100-104)."""
    s32 = np.float32(scale)
    assert (np.isnan(scale) and np.isnan(s32)) or float(s32) == float(scale), scale
    return int(np.array([s32], dtype=np.float32).view(np.uint32)[0])


def main():
    torch.set_num_threads(8)
    ref = load_reference()
    print("torch", torch.__version__, "engine", torch.backends.quantized.engine)
    prev_np, new_np = delta_cases.dict_pair()
    order = [name for name, _, _ in delta_cases.DICT_SHAPES]
    new_order = order[::-1]
    prev = {n: torch.from_numpy(prev_np[n].copy()) for n in order}
    new = {n: torch.from_numpy(new_np[n].copy()) for n in new_order}
    arrays = {"order": np.array(order), "new_order": np.array(new_order)}
    for n in order:
        arrays[f"prev__{n}"] = prev_np[n]
        arrays[f"new__{n}"] = new_np[n]
    for bits in (8, 4):
        diff = ref.model.diff_parameters(prev, new)
        qp, _ = ref.quant.SLQChannel(bits=bits).on_client_send(diff)
        names = list(qp.params.keys())
        qnames = [n for n in names if qp.params[n].data.ndim > 1]
        arrays[f"b{bits}__order"] = np.array(names)
        arrays[f"b{bits}__qnames"] = np.array(qnames)
        arrays[f"b{bits}__scale_bits"] = np.array([scale_bits(qp.params[n].scale) for n in qnames], dtype=np.uint32)
        arrays[f"b{bits}__size"] = np.array(qp.size, dtype=np.int64)
        for n in names:
            p = qp.params[n]
            assert p.bits == bits
            if n in qnames:
                assert p.data.dtype == torch.qint8 and p.data.q_zero_point() == 0 and tuple(p.shape) == prev[n].shape
                arrays[f"b{bits}__q__{n}"] = p.data.int_repr().numpy()
            else:
                assert p.scale == 1
                v = p.data.numpy()
                if f"pass__{n}" in arrays:   # the passthrough entries do not depend on bits
                    assert np.array_equal(arrays[f"pass__{n}"], v) and arrays[f"pass__{n}"].dtype == v.dtype
                arrays[f"pass__{n}"] = v
    np.savez_compressed(OUT, **arrays)
    size = os.path.getsize(OUT)
    print(f"wrote {OUT}: {size} bytes, {len(arrays)} arrays")
    assert size <= MAX_BYTES, f"{size} bytes: the fixture must stay within {MAX_BYTES}"


if __name__ == "__main__":
    main()
