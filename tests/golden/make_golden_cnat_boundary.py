"""Golden vectors for CNAT on every power-of-two band of its exponent rule, in fp32 / fp16 / bf16 / fp64, made by
EXECUTING the reference on the tensors of tests/cnat_boundary_cases.py.

Run in the build container (the reference tree exists only there):

    python tests/golden/make_golden_cnat_boundary.py

Encode. ``CNATChannel(bits).on_client_send`` runs in place (``Src/ADFL/Channel/quant.py:509-534`` loaded by
``ref_loader``) on every tensor, in the tensor's dtype, with ``torch.rand_like`` replaced, for the duration of the
call, by the tensor's placed uniforms. Recorded: the exponent and sign bytes (in construction order, before
cnat_boundary_cases' shuffle: runs compress; fp32's `inside` / `outside` hold mixed's elements, the reference's bytes
for them are asserted equal to mixed's here and not stored twice) and the payload's scale (fp64 bits of the Python
float, or the marker of the 0-dim tensor the norm == 0 branch returns).

Decode. Hand-made ``QuantParameter`` payloads carrying all 256 exponent bytes x signs {1, -1, 0} go through
``CNATChannel.on_server_receive`` (quant.py:537-545) under every norm of cnat_boundary_cases.DEC_NORMS; the fp32
outputs are recorded in full, and so is ``simple_aggregate`` (``Src/ADFL/model.py:221-234``) of that one decode, the
server's mean with K = 1.

No input is stored: the tests rebuild them from cnat_boundary_cases and check the SHA-256 recorded here.

Outputs (data only):
  tests/golden/cnat_boundary.npz             per encode case: e (i8), signs (i8); per decode case: deq, mean (f32)
  tests/golden/cnat_boundary_manifest.json   per tensor: size, input digest; per case: scale; the left-out counts
The archive is written with fixed member timestamps, so a second run reproduces it byte for byte.
"""

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import boundary_cases as bc  # noqa: E402
import cnat_boundary_cases as cb  # noqa: E402
from make_golden_stoch_boundary import write_npz  # noqa: E402
from ref_loader import load_reference  # noqa: E402

TDT = {cb.F32N: torch.float32, cb.F16N: torch.float16, cb.BF16N: torch.bfloat16, cb.F64N: torch.float64}


def to_torch(raw: np.ndarray, dtn: str) -> torch.Tensor:
    raw = np.ascontiguousarray(raw).reshape(-1)
    if raw.dtype == np.uint16:
        return torch.from_numpy(raw.view(np.int16).copy()).view(TDT[dtn])
    return torch.from_numpy(raw.copy())


def scale_record(scale) -> dict:
    if isinstance(scale, torch.Tensor):
        return {"tensor": True, "value": float(scale)}
    assert isinstance(scale, float)
    return {"f64_bits": int(np.array([scale], dtype=np.float64).view(np.uint64)[0])}


def run_encode(ref, t, bits):
    ch = ref.quant.CNATChannel(bits)
    x = to_torch(t.x, t.dtn).reshape(1, -1)
    ut = to_torch(t.u, t.dtn).reshape(1, -1)
    calls = []
    orig = torch.rand_like

    def fake_rand_like(p, *a, **k):
        assert p.shape == ut.shape and p.dtype == ut.dtype
        calls.append(1)
        return ut.clone()

    torch.rand_like = fake_rand_like
    try:
        qp, _ = ch.on_client_send({"w": x})
    finally:
        torch.rand_like = orig
    assert len(calls) == 1
    return qp.params["w"]


def run_decode(ref, norm):
    data = torch.from_numpy(bc.DEC_LEVELS.view(np.int8).copy()).reshape(1, -1)
    signs = torch.from_numpy(bc.DEC_SIGNS.copy()).reshape(1, -1)
    qp = ref.model.QuantParameters({}, 0)
    qp.params["w"] = ref.model.QuantParameter(data=data, bits=8, scale=float(norm), signs=signs, shape=data.shape,
                                              dtype=torch.float32, q_dtype=data.dtype)
    dec, _ = ref.quant.CNATChannel(8).on_server_receive(qp)
    out = dec["w"].numpy().reshape(-1)
    mean = ref.model.simple_aggregate([dec])["w"].numpy().reshape(-1)   # one client's update through the server's mean
    assert out.dtype == mean.dtype == np.float32 and out.size == mean.size == bc.DEC_LEVELS.size
    return out, mean


def main():
    torch.set_num_threads(1)
    ref = load_reference()
    arrays, cases, dec = {}, [], []
    for dtn, name, bits in cb.ENC_CASES:
        t = cb.tensor(dtn, name)
        p = run_encode(ref, t, bits)
        assert p.data.dtype == torch.int8 and p.signs.dtype == torch.int8 and p.data.numel() == t.n
        cname = cb.case_name(dtn, name, bits)
        case = {"name": cname, "dtype": dtn, "tensor": name, "bits": bits, "scale": scale_record(p.scale)}
        e, signs = p.data.numpy().reshape(-1), p.signs.numpy().reshape(-1)
        if t.src is None:
            arrays[f"{cname}__e"], arrays[f"{cname}__signs"] = t.unshuffle(e), t.unshuffle(signs)
        else:   # fp32 inside / outside: the same elements as mixed's, and the reference gives them the same bytes
            e_mixed, s_mixed = cb.recorded(arrays, dtn, name, bits)
            assert np.array_equal(e, e_mixed) and np.array_equal(signs, s_mixed), cname
            case["bytes_from"] = cb.case_name(dtn, "mixed", bits)
        cases.append(case)
    for nid, norm in cb.DEC_NORMS.items():
        arrays[f"dec_{nid}__deq"], arrays[f"dec_{nid}__mean"] = run_decode(ref, norm)
        norm_bits = int(np.array([norm], np.float32).view(np.uint32)[0])
        dec.append({"name": f"dec_{nid}", "norm_id": nid, "norm_bits": norm_bits})
    tensors = {dtn: {name: {"n": cb.tensor(dtn, name).n, "inputs_sha256": cb.tensor(dtn, name).digest()}
                     for name in cb.TENSOR_NAMES[dtn]} for dtn in cb.DTYPES}
    write_npz(cb.FIXTURE, arrays)
    with open(cb.MANIFEST, "w") as f:
        json.dump({"torch": torch.__version__, "generator": "tests/golden/make_golden_cnat_boundary.py",
                   "left_out": {dtn: len(cb.left_out(dtn)) for dtn in cb.DTYPES}, "tensors": tensors,
                   "encode": cases, "decode": dec}, f, indent=1)
        f.write("\n")
    print(f"{len(cases)} encode and {len(dec)} decode cases, {os.path.getsize(cb.FIXTURE)} bytes")


if __name__ == "__main__":
    main()
