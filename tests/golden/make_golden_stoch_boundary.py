"""Golden vectors for QSGD / RQSGD at the decision boundaries of the level rule and of the fast division, made by
EXECUTING the reference on the tensors of tests/boundary_cases.py.

Run in the build container (the reference tree exists only there):

    python tests/golden/make_golden_stoch_boundary.py

Encode. ``RQSGDChannel(bits).on_client_send`` runs in place (``Src/ADFL/Channel/quant.py:330-398`` loaded by
``ref_loader``) on every encode tensor with ``torch.rand_like`` replaced, for the duration of the call, by the
tensor's placed uniforms. The anchor element makes the reference's own max-norm the intended one; that is asserted
bit for bit. Recorded: the level and sign bytes (in construction order, before boundary_cases' shuffle: runs
compress), the decoded tensor in the same order, the norm and the minimum factor (fp32 bits).

Decode. Hand-made ``QuantParameter`` payloads carrying the decode tensors' bytes and norms go through
``QSGDChannel`` / ``RQSGDChannel.on_server_receive`` (RQSGD with a normal and with a denormal minimum factor);
every output is recorded in full.

No input is stored: the tests regenerate them from boundary_cases and check the SHA-256 recorded here.

Outputs (data only):
  tests/golden/stoch_boundary.npz             per encode case: q (u8), signs (i8), deq (f32); per decode case: qsgd,
                                              rqsgd_normal, rqsgd_denormal (f32)
  tests/golden/stoch_boundary_manifest.json   per case: bits, norm id, size, fp32 bits of norm / min, input digest
The archive is written with fixed member timestamps, so a second run reproduces it byte for byte.
"""

import io
import json
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import boundary_cases as bc  # noqa: E402
from ref_loader import load_reference  # noqa: E402


def f32_bits(v) -> int:
    return int(np.array([float(v)], dtype=np.float32).view(np.uint32)[0])


def run_encode(ref, case):
    ch = ref.quant.RQSGDChannel(case.bits)
    t = torch.from_numpy(case.x.copy()).reshape(1, -1)
    ut = torch.from_numpy(case.u.copy()).reshape(1, -1)
    calls = []
    orig = torch.rand_like

    def fake_rand_like(p, *a, **k):
        assert p.shape == ut.shape and p.dtype == torch.float32
        calls.append(1)
        return ut.clone()

    torch.rand_like = fake_rand_like
    try:
        qp, _ = ch.on_client_send({"w": t})
    finally:
        torch.rand_like = orig
    assert len(calls) == 1
    dec, _ = ch.on_server_receive(qp)
    return qp.params["w"], dec["w"].numpy().reshape(-1)


def run_decode(ref, codec: str, bits: int, norm, mn=None):
    cls = ref.quant.QSGDChannel if codec == "qsgd" else ref.quant.RQSGDChannel
    data = torch.from_numpy(bc.DEC_LEVELS.copy()).reshape(1, -1)
    signs = torch.from_numpy(bc.DEC_SIGNS.copy()).reshape(1, -1)
    kw = {"scale_2": float(mn)} if codec == "rqsgd" else {}
    qp = ref.model.QuantParameters({}, 0)
    qp.params["w"] = ref.model.QuantParameter(data=data, bits=bits, scale=float(norm), signs=signs, shape=data.shape,
                                              dtype=torch.float32, q_dtype=data.dtype, **kw)
    dec, _ = cls(bits).on_server_receive(qp)
    out = dec["w"].numpy().reshape(-1)
    assert out.dtype == np.float32 and out.size == bc.DEC_LEVELS.size
    return out


def write_npz(path: str, arrays: dict):
    """np.savez_compressed's format with fixed member timestamps (numpy stamps the members with the clock)."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    torch.set_num_threads(1)
    ref = load_reference()
    arrays, enc, dec = {}, [], []
    for bits, nid in bc.ENC_CASES:
        c = bc.encode_case(bits, nid)
        p, deq = run_encode(ref, c)
        assert p.data.dtype == torch.uint8 and p.signs.dtype == torch.int8
        assert f32_bits(p.scale) == int(bc.bits_of(c.norm)), (bits, nid, p.scale, c.norm)   # the anchor's norm
        assert float(np.float32(p.scale)) == float(p.scale) and float(np.float32(p.scale_2)) == float(p.scale_2)
        name = f"enc_b{bits}_{nid}"
        arrays[f"{name}__q"] = c.unshuffle(p.data.numpy().reshape(-1))
        arrays[f"{name}__signs"] = c.unshuffle(p.signs.numpy().reshape(-1))
        arrays[f"{name}__deq"] = c.unshuffle(deq)
        enc.append({"name": name, "bits": bits, "norm_id": nid, "n": c.n, "norm_bits": f32_bits(p.scale),
                    "min_bits": f32_bits(p.scale_2), "inputs_sha256": bc.digest_inputs(c)})
    for bits, nid in bc.DEC_CASES:
        norm = bc.DEC_NORMS[nid]
        name = f"dec_b{bits}_{nid}"
        arrays[f"{name}__qsgd"] = run_decode(ref, "qsgd", bits, norm)
        for mid, mn in bc.DEC_MINS.items():
            arrays[f"{name}__rqsgd_{mid}"] = run_decode(ref, "rqsgd", bits, norm, mn)
        dec.append({"name": name, "bits": bits, "norm_id": nid, "norm_bits": int(bc.bits_of(norm)),
                    "min_bits": {mid: int(bc.bits_of(mn)) for mid, mn in bc.DEC_MINS.items()}})
    write_npz(bc.FIXTURE, arrays)
    with open(bc.MANIFEST, "w") as f:
        json.dump({"torch": torch.__version__, "generator": "tests/golden/make_golden_stoch_boundary.py",
                   "encode": enc, "decode": dec}, f, indent=1)
        f.write("\n")
    print(f"{len(enc)} encode and {len(dec)} decode cases, {os.path.getsize(bc.FIXTURE)} bytes")


if __name__ == "__main__":
    main()
