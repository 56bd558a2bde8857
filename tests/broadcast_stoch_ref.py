"""QAFeL's broadcast through the stochastic channels restated in numpy: oracle/stoch_oracle.py's quantize and
dequantize functions composed with the hidden-state update, one tensor at a time.

    x = fp32(g - h); (q, signs, norm, min) = the codec's encode of x under the uniforms u;
    d = the codec's decode of exactly those bytes and scalars (+0 everywhere when norm == 0); h' = fp32(h + d)

test_broadcast_stoch_golden.py pins it to the executed reference (tests/golden/broadcast_stoch_small.npz); the GPU
tests compare the fused kernels and the channels with it.
"""

import numpy as np

import stoch_oracle as so


def encode(x: np.ndarray, codec: str, bits: int, u: np.ndarray):
    """(q, signs, norm, min factor or None) of one fp32 tensor as the reference's _quantize_tensor returns them."""
    levels = 2 ** bits - 1
    if codec == "rqsgd":
        norm = so.linf_norm(x)
        q, s = so.qsgd_quantize(x, levels, norm, u)
        return q, s, norm, (so.lminf_norm(x) if norm != 0 else None)
    norm = so.torch_l2_norm(x)
    q, s = (so.cnat_quantize(x, bits, norm, u) if codec == "cnat" else so.qsgd_quantize(x, levels, norm, u))
    return q, s, norm, None


def decode(q: np.ndarray, s: np.ndarray, codec: str, bits: int, norm, mn) -> np.ndarray:
    levels = 2 ** bits - 1
    if codec == "cnat":
        return so.cnat_dequantize(q.view(np.int8) if q.dtype == np.int8 else q, s, norm)
    if codec == "qsgd":
        return so.qsgd_dequantize(q, s, levels, norm)
    return so.rqsgd_dequantize(q, s, levels, norm, np.float32(0) if mn is None else mn)


def step(h: np.ndarray, g: np.ndarray, codec: str, bits: int, u: np.ndarray):
    """One tensor's broadcast: (q, signs, norm, min, h')."""
    with np.errstate(invalid="ignore", over="ignore"):
        x = (g - h).astype(np.float32)
        q, s, norm, mn = encode(x, codec, bits, u)
        d = decode(q, s, codec, bits, norm, mn)
        h2 = (h + d).astype(np.float32)
    return q, s, norm, mn, h2
