"""A numpy restatement of QAFeL's broadcast arithmetic (include/adfl_slq.h, adfl_slq_encode_delta_update_batched),
for the tests: x = fp32(g - h), the SLQ encode of x by the oracle, then h' = fp32(h + fp32(scale * c)) with c the
code the channel's decode reads back from the stored bytes — the int8 code itself, or nibble - 8 of the
pack_4bit byte (so a code 127 aliases into both nibbles, and an odd tensor's pad is a zero code)."""

import numpy as np

import slq_oracle as so


def readback_int4(q: np.ndarray) -> np.ndarray:
    """The codes unpack_4bit reads back from pack_4bit(q) (compression.py:35-66), per element of q."""
    flat = q.reshape(-1).astype(np.int64)
    if flat.size % 2:
        flat = np.concatenate([flat, [0]])        # the pad is a zero code
    hi, lo = flat[0::2] + 8, flat[1::2] + 8
    byte = ((hi << 4) | lo) & 0xff                # int8 wraparound; lo is not masked to a nibble
    out = np.empty(flat.size, dtype=np.int64)
    out[0::2] = ((byte >> 4) & 0xf) - 8
    out[1::2] = (byte & 0xf) - 8
    return out[:q.size].reshape(q.shape).astype(np.int8)


def update(h: np.ndarray, scale, codes: np.ndarray) -> np.ndarray:
    """fp32(h + fp32(scale * c)): two separately rounded fp32 operations."""
    with np.errstate(all="ignore"):
        d = (np.float32(scale) * codes.astype(np.float32)).astype(np.float32)
        return (h.astype(np.float32) + d).astype(np.float32)


def step(h: np.ndarray, g: np.ndarray, bits: int, packed: bool = False, encode=None):
    """One tensor of one broadcast: (int8 codes as encoded, fp32 scale, h')."""
    with np.errstate(all="ignore"):
        x = (g - h).astype(np.float32)
    q, scale = (encode or so.np_encode)(x, bits)
    q = np.asarray(q, dtype=np.int8).reshape(h.shape)
    return q, np.float32(scale), update(h, scale, readback_int4(q) if packed else q)
