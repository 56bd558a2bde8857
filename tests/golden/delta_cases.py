"""The shapes and the dict pair of the send_delta tests, listed once: the golden generator
(make_golden_delta.py) and the tests (test_delta_golden.py, test_gpu_delta_encode.py, test_gpu_channel_delta.py)
all take them from here.

R is the largest tensor the one-launch (resident) delta encode takes: ADFL_SLQ_DELTA_RESIDENT_CHUNKS chunks
of ADFL_SLQ_CHUNK_ELEMS elements, read from include/adfl_slq.h.
"""

import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(os.path.dirname(HERE)), "include", "adfl_slq.h")


def header_constant(name: str) -> int:
    m = re.search(rf"^#define {name} (\d+)\s*$", open(HEADER).read(), flags=re.M)
    assert m, name
    return int(m.group(1))


CHUNK_ELEMS = header_constant("ADFL_SLQ_CHUNK_ELEMS")
DELTA_RESIDENT_CHUNKS = header_constant("ADFL_SLQ_DELTA_RESIDENT_CHUNKS")
R = DELTA_RESIDENT_CHUNKS * CHUNK_ELEMS

# every size at which a kernel takes another path: below / at / above the 16-element head, the 1024- and
# 2048-element wave tiles, the 8192-element chunk, and the resident bound R
SMALL_SIZES = [1, 15, 16, 17, 31, 33, 1023, 1024, 1025, 2047, 2049, 8191, 8192, 8193]
RESIDENT_SIZES = SMALL_SIZES + [R - 1, R]      # together: one resident launch
ALL_SIZES = RESIDENT_SIZES + [R + 1]           # R + 1 forces the two passes

# the dict pair of delta_small.npz, in params_prev's key order
DICT_SHAPES = [
    ("conv.weight", (16, 3, 3, 3), np.float32),
    ("conv.bias", (16,), np.float32),
    ("bn.num_batches_tracked", (), np.int64),
    ("fc.weight", (33, 17), np.float32),
    ("fc.bias", (33,), np.float32),
    ("col.weight", (8193, 1), np.float32),
    ("big.weight", (1, R + 1), np.float32),
]


def grid(n: int, seed: int, levels: int, step: float) -> np.ndarray:
    """n fp32 values on a grid of `levels` multiples of `step` around zero: few distinct values, so the
    fixture's large tensors compress (the .npz stays small) while every element still differs from its
    neighbours."""
    rng = np.random.default_rng(seed)
    return ((rng.integers(0, levels, size=n) - levels // 2).astype(np.float32) * np.float32(step)).astype(np.float32)


def dict_pair():
    """(prev, new) as name -> numpy array dicts in DICT_SHAPES order: the small weights are normal data with
    prev = new + 1e-3 * noise (the realistic case), the two large ones grid data (see grid) whose largest
    |new - prev| sits in the last chunk, the biases normal data, the counter 7 -> 12."""
    prev, new = {}, {}
    for i, (name, shape, dt) in enumerate(DICT_SHAPES):
        n = int(np.prod(shape)) if len(shape) else 1
        if dt == np.int64:
            prev[name], new[name] = np.array(7, dtype=np.int64), np.array(12, dtype=np.int64)
            continue
        if n > 4096:
            b = grid(n, 100 + i, 8, 0.125)
            a = (b + grid(n, 200 + i, 8, 2.0 ** -10)).astype(np.float32)
            a[n - 3] = b[n - 3] - np.float32(0.015625)   # the maximum of |new - prev|, in the last chunk
        else:
            rng = np.random.default_rng(300 + i)
            b = rng.standard_normal(n, dtype=np.float32)
            a = (b + np.float32(1e-3) * rng.standard_normal(n, dtype=np.float32)).astype(np.float32)
        prev[name], new[name] = a.reshape(shape), b.reshape(shape)
    return prev, new
