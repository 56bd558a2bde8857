"""The synchronous DELTA server step's golden cases, shared by make_golden_sync_delta.py (which executes the
reference over them) and the tests: the seeded global parameters g, the (channel, K) list, and the fixture's key
names. The client updates are make_golden_aggregate.py's (client_arrays / client_dict), so every case's mean is
the one tests/golden/aggregate.npz already pins."""

import json
import os

import numpy as np

import recipes
from make_golden_aggregate import BIASES, K_SLQ, K_SLQ4, K_STOCH, SHAPES, STOCH

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "sync_delta.npz")
MANIFEST = os.path.join(HERE, "sync_delta_manifest.json")
MAX_BYTES = 256 * 1024          # the two files together

G_SEED = 770_000
G_MULT = 0.05
COUNTER = 11                    # g's int64 bn.num_batches_tracked
COUNTER_NAME = "bn.num_batches_tracked"
# chosen elements of g: (tensor, flat index, fp32 bits)
G_SPECIAL = [("conv.weight", 0, 0x80000000),    # -0.0
             ("conv.weight", 1, 0x00001C8F),    # a denormal (about 1.02e-41)
             ("conv.weight", 2, 0x7F800000),    # +inf
             ("big.weight", 33, 0xFF800000),    # -inf, in a later chunk-relative tile position
             ("one.weight", 0, 0x80000000)]     # -0.0 in the one-element tensor

SLQ8_K = [1, 2, 5, 16, 17, 20, 64]
SLQ4_K = [5, 16]
STOCH_K = [5, 16]
assert set(SLQ8_K) <= set(K_SLQ) and set(SLQ4_K) <= set(K_SLQ4) and set(STOCH_K) <= set(K_STOCH)
# (channel tag as aggregate.npz names it, K, alpha, beta)
CASES = ([("slq8", k, 1.0, 1.0) for k in SLQ8_K] + [("slq4", k, 1.0, 1.0) for k in SLQ4_K]
         + [(c, k, 1.0, 1.0) for c in STOCH for k in STOCH_K]
         + [("slq8", 5, 0.4, 0.6), ("qsgd", 5, 0.4, 0.6)])
# cases whose every tensor is stored in full; elsewhere tensors above FULL_MAX elements have only their SHA-256
FULL_CASES = {("slq8", 16, 1.0, 1.0), ("qsgd", 5, 0.4, 0.6)}
FULL_MAX = 512
NAMES = list(SHAPES) + list(BIASES) + [COUNTER_NAME]


def g_arrays() -> dict:
    """The global parameters as numpy arrays, in an order that differs from the updates' (fc.bias first)."""
    out = {}
    for i, (name, shape) in enumerate(list(BIASES.items()) + list(SHAPES.items())):
        out[name] = recipes.randn(shape, G_SEED + i, G_MULT)
    for name, idx, bits in G_SPECIAL:
        out[name].reshape(-1).view(np.uint32)[idx] = bits
    out[COUNTER_NAME] = np.array(COUNTER, dtype=np.int64)
    return out


def case_tag(ch: str, k: int, alpha: float, beta: float) -> str:
    return f"{ch}__k{k}" if (alpha, beta) == (1.0, 1.0) else f"{ch}__k{k}__a{alpha}_b{beta}"


def axpby(g: np.ndarray, mean: np.ndarray, alpha: float, beta: float) -> np.ndarray:
    """fp32 (alpha * g) + (beta * mean) with three separate roundings, as torch computes the reference's statement:
    a Python scalar times an fp32 (or int64: promoted to fp32) tensor is an fp32 product."""
    f = np.float32
    with np.errstate(all="ignore"):
        a = (f(alpha) * np.asarray(g).astype(f)).astype(f)
        b = (f(beta) * np.asarray(mean).astype(f)).astype(f)
        return (a + b).astype(f)


def load():
    with open(MANIFEST) as fh:
        return np.load(FIXTURE), json.load(fh)
