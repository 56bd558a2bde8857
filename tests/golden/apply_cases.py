"""The dict, the runs and the coefficient cases of the decode + axpby tests, listed once: the golden generator
(make_golden_apply.py) and the tests (test_apply_golden.py, test_gpu_channel_apply.py) take them from here.

The inputs are regenerated from fixed seeds and are not stored in apply_small.npz (the fixture pins their
digests); what it stores are the reference's payloads and digests of everything the reference computed from
them. A full fp32 output of this dict is 160 KB and there are 40 of them, so the fixture keeps one SHA-256 per
output tensor (bit-exact all the same: the data holds no NaN) and the small entries in full.
"""

import hashlib
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "apply_small.npz")

DICT_SHAPES = [
    ("conv.weight", (64, 3, 3, 3), np.float32),
    ("fc.weight", (10, 513), np.float32),
    ("emb.weight", (1001, 33), np.float32),
    ("fc.bias", (10,), np.float32),
    ("bn.num_batches_tracked", (), np.int64),
]
CODED = [n for n, s, _ in DICT_SHAPES if len(s) > 1]

# run name -> (the reference channel's class, bits)
RUNS = {"slq_b8": ("SLQChannel", 8), "slq_b4": ("SLQChannel", 4), "qsgd_b8": ("QSGDChannel", 8),
        "rqsgd_b8": ("RQSGDChannel", 8), "cnat_b8": ("CNATChannel", 8)}

FEDASYNC_ALPHA = 0.6
FEDASYNC_STALENESS = (0, 1, 3, 7)        # FedAsync POLY, a = 0.5 (Strategy/fed_async.py:21,94-95)
FEDBUFF_STALENESS = (0, 2, 5)            # three updates of one buffer (Strategy/fed_buff.py:72-80,114-115)


def _dict(seed: int, scale: float, counter: int):
    out = {}
    for i, (name, shape, dt) in enumerate(DICT_SHAPES):
        if dt == np.int64:
            out[name] = np.array(counter, dtype=np.int64)
            continue
        n = int(np.prod(shape))
        v = np.random.default_rng(seed + i).standard_normal(n, dtype=np.float32) * np.float32(scale)
        out[name] = v.astype(np.float32).reshape(shape)
    return out


def update():
    """The client's update (what the reference's channels encode)."""
    return _dict(410, 1e-2, 3)


def base():
    """The server's model / the strategy's g_params."""
    return _dict(510, 1.0, 41)


def digest(a: np.ndarray) -> str:
    a = np.ascontiguousarray(a)
    return f"{a.dtype}:{'x'.join(map(str, a.shape))}:{hashlib.sha256(a.tobytes()).hexdigest()}"


def poly(staleness: int, a: float = 0.5) -> float:
    """FedAsync._poly / FedBuff._staleness_factor as Python computes them."""
    return (staleness + 1) ** (-a)


_cache = {}


def fixture():
    if "z" not in _cache:
        z = np.load(FIXTURE)
        _cache["z"] = z
        _cache["m"] = json.loads(str(z["manifest"]))
    return _cache["z"], _cache["m"]
