"""The buffered servers' flush restated in numpy, and the dict, seeds, K, lr and staleness values of its tests,
listed once: the golden generator (golden/make_golden_flush.py) and the tests (test_flush_golden.py,
test_gpu_flush_ops.py, test_gpu_flush_channel.py) take them from here.

The restatement is what include/adfl_slq.h states for adfl_fedbuff_flush_batched / adfl_fadas_flush_batched: fp32
throughout, every operation rounded once. numpy's fp32 `*`, `+`, `/` and `sqrt` are IEEE-754 correctly rounded
(one SSE / AVX instruction each, never contracted); the fused multiply-add is computed exactly (``fma32``), not
through a rounded fp64 sum.
"""

import hashlib
import json
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "flush_small.npz")

F32 = np.float32

DICT_SHAPES = [
    ("conv.weight", (64, 3, 3, 3), np.float32),
    ("fc.weight", (10, 513), np.float32),
    ("emb.weight", (37, 33), np.float32),
    ("fc.bias", (10,), np.float32),
    ("bn.num_batches_tracked", (), np.int64),
]
FLOAT_NAMES = [n for n, _, dt in DICT_SHAPES if dt == np.float32]

K = 3                                   # max_buffer_size of both strategies
LR = 0.05
FEDBUFF_STALENESS = (0, 2, 5)           # FedBuff(3, 0.05, True): one flush
FADAS_STALENESS = ((0, 1, 2), (3, 25, 4), (0, 0, 1))   # FADAS(3, 0.05): three flushes; 25 > max_delay = 10
BETA_1, BETA_2, EPS, MAX_DELAY = 0.9, 0.999, 1e-8, 10  # FADAS's defaults (Strategy/fadas.py:17-21)

# |out - ref| <= MASK_C * ulp(|step * m' / den|) + ulp(|out|) where torch's CPU sqrt is an ulp off. Measured by
# golden/make_golden_flush.py on the fixture, the reference's params_prime against the restatement: the largest
# (|diff| - ulp(|out|)) / ulp(|upd|) is 0.938 (manifest["measured"]); twice that, because a one-ulp denominator
# error passes through one division and one addition, is 1.876, rounded up to the next integer. At most MASK_CAP
# of a tensor may be such elements (the reference alone measured 0.62 % on uniform data, 0.88 % at most here).
MASK_C = 2
MASK_CAP = 0.02


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


def update(strategy: str, rnd: int, k: int):
    """The k-th client update (a decoded delta) of flush `rnd` (0-based) of "fedbuff" / "fadas"."""
    base = 7000 if strategy == "fedbuff" else 8000
    return _dict(base + 100 * rnd + 10 * k, 1e-2, 1 + k)


def g_params(strategy: str, rnd: int):
    """The server's model at flush `rnd`."""
    return _dict((9000 if strategy == "fedbuff" else 9500) + 10 * rnd, 1.0, 41 + rnd)


def digest(a: np.ndarray) -> str:
    a = np.ascontiguousarray(a)
    return f"{a.dtype}:{'x'.join(map(str, a.shape))}:{hashlib.sha256(a.tobytes()).hexdigest()}"


# ---------------------------------------------------------------------------------------------------------
# the arithmetic
# ---------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fp32(a * b + c) with ONE rounding, exactly: the product of two fp32 values is exact in fp64 (48 bits);
    its sum with c is taken with Knuth's TwoSum, whose residual is exact; the fp64 sum is then made round-to-odd
    (an inexact even sum moves to its odd neighbour on the residual's side), and rounding a round-to-odd value
    of 53 >= 24 + 2 bits to fp32 equals rounding the exact value (Boldo & Melquiond)."""
    a, b, c = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        s = np.array(s, dtype=np.float64, ndmin=1)
        e = np.broadcast_to(e, s.shape)
        fix = np.isfinite(s) & (e != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32).reshape(np.broadcast(a, b, c).shape)


def staleness_factor(staleness: int) -> float:
    """FedBuff._staleness_factor (Strategy/fed_buff.py:114-115), a = 0.5."""
    return (1 + staleness) ** (-0.5)


def fedbuff_buffer(updates, staleness):
    """FedBuff's fp32 buffer entry after its updates (fed_buff.py:72-80): each scaled by fp32(factor), then
    summed (`mul_(1).add_(d, alpha=1)` is one fp32 addition)."""
    with np.errstate(all="ignore"):
        buf = None
        for u, s in zip(updates, staleness):
            d = F32(staleness_factor(s)) * np.asarray(u, np.float32)
            buf = d if buf is None else buf + d
        return buf


def fadas_buffer(updates):
    """FADAS's fp32 buffer entry (fadas.py:60-63): a plain fp32 sum of the updates."""
    with np.errstate(all="ignore"):
        buf = np.asarray(updates[0], np.float32)
        for u in updates[1:]:
            buf = buf + np.asarray(u, np.float32)
        return buf


def fedbuff_flush(buf, g, k: int, lr: float):
    """adfl_fedbuff_flush_batched per element."""
    with np.errstate(all="ignore"):
        b = np.asarray(buf, np.float32) / F32(k)
        return (F32(1.0) * np.asarray(g, np.float32)) + (F32(lr) * b)


def delay_lr(lr: float, max_staleness: int, max_delay: int = MAX_DELAY) -> float:
    """FADAS._apply_delay_correction (fadas.py:113-120), delay_adaptive=True."""
    return lr if max_staleness <= max_delay else min(lr, lr / max_staleness)


def fadas_scalars(beta_1: float, beta_2: float, eps: float, lr_t: float, rnd: int):
    """(beta1, 1 - beta1, beta2, 1 - beta2, sqrt(bias_correction_2), eps, step_size): Python doubles, as
    fadas.py:97-101,127-128 computes them; `rnd` is FADAS.round (1 at the first flush)."""
    return (beta_1, 1 - beta_1, beta_2, 1 - beta_2, math.sqrt(1 - beta_2 ** rnd), eps, lr_t / (1 - beta_1 ** rnd))


def fadas_flush(buf, g, m, v, v_hat, k: int, scalars, sqrt_ulps: int = 0):
    """adfl_fadas_flush_batched per element. Returns a dict: b (the averaged buffer), m, v, v_hat (the new
    moments), den, upd = fp32(fp32(step * m') / den) and out. Inputs are not modified. sqrt_ulps = -1 / +1: the
    square root moved to the fp32 value below / above the correctly rounded one (what a faithfully, not correctly,
    rounded sqrt may return), everything after it as stated."""
    b1, omb1, b2, omb2, sqrt_bc2, eps, step = (F32(s) for s in scalars)
    buf, g, m, v, v_hat = (np.asarray(x, np.float32) for x in (buf, g, m, v, v_hat))
    with np.errstate(all="ignore"):
        b = buf / F32(k)
        m1 = fma32(b, omb1, m * b1)
        v1 = fma32(omb2 * b, b, v * b2)
        h1 = np.maximum(v_hat, v1)                       # NaN when either is NaN, like torch.maximum
        root = np.sqrt(h1)
        if sqrt_ulps:
            root = np.nextafter(root, F32(np.inf if sqrt_ulps > 0 else -np.inf))
        den = (root / sqrt_bc2) + eps
        upd = (step * m1) / den
        out = g + upd
    return {"b": b, "m": m1, "v": v1, "v_hat": h1, "den": den, "upd": upd, "out": out}


def explained_by_sqrt(ref, buf, g, m, v, v_hat, k: int, scalars):
    """Elementwise: `ref` equals, bit for bit, FADAS's params_prime restated with the square root at the correctly
    rounded value or at one of its two fp32 neighbours. torch's CPU fp32 sqrt is faithfully but not correctly
    rounded, and how often it misses depends on the CPU (one ulp low on 0.6 % of inputs on one Xeon, one ulp off
    either way on 20 % on an EPYC 9575F): this is the exact set of values its params_prime may take."""
    ok = np.zeros(np.shape(ref), bool)
    for ulps in (0, -1, 1):
        ok |= same_bits(ref, fadas_flush(buf, g, m, v, v_hat, k, scalars, ulps)["out"])
    return ok


def same_bits(a, b):
    """Elementwise: identical fp32 bit patterns, or both NaN (IEEE 754 leaves the sign and payload of a NaN an
    operation produces to the implementation; x86 and gfx950 differ there and so do torch's own code paths)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def ulp(x):
    """The spacing of fp32 at |x|."""
    return np.spacing(np.abs(np.asarray(x, np.float32)))


def masked_close(out, ref, upd):
    """The bound inside the sqrt mask: |out - ref| <= MASK_C * ulp(|upd|) + ulp(|out|), in fp64."""
    d = np.abs(np.asarray(out, np.float64) - np.asarray(ref, np.float64))
    return d <= MASK_C * ulp(upd).astype(np.float64) + ulp(out).astype(np.float64)


_cache = {}


def fixture():
    if "z" not in _cache:
        z = np.load(FIXTURE)
        _cache["z"] = z
        _cache["m"] = json.loads(str(z["manifest"]))
    return _cache["z"], _cache["m"]
