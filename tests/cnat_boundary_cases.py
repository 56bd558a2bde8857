"""CNAT inputs placed on every power-of-two band of the exponent rule, in all four dtypes, listed once: the golden
generator (golden/make_golden_cnat_boundary.py) and the tests (test_cnat_boundary_golden.py,
test_gpu_cnat_boundary.py) take them from here. Pure numpy, deterministic; nothing here reads a band table.

The reference takes floor / ceil of log2(v), v = R(|x| + eps), in the tensor's dtype. The kernels restate that
as an integer rule: fl(log2 v) is the integer k exactly while v lies in a band of a few ulps around 2^k
(csrc/cnat_log2_table.h for fp32, csrc/cnat_log2_dt_table.h for fp16 / bf16 / fp64); the fp32 kernel also has a
fast form that decides without the table when v is outside a fixed window around every power of two, and flags
its wave (256 consecutive elements) otherwise.

x values, by dtype (each element carries k, the nearest power of two of its v, and v's ulp offset from 2^k):
  fp16, bf16  every bit pattern: the finite ones in `main` (+x, -x interleaved), NaN / inf in `special`;
  fp32        for every k in [-23, 128] every v within 64 ulps of 2^k on each side (below 2^k: ulps of the lower
              binade), as x with fl(|x| + 2^-23) == v;
  fp64        for every k in [-52, 1024]: 2^k and its neighbours, each edge of the band (found by scanning the
              oracle's log2 over +-512 ulps) with two values inside and two outside, and the values 512 ulps away.
A target v may be left out only when the monotone map x -> v steps over it (adjacent x give a v below and a v
above it: in [2, 4) the sum |x| + eps is a tie, which rounds to the even neighbour). Signs alternate; +0, -0, the
smallest and the largest denormal and the largest finite value are appended.

Uniforms: for every x, prob from the oracle's arithmetic, then u = the largest grid value <= prob (clipped to
[0, max]), one grid step down, one up, 0 and the grid maximum; repeats and out-of-range variants collapse.

fp32 placement: `inside` holds the elements the fast form's restated flag predicate marks, `outside` the others
(the only place the fast form decides near a band), `mixed` a fixed-seed shuffle of both with generic filler.
The predicate reads the window from the generated header, to sort elements only: expected bytes never depend
on it (those of `inside` / `outside` are read from mixed's record, element by element). fp64 has `main` (run at
8 bits) and `sub`, a one-in-eight subset (the other widths).

Every construction checks that it hit its target and raises otherwise.
"""

import hashlib
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for _p in (os.path.join(REPO, "oracle"),):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import stoch_dt_oracle as do  # noqa: E402
import stoch_oracle as so  # noqa: E402

FIXTURE = os.path.join(HERE, "golden", "cnat_boundary.npz")
MANIFEST = os.path.join(HERE, "golden", "cnat_boundary_manifest.json")
FP32_HEADER = os.path.join(REPO, "ad-federatedlearning_amd", "csrc", "cnat_log2_table.h")

F32N, F16N, BF16N, F64N = "float32", "float16", "bfloat16", "float64"
DTYPES = (F32N, F16N, BF16N, F64N)
DT = {F16N: do.DT_F16, BF16N: do.DT_BF16, F64N: do.DT_F64}
BITS = (8, 4, 3, 2, 9)
GRID_BITS = {F32N: 24, F16N: 11, BF16N: 8, F64N: 53}
MBITS = {F32N: 23, F16N: 10, BF16N: 7, F64N: 52}
BIAS = {F32N: 127, F16N: 15, BF16N: 127, F64N: 1023}
EPS = {F32N: 2.0 ** -23, F16N: 2.0 ** -10, BF16N: 2.0 ** -7, F64N: 2.0 ** -52}
K_RANGE = {F32N: (-23, 128), F16N: (-10, 16), BF16N: (-7, 128), F64N: (-52, 1024)}   # 2^kmax is the dtype's inf
F32_REACH = 64           # fp32: ulps placed on each side of every power of two
F64_SCAN = 512           # fp64: the band edges are looked for within this many ulps, and these two are placed
F64_SUB = 8              # fp64, bits != 8: every eighth x
WAVE_SPAN = 256          # one wave's 64 float4 groups
MIN_CLEAN_SPANS = 32
FILLER_N = 8192
SEARCH = (0, -1, 1, -2, 2)   # preimage candidates: the value nearest v - eps, then its neighbours

KINDS = ("band", "zero", "denormal", "max_finite", "special", "filler")
K_BAND, K_ZERO, K_DENORM, K_MAX, K_SPECIAL, K_FILLER = range(6)
VARIANTS = ("u=floor_grid(prob)", "u=one step down", "u=one step up", "u=0", "u=max")
V_EQ, V_DOWN, V_UP, V_ZERO, V_MAX = range(5)


# ------------------------------------------------------------------------------------------------
# the dtype's arithmetic (the oracles') on compute values: fp32 for fp32 / fp16 / bf16, fp64 for fp64
# ------------------------------------------------------------------------------------------------
def ctype(dtn):
    return np.float64 if dtn == F64N else np.float32


def raw_type(dtn):
    return {F32N: np.float32, F16N: np.uint16, BF16N: np.uint16, F64N: np.float64}[dtn]


def to_compute(raw, dtn):
    return np.asarray(raw, dtype=np.float32) if dtn == F32N else do.to_compute(raw, DT[dtn])


def from_compute(v, dtn):
    return np.asarray(v, dtype=np.float32) if dtn == F32N else do.from_compute(v, DT[dtn])


def position(v, dtn) -> np.ndarray:
    """The bit pattern of a non-negative value of the dtype as int64: consecutive values, consecutive integers."""
    if dtn == F32N:
        return np.asarray(v, dtype=np.float32).view(np.uint32).astype(np.int64)
    if dtn == F64N:
        return np.asarray(v, dtype=np.float64).view(np.int64)
    return do.from_compute(v, DT[dtn]).astype(np.int64)


def at_position(pos, dtn) -> np.ndarray:
    pos = np.asarray(pos, dtype=np.int64)
    if dtn == F32N:
        return pos.astype(np.uint32).view(np.float32)
    if dtn == F64N:
        return pos.view(np.float64)
    return do.to_compute(pos.astype(np.uint16), DT[dtn])


def pow2_position(k, dtn):
    """position(2^k); for k = kmax the dtype's inf."""
    return (np.asarray(k, dtype=np.int64) + BIAS[dtn]) << MBITS[dtn]


def label(pos, dtn):
    """(k, off): the power of two nearest to the value at `pos` and the value's ulp offset from it (below 2^k in
    ulps of the lower binade)."""
    pos = np.asarray(pos, dtype=np.int64)
    k = ((pos + (1 << (MBITS[dtn] - 1))) >> MBITS[dtn]) - BIAS[dtn]
    return k.astype(np.int32), (pos - pow2_position(k, dtn)).astype(np.int32)


def v_of(xa, dtn):
    """R(|x| + eps)."""
    with np.errstate(over="ignore", invalid="ignore"):
        if dtn == F32N:
            return np.asarray(xa, dtype=np.float32) + so.EPS32
        return do.R(xa + ctype(dtn)(EPS[dtn]), DT[dtn])


def log2_of(v, dtn):
    return so.log2_f32(v) if dtn == F32N else do.log2_dt(v, DT[dtn]).astype(ctype(dtn))


def prob_of(xa, dtn):
    """(prob, floor, ceil) in the oracle's arithmetic (stoch_oracle.cnat_quantize / stoch_dt_oracle.cnat_quantize)."""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        lg = log2_of(v_of(xa, dtn), dtn)
        f, c = np.floor(lg), np.ceil(lg)
        if dtn == F32N:
            return (so._pow2(c) - xa) / so._pow2(f), f, c
        dt = DT[dtn]
        return do.R(do.R(do._pow2(c, dt) - xa, dt) / do._pow2(f, dt), dt), f, c


def quantize(raw_x, dtn, bits, raw_u):
    """The oracle's CNAT bytes with a non-zero norm (the exponents do not depend on it)."""
    if dtn == F32N:
        return so.cnat_quantize(raw_x, bits, 1.0, raw_u)
    return do.cnat_quantize(raw_x, DT[dtn], bits, 1.0, raw_u)


# ------------------------------------------------------------------------------------------------
# x
# ------------------------------------------------------------------------------------------------
def _preimages(target, dtn):
    """For every target position of v: the position of an |x| with R(|x| + eps) == v among the value nearest
    v - eps and its two neighbours on each side (a non-zero x where there is one), or -1 where the map provably
    steps over the target. Raises for a miss without that proof."""
    ct = ctype(dtn)
    top = int(pow2_position(K_RANGE[dtn][1], dtn)) - 1                    # the largest finite value
    v = at_position(target, dtn)
    near = (v.astype(np.float64) - EPS[dtn]).astype(ct)                   # nearest value of the dtype to v - eps
    cand = np.clip(position(near, dtn)[:, None] + np.array(sorted(SEARCH))[None, :], 0, top)
    got = position(v_of(at_position(cand.reshape(-1), dtn), dtn), dtn).reshape(cand.shape)
    hit = got == target[:, None]
    out = np.full(target.size, -1, dtype=np.int64)
    for o in reversed(SEARCH):                                            # the earliest of SEARCH wins ...
        j = sorted(SEARCH).index(o)
        out = np.where(hit[:, j], cand[:, j], out)
    nonzero = hit & (cand > 0)                                            # ... but a non-zero x beats x == 0
    first_nz = np.where(nonzero.any(axis=1), cand[np.arange(target.size), nonzero.argmax(axis=1)], -1)
    out = np.where((out == 0) & (first_nz > 0), first_nz, out)
    missing = out < 0
    stepped = ((got[:, :-1] < target[:, None]) & (got[:, 1:] > target[:, None])
               & (cand[:, 1:] - cand[:, :-1] == 1)).any(axis=1)
    if (missing & ~stepped).any():
        bad = np.nonzero(missing & ~stepped)[0][:4]
        raise AssertionError(f"cnat_boundary_cases: {dtn}: no x for v at {[label(target[i], dtn) for i in bad]}")
    return out


_scan_cache = {}


def scanned_bands(dtn):
    """{k: (below, above)}: how many ulps under / over 2^k the oracle's fl(log2 v) still equals k, found by scanning
    +-F64_SCAN (fp64) or +-F32_REACH ulps; raises unless the band is contiguous and narrower than the scan."""
    if dtn in _scan_cache:
        return _scan_cache[dtn]
    kmin, kmax = K_RANGE[dtn]
    w = F64_SCAN if dtn == F64N else F32_REACH
    lo, hi = int(pow2_position(kmin, dtn)), int(pow2_position(kmax, dtn))
    offs = np.arange(-w, w + 1, dtype=np.int64)
    bands = {}
    for k in range(kmin, kmax + 1):
        pos = int(pow2_position(k, dtn)) + offs
        ok = (pos >= lo) & (pos < hi)
        inb = np.zeros(offs.size, dtype=bool)
        inb[ok] = log2_of(at_position(pos[ok], dtn), dtn) == k
        idx = np.nonzero(inb)[0]
        if k < kmax and not inb[w]:
            raise AssertionError(f"cnat_boundary_cases: {dtn}: fl(log2 2^{k}) != {k}")
        if idx.size == 0:                       # k == kmax with no value under inf rounding up to it
            bands[k] = (0, 0)
            continue
        a, b = int(idx.max()) - w, w - int(idx.min())
        if not inb[idx.min():idx.max() + 1].all() or b >= w or (a >= w and k < kmax) or (ok[0] and inb[0]):
            raise AssertionError(f"cnat_boundary_cases: {dtn}: the band of k = {k} is not inside the scan")
        bands[k] = (b, max(a, 0))
    _scan_cache[dtn] = bands
    return bands


def edge_offsets(b, a):
    """The band's last value on each side, one more inside, and the first two outside."""
    offs = {-b, -b - 1, -b - 2, a, a + 1, a + 2}
    if b >= 1:
        offs.add(-b + 1)
    if a >= 1:
        offs.add(a - 1)
    return offs


def _targets(dtn):
    """(position of v, k, off) of every placed target of fp32 / fp64, in order."""
    kmin, kmax = K_RANGE[dtn]
    lo, hi = int(pow2_position(kmin, dtn)), int(pow2_position(kmax, dtn))
    pos, ks = [], []
    for k in range(kmin, kmax + 1):
        if dtn == F32N:
            offs = range(-F32_REACH, F32_REACH + 1)
        else:
            b, a = scanned_bands(dtn)[k]
            offs = sorted(edge_offsets(b, a) | {-1, 0, 1, -F64_SCAN, F64_SCAN})
        p = int(pow2_position(k, dtn)) + np.array(list(offs), dtype=np.int64)
        p = p[(p >= lo) & (p < hi)]             # under eps no x maps there; at or above inf is no target
        pos.append(p)
        ks.append(np.full(p.size, k, dtype=np.int32))
    pos, ks = np.concatenate(pos), np.concatenate(ks)
    return pos, ks, (pos - pow2_position(ks, dtn)).astype(np.int32)


class Elements:
    """One dtype's elements in construction order, already expanded by the uniform variants: x, u (stored form:
    fp32 / uint16 bits / fp64), k, off, var, kind per element, base (the index of the element's x in the
    unexpanded list) and, for fp32 / fp64, left_out = [(k, off)] of the targets the map steps over."""

    def __init__(self, dtn, special=False):
        self.dtn = dtn
        ct = ctype(dtn)
        self.left_out = []
        if special:
            xs, kind = self._special(), None
        elif dtn in (F16N, BF16N):
            n_fin = int(pow2_position(K_RANGE[dtn][1], dtn))
            p = np.arange(n_fin, dtype=np.int64)
            raw = np.stack([p, p | 0x8000], axis=1).reshape(-1).astype(np.uint16)
            xs = to_compute(raw, dtn)
            kind = np.full(xs.size, K_BAND, np.int8)
            kind[xs == 0] = K_ZERO
        else:
            tpos, tk, toff = _targets(dtn)
            xpos = _preimages(tpos, dtn)
            keep = xpos >= 0
            self.left_out = list(zip(tk[~keep].tolist(), toff[~keep].tolist()))
            xa = at_position(xpos[keep], dtn)
            if not np.array_equal(position(v_of(xa, dtn), dtn), tpos[keep]):
                raise AssertionError(f"cnat_boundary_cases: {dtn}: an x misses its target")
            xs = xa * np.where(np.arange(xa.size) % 2 == 0, ct(1), ct(-1))
            top = int(pow2_position(K_RANGE[dtn][1], dtn)) - 1
            dmax = (1 << MBITS[dtn]) - 1
            extra = np.concatenate([np.array([0.0, -0.0], dtype=ct), at_position([1, dmax, top], dtn)])
            kind = np.concatenate([np.full(xs.size, K_BAND, np.int8),
                                   np.array([K_ZERO, K_ZERO, K_DENORM, K_DENORM, K_MAX], np.int8)])
            xs = np.concatenate([xs, extra]).astype(ct)
        if kind is None:
            kind = np.full(xs.size, K_SPECIAL, np.int8)
        self._expand(xs.astype(ct), kind)

    def _special(self):
        dtn = self.dtn
        if dtn in (F16N, BF16N):
            p = np.arange(int(pow2_position(K_RANGE[dtn][1], dtn)), 0x8000, dtype=np.int64)
            return to_compute(np.stack([p, p | 0x8000], axis=1).reshape(-1).astype(np.uint16), dtn)
        ct = ctype(dtn)
        return np.array([np.inf, -np.inf, np.nan, -np.nan, 1.0, -3.0], dtype=ct)   # two finite ones beside them

    def _expand(self, xs, kind):
        dtn = self.dtn
        g_bits = GRID_BITS[dtn]
        xa = np.abs(xs)
        prob, f, c = prob_of(xa, dtn)
        step, u_max = 2.0 ** -g_bits, 1.0 - 2.0 ** -g_bits
        with np.errstate(invalid="ignore"):
            g = np.floor(np.clip(prob.astype(np.float64), 0.0, u_max) * 2.0 ** g_bits) * step   # exact in fp64
        cand = np.stack([g, g - step, g + step, np.zeros_like(g), np.full_like(g, u_max)], axis=1)
        with np.errstate(invalid="ignore"):
            valid = np.isfinite(cand) & (cand >= 0) & (cand <= u_max)
        for j in range(1, 5):                                  # repeats collapse onto the earlier variant
            for i in range(j):
                valid[:, j] &= ~(valid[:, i] & (cand[:, i] == cand[:, j]))
        row, col = np.nonzero(valid)                           # row-major: an x's variants stay together
        self.base = row.astype(np.int64)
        self.n_x = xs.size
        self.x = from_compute(xs[row], dtn)
        u = cand[row, col].astype(ctype(dtn))
        if not np.array_equal(u.astype(np.float64), cand[row, col]):
            raise AssertionError(f"cnat_boundary_cases: {dtn}: a uniform is off the dtype's grid")
        self.u = from_compute(u, dtn)
        self.var = col.astype(np.int8)
        self.kind = kind[row]
        with np.errstate(invalid="ignore"):
            self.k, self.off = label(position(np.where(np.isnan(xa), 0, v_of(xa, dtn)), dtn), dtn)
        self.k, self.off = self.k[row], self.off[row]
        self.n = self.x.size
        # the variants sit on the strict `<`: one step down takes the floor; on the grid, u == prob takes the ceil
        e8, _ = quantize(self.x, dtn, 8, self.u)
        fin = np.isfinite(prob) & (xs != 0)
        clamp = lambda t: do.to_i8(np.clip(np.where(np.isnan(t), 0, t), -128, 127))   # noqa: E731
        down = fin[row] & (self.var == V_DOWN)
        eq = fin[row] & (self.var == V_EQ) & (g == prob)[row]
        if not (np.array_equal(e8[down], clamp(f)[row][down]) and np.array_equal(e8[eq], clamp(c)[row][eq])
                and (down.any() and eq.any() or not (kind == K_BAND).any())):
            raise AssertionError(f"cnat_boundary_cases: {dtn}: the u variants do not sit on the strict `<`")

    def take(self, idx):
        """The sub-list `idx` (element indices) as a Tensor's fields."""
        return {f: getattr(self, f)[idx] for f in ("x", "u", "k", "off", "var", "kind", "base")}


# ------------------------------------------------------------------------------------------------
# the fp32 fast form's flag, restated (for placement only)
# ------------------------------------------------------------------------------------------------
def fast_window():
    """(kCnatMaxBelow, kCnatMaxAbove) as the generated header states them."""
    text = open(FP32_HEADER).read()
    below = re.search(r"kCnatMaxBelow = (\d+)u;", text)
    above = re.search(r"kCnatMaxAbove = (\d+)u;", text)
    if not below or not above:
        raise AssertionError("cnat_boundary_cases: the fp32 header does not state its window")
    return int(below.group(1)), int(above.group(1))


def fast_form_flags(x) -> np.ndarray:
    """cnat_exp_fast's `bad` restated: True where an element sends its wave to the exact form."""
    below, above = fast_window()
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.abs(x) + so.EPS32
        bits = v.view(np.uint32).astype(np.int64)
        return (x != 0) & (~(v < np.float32(2.0 ** 127)) | (((bits + below) & 0x7FFFFF) <= above + below))


# ------------------------------------------------------------------------------------------------
# tensors
# ------------------------------------------------------------------------------------------------
class Tensor:
    """One tensor as the reference and the kernels take it. Fields in the tensor's order: x, u (stored form), k, off,
    var, kind. perm: tensor[i] = construction[perm[i]] (None: the tensor is in construction order, the
    fixture's); src: for fp32's `inside` / `outside`, the construction index in `mixed` of every element — their
    expected bytes are read from mixed's record through it, so they do not depend on the window that sorted
    them; flags: fp32 only."""

    def __init__(self, dtn, name, fields, perm=None, src=None):
        self.dtn, self.name, self.perm, self.src = dtn, name, perm, src
        for f, a in fields.items():
            setattr(self, f, a if perm is None else a[perm])
        self.n = self.x.size
        self.flags = fast_form_flags(self.x) if dtn == F32N else None

    def shuffle(self, a_c):
        return a_c if self.perm is None else a_c[self.perm]

    def unshuffle(self, a):
        if self.perm is None:
            return a
        out = np.empty_like(a)
        out[self.perm] = a
        return out

    def digest(self) -> str:
        x, u = np.ascontiguousarray(self.x), np.ascontiguousarray(self.u)
        return hashlib.sha256(x.tobytes() + u.tobytes()).hexdigest()

    def clean_spans(self) -> int:
        """Whole 256-element spans without a flagged element."""
        m = self.n // WAVE_SPAN * WAVE_SPAN
        return int((~self.flags[:m].reshape(-1, WAVE_SPAN).any(axis=1)).sum())

    def describe(self, i: int) -> str:
        xv = to_compute(self.x[i:i + 1], self.dtn)[0]
        uv = to_compute(self.u[i:i + 1], self.dtn)[0]
        flagged = "" if self.flags is None else f" flagged={bool(self.flags[i])}"
        return (f"{self.dtn} {self.name}[{i}] x={xv!r} u={uv!r} {KINDS[self.kind[i]]} k={self.k[i]} "
                f"ulps_from_2^k={self.off[i]} {VARIANTS[self.var[i]]}{flagged}")


TENSOR_NAMES = {F32N: ("mixed", "inside", "outside", "special"), F16N: ("main", "special"),
                BF16N: ("main", "special"), F64N: ("main", "sub", "special")}
_elements, _tensors = {}, {}


def elements(dtn, special=False) -> Elements:
    if (dtn, special) not in _elements:
        _elements[(dtn, special)] = Elements(dtn, special)
    return _elements[(dtn, special)]


def _filler_fields():
    r = np.random.default_rng(0xC4A7)
    x = (r.standard_normal(FILLER_N) * 10.0 ** r.uniform(-6, 3, FILLER_N)).astype(np.float32)
    u = (r.integers(0, 1 << 24, FILLER_N).astype(np.float64) * 2.0 ** -24).astype(np.float32)
    k, off = label(position(v_of(np.abs(x), F32N), F32N), F32N)
    return {"x": x, "u": u, "k": k, "off": off, "var": np.full(FILLER_N, -1, np.int8),
            "kind": np.full(FILLER_N, K_FILLER, np.int8), "base": np.full(FILLER_N, -1, np.int64)}


def _build(dtn, name) -> Tensor:
    if name == "special":
        el = elements(dtn, True)
        return Tensor(dtn, name, el.take(np.arange(el.n)))
    el = elements(dtn)
    if dtn == F32N:
        flags = fast_form_flags(el.x)
        if name == "inside":
            t = Tensor(dtn, name, el.take(np.nonzero(flags)[0]), src=np.nonzero(flags)[0])
            if not t.flags.all() or t.clean_spans() != 0:
                raise AssertionError("cnat_boundary_cases: `inside` holds an unflagged element")
            return t
        if name == "outside":
            t = Tensor(dtn, name, el.take(np.nonzero(~flags)[0]), src=np.nonzero(~flags)[0])
            far = (t.kind == K_BAND) & ((t.off < -fast_window()[0]) | (t.off > fast_window()[1]))
            if t.flags.any() or t.clean_spans() < MIN_CLEAN_SPANS or not far.any():
                raise AssertionError("cnat_boundary_cases: `outside` misses its placement")
            return t
        fill = _filler_fields()
        both = {f: np.concatenate([a, fill[f]]) for f, a in el.take(np.arange(el.n)).items()}
        t = Tensor(dtn, name, both, perm=np.random.default_rng(0xC4A8).permutation(el.n + FILLER_N))
        spans = t.flags[:t.n // WAVE_SPAN * WAVE_SPAN].reshape(-1, WAVE_SPAN)
        if not (spans.any(axis=1) & ~spans.all(axis=1)).any():
            raise AssertionError("cnat_boundary_cases: no span of `mixed` mixes flagged and unflagged elements")
        return t
    if name == "sub":
        return Tensor(dtn, name, el.take(np.nonzero(el.base % F64_SUB == 0)[0]))
    return Tensor(dtn, name, el.take(np.arange(el.n)))


def tensor(dtn, name) -> Tensor:
    if (dtn, name) not in _tensors:
        _tensors[(dtn, name)] = _build(dtn, name)
    return _tensors[(dtn, name)]


def bits_for(dtn, name):
    """The bit widths a tensor runs at: fp64's full set at 8 bits only, its subset at the others."""
    if dtn == F64N and name != "special":
        return (8,) if name == "main" else tuple(b for b in BITS if b != 8)
    return BITS


ENC_CASES = [(dtn, name, bits) for dtn in DTYPES for name in TENSOR_NAMES[dtn] for bits in bits_for(dtn, name)]


def case_name(dtn, name, bits) -> str:
    return f"{dtn}_{name}_b{bits}"


def recorded(g, dtn, name, bits):
    """The reference's (exponent bytes, sign bytes) of a case, from the loaded fixture `g`, in the tensor's order."""
    t = tensor(dtn, name)
    if t.src is not None:
        rec = case_name(dtn, "mixed", bits)
        return g[rec + "__e"][t.src], g[rec + "__signs"][t.src]
    rec = case_name(dtn, name, bits)
    return t.shuffle(g[rec + "__e"]), t.shuffle(g[rec + "__signs"])


def left_out(dtn):
    """[(k, off)] of the targets the map x -> v steps over (fp16 / bf16 place x, not v: none)."""
    return elements(dtn).left_out if dtn in (F32N, F64N) else []


# ------------------------------------------------------------------------------------------------
# decode: all 256 exponent bytes x signs {1, -1, 0} (boundary_cases.DEC_LEVELS / DEC_SIGNS) under these norms
# ------------------------------------------------------------------------------------------------
F32_MAX = np.finfo(np.float32).max
DEC_NORMS = {
    "one": np.float32(1.0),
    "gen": np.float32(1.2345678),
    "f32_max": np.float32(F32_MAX),
    "gen_tiny": np.float32(np.float32(1.2345678) * np.float32(2.0 ** -126)),   # results denormal below exponent 0
    "denormal": np.asarray([0x0005A5A5], dtype=np.uint32).view(np.float32)[0],
    "inf": np.float32(np.inf),
    "nan": np.float32(np.nan),
}
_TINY = np.float32(2.0 ** -126)
if not (DEC_NORMS["gen_tiny"] >= _TINY and DEC_NORMS["gen_tiny"] / np.float32(2.0) < _TINY):
    raise AssertionError("cnat_boundary_cases: the tiny decode norm misses its place")


def first_diffs(got, want, limit: int = 6):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    if got.dtype == np.float32:
        ne = ~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want)))
    else:
        ne = got != want
    return np.nonzero(ne)[0][:limit]
