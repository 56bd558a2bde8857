"""QSGD / RQSGD inputs placed on the decision boundaries of the level rule and of the fast division, listed once:
the golden generator (golden/make_golden_stoch_boundary.py) and the tests (test_stoch_boundary_golden.py,
test_gpu_stoch_boundary.py) take them from here. Pure numpy, deterministic.

The fp32 kernels (csrc/stoch_device.h) compute a level as floor(scaled) + (u < scaled - floor(scaled)) with
scaled = RN(RN(s * |x|) / norm), in an exact form (a correctly rounded division) and in a fast form (a per-tensor
reciprocal with one correction step) that is valid only while the divisor and the dividend lie in [2^-60, 2^60]
(or the dividend is 0) and scaled < 2^24; an element outside that window flags its wave, which then takes the
exact form. The window is what keeps the quotient normal: 2^-60 / 2^60 = 2^-120 > 2^-126. A denormal quotient
can lie exactly half way between two fp32 values, and there the corrected reciprocal product rounds by the sign
of the reciprocal's error instead of to even (the `tie` elements below).

Encode tensors, one per (bits, norm id):
  anchor       |x| == norm with u = 0: RQSGD's own max-norm is then exactly `norm`;
  crossings    for every level k in 1..min(s, 255) (at 9 bits also 256, 257, 384, 510, 511) the fp32 x_k at which
               floor(scaled) steps from k - 1 to k (found by search with the restated arithmetic), and its two
               fp32 neighbours on each side;
  u variants   every such x with u in {prob, nextafter(prob, 0), nextafter(prob, 1), 0}, prob = scaled - floor;
  zeros, edges +0, -0, one denormal x; for the window-edge norms x with s * |x| on either side of 2^-60;
  ties         (2 bits, norm 3 * 2^58) x with s * |x| in [2^-70, 2^-60) whose quotient is a denormal tie.
The elements are shuffled with a fixed seed, so boundary elements fall in 4-element groups (fast form), chunk
heads and tails (exact form) alike. Short lists are repeated (signs flipped) to at least MIN_CORE elements, so
that the few flagged elements leave whole waves (256 consecutive elements) to the fast form.

Decode tensors, one per (bits in {4, 8}, norm id): all 256 level bytes x signs {1, -1, 0}.

Every construction checks that it hit its target and raises otherwise.
"""

import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.join(os.path.dirname(HERE), "oracle"),):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import stoch_oracle as so  # noqa: E402

F32 = np.float32
FIXTURE = os.path.join(HERE, "golden", "stoch_boundary.npz")
MANIFEST = os.path.join(HERE, "golden", "stoch_boundary_manifest.json")

ENC_BITS = (2, 4, 8, 9)
DEC_BITS = (4, 8)
WAVE_SPAN = 256          # one wave's 64 float4 groups
MIN_CORE = 1500          # crossings are repeated up to this many elements
SEARCH = 8               # the floor crossing is looked for within this many ulps of fp32(k * norm / s)
LO, HI = F32(2.0 ** -60), F32(2.0 ** 60)
U_MAX = np.nextafter(F32(1), F32(0))

# element kinds and uniform variants (the failure messages name them)
KINDS = ("crossing", "anchor", "zero", "denormal_x", "window_x", "tie")
K_CROSS, K_ANCHOR, K_ZERO, K_DENORM, K_WINDOW, K_TIE = range(6)
VARIANTS = ("u==prob", "u=prob-1ulp", "u=prob+1ulp", "u=0", "u=0.5")
V_EQ, V_BELOW, V_ABOVE, V_ZERO, V_HALF = range(5)


def f32_from_bits(b) -> np.ndarray:
    return np.asarray(b, dtype=np.uint32).view(np.float32)


def bits_of(v) -> np.ndarray:
    return np.asarray(v, dtype=np.float32).view(np.uint32)


DENORMAL_NORM = f32_from_bits(0x0005A5A5)[()]
DENORMAL_X = f32_from_bits(0x00000123)[()]

# norm id -> value; the per-bits ones (found by search) are added by enc_norms()
ENC_NORMS = {
    "one": F32(1.0),
    "pow2_m7": F32(2.0 ** -7),
    "all_ones": np.nextafter(F32(2), F32(0)),
    "one_plus_ulp": F32(1.0) + F32(2.0 ** -23),
    "gen_a": F32(1.2345678),
    "gen_b": F32(3.1415927e-3),
    "gen_c": F32(7.7777777e4),
    "win_lo": LO,
    "below_win_lo": np.nextafter(LO, F32(0)),
    "win_hi": HI,
    "above_win_hi": np.nextafter(HI, F32(np.inf)),
    "denormal": DENORMAL_NORM,
}
WINDOW_EDGE_INSIDE = ("win_lo", "win_hi")             # the divisor passes: flagged and unflagged elements mix
WINDOW_EDGE_OUTSIDE = ("below_win_lo", "above_win_hi", "denormal")   # the divisor fails: every element is flagged
TIE_NORM = F32(3.0 * 2.0 ** 58)                       # bits = 2 only: s * x is exact for the tie elements
TIE_M = tuple(1398103 + 2 * i for i in (0, 1, 2, 3, 1000000, 1000001, 2000000, 2000001))   # x = m * 2^-92


def scaled_of(xabs, s: int, norm) -> np.ndarray:
    """RN(RN(s * |x|) / norm): so.qsgd_quantize's arithmetic (quant.py:230 / :371)."""
    with np.errstate(all="ignore"):
        return (F32(s) * np.asarray(xabs, dtype=np.float32)) / F32(norm)


def _find_anchor_norm(s: int, above: bool) -> np.float32:
    """The first mantissa m = 1 + j * 2^-23 of a fixed scan with RN(RN(s * m) / m) > s (above) or < s."""
    j = np.arange(0x12345, 0x12345 + 4096, dtype=np.int64)
    m = f32_from_bits((0x3F800000 + j * 977 % (1 << 23)).astype(np.uint32))
    sc = (F32(s) * m) / m
    hit = np.nonzero(sc > F32(s) if above else sc < F32(s))[0]
    if hit.size == 0:
        raise AssertionError(f"boundary_cases: no norm with RN(RN(s*m)/m) {'>' if above else '<'} s for s = {s}")
    return m[hit[0]]


def enc_norms(bits: int) -> dict:
    s = 2 ** bits - 1
    norms = dict(ENC_NORMS)
    norms["gt_s"] = _find_anchor_norm(s, True)
    norms["lt_s"] = _find_anchor_norm(s, False)
    if bits == 2:
        norms["tie"] = TIE_NORM
    return norms


ENC_CASES = [(bits, nid) for bits in ENC_BITS for nid in enc_norms(bits)]


def fast_form_flags(x, s: int, norm) -> np.ndarray:
    """The `bad` conditions of make_div / div_fast / qsgd_level_fast restated: True where an element sends its
    wave to the exact form."""
    x = np.asarray(x, dtype=np.float32)
    b = F32(norm)
    if not (b >= LO and b <= HI):
        return np.ones(x.shape, dtype=bool)
    with np.errstate(all="ignore"):
        aa = F32(s) * np.abs(x)
        bad = ~((aa <= HI) & ((aa >= LO) | (aa == 0)))
        bad |= ~(scaled_of(np.abs(x), s, norm) < F32(16777216.0))
    return bad


def levels_of(s: int):
    """The levels whose crossings are placed: 1..min(s, 255), and past a byte the first levels that wrap through
    the u8 conversion, one in the middle and the last two."""
    return list(range(1, min(s, 255) + 1)) + ([256, 257, (s + 257) // 2, s - 1, s] if s > 255 else [])


def _crossings(s: int, norm: np.float32):
    """For every level k of levels_of(s): the bit pattern of the smallest fp32 x <= norm with floor(scaled) >= k,
    or -1 when there is none (k = s against a norm with RN(RN(s * norm) / norm) < s). Raises when the step is not
    inside the search window."""
    k = np.array(levels_of(s), dtype=np.int64)
    nb = int(bits_of(norm))
    guess = bits_of((k.astype(np.float64) * float(norm) / s).astype(np.float32)).astype(np.int64)
    cand = np.clip(guess[:, None] + np.arange(-SEARCH, SEARCH + 1)[None, :], 0, nb)
    ge = np.floor(scaled_of(f32_from_bits(cand.astype(np.uint32)), s, norm)) >= k[:, None].astype(np.float32)
    if ge[:, 0].any():
        raise AssertionError(f"boundary_cases: s = {s}, norm = {norm!r}: a crossing lies below the search window")
    first = ge.argmax(axis=1)
    cross = np.where(ge.any(axis=1), cand[np.arange(k.size), first], -1)
    miss = np.nonzero(cross < 0)[0]
    if miss.size and not (miss.size == 1 and k[miss[0]] == s and cand[miss[0], -1] == nb):
        raise AssertionError(f"boundary_cases: s = {s}, norm = {norm!r}: no crossing for levels {k[miss]}")
    return k, cross


def _variants(x, s: int, norm, which=(V_EQ, V_BELOW, V_ABOVE, V_ZERO)):
    """(index into x, u, variant) for every requested variant of every element."""
    sc = scaled_of(np.abs(x), s, norm)
    with np.errstate(all="ignore"):
        prob = (sc - np.floor(sc)).astype(np.float32)
    idx, us, vs = [], [], []
    for v in which:
        keep = np.ones(x.size, dtype=bool)
        if v == V_EQ:
            u = prob
        elif v == V_BELOW:
            keep = prob > 0
            u = np.nextafter(prob, F32(0))
        elif v == V_ABOVE:
            u = np.minimum(np.nextafter(prob, F32(1)), U_MAX)
        elif v == V_ZERO:
            u = np.zeros_like(prob)
        else:
            u = np.full_like(prob, 0.5)
        keep &= np.isfinite(u)
        idx.append(np.nonzero(keep)[0])
        us.append(u[keep])
        vs.append(np.full(int(keep.sum()), v, dtype=np.int8))
    return np.concatenate(idx), np.concatenate(us).astype(np.float32), np.concatenate(vs)


class EncodeCase:
    """One encode tensor. x, u: the tensor (shuffled). k, off, var, kind: per element, the crossing's level (-1:
    none), the element's ulp offset from the crossing, its uniform variant and its kind. perm: tensor[i] =
    construction[perm[i]]; `unshuffle` puts a per-element array back into construction order (the fixture's)."""

    def __init__(self, bits: int, nid: str):
        self.bits, self.nid, self.s = bits, nid, 2 ** bits - 1
        self.norm = norm = F32(enc_norms(bits)[nid])
        s = self.s
        nb = int(bits_of(norm))
        k, cross = _crossings(s, norm)
        px, pk, po = [], [], []
        for kk, c in zip(k.tolist(), cross.tolist()):
            base, offs = (c, range(-2, 3)) if c >= 0 else (nb, range(-2, 1))
            for o in offs:
                if 1 <= base + o <= nb:
                    px.append(base + o)
                    pk.append(kk)
                    po.append(o)
        cx = f32_from_bits(np.array(px, dtype=np.uint32))
        ck, co = np.array(pk, dtype=np.int32), np.array(po, dtype=np.int8)
        self.crossing = dict(zip(k.tolist(), cross.tolist()))
        # every level with a crossing has an element on each side of it (by the restated arithmetic itself)
        fl = np.floor(scaled_of(cx, s, norm))
        for kk, c in self.crossing.items():
            m = ck == kk
            below, above = (fl[m] < kk).any(), (fl[m] >= kk).any()
            if not below or (c >= 0 and not above):
                raise AssertionError(f"boundary_cases: b{bits} {nid}: level {kk} lacks a side of its crossing")
        cx = cx * np.where(np.arange(cx.size) % 2 == 0, F32(1), F32(-1))      # alternating signs
        i, u, v = _variants(cx, s, norm)
        x_core, u_core, v_core, k_core, o_core = cx[i], u, v, ck[i], co[i]
        reps = -(-MIN_CORE // x_core.size)
        xs = [x_core * F32(-1 if r % 2 else 1) for r in range(reps)]
        parts = [(np.concatenate(xs), np.tile(u_core, reps), np.tile(k_core, reps), np.tile(o_core, reps),
                  np.tile(v_core, reps), K_CROSS)]

        def extra(xv, kind, which):
            xv = np.asarray(xv, dtype=np.float32)
            j, uu, vv = _variants(xv, s, norm, which)
            parts.append((xv[j], uu, np.full(j.size, -1, np.int32), np.zeros(j.size, np.int8), vv, kind))

        extra([0.0, -0.0], K_ZERO, (V_ZERO, V_HALF))
        if int(bits_of(DENORMAL_X)) < nb:
            extra([DENORMAL_X], K_DENORM, (V_EQ, V_BELOW))
        if nid in ("win_hi", "above_win_hi"):   # s * |x| on either side of 2^-60 (for win_lo: level 1's crossing)
            e = int(bits_of(F32(2.0 ** -60 / s)))
            wx = f32_from_bits(np.arange(e - 2, e + 3, dtype=np.uint32))
            extra(wx * np.array([1, -1, 1, -1, 1], np.float32), K_WINDOW, (V_EQ, V_BELOW))
        if nid == "tie":
            tx = (np.array(TIE_M, dtype=np.float64) * 2.0 ** -92).astype(np.float32)
            a = F32(s) * tx
            q = scaled_of(tx, s, norm)
            if not ((a >= F32(2.0 ** -70)).all() and (a < LO).all() and (q < F32(2.0 ** -126)).all()
                    and (a.astype(np.float64) == 3.0 * np.array(TIE_M, dtype=np.float64) * 2.0 ** -92).all()
                    and (q.astype(np.float64) * 2.0 ** 149 == np.rint(np.array(TIE_M) / 2.0)).all()):
                raise AssertionError("boundary_cases: the tie elements miss their target")
            extra(tx * np.where(np.arange(tx.size) % 2 == 0, F32(1), F32(-1)), K_TIE,
                  (V_EQ, V_BELOW, V_ABOVE, V_ZERO))
        anchor = (np.array([norm], np.float32), np.zeros(1, np.float32), np.array([-1], np.int32),
                  np.zeros(1, np.int8), np.array([V_ZERO], np.int8), K_ANCHOR)
        parts.insert(0, anchor)
        cat = lambda j, dt: np.concatenate([np.asarray(p[j]) for p in parts]).astype(dt)  # noqa: E731
        x_c, u_c = cat(0, np.float32), cat(1, np.float32)
        k_c, off_c, var_c = cat(2, np.int32), cat(3, np.int8), cat(4, np.int8)
        kind_c = np.concatenate([np.full(np.asarray(p[0]).size, p[5], np.int8) for p in parts])
        self.n = n = x_c.size
        self.perm = perm = np.random.default_rng(0xB0DA + 131 * bits + sum(map(ord, nid))).permutation(n)
        self.x, self.u = x_c[perm], u_c[perm]
        self.k, self.off, self.var, self.kind = k_c[perm], off_c[perm], var_c[perm], kind_c[perm]
        self.anchor = int(np.nonzero(perm == 0)[0][0])
        self.flags = fast_form_flags(self.x, s, norm)
        self._self_check()

    def unshuffle(self, a: np.ndarray) -> np.ndarray:
        out = np.empty_like(a)
        out[self.perm] = a
        return out

    def shuffle(self, a_c: np.ndarray) -> np.ndarray:
        return a_c[self.perm]

    def _self_check(self):
        tag = f"boundary_cases: b{self.bits} {self.nid}"
        a = self.anchor
        if not (np.abs(self.x).max() == self.norm and abs(self.x[a]) == self.norm and self.u[a] == 0):
            raise AssertionError(f"{tag}: the anchor is not the tensor's maximum")
        if not (self.var == V_EQ).any():
            raise AssertionError(f"{tag}: no element with u == prob")
        sc = scaled_of(self.norm, self.s, self.norm)
        if self.nid == "gt_s" and not (np.floor(sc) == self.s and sc > self.s):
            raise AssertionError(f"{tag}: RN(RN(s*norm)/norm) is not above s")
        if self.nid == "lt_s" and not sc < self.s:
            raise AssertionError(f"{tag}: RN(RN(s*norm)/norm) is not below s")
        nflag = int(self.flags.sum())
        if self.nid in WINDOW_EDGE_INSIDE:
            if nflag in (0, self.n):
                raise AssertionError(f"{tag}: {nflag} of {self.n} elements flagged")
            spans = [self.flags[i:i + WAVE_SPAN] for i in range(0, self.n, WAVE_SPAN)]
            if not any(f.any() and not f.all() for f in spans):
                raise AssertionError(f"{tag}: no 256-element span mixes flagged and unflagged elements")
        if self.nid in WINDOW_EDGE_OUTSIDE and nflag != self.n:
            raise AssertionError(f"{tag}: a divisor outside the window must flag every element")
        # the restated prob is so.qsgd_quantize's: u == prob stays, one ulp below rounds up
        q, _ = so.qsgd_quantize(self.x, self.s, self.norm, self.u)
        lo = so.to_u8(np.floor(scaled_of(np.abs(self.x), self.s, self.norm)))
        eq, below = self.var == V_EQ, self.var == V_BELOW
        if not (np.array_equal(q[eq], lo[eq]) and np.array_equal(q[below], (lo[below] + 1).astype(np.uint8))):
            raise AssertionError(f"{tag}: the u variants do not sit on the strict `<`")

    def describe(self, i: int) -> str:
        return (f"[{i}] x={self.x[i]!r} u={self.u[i]!r} {KINDS[self.kind[i]]} k={self.k[i]} "
                f"ulps_from_crossing={self.off[i]} {VARIANTS[self.var[i]]} flagged={bool(self.flags[i])}")


_enc_cache = {}


def encode_case(bits: int, nid: str) -> EncodeCase:
    if (bits, nid) not in _enc_cache:
        _enc_cache[(bits, nid)] = EncodeCase(bits, nid)
    return _enc_cache[(bits, nid)]


# ------------------------------------------------------------------------------------------------
# decode
# ------------------------------------------------------------------------------------------------
F32_MAX = np.finfo(np.float32).max
DEC_NORMS = {
    "one": F32(1.0),
    "all_ones": np.nextafter(F32(2), F32(0)),
    "gen_a": F32(1.2345678),
    "gen_b": F32(3.1415927e-3),
    "cross_hi": F32(2.0 ** 60 / 100.5),     # norm * l passes 2^60 between level bytes 100 and 101
    "cross_lo": F32(2.0 ** -60 / 100.5),    # ... and 2^-60
    "inf_above_200": F32(F32_MAX / F32(200.5)),   # norm * l is inf from level byte 201 on (inf * sign 0 = NaN)
    "f32_max": F32(F32_MAX),
    "denormal": DENORMAL_NORM,
    "zero": F32(0.0),
    "inf": F32(np.inf),
    "nan": F32(np.nan),
}
DEC_MINS = {"normal": F32(0.0123), "denormal": f32_from_bits(0x00000ABC)[()]}
DEC_LEVELS = np.repeat(np.arange(256, dtype=np.uint8), 3)
DEC_SIGNS = np.tile(np.array([1, -1, 0], dtype=np.int8), 256)
DEC_CASES = [(bits, nid) for bits in DEC_BITS for nid in DEC_NORMS]


def _check_decode_norms():
    l = np.arange(256, dtype=np.float32)
    with np.errstate(all="ignore"):
        hi, lo, ov = DEC_NORMS["cross_hi"] * l, DEC_NORMS["cross_lo"] * l, DEC_NORMS["inf_above_200"] * l
        top = DEC_NORMS["f32_max"] * F32(2)
    if not ((hi[1:] <= HI).any() and (hi > HI).any() and (lo[1:] < LO).any() and (lo >= LO).any()
            and np.isfinite(ov).any() and np.isinf(ov[255]) and np.isinf(top)):
        raise AssertionError("boundary_cases: a decode norm misses its window edge")


_check_decode_norms()


def digest_inputs(case: EncodeCase) -> str:
    return hashlib.sha256(case.x.tobytes() + case.u.tobytes()).hexdigest()


def first_diffs(got, want, limit: int = 6):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    if got.dtype == np.float32:
        ne = ~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want)))
    else:
        ne = got != want
    return np.nonzero(ne)[0][:limit]
