"""Shared by the packed QSGD / RQSGD tests: a numpy restatement of the packed wire format (include/adfl_stoch.h,
"packed planes") and the state dicts the GPU tests encode.

Format, for a tensor of n elements with index i:
  sign plane   ceil(n / 8) bytes; bit i & 7 (least significant first) of byte i >> 3 is 1 exactly when the unpacked
               sign byte is -1; unused bits of the last byte are 0
  level plane  bits > 4: n bytes, the level byte; bits <= 4: ceil(n / 2) bytes, byte j = (level[2j] << 4) |
               level[2j + 1], the low nibble 0 when n is odd
"""

import numpy as np
import torch

# the byte, dword, wave-tile, chunk and resident-block edges
SIZES = [1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 8191, 8192, 8193, 65536, 65537]
ALONE = [1, 9, 65, 1025, 8193, 65537]           # run on their own as well (uniform shift 0: the vector path + tail)
ALIGNED = [8, 16, 64, 1024, 8192, 65536, 17]    # every compact offset a multiple of 4: the vector path in a bucket
VALUES = ["base", "zeros", "inf", "nan", "denormal"]
BITS = [8, 5, 4, 2, 1]
CODECS = ["qsgd", "rqsgd"]


def plane_bytes(n: int, bits: int):
    return (n if bits > 4 else (n + 1) // 2), (n + 7) // 8


def pack(levels: np.ndarray, neg: np.ndarray, bits: int):
    """(level plane, sign plane) of a tensor's level bytes and its `sign byte == -1` mask."""
    levels = np.ascontiguousarray(levels, dtype=np.uint8).reshape(-1)
    neg = np.ascontiguousarray(neg, dtype=bool).reshape(-1)
    n = levels.size
    assert neg.size == n and (bits > 4 or int(levels.max(initial=0)) <= 15)
    sb = np.zeros((n + 7) // 8, np.uint8)
    for b in range(8):
        part = neg[b::8].astype(np.uint8)
        sb[:part.size] |= part << b
    if bits > 4:
        return levels.copy(), sb
    padded = np.zeros(2 * ((n + 1) // 2), np.uint8)
    padded[:n] = levels
    return ((padded[0::2] << 4) | padded[1::2]).astype(np.uint8), sb


def unpack(lv: np.ndarray, sb: np.ndarray, n: int, bits: int):
    """(level bytes, `sign byte == -1` mask) of an n-element tensor's planes; asserts the unused bits are 0."""
    lv = np.ascontiguousarray(lv, dtype=np.uint8).reshape(-1)
    sb = np.ascontiguousarray(sb, dtype=np.uint8).reshape(-1)
    assert (lv.size, sb.size) == plane_bytes(n, bits), (lv.size, sb.size, n, bits)
    neg = ((sb[:, None] >> np.arange(8, dtype=np.uint8)[None, :]) & 1).astype(bool).reshape(-1)
    assert not neg[n:].any(), "unused sign bits must be 0"
    if bits > 4:
        return lv.copy(), neg[:n]
    levels = np.stack([lv >> 4, lv & 15], axis=1).reshape(-1)
    assert not levels[n:].any(), "the low nibble behind an odd tensor's last element must be 0"
    return levels[:n], neg[:n]


def values(kind: str, n: int, seed: int) -> torch.Tensor:
    """A (1, n) fp32 tensor of one of VALUES. base: normal(0, 1) with +0 and -0 planted, -0 at the last element."""
    g = np.random.default_rng(1000 * seed + n)
    x = g.standard_normal(n).astype(np.float32)
    if kind == "zeros":
        x[:] = 0.0
    elif kind == "denormal":
        x = (g.integers(1, 1 << 20, n).astype(np.uint32) | (g.integers(0, 2, n).astype(np.uint32) << 31)).view(np.float32)
    else:
        x[::7] = 0.0
        x[3::11] = -0.0
        x[-1] = -0.0
        if n > 1:
            x[0] = 0.0
        if kind == "inf":
            x[n // 2] = np.inf
        elif kind == "nan":
            x[n // 3] = np.nan
    return torch.from_numpy(x.copy()).reshape(1, n)


def big_dict(device="cpu"):
    """Every size x every value set, with a bias, an int64 counter and an empty (0, 3) tensor in between."""
    p = {}
    for k, kind in enumerate(VALUES):
        for n in SIZES:
            p[f"{kind}.{n}.weight"] = values(kind, n, k)
        if k == 0:
            p["fc.bias"] = torch.arange(10, dtype=torch.float32) - 4.5
            p["bn.num_batches_tracked"] = torch.tensor(7, dtype=torch.int64)
            p["empty.weight"] = torch.zeros(0, 3)
    return {n: t.to(device) for n, t in p.items()}


def aligned_dict(device="cpu"):
    """Sizes whose compact offsets are all multiples of 4 (the last one odd): the float4 path inside a bucket."""
    p = {f"w{n}.weight": values("base", n, 9) for n in ALIGNED}
    p["fc.bias"] = torch.linspace(-1, 1, 5)
    return {n: t.to(device) for n, t in p.items()}


def small_dict(device="cpu"):
    p = {"conv.weight": values("base", 27 * 64, 3).reshape(64, 3, 3, 3), "fc.weight": values("base", 1025, 4),
         "fc.bias": torch.linspace(-2, 2, 10), "bn.num_batches_tracked": torch.tensor(3, dtype=torch.int64),
         "odd.weight": values("base", 9, 5), "zero.weight": torch.zeros(2, 33)}
    return {n: t.to(device) for n, t in p.items()}


def compact_numel(params) -> int:
    return sum(t.numel() for t in params.values() if t.ndim > 1)


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Equal as int32 views where not NaN, NaN at the same positions; same shape, dtype and device type."""
    if a.shape != b.shape or a.dtype != b.dtype or a.device.type != b.device.type:
        return False
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.dtype != torch.float32:
        return torch.equal(a, b)
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(a[~na].view(torch.int32), b[~nb].view(torch.int32))


def same_scalar(a, b) -> bool:
    """Payload scales: the same type, and the same fp64 bits (NaN equals NaN) or the same 0-dim tensor."""
    if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
        return (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.dtype == b.dtype
                and a.shape == b.shape and same_bits(a.float(), b.float()))
    if type(a) is not type(b):
        return False
    fa, fb = np.float64(a), np.float64(b)
    return (np.isnan(fa) and np.isnan(fb)) or fa.view(np.uint64) == fb.view(np.uint64)


def assert_unpacks_to(packed, parent, bits: int, what: str = "") -> None:
    """`packed` (a Packed*Channel payload) unpacks to `parent` (the parent channel's payload of the same dict)."""
    assert list(packed.params) == list(parent.params), what
    size = 0
    for name, q in parent.params.items():
        p = packed.params[name]
        tag = f"{what} {name}"
        assert p.bits == q.bits == bits and p.shape == q.shape and p.dtype == q.dtype, tag
        coded = q.data.ndim > 1 and q.data.numel() > 0
        if not coded:   # passthrough, or the empty tensor's zero branch: field for field the parent's
            assert p.q_dtype == q.q_dtype and p.data.dtype == q.data.dtype and p.data.shape == q.data.shape, tag
            assert torch.equal(p.data.cpu(), q.data.cpu()) and p.data.device == q.data.device, tag
            assert p.signs.dtype == q.signs.dtype and torch.equal(p.signs.cpu(), q.signs.cpu()), tag
            assert same_scalar(p.scale, q.scale) and same_scalar(p.scale_2, q.scale_2), tag
            size += p.data.nbytes
            continue
        n = q.data.numel()
        assert p.q_dtype == torch.uint8 and p.data.dtype == torch.uint8 and p.signs.dtype == torch.uint8, tag
        assert p.data.ndim == 1 and p.signs.ndim == 1 and p.data.device == q.data.device == p.signs.device, tag
        levels, neg = unpack(p.data.cpu().numpy(), p.signs.cpu().numpy(), n, bits)
        np.testing.assert_array_equal(levels, q.data.cpu().numpy().reshape(-1).view(np.uint8), err_msg=tag)
        np.testing.assert_array_equal(neg, q.signs.cpu().numpy().reshape(-1) < 0, err_msg=tag)
        assert same_scalar(p.scale, q.scale), (tag, p.scale, q.scale)
        assert same_scalar(p.scale_2, q.scale_2), (tag, p.scale_2, q.scale_2)
        size += p.data.nbytes + p.signs.nbytes
    assert packed.size == size, what
