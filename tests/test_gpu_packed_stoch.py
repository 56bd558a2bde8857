"""GPU: the packed QSGD / RQSGD channels and kernels (bits + 1 bits per weight) against the channels they pack.

* encode: with one seed, and with the same injected uniforms, unpack(Packed*Channel payload) is the parent channel's
  payload — levels, `sign byte == -1`, scale and scale_2 bit for bit, the other entries field for field, key order —
  for every size / value set / bits / codec, from CPU dicts and device dicts (packed_stoch_cases);
* golden: the reference's recorded uniforms give its recorded levels, signs and dequantized floats;
* decode / apply: on_server_receive, receive_axpby, receive_scaled and receive_scaled_add_ of the packed payload equal
  the parent's of its own, bit for bit; the hooks that are not fused equal the parent's results;
* the torch.ops.adfl_apply ops equal the adfl_amd.stoch functions.
"""

import copy
import functools
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from golden_util import same_f32

import packed_stoch_cases as pc

pytestmark = pytest.mark.gpu

from adfl_amd import flush, ops, stoch  # noqa: E402
from adfl_amd.Channel import (PackedQSGDChannel, PackedRQSGDChannel, QSGDChannel, RQSGDChannel,  # noqa: E402
                              UPackedQSGDChannel, UQSGDChannel)
from adfl_amd.model import QuantParameters  # noqa: E402

DEV = torch.device("cuda", 0)
PARENT = {"qsgd": QSGDChannel, "rqsgd": RQSGDChannel}
PACKED = {"qsgd": PackedQSGDChannel, "rqsgd": PackedRQSGDChannel}
CODEC_BITS = [(c, b) for c in pc.CODECS for b in pc.BITS]
DICTS = {"big": pc.big_dict, "aligned": pc.aligned_dict, "small": pc.small_dict}
SEED = 20240607


@functools.lru_cache(maxsize=None)
def params_of(which: str, where: str):
    return DICTS[which](DEV if where == "cuda" else "cpu")


@functools.lru_cache(maxsize=None)
def uniforms_of(which: str):
    n = pc.compact_numel(params_of(which, "cpu"))
    g = torch.Generator().manual_seed(n)
    return torch.rand(n + 64, generator=g).to(DEV)


def encode(cls, bits: int, params, mode: str, uniforms=None, seed: int = SEED):
    """(payload, torch's CPU generator state afterwards)."""
    ch = cls(bits)
    torch.manual_seed(seed)
    if mode == "seed":
        q = ch.on_client_send(params)[0]
    else:
        q = ch._quantize_params(params, bits, uniforms=uniforms)
    return q, torch.get_rng_state()


@functools.lru_cache(maxsize=None)
def parent_payload(codec: str, bits: int, which: str, where: str, mode: str):
    """The parent channel's payload of a shared dict: computed once, never modified."""
    return encode(PARENT[codec], bits, params_of(which, where), mode, uniforms_of(which) if mode != "seed" else None)


def packed_payload(codec: str, bits: int, which: str, where: str, mode: str):
    return encode(PACKED[codec], bits, params_of(which, where), mode, uniforms_of(which) if mode != "seed" else None)


# ---- 4. encode --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["big", "aligned"])
@pytest.mark.parametrize("codec,bits", CODEC_BITS)
def test_encode_unpacks_to_the_parents_payload(codec, bits, which):
    for where in ("cpu", "cuda"):
        for mode in ("seed", "uniforms"):
            want, rng_want = parent_payload(codec, bits, which, where, mode)
            got, rng_got = packed_payload(codec, bits, which, where, mode)
            pc.assert_unpacks_to(got, want, bits, f"{which} {where} {mode}")
            assert torch.equal(rng_got, rng_want), "the same draws from torch's CPU generator"
            for p in got.params.values():
                assert p.data.device.type == where and p.signs.device.type in (where, "cpu")
    again, _ = packed_payload(codec, bits, which, "cpu", "seed")
    first, _ = packed_payload(codec, bits, which, "cpu", "seed")
    for name, p in first.params.items():
        assert torch.equal(p.data, again.params[name].data) and torch.equal(p.signs, again.params[name].signs), name


@pytest.mark.parametrize("n", pc.ALONE)
@pytest.mark.parametrize("codec,bits", [("qsgd", 8), ("qsgd", 4), ("rqsgd", 5), ("rqsgd", 1)])
def test_encode_one_tensor_alone(codec, bits, n):
    for k, kind in enumerate(pc.VALUES):
        params = {"w": pc.values(kind, n, 20 + k)}
        u = torch.rand(n + 64, generator=torch.Generator().manual_seed(n + k)).to(DEV)
        for mode, where in (("seed", "cpu"), ("uniforms", "cuda")):
            p = params if where == "cpu" else {"w": params["w"].to(DEV)}
            want, _ = encode(PARENT[codec], bits, p, mode, u)
            got, _ = encode(PACKED[codec], bits, p, mode, u)
            pc.assert_unpacks_to(got, want, bits, f"{kind} {n} {mode}")


def test_encode_rejects_what_the_format_does_not_carry():
    ch = PackedQSGDChannel(8)
    for dt in (torch.float16, torch.bfloat16, torch.float64):
        with pytest.raises(NotImplementedError, match="'h.weight'"):
            ch.on_client_send({"a.weight": torch.randn(4, 4), "h.weight": torch.randn(4, 4).to(dt)})
    with pytest.raises(ValueError, match="fp32"):
        ch._quantize_params({"a.weight": torch.randn(4, 4)}, 8, uniforms=torch.rand(64, device=DEV).double())
    q = QSGDChannel(8).on_client_send({"a.weight": torch.randn(4, 4)})[0]
    with pytest.raises(ValueError, match="not a packed payload"):
        ch.on_server_receive(q)                                  # the parent's two byte planes are another format


# ---- 5. golden --------------------------------------------------------------------------------------------------
MANIFEST = json.load(open(os.path.join(GOLDEN, "stoch_manifest.json")))
ARR = np.load(os.path.join(GOLDEN, "stoch.npz"))
GOLD = [c for c in MANIFEST["cases"] if c["codec"] in pc.CODECS and c["bits"] <= 8]


def _scale(rec) -> np.float32:
    if "int" in rec:
        return np.float32(rec["int"])
    return np.array([rec["bits"]], np.uint32).view(np.float32)[0]


@pytest.mark.parametrize("c", GOLD, ids=[c["name"] for c in GOLD])
def test_golden_case(c):
    n_, bits, codec = c["name"], c["bits"], c["codec"]
    x, u, q_ref, s_ref, d_ref = (ARR[f"{n_}__{k}"].reshape(-1) for k in ("x", "u", "q", "signs", "deq"))
    n = x.size
    lay = ops.BucketLayout([n])
    xd, ud = torch.zeros(lay.total), torch.zeros(lay.total)   # the aligned layout's extent: n rounded up to 64
    xd[:n], ud[:n] = torch.from_numpy(x.copy()), torch.from_numpy(u.copy())
    xd, ud = xd.to(DEV), ud.to(DEV)
    norm = torch.tensor([_scale(c["scale"])], dtype=torch.float32, device=DEV)
    mins = torch.tensor([_scale(c["scale_2"])], dtype=torch.float32, device=DEV)
    if codec == "qsgd":   # the reference's own norm, as tests/test_gpu_stoch.py injects it
        lv, sb = stoch.quantize_packed_batched(codec, xd, lay, bits, norm, uniforms=ud)
    else:
        lv, sb, nr, mn = stoch.encode_packed_batched(codec, xd, lay, bits, uniforms=ud)
        assert same_f32(nr.cpu().numpy(), norm.cpu().numpy())
        if "tensor" not in c["scale"]:
            assert same_f32(mn.cpu().numpy(), mins.cpu().numpy())
    nl, ns = pc.plane_bytes(n, bits)
    levels, neg = pc.unpack(lv.cpu().numpy()[:nl], sb.cpu().numpy()[:ns], n, bits)
    np.testing.assert_array_equal(levels, q_ref.view(np.uint8))
    np.testing.assert_array_equal(neg, s_ref < 0)
    out = stoch.dequantize_packed_batched(codec, lv, sb, norm, lay, bits, mins=mins if codec == "rqsgd" else None)
    assert same_f32(out.cpu().numpy()[:n], d_ref)


# ---- 6. decode --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def parent_decode(codec: str, bits: int, which: str, where: str):
    return PARENT[codec](bits).on_server_receive(parent_payload(codec, bits, which, where, "seed")[0])[0]


@pytest.mark.parametrize("which", ["big", "aligned"])
@pytest.mark.parametrize("codec,bits", CODEC_BITS)
def test_decode_equals_the_parents_decode(codec, bits, which):
    """big: one tensor in every 64-element slot from offset 64 on (sign bytes 8-byte aligned, not 16), every tail."""
    for where in ("cpu", "cuda"):
        want = parent_decode(codec, bits, which, where)
        payload, _ = packed_payload(codec, bits, which, where, "seed")
        got, secs = PACKED[codec](bits).on_server_receive(payload)
        assert list(got) == list(want) and secs >= 0
        for name, t in want.items():
            assert pc.same_bits(got[name], t), (where, name)
            assert got[name].device == t.device
        assert got["fc.bias"].data_ptr() == params_of(which, where)["fc.bias"].data_ptr()   # passthrough, quant.py:112


def test_every_64_aligned_offset_decodes_and_applies():
    """Tensors of 1 .. 200 elements at consecutive 64-element slots: offsets that are multiples of 64 but not of
    128, every byte and nibble tail, through the three kernels directly."""
    sizes = list(range(1, 201, 3)) + [8192 + 64, 1024 + 32]
    lay, comp = ops.BucketLayout(sizes), ops.BucketLayout(sizes, align=1)
    assert (lay.offsets % 64 == 0).all() and (lay.offsets % 128 != 0).any()
    g = torch.Generator().manual_seed(5)
    xs = [torch.randn(n, generator=g) for n in sizes]
    flat_a, flat_c = torch.zeros(lay.total), torch.zeros(comp.total)
    for x, oa, oc in zip(xs, lay.offsets.tolist(), comp.offsets.tolist()):
        flat_a[oa:oa + x.numel()] = x
        flat_c[oc:oc + x.numel()] = x
    flat_a, flat_c = flat_a.to(DEV), flat_c.to(DEV)
    for codec, bits in (("qsgd", 8), ("rqsgd", 4), ("qsgd", 3), ("rqsgd", 7)):
        lv, sb, nr, mn = stoch.encode_packed_batched(codec, flat_a, lay, bits, seed=11, counter=3,
                                                     ushift=comp.offsets - lay.offsets)
        if codec == "qsgd":
            ql, qs = stoch.qsgd_quantize_batched(flat_c, comp, bits, nr, seed=11, counter=3)
            want = stoch.qsgd_decode_batched(ql, qs, nr, comp, bits)
        else:
            ql, qs, nr2, mn2 = stoch.rqsgd_encode_batched(flat_c, comp, bits, seed=11, counter=3)
            assert torch.equal(nr, nr2) and torch.equal(mn, mn2)
            want = stoch.rqsgd_decode_batched(ql, qs, nr, mn, comp, bits)
        out = stoch.dequantize_packed_batched(codec, lv, sb, nr, lay, bits, mins=mn)
        base = torch.randn(lay.total, generator=g).to(DEV)
        axp = torch.empty_like(base)
        stoch.dequantize_axpby_packed_batched(codec, lv, sb, nr, lay, bits, base, axp, 0.4, 0.6, mins=mn)
        lvh, sbh, qlh, qsh = (t.cpu().numpy() for t in (lv, sb, ql, qs))
        for n, oa, oc in zip(sizes, lay.offsets.tolist(), comp.offsets.tolist()):
            nl, ns = pc.plane_bytes(n, bits)
            lo = oa if bits > 4 else oa // 2
            levels, neg = pc.unpack(lvh[lo:lo + nl], sbh[oa // 8:oa // 8 + ns], n, bits)
            np.testing.assert_array_equal(levels, qlh[oc:oc + n], err_msg=f"{codec} {bits} {n}")
            np.testing.assert_array_equal(neg, qsh[oc:oc + n] < 0, err_msg=f"{codec} {bits} {n}")
            d = want[oc:oc + n]
            assert pc.same_bits(out[oa:oa + n], d), (codec, bits, n)
            assert pc.same_bits(axp[oa:oa + n], (0.4 * base[oa:oa + n]) + (0.6 * d)), (codec, bits, n)


# ---- 7. apply ---------------------------------------------------------------------------------------------------
def _bases(decoded, where: str, seed: int, misalign=None):
    g = torch.Generator().manual_seed(seed)
    out = {}
    for n, t in decoded.items():
        if t.dtype != torch.float32:
            out[n] = t.clone().to(DEV if where == "cuda" else "cpu")
            continue
        b = torch.randn(t.shape, generator=g)
        if n == misalign:   # contiguous, 4 bytes past a 16-byte boundary
            store = torch.empty(t.numel() + 1)
            store[1:] = b.reshape(-1)
            b = store[1:].view(t.shape)
            assert b.data_ptr() % 16 == 4
        out[n] = b.to(DEV) if where == "cuda" else b
    return out


@pytest.mark.parametrize("which", ["small", "aligned"])
@pytest.mark.parametrize("codec,bits", [("qsgd", 8), ("qsgd", 4), ("rqsgd", 8), ("rqsgd", 2)])
def test_apply_equals_the_parents(codec, bits, which):
    parent, packed = PARENT[codec](bits), PACKED[codec](bits)
    q_par = parent_payload(codec, bits, which, "cpu", "seed")[0]
    q_pak = packed_payload(codec, bits, which, "cpu", "seed")[0]
    decoded = parent_decode(codec, bits, which, "cpu")
    big = max(decoded, key=lambda n: decoded[n].numel())
    for where, misalign in (("cuda", None), ("cpu", None), ("cpu", big)):
        base = _bases(decoded, where, 3, misalign)
        want, _ = parent.receive_axpby(q_par, base, 0.4, 0.6)
        got, _ = packed.receive_axpby(q_pak, base, 0.4, 0.6)
        assert list(got) == list(want)
        for n in want:
            assert pc.same_bits(got[n], want[n]), ("axpby", where, misalign, n)
            assert got[n].data_ptr() != base[n].data_ptr() or got[n].numel() == 0
        for k in (1, 3):   # in place, into k models
            t_par = [_bases(decoded, where, 10 + j, misalign) for j in range(k)]
            t_pak = [{n: t.clone() for n, t in m.items()} for m in t_par]
            if misalign:
                for m in t_pak:   # clone() realigns: rebuild the misaligned tensor
                    m[misalign] = _bases({misalign: decoded[misalign]}, where, 0, misalign)[misalign].copy_(m[misalign])
            keep = [{n: t.data_ptr() for n, t in m.items()} for m in t_pak]
            # copies: the scaled routes scale a passthrough entry's own tensor in place (fed_buff.py:72-75)
            parent.receive_scaled_add_(copy.deepcopy(q_par), t_par, 0.37)
            packed.receive_scaled_add_(copy.deepcopy(q_pak), t_pak, 0.37)
            for a, b, ptrs in zip(t_pak, t_par, keep):
                for n in b:
                    assert pc.same_bits(a[n], b[n]), ("scaled_add_", where, misalign, k, n)
                    assert a[n].data_ptr() == ptrs[n]
    for where in ("cpu", "cuda"):
        want, _ = parent.receive_scaled(copy.deepcopy(parent_payload(codec, bits, which, where, "seed")[0]), -0.37)
        got, _ = packed.receive_scaled(copy.deepcopy(packed_payload(codec, bits, which, where, "seed")[0]), -0.37)
        assert list(got) == list(want)
        for n in want:
            assert pc.same_bits(got[n], want[n]), ("scaled", where, n)


# ---- 8. the hooks that are not fused ----------------------------------------------------------------------------
@pytest.mark.parametrize("codec,bits", [("qsgd", 8), ("rqsgd", 4)])
def test_non_fused_routes_equal_the_parents(codec, bits):
    parent, packed = PARENT[codec](bits), PACKED[codec](bits)
    params = params_of("small", "cpu")
    K = 3
    q_par = [encode(PARENT[codec], bits, params, "seed", seed=SEED + k)[0] for k in range(K)]
    q_pak = [encode(PACKED[codec], bits, params, "seed", seed=SEED + k)[0] for k in range(K)]
    decoded = parent.on_server_receive(q_par[0])[0]

    def same_dict(got, want, what):
        assert list(got) == list(want), what
        for n in want:
            assert pc.same_bits(got[n], want[n]), (what, n)

    for where in ("cpu", "cuda"):   # receive_add_
        t_par = [_bases(decoded, where, 40 + j) for j in range(2)]
        t_pak = [{n: t.clone() for n, t in m.items()} for m in t_par]
        parent.receive_add_(q_par[0], t_par)
        packed.receive_add_(q_pak[0], t_pak)
        for a, b in zip(t_pak, t_par):
            same_dict(a, b, f"receive_add_ {where}")
    same_dict(packed.receive_mean(q_pak)[0], parent.receive_mean(q_par)[0], "receive_mean")
    for where in ("cpu", "cuda"):
        base = _bases(decoded, where, 50)
        same_dict(packed.receive_mean_axpby(q_pak, base, 1.0, 1.0)[0], parent.receive_mean_axpby(q_par, base, 1.0, 1.0)[0],
                  f"receive_mean_axpby {where}")
        g = _bases(decoded, where, 51)
        for has_buf in (True, False):
            b_par = _bases(decoded, where, 52) if has_buf else None
            b_pak = {n: t.clone() for n, t in b_par.items()} if has_buf else None
            want, _ = parent.receive_scaled_flush(copy.deepcopy(q_par[1]), b_par, g, 0.5, K, 0.1)
            got, _ = packed.receive_scaled_flush(copy.deepcopy(q_pak[1]), b_pak, g, 0.5, K, 0.1)
            same_dict(got, want, f"receive_scaled_flush {where} {has_buf}")
        m_par, m_pak = flush.FadasMoments(), flush.FadasMoments()
        b_par = _bases(decoded, where, 53)
        b_pak = {n: t.clone() for n, t in b_par.items()}
        want = m_par.receive_flush(parent, copy.deepcopy(q_par[2]), b_par, g, K, 0.05, 1, keep_non_fp32=True)
        got = m_pak.receive_flush(packed, copy.deepcopy(q_pak[2]), b_pak, g, K, 0.05, 1, keep_non_fp32=True)
        same_dict(got, want, f"FadasMoments.receive_flush {where}")
    for where in ("cpu", "cuda"):   # send_delta, broadcast_delta_: one seed, one payload
        new = params_of("small", where)
        prev = {n: (t * 0.75 if t.is_floating_point() else t - 1) for n, t in new.items()}
        torch.manual_seed(SEED)
        want, _ = parent.send_delta(prev, new)
        rng = torch.get_rng_state()
        torch.manual_seed(SEED)
        got, _ = packed.send_delta(prev, new)
        assert torch.equal(torch.get_rng_state(), rng)
        pc.assert_unpacks_to(got, want, bits, f"send_delta {where}")
        h_par = {n: t.clone() for n, t in prev.items()}
        h_pak = {n: t.clone() for n, t in prev.items()}
        torch.manual_seed(SEED)
        want, _ = parent.broadcast_delta_(h_par, new)
        torch.manual_seed(SEED)
        got, _ = packed.broadcast_delta_(h_pak, new)
        pc.assert_unpacks_to(got, want, bits, f"broadcast_delta_ {where}")
        same_dict(h_pak, h_par, f"broadcast_delta_ hidden {where}")


def test_unidirectional_packed_channel_is_the_identity_downstream():
    ch, par = UPackedQSGDChannel(8), UQSGDChannel(8)
    params = params_of("small", "cpu")
    down = ch.on_server_send(params)[0]
    assert type(down) is type(par.on_server_send(params)[0])
    assert not isinstance(down, QuantParameters)
    up = encode(UPackedQSGDChannel, 8, params, "seed")[0]
    pc.assert_unpacks_to(up, parent_payload("qsgd", 8, "small", "cpu", "seed")[0], 8, "uni-directional")
    got = ch.on_server_receive(up)[0]
    for n, t in parent_decode("qsgd", 8, "small", "cpu").items():
        assert pc.same_bits(got[n], t), n


# ---- 9. custom ops ----------------------------------------------------------------------------------------------
def _op_bucket():
    sizes = [40, 100, 9, 1025, 8200]
    lay = ops.BucketLayout(sizes)
    flat = torch.randn(lay.total, generator=torch.Generator().manual_seed(2)).to(DEV)
    return lay, flat, torch.from_numpy(lay.offsets.copy()), torch.from_numpy(lay.sizes.copy())


@pytest.mark.parametrize("codec,bits", [("qsgd", 8), ("rqsgd", 4)])
def test_custom_ops_equal_the_python_entries(codec, bits):
    A = torch.ops.adfl_apply
    lay, flat, off, siz = _op_bucket()
    lv, sb, nr, mn = A.stoch_encode_packed_batched(flat, off, siz, codec, bits, 42, 6)
    w_lv, w_sb, w_nr, w_mn = stoch.encode_packed_batched(codec, flat, lay, bits, seed=42, counter=6,
                                                         levels=torch.zeros_like(lv), signbits=torch.zeros_like(sb))
    assert torch.equal(lv, w_lv) and torch.equal(sb, w_sb) and torch.equal(nr, w_nr)
    assert torch.equal(mn, w_mn if w_mn is not None else torch.zeros_like(nr))
    out = A.stoch_decode_packed_batched(lv, sb, nr, mn, off, siz, codec, bits)
    want = stoch.dequantize_packed_batched(codec, lv, sb, nr, lay, bits, mins=mn,
                                           out=torch.zeros(out.numel(), device=DEV))
    assert out.dtype == torch.float32 and pc.same_bits(out, want)
    base = torch.randn(lay.total, generator=torch.Generator().manual_seed(3)).to(DEV)
    got = A.stoch_decode_axpby_packed_batched(lv, sb, nr, mn, base, off, siz, codec, bits, 0.4, 0.6)
    want = torch.zeros_like(base)
    stoch.dequantize_axpby_packed_batched(codec, lv, sb, nr, lay, bits, base, want, 0.4, 0.6, mins=mn)
    assert pc.same_bits(got, want)


def test_custom_ops_opcheck_and_errors():
    A = torch.ops.adfl_apply
    lay, flat, off, siz = _op_bucket()
    for codec, bits in (("qsgd", 8), ("rqsgd", 4)):
        torch.library.opcheck(A.stoch_encode_packed_batched, (flat, off, siz, codec, bits, 1, 2))
        lv, sb, nr, mn = A.stoch_encode_packed_batched(flat, off, siz, codec, bits, 1, 2)
        torch.library.opcheck(A.stoch_decode_packed_batched, (lv, sb, nr, mn, off, siz, codec, bits))
        torch.library.opcheck(A.stoch_decode_axpby_packed_batched, (lv, sb, nr, mn, flat, off, siz, codec, bits, 0.4, 0.6))
    with pytest.raises(ValueError):
        A.stoch_encode_packed_batched(flat.double(), off, siz, "qsgd", 8, 1, 2)
    with pytest.raises(ValueError):
        A.stoch_encode_packed_batched(flat.cpu(), off, siz, "qsgd", 8, 1, 2)
    with pytest.raises(ValueError):
        A.stoch_encode_packed_batched(flat, off, siz, "cnat", 8, 1, 2)
    with pytest.raises(ValueError):
        A.stoch_encode_packed_batched(flat, off, siz, "qsgd", 9, 1, 2)
    with pytest.raises(ValueError):
        A.stoch_encode_packed_batched(flat, off + 1, siz, "qsgd", 8, 1, 2)     # offsets not multiples of 64
    with pytest.raises(ValueError):
        A.stoch_decode_packed_batched(lv.view(torch.int8), sb, nr, mn, off, siz, "rqsgd", 4)
    with pytest.raises(ValueError):
        A.stoch_decode_packed_batched(lv.cpu(), sb.cpu(), nr, mn, off, siz, "rqsgd", 4)
    with pytest.raises(ValueError):
        A.stoch_decode_axpby_packed_batched(lv, sb, nr, mn, flat.double(), off, siz, "rqsgd", 4, 0.4, 0.6)
    with pytest.raises(ValueError):
        A.stoch_decode_axpby_packed_batched(lv, sb, nr.cpu(), mn, flat, off, siz, "rqsgd", 4, 0.4, 0.6)
