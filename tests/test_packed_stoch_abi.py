"""CPU: the packed QSGD / RQSGD wire format (bits + 1 bits per weight) without a device — the C ABI's exports,
binding table, header declarations and argument checks (nothing is launched by any call here), the unchanged ABI
version, the custom ops' registration and fake implementations, the channel classes' surface, the byte counts against
the bandwidth formula, and the numpy restatement of the format the GPU tests unpack payloads with."""

import ctypes
import importlib
import os
import pickle
import re
import time

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import adfl_amd
from adfl_amd import _lib
from adfl_amd import stoch as sops
from adfl_amd._build import LIB_PATH, SOURCES
from adfl_amd.Channel import quant
from adfl_amd.Channel._base import _CodecChannel
from adfl_amd.Channel.quant import QSGDChannel, RQSGDChannel, UQSGDChannel, URQSGDChannel
import delta_cases
import packed_stoch_cases as pc

CHANNELS = importlib.import_module("adfl_amd.Channel")   # adfl_amd.Channel itself is the base class, re-exported

HEADER = os.path.join(os.path.dirname(delta_cases.HEADER), "adfl_stoch.h")
QUANT, DEQ, AXPBY = ("adfl_stoch_quantize_packed_batched", "adfl_stoch_dequantize_packed_batched",
                     "adfl_stoch_dequantize_axpby_packed_batched")
E_ARG, E_BITS, E_ALIGN = -1, -2, -3
QSGD, RQSGD, CNAT = 0, 1, 2
PACKED = {"PackedQSGDChannel": QSGDChannel, "PackedRQSGDChannel": RQSGDChannel, "UPackedQSGDChannel": UQSGDChannel,
          "UPackedRQSGDChannel": URQSGDChannel}


# ---- 1. ABI -----------------------------------------------------------------------------------------------------
def test_symbols_declared_bound_and_exported():
    raw = ctypes.CDLL(LIB_PATH)
    header = open(HEADER).read()
    for name in (QUANT, DEQ, AXPBY):
        assert name in _lib.SIGNATURES and hasattr(raw, name), name
        assert len(re.findall(rf"\bint {name}\(", header)) == 1, name
    s = _lib.SIGNATURES
    P, I32, I64, U64, INT, F32 = _lib.P, _lib.I32, _lib.I64, _lib.U64, _lib.INT, _lib.F32
    # int32 codec in front of adfl_qsgd_quantize_batched's arguments, with d_ushift behind d_uniforms
    assert s[QUANT] == (INT, [I32, P, P, I64, INT, P, P, P, U64, U64, P, P, P])
    assert s[QUANT][1][1:7] + s[QUANT][1][8:] == s["adfl_qsgd_quantize_batched"][1]
    # int32 codec in front of adfl_rqsgd_dequantize_batched's arguments
    assert s[DEQ] == (INT, [I32] + s["adfl_rqsgd_dequantize_batched"][1])
    # adfl_stoch_dequantize_axpby_batched's own
    assert s[AXPBY] == s["adfl_stoch_dequantize_axpby_batched"] == (INT, [I32, P, P, P, I64, INT, P, P, P, P, I32, I32,
                                                                         F32, F32, P])
    decl = {n: re.sub(r"\s+", " ", re.search(rf"\bint {n}\((.*?)\);", header, flags=re.S).group(1))
            for n in (QUANT, DEQ, AXPBY)}
    assert decl[QUANT] == ("int32_t codec, const float* d_x, const adfl_slq_chunk* d_chunks, int64_t nchunks, int bits, "
                           "const float* d_norms, const float* d_uniforms, const int64_t* d_ushift, uint64_t seed, "
                           "uint64_t counter, uint8_t* d_levels, uint8_t* d_signbits, void* stream")
    assert decl[DEQ] == ("int32_t codec, const uint8_t* d_levels, const uint8_t* d_signbits, "
                         "const adfl_slq_chunk* d_chunks, int64_t nchunks, int bits, const float* d_norms, "
                         "const float* d_mins, float* d_out, void* stream")
    assert decl[AXPBY] == ("int32_t codec, const uint8_t* d_levels, const uint8_t* d_signbits, "
                           "const adfl_slq_chunk* d_chunks, int64_t nchunks, int bits, const float* d_norms, "
                           "const float* d_mins, const float* const* d_base, float* const* d_out, int32_t ntensors, "
                           "int32_t ntargets, float alpha, float beta, void* stream")
    assert any(os.path.basename(p) == "stoch_packed.hip" for p in SOURCES)


def test_abi_version_is_still_3():
    assert delta_cases.header_constant("ADFL_SLQ_ABI_VERSION") == _lib.ABI_VERSION == 3
    assert _lib.load().adfl_slq_abi_version() == 3


def test_quantize_argument_errors_return_codes_without_launching():
    f = _lib.load().adfl_stoch_quantize_packed_batched
    p = 16   # any non-null, 16-byte aligned value: no call below gets as far as a launch

    def call(codec=QSGD, x=p, chunks=p, nchunks=1, bits=8, nr=p, unif=None, ushift=None, lv=p, sb=p):
        return f(codec, x, chunks, nchunks, bits, nr, unif, ushift, 1, 2, lv, sb, None)

    for codec in (QSGD, RQSGD):
        assert call(codec, x=None) == E_ARG
        assert call(codec, chunks=None) == E_ARG
        assert call(codec, nr=None) == E_ARG
        assert call(codec, lv=None) == E_ARG
        assert call(codec, sb=None) == E_ARG
        for n in (0, -1, 1 << 31):
            assert call(codec, nchunks=n) == E_ARG
        for bits in (0, 9, 16, -1):
            assert call(codec, bits=bits) == E_BITS
        assert call(codec, x=20) == E_ALIGN
        assert call(codec, lv=24) == E_ALIGN
        assert call(codec, sb=8) == E_ALIGN
        assert call(codec, unif=4) == E_ALIGN
    for codec in (CNAT, 3, -1):
        assert call(codec) == E_ARG
    assert call(CNAT, bits=0) == E_ARG and call(bits=0, x=20) == E_BITS   # argument, then bits, then alignment


def test_dequantize_argument_errors_return_codes_without_launching():
    f = _lib.load().adfl_stoch_dequantize_packed_batched
    p = 16

    def call(codec=QSGD, lv=p, sb=p, chunks=p, nchunks=1, bits=8, nr=p, mn=p, out=p):
        return f(codec, lv, sb, chunks, nchunks, bits, nr, mn, out, None)

    for codec in (QSGD, RQSGD):
        for null in ("lv", "sb", "chunks", "nr", "out"):
            assert call(codec, **{null: None}) == E_ARG, null
        for n in (0, -1, 1 << 31):
            assert call(codec, nchunks=n) == E_ARG
        for bits in (0, 9, -1):
            assert call(codec, bits=bits) == E_BITS
        for odd in ("lv", "sb", "out"):
            assert call(codec, **{odd: 8}) == E_ALIGN, odd
    assert call(RQSGD, mn=None) == E_ARG      # RQSGD decodes zero levels to min * sign
    assert call(QSGD, mn=None, lv=8) == E_ALIGN   # QSGD takes no mins: the call gets past the argument check
    for codec in (CNAT, 7):
        assert call(codec) == E_ARG


def test_dequantize_axpby_argument_errors_return_codes_without_launching():
    f = _lib.load().adfl_stoch_dequantize_axpby_packed_batched
    p = 16

    def call(codec=QSGD, lv=p, sb=p, chunks=p, nchunks=1, bits=8, nr=p, mn=p, base=p, out=p, nt=1, nk=1):
        return f(codec, lv, sb, chunks, nchunks, bits, nr, mn, base, out, nt, nk, 0.5, 0.5, None)

    for codec in (QSGD, RQSGD):
        for null in ("lv", "sb", "chunks", "nr", "out"):
            assert call(codec, **{null: None}) == E_ARG, null
        for n in (0, -1, 1 << 31):
            assert call(codec, nchunks=n) == E_ARG
        assert call(codec, nt=0) == E_ARG and call(codec, nk=0) == E_ARG
        for bits in (0, 9, -1):
            assert call(codec, bits=bits) == E_BITS
        assert call(codec, lv=8) == E_ALIGN and call(codec, sb=4) == E_ALIGN
        assert call(codec, base=None, lv=8) == E_ALIGN    # no base is the SCALE form, not an error
    assert call(RQSGD, mn=None) == E_ARG
    for codec in (CNAT, 9):
        assert call(codec) == E_ARG


def test_custom_ops_registered_in_adfl_apply_with_fakes():
    A = torch.ops.adfl_apply
    for op in ("stoch_encode_packed_batched", "stoch_decode_packed_batched", "stoch_decode_axpby_packed_batched"):
        assert hasattr(A, op) and not hasattr(torch.ops.adfl, op), op
    names = {n.split(".")[0] for n in torch._C._dispatch_get_all_op_names() if n.startswith("adfl::")}
    assert len(names) == 19, sorted(names)                      # the codec namespace is unchanged
    off, siz = torch.tensor([0, 64, 192]), torch.tensor([40, 100, 9])
    with FakeTensorMode(allow_non_fake_inputs=True) as mode:
        flat = mode.from_tensor(torch.empty(201))
        for bits, nl in ((8, 201), (5, 201), (4, 101), (1, 101)):
            lv, sb, nr, mn = A.stoch_encode_packed_batched(flat, off, siz, "rqsgd", bits, 1, 2)
            assert [(t.shape, t.dtype) for t in (lv, sb, nr, mn)] == [((nl,), torch.uint8), ((26,), torch.uint8),
                                                                      ((3,), torch.float32), ((3,), torch.float32)]
            out = A.stoch_decode_packed_batched(lv, sb, nr, mn, off, siz, "rqsgd", bits)
            assert out.dtype == torch.float32 and out.shape == ((201,) if bits > 4 else (202,))
            out = A.stoch_decode_axpby_packed_batched(lv, sb, nr, mn, flat, off, siz, "qsgd", bits, 0.4, 0.6)
            assert out.dtype == torch.float32 and out.shape == (201,)


# ---- 2. surface -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PACKED))
def test_channel_surface(name):
    cls = getattr(CHANNELS, name)
    assert cls is getattr(quant, name) is getattr(adfl_amd, name) and cls.__module__ == "adfl_amd.Channel.stoch"
    assert CHANNELS.__all__[-4:] == list(PACKED)       # appended: the earlier names keep their places
    assert issubclass(cls, _CodecChannel) and cls.CODEC == PACKED[name].CODEC
    assert cls.NORM_BYTES == PACKED[name].NORM_BYTES and cls.SIGN_BITS == 1
    ch = cls(4)
    assert ch.__dict__ == {"bits": 4, "levels": 15} == PACKED[name](4).__dict__
    assert ch.to_json() == {"name": name, "bits": 4}
    back = pickle.loads(pickle.dumps(ch))
    assert type(back) is cls and back.__dict__ == ch.__dict__
    for bits in (0, 9, 16, -1):
        with pytest.raises(ValueError, match=r"bits must be in \[1, 8\]"):
            cls(bits)
    for bits in range(1, 9):
        assert cls(bits).levels == 2 ** bits - 1
    # the fused hooks that would read two whole byte planes decline
    assert ch._flush_groups(None, []) == []
    assert ch._mean_host_updates([], []) is None and ch._mean_host_classify([], []) is None
    assert ch._mean_fused_names([], ["w"]) == []
    # receive_add_ is the shared body: the fused decode + axpby from the packed planes, in place with (1, 1)
    assert cls.receive_add_ is _CodecChannel.receive_add_
    for hook in ("_flush_payload", "_mean_payloads", "_mean_apply", "_quantize_delta"):
        with pytest.raises(NotImplementedError):
            getattr(ch, hook)()
    uni = name.startswith("U")
    assert (cls.on_server_send is not _CodecChannel.on_server_send) == uni


@pytest.mark.parametrize("name", list(PACKED))
def test_simulate_bandwidth_is_the_parents(name, monkeypatch):
    slept = []
    monkeypatch.setattr(time, "sleep", slept.append)
    params = {"a.weight": torch.zeros(64, 24), "a.bias": torch.zeros(24), "b.weight": torch.zeros(3, 8, 5, 5),
              "n": torch.tensor(3)}
    for bits in (8, 4, 1):
        got = getattr(CHANNELS, name)(bits).simulate_bandwidth(params, 100.0)
        want = PACKED[name](bits).simulate_bandwidth(params, 100.0)
        assert got == want == slept[-1] == slept[-2]
        weights = 64 * 24 + 600
        norm_bytes = 8 if "RQSGD" in name else 4
        assert got == (weights * (bits + 1) / 8 + 25 * 4 + 2 * norm_bytes) / (100.0 * 1_000_000 / 8)


def test_packed_plane_bytes_matches_its_formula():
    for bits in range(1, 9):
        for n in pc.SIZES + [3, 4, 5, 100, 1 << 26]:
            lv, sb = sops.packed_plane_bytes(n, bits)
            assert (lv, sb) == pc.plane_bytes(n, bits) == ((n if bits > 4 else -(-n // 2)), -(-n // 8))
    assert "packed_plane_bytes" in sops.__all__
    assert {"quantize_packed_batched", "dequantize_packed_batched", "dequantize_axpby_packed_batched"} <= set(sops.__all__)


@pytest.mark.parametrize("bits", [8, 4])
def test_coded_bytes_equal_the_bandwidth_formulas_weight_term(bits):
    """n % 8 == 0: the coded entries' share of QuantParameters.size (both planes) is num_non_bias_w * (bits + 1) / 8,
    the weight term simulate_bandwidth charges."""
    sizes = [8, 64, 1024, 8192, 27 * 64]
    assert sum(sum(sops.packed_plane_bytes(n, bits)) for n in sizes) == sum(sizes) * (bits + 1) / 8


def test_python_layer_checks_codec_bits_and_layout_before_any_launch():
    lay = adfl_amd.ops.BucketLayout([10, 20], align=1)
    with pytest.raises(ValueError, match="multiple of 64"):
        sops._packed_args("qsgd", lay, 8)
    lay = adfl_amd.ops.BucketLayout([10, 20])
    assert sops._packed_args("qsgd", lay, 8) == (128, 16) and sops._packed_args("rqsgd", lay, 3) == (64, 16)
    with pytest.raises(ValueError, match="CNAT"):
        sops._packed_args("cnat", lay, 8)
    for bits in (0, 9):
        with pytest.raises(ValueError, match=r"\[1, 8\]"):
            sops._packed_args("qsgd", lay, bits)
    host = torch.zeros(128, dtype=torch.uint8)
    with pytest.raises(ValueError):   # host planes never reach a kernel
        sops.dequantize_packed_batched("qsgd", host, host, torch.zeros(2), lay, 8)
    with pytest.raises(ValueError, match="uint8"):
        sops.dequantize_packed_batched("qsgd", host.view(torch.int8), host, torch.zeros(2), lay, 8)


# ---- 3. the format helper ---------------------------------------------------------------------------------------
def test_format_helper_on_a_hand_written_17_element_example():
    levels = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 9], np.uint8)
    signs = np.array([1, -1, 0, -1, 1, 1, -1, -1, 0, 0, -1, 1, 1, 1, 1, -1, -1], np.int8)
    want_sb = np.array([0b11001010, 0b10000100, 0b00000001], np.uint8)
    lv4, sb = pc.pack(levels, signs < 0, 4)
    np.testing.assert_array_equal(sb, want_sb)
    np.testing.assert_array_equal(lv4, np.array([0x01, 0x23, 0x45, 0x67, 0x89, 0xAB, 0xCD, 0xEF, 0x90], np.uint8))
    lv8, sb8 = pc.pack(levels * 16 + 3, signs < 0, 8)
    np.testing.assert_array_equal(sb8, want_sb)
    np.testing.assert_array_equal(lv8, levels * 16 + 3)
    for bits, lv in ((4, lv4), (1, lv4), (8, lv8), (5, lv8)):
        assert (lv.size, sb.size) == pc.plane_bytes(17, bits) == sops.packed_plane_bytes(17, bits)
        got_l, got_neg = pc.unpack(lv, sb, 17, bits)
        np.testing.assert_array_equal(got_l, levels if bits <= 4 else levels * 16 + 3)
        np.testing.assert_array_equal(got_neg, signs < 0)
    with pytest.raises(AssertionError, match="unused sign bits"):
        pc.unpack(lv4, np.array([0, 0, 2], np.uint8), 17, 4)
    with pytest.raises(AssertionError, match="low nibble"):
        pc.unpack(np.array([0, 0, 0, 0, 0, 0, 0, 0, 0x91], np.uint8), sb, 17, 4)
    # pack_4bit's nibble order (Src/ADFL/compression.py:35-48): the even element in the high nibble
    assert pc.pack(np.array([0xA, 0x5], np.uint8), np.zeros(2, bool), 4)[0].tolist() == [0xA5]
    rng = np.random.default_rng(0)
    for n in pc.SIZES[:14]:
        for bits in pc.BITS:
            lv = rng.integers(0, 1 << bits, n).astype(np.uint8)
            neg = rng.integers(0, 2, n).astype(bool)
            a, b = pc.unpack(*pc.pack(lv, neg, bits), n, bits)
            assert np.array_equal(a, lv) and np.array_equal(b, neg)
