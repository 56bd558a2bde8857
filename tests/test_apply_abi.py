"""CPU: the fused decode + axpby entries' C ABI — declared in the headers, bound in _lib.SIGNATURES, exported by
the library, the ABI version unchanged, and every argument error answered with ADFL_E_ARG before anything is
launched (no call here reaches a kernel) — and the three custom ops' registration and fake implementations."""

import ctypes
import os
import re

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import adfl_amd  # noqa: F401  registers torch.ops.adfl.*
from adfl_amd import _lib
from adfl_amd._build import LIB_PATH

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
SLQ, SLQ4, STOCH = ("adfl_slq_dequantize_axpby_batched", "adfl_slq_dequantize_axpby_batched_int4",
                    "adfl_stoch_dequantize_axpby_batched")
E_ARG = -1


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, name)).read(), flags=re.S)


def test_declared_bound_and_exported():
    slq_h, stoch_h = _header("adfl_slq.h"), _header("adfl_stoch.h")
    assert re.search(rf"\bint\s+{SLQ}\s*\(", slq_h) and re.search(rf"\bint\s+{SLQ4}\s*\(", slq_h)
    assert re.search(rf"\bint\s+{STOCH}\s*\(", stoch_h)
    raw = ctypes.CDLL(LIB_PATH)
    for name in (SLQ, SLQ4, STOCH):
        assert name in _lib.SIGNATURES, name
        assert hasattr(raw, name), name
    assert _lib.SIGNATURES[SLQ] == _lib.SIGNATURES[SLQ4]
    # the decode + add entry with a second pointer table and the two coefficients
    assert len(_lib.SIGNATURES[SLQ][1]) == len(_lib.SIGNATURES["adfl_slq_dequantize_add_batched"][1]) + 3
    assert _lib.SIGNATURES[SLQ][1].count(ctypes.c_float) == 2 == _lib.SIGNATURES[STOCH][1].count(ctypes.c_float)


def test_abi_version_is_still_3():
    assert "#define ADFL_SLQ_ABI_VERSION 3" in open(os.path.join(INCLUDE, "adfl_slq.h")).read()
    assert _lib.ABI_VERSION == 3 and _lib.load().adfl_slq_abi_version() == 3


@pytest.mark.parametrize("name", [SLQ, SLQ4])
def test_slq_argument_errors_return_codes_without_launching(name):
    fn = getattr(_lib.load(), name)
    p = 16   # any non-null, aligned value: no call below gets as far as a launch
    # (payload, chunks, nchunks, scales, base, out, ntensors, ntargets, alpha, beta, stream)
    assert fn(None, p, 1, p, p, p, 1, 1, 1.0, 1.0, None) == E_ARG       # null payload
    assert fn(p, None, 1, p, p, p, 1, 1, 1.0, 1.0, None) == E_ARG       # null chunk table
    assert fn(p, p, 1, None, p, p, 1, 1, 1.0, 1.0, None) == E_ARG       # null scales
    assert fn(p, p, 1, p, p, None, 1, 1, 1.0, 1.0, None) == E_ARG       # null output table
    assert fn(p, p, 1, p, None, None, 1, 1, 1.0, 1.0, None) == E_ARG    # SCALE (null base) still needs outputs
    assert fn(p, p, 0, p, p, p, 1, 1, 1.0, 1.0, None) == E_ARG          # nchunks 0
    assert fn(p, p, -1, p, p, p, 1, 1, 1.0, 1.0, None) == E_ARG
    assert fn(p, p, 1 << 31, p, p, p, 1, 1, 1.0, 1.0, None) == E_ARG    # oversized
    assert fn(p, p, 1, p, p, p, 0, 1, 1.0, 1.0, None) == E_ARG          # ntensors 0
    assert fn(p, p, 1, p, p, p, 1, 0, 1.0, 1.0, None) == E_ARG          # ntargets 0
    assert fn(p, p, 1, p, p, p, 1, -2, 1.0, 1.0, None) == E_ARG
    assert fn(20, p, 1, p, p, p, 1, 1, 1.0, 1.0, None) == -3            # payload base not 16-byte aligned


@pytest.mark.parametrize("codec", [_lib.CODEC_QSGD, _lib.CODEC_RQSGD, _lib.CODEC_CNAT])
def test_stoch_argument_errors_return_codes_without_launching(codec):
    fn = _lib.load().adfl_stoch_dequantize_axpby_batched
    p = 16
    # (codec, levels, signs, chunks, nchunks, bits, norms, mins, base, out, ntensors, ntargets, alpha, beta, stream)
    assert fn(9, p, p, p, 1, 8, p, p, p, p, 1, 1, 1.0, 1.0, None) == E_ARG          # unknown codec
    assert fn(codec, None, p, p, 1, 8, p, p, p, p, 1, 1, 1.0, 1.0, None) == E_ARG   # null levels
    assert fn(codec, p, None, p, 1, 8, p, p, p, p, 1, 1, 1.0, 1.0, None) == E_ARG   # null signs
    assert fn(codec, p, p, None, 1, 8, p, p, p, p, 1, 1, 1.0, 1.0, None) == E_ARG   # null chunk table
    assert fn(codec, p, p, p, 1, 8, None, p, p, p, 1, 1, 1.0, 1.0, None) == E_ARG   # null norms
    assert fn(codec, p, p, p, 1, 8, p, p, p, None, 1, 1, 1.0, 1.0, None) == E_ARG   # null output table
    assert fn(codec, p, p, p, 0, 8, p, p, p, p, 1, 1, 1.0, 1.0, None) == E_ARG      # nchunks 0
    assert fn(codec, p, p, p, 1 << 31, 8, p, p, p, p, 1, 1, 1.0, 1.0, None) == E_ARG
    assert fn(codec, p, p, p, 1, 8, p, p, p, p, 0, 1, 1.0, 1.0, None) == E_ARG      # ntensors 0
    assert fn(codec, p, p, p, 1, 8, p, p, p, p, 1, 0, 1.0, 1.0, None) == E_ARG      # ntargets 0
    assert fn(codec, 20, p, p, 1, 8, p, p, p, p, 1, 1, 1.0, 1.0, None) == -3        # misaligned plane
    if codec == _lib.CODEC_RQSGD:
        assert fn(codec, p, p, p, 1, 8, p, None, p, p, 1, 1, 1.0, 1.0, None) == E_ARG   # RQSGD needs mins
    if codec != _lib.CODEC_CNAT:   # bits are unused for CNAT, as in the mean entry
        assert fn(codec, p, p, p, 1, 0, p, p, p, p, 1, 1, 1.0, 1.0, None) == E_ARG
        assert fn(codec, p, p, p, 1, 17, p, p, p, p, 1, 1, 1.0, 1.0, None) == E_ARG


def test_custom_ops_registered_with_fakes():
    A = torch.ops.adfl_apply
    for name in ("slq_decode_axpby_batched", "slq_decode_axpby_batched_int4", "stoch_decode_axpby_batched"):
        assert hasattr(A, name), name
    off, siz = torch.tensor([0, 100, 50]), torch.tensor([40, 7, 50])
    with FakeTensorMode(allow_non_fake_inputs=True) as mode:
        q = mode.from_tensor(torch.empty(107, dtype=torch.int8))
        p4 = mode.from_tensor(torch.empty(54, dtype=torch.uint8))
        lv = mode.from_tensor(torch.empty(107, dtype=torch.uint8))
        sc = mode.from_tensor(torch.empty(3))
        base = mode.from_tensor(torch.empty(107))
        for out in (A.slq_decode_axpby_batched(q, sc, base, off, siz, 0.4, 0.6),
                    A.slq_decode_axpby_batched_int4(p4, sc, base, off, siz, 0.4, 0.6),
                    A.stoch_decode_axpby_batched(lv, q, sc, sc, base, off, siz, "rqsgd", 8, 0.4, 0.6)):
            assert out.shape == (107,) and out.dtype == torch.float32
