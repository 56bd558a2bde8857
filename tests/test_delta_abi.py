"""CPU: the delta encode's C ABI, binding table, header constant, argument checks (nothing is launched by
any call here) and the two custom ops' registration and fake implementations."""

import ctypes
import re

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import adfl_amd  # noqa: F401  registers torch.ops.adfl.*
from adfl_amd import _lib
from adfl_amd._build import LIB_PATH
import delta_cases

NEW = ["adfl_slq_encode_delta_batched", "adfl_slq_encode_delta_batched_work", "adfl_slq_encode_delta_batched_int4",
       "adfl_slq_encode_delta_batched_int4_work"]
E_ARG = -1


def test_symbols_bound_and_exported():
    raw = ctypes.CDLL(LIB_PATH)
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert hasattr(raw, name), name
    assert _lib.SIGNATURES[NEW[0]] == _lib.SIGNATURES[NEW[2]]
    assert _lib.SIGNATURES[NEW[1]] == _lib.SIGNATURES[NEW[3]]
    # the non-delta counterparts with one more source pointer
    assert len(_lib.SIGNATURES[NEW[0]][1]) == len(_lib.SIGNATURES["adfl_slq_encode_batched"][1]) + 1
    assert len(_lib.SIGNATURES[NEW[1]][1]) == len(_lib.SIGNATURES["adfl_slq_encode_batched_work"][1]) + 1


def test_resident_bound_constant_and_abi_version():
    assert delta_cases.DELTA_RESIDENT_CHUNKS == _lib.DELTA_RESIDENT_CHUNKS
    assert _lib.DELTA_RESIDENT_CHUNKS in (4, 8)
    assert _lib.DELTA_RESIDENT_CHUNKS <= _lib.RESIDENT_CHUNKS   # the resident work list serves both
    assert delta_cases.header_constant("ADFL_SLQ_ABI_VERSION") == _lib.ABI_VERSION == 3
    assert _lib.load().adfl_slq_abi_version() == 3


@pytest.mark.parametrize("int4", [False, True])
def test_argument_errors_return_codes_without_launching(int4):
    lib = _lib.load()
    two = lib.adfl_slq_encode_delta_batched_int4 if int4 else lib.adfl_slq_encode_delta_batched
    work = lib.adfl_slq_encode_delta_batched_int4_work if int4 else lib.adfl_slq_encode_delta_batched_work
    ok_bits, over = (4, 5) if int4 else (8, 9)
    p = 16   # any non-null, aligned value: no call below gets as far as a launch
    # (new, prev, chunks, nchunks, bits, payload, scales, partials, stream)
    assert two(None, p, p, 1, ok_bits, p, p, p, None) == E_ARG       # null `new` table
    assert two(p, None, p, 1, ok_bits, p, p, p, None) == E_ARG       # null `prev` table
    assert two(None, None, p, 1, ok_bits, p, p, p, None) == E_ARG
    assert two(p, p, None, 1, ok_bits, p, p, p, None) == E_ARG       # null chunk table
    assert two(p, p, p, 1, ok_bits, None, p, p, None) == E_ARG       # null payload
    assert two(p, p, p, 1, ok_bits, p, None, p, None) == E_ARG       # null scales
    assert two(p, p, p, 1, ok_bits, p, p, None, None) == E_ARG       # null partials
    assert two(p, p, p, 1, 0, p, p, p, None) == E_ARG                # bits
    assert two(p, p, p, 1, over, p, p, p, None) == E_ARG
    assert two(p, p, p, -1, ok_bits, p, p, p, None) == E_ARG         # nchunks < 0
    assert two(p, p, p, 0, ok_bits, p, p, p, None) == E_ARG
    assert two(p, p, p, 1 << 31, ok_bits, p, p, p, None) == E_ARG    # oversized
    assert two(p, p, p, 1, ok_bits, 20, p, p, None) == -3            # payload base not 16-byte aligned
    # (new, prev, chunks, nchunks, work, nwork, bits, payload, scales, partials, stream)
    for nwork in (0, 1):   # 0: the two-pass entry's checks; 1: the resident entry's
        assert work(None, p, p, 1, p, nwork, ok_bits, p, p, p, None) == E_ARG
        assert work(p, None, p, 1, p, nwork, ok_bits, p, p, p, None) == E_ARG
        assert work(p, p, p, 1, p, nwork, 0, p, p, p, None) == E_ARG
        assert work(p, p, p, 1, p, nwork, over, p, p, p, None) == E_ARG
        assert work(p, p, p, -1, p, nwork, ok_bits, p, p, p, None) == E_ARG
    assert work(p, p, p, 1, None, 1, ok_bits, p, p, p, None) == E_ARG   # null work list
    assert work(p, p, p, 1, p, -1, ok_bits, p, p, p, None) == E_ARG     # nwork < 0
    assert work(p, p, p, 1, p, 2, ok_bits, p, p, p, None) == E_ARG      # nwork > nchunks


def test_custom_ops_registered_with_fakes_like_the_non_delta_ops():
    A = torch.ops.adfl
    for name in ("slq_encode_delta_batched", "slq_encode_delta_batched_int4"):
        assert hasattr(A, name), name
        schema = str(getattr(A, name).default._schema)
        # torch prints an `int` argument of a Python-registered op as SymInt
        assert re.search(r"\(Tensor new, Tensor prev, Tensor offsets, Tensor sizes, (Sym)?[Ii]nt bits\) -> "
                         r"\(Tensor, Tensor\)", schema), schema
    off, siz = torch.tensor([0, 100, 50]), torch.tensor([40, 7, 50])
    with FakeTensorMode(allow_non_fake_inputs=True) as mode:
        new = mode.from_tensor(torch.empty(107))
        prev = mode.from_tensor(torch.empty(107))
        q, s = A.slq_encode_delta_batched(new, prev, off, siz, 8)
        q0, s0 = A.slq_encode_batched(new, off, siz, 8)
        assert (q.shape, q.dtype, s.shape, s.dtype) == (q0.shape, q0.dtype, s0.shape, s0.dtype)
        assert q.shape == (107,) and q.dtype == torch.int8 and s.shape == (3,) and s.dtype == torch.float32
        p, s4 = A.slq_encode_delta_batched_int4(new, prev, off, siz, 4)
        p0, s40 = A.slq_encode_batched_int4(new, off, siz, 4)
        assert (p.shape, p.dtype, s4.shape, s4.dtype) == (p0.shape, p0.dtype, s40.shape, s40.dtype)
        assert p.shape == (54,) and p.dtype == torch.uint8
