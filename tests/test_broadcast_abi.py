"""CPU: the broadcast (delta encode + hidden-state update) C ABI: exports, binding table, argument checks (nothing
is launched by any call here), the unchanged ABI version, and the two custom ops' registration, schema and fake
implementations."""

import ctypes
import re

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import adfl_amd  # noqa: F401  registers the torch.ops namespaces
from adfl_amd import _lib, ops
from adfl_amd._build import LIB_PATH
from adfl_amd.Channel.quant import (CNATChannel, PackedSLQChannel, QSGDChannel, RQSGDChannel, SLQChannel,
                                    USLQChannel)
import delta_cases

NEW = ["adfl_slq_encode_delta_update_batched", "adfl_slq_encode_delta_update_batched_work",
       "adfl_slq_encode_delta_update_batched_int4", "adfl_slq_encode_delta_update_batched_int4_work"]
E_ARG, E_ALIGN = -1, -3


def test_symbols_bound_and_exported_with_the_delta_entries_signatures():
    raw = ctypes.CDLL(LIB_PATH)
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert hasattr(raw, name), name
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name.replace("_update", "")], name
    header = open(delta_cases.HEADER).read()
    for name in NEW:
        assert re.search(rf"\bint {name}\(const float\* const\* d_new, float\* const\* d_hidden,", header), name


def test_abi_version_is_still_3():
    assert delta_cases.header_constant("ADFL_SLQ_ABI_VERSION") == _lib.ABI_VERSION == 3
    assert _lib.load().adfl_slq_abi_version() == 3


@pytest.mark.parametrize("int4", [False, True])
def test_argument_errors_return_codes_without_launching(int4):
    lib = _lib.load()
    two = lib.adfl_slq_encode_delta_update_batched_int4 if int4 else lib.adfl_slq_encode_delta_update_batched
    work = (lib.adfl_slq_encode_delta_update_batched_int4_work if int4
            else lib.adfl_slq_encode_delta_update_batched_work)
    ok_bits, over = (4, 5) if int4 else (8, 9)
    p = 16   # any non-null, aligned value: no call below gets as far as a launch
    # (new, hidden, chunks, nchunks, bits, payload, scales, partials, stream)
    assert two(None, p, p, 1, ok_bits, p, p, p, None) == E_ARG       # null `new` table
    assert two(p, None, p, 1, ok_bits, p, p, p, None) == E_ARG       # null `hidden` table
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
    assert two(p, p, p, 1, ok_bits, 20, p, p, None) == E_ALIGN       # payload base not 16-byte aligned
    # (new, hidden, chunks, nchunks, work, nwork, bits, payload, scales, partials, stream)
    for nwork in (0, 1):   # 0: the two-pass entry's checks; 1: the resident entry's
        assert work(None, p, p, 1, p, nwork, ok_bits, p, p, p, None) == E_ARG
        assert work(p, None, p, 1, p, nwork, ok_bits, p, p, p, None) == E_ARG
        assert work(p, p, None, 1, p, nwork, ok_bits, p, p, p, None) == E_ARG
        assert work(p, p, p, 1, p, nwork, ok_bits, None, p, p, None) == E_ARG
        assert work(p, p, p, 1, p, nwork, ok_bits, p, None, p, None) == E_ARG
        assert work(p, p, p, 1, p, nwork, 0, p, p, p, None) == E_ARG
        assert work(p, p, p, 1, p, nwork, over, p, p, p, None) == E_ARG
        assert work(p, p, p, -1, p, nwork, ok_bits, p, p, p, None) == E_ARG
        assert work(p, p, p, 1, p, nwork, ok_bits, 20, p, p, None) == E_ALIGN
    assert work(p, p, p, 1, None, 1, ok_bits, p, p, p, None) == E_ARG   # null work list
    assert work(p, p, p, 1, p, -1, ok_bits, p, p, p, None) == E_ARG     # nwork < 0
    assert work(p, p, p, 1, p, 2, ok_bits, p, p, p, None) == E_ARG      # nwork > nchunks


def test_custom_ops_registered_in_adfl_apply_mutating_hidden_with_fakes():
    A = torch.ops.adfl_apply
    for name in ("slq_encode_delta_update_batched", "slq_encode_delta_update_batched_int4"):
        assert hasattr(A, name), name
        assert not hasattr(torch.ops.adfl, name)          # torch.ops.adfl.* is the codec proper, pinned
        schema = str(getattr(A, name).default._schema)
        # torch prints an `int` argument of a Python-registered op as SymInt, a mutated argument as Tensor(a!)
        assert re.search(r"\(Tensor new, Tensor\(\w+!\) hidden, Tensor offsets, Tensor sizes, (Sym)?[Ii]nt bits\) -> "
                         r"\(Tensor, Tensor\)", schema), schema
    off, siz = torch.tensor([0, 100, 50]), torch.tensor([40, 7, 50])
    with FakeTensorMode(allow_non_fake_inputs=True) as mode:
        new = mode.from_tensor(torch.empty(107))
        hidden = mode.from_tensor(torch.empty(107))
        q, s = A.slq_encode_delta_update_batched(new, hidden, off, siz, 8)
        q0, s0 = torch.ops.adfl.slq_encode_delta_batched(new, hidden, off, siz, 8)
        assert (q.shape, q.dtype, s.shape, s.dtype) == (q0.shape, q0.dtype, s0.shape, s0.dtype)
        assert q.shape == (107,) and q.dtype == torch.int8 and s.shape == (3,) and s.dtype == torch.float32
        p, s4 = A.slq_encode_delta_update_batched_int4(new, hidden, off, siz, 4)
        p0, s40 = torch.ops.adfl.slq_encode_delta_batched_int4(new, hidden, off, siz, 4)
        assert (p.shape, p.dtype, s4.shape, s4.dtype) == (p0.shape, p0.dtype, s40.shape, s40.dtype)
        assert p.shape == (54,) and p.dtype == torch.uint8


def test_host_layers_expose_the_broadcast():
    assert callable(ops.encode_delta_update_batched) and callable(ops.encode_delta_update_batched_int4)
    for cls in (SLQChannel, USLQChannel, PackedSLQChannel, QSGDChannel, RQSGDChannel, CNATChannel):
        assert callable(getattr(cls, "broadcast_delta_")), cls.__name__
    # the uni-directional classes take the identity route, the SLQ classes the fused override
    assert USLQChannel.broadcast_delta_ is not SLQChannel.broadcast_delta_
    assert PackedSLQChannel.broadcast_delta_ is SLQChannel.broadcast_delta_
    assert QSGDChannel.broadcast_delta_ is not SLQChannel.broadcast_delta_


def test_ops_reject_a_hidden_that_cannot_be_written_in_place():
    lay = ops.BucketLayout([8, 8])
    with pytest.raises(ValueError, match="device"):
        ops.encode_delta_update_batched(torch.zeros(lay.total), torch.zeros(lay.total), lay, 8)
