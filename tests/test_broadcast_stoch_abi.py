"""CPU: the stochastic broadcast (delta encode + hidden-state update) C ABI: exports, binding table, header
declarations, argument checks (nothing is launched by any call here), the unchanged ABI version, and the custom
op's registration, schema and fake implementation."""

import ctypes
import os
import re

import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import adfl_amd  # noqa: F401  registers the torch.ops namespaces
from adfl_amd import _lib
from adfl_amd import stoch as sops
from adfl_amd._build import LIB_PATH
from adfl_amd.Channel._base import _CodecChannel
from adfl_amd.Channel.quant import (CNATChannel, QSGDChannel, RQSGDChannel, SLQChannel, UCNATChannel, UQSGDChannel,
                                    URQSGDChannel)
import delta_cases

HEADER = os.path.join(os.path.dirname(delta_cases.HEADER), "adfl_stoch.h")
RQ = ["adfl_rqsgd_encode_delta_update_batched", "adfl_rqsgd_encode_delta_update_batched_work"]
QS = "adfl_qsgd_quantize_update_batched"
E_ARG, E_BITS, E_ALIGN, E_WORKSPACE = -1, -2, -3, -4


def test_symbols_exported_bound_and_declared():
    raw = ctypes.CDLL(LIB_PATH)
    header = open(HEADER).read()
    for name in RQ + [QS]:
        assert name in _lib.SIGNATURES, name
        assert hasattr(raw, name), name
    for name in RQ:   # the delta entries' arguments, d_ushift included, with the hidden table in prev's place
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name.replace("_update", "")], name
        assert re.search(rf"\bint {name}\(const float\* const\* d_new, float\* const\* d_hidden,", header), name
        decl = re.search(rf"\bint {name}\((.*?)\);", header, flags=re.S).group(1)
        assert "const int64_t* d_ushift" in decl, name
    # adfl_qsgd_quantize_batched plus the hidden table and its length
    assert _lib.SIGNATURES[QS][1][:11] == _lib.SIGNATURES["adfl_qsgd_quantize_batched"][1][:11]
    assert len(_lib.SIGNATURES[QS][1]) == len(_lib.SIGNATURES["adfl_qsgd_quantize_batched"][1]) + 2
    decl = re.search(rf"\bint {QS}\((.*?)\);", header, flags=re.S).group(1)
    assert re.search(r"int8_t\* d_signs, float\* const\* d_hidden, int64_t ntensors,\s+void\* stream", decl), decl


def test_abi_version_is_still_3():
    assert delta_cases.header_constant("ADFL_SLQ_ABI_VERSION") == _lib.ABI_VERSION == 3
    assert _lib.load().adfl_slq_abi_version() == 3


def test_rqsgd_update_argument_errors_return_codes_without_launching():
    lib = _lib.load()
    two, work = lib.adfl_rqsgd_encode_delta_update_batched, lib.adfl_rqsgd_encode_delta_update_batched_work
    p = 16   # any non-null, aligned value: no call below gets as far as a launch
    ws = 16  # adfl_stoch_workspace_bytes(1)
    assert lib.adfl_stoch_workspace_bytes(1) == ws

    def call(new=p, hidden=p, chunks=p, nchunks=1, bits=8, unif=None, ushift=None, wsp=p, wsb=ws, lv=p, sg=p, nr=p,
             mn=p, work_args=None):
        args = (bits, unif, ushift, 1, 2, wsp, wsb, lv, sg, nr, mn, None)
        if work_args is None:
            return two(new, hidden, chunks, nchunks, *args)
        return work(new, hidden, chunks, nchunks, *work_args, *args)

    for wa in (None, (p, 0), (p, 1)):   # the two-pass entry, the _work entry as two-pass, with a work list
        assert call(new=None, work_args=wa) == E_ARG          # null tables
        assert call(hidden=None, work_args=wa) == E_ARG
        assert call(chunks=None, work_args=wa) == E_ARG
        assert call(lv=None, work_args=wa) == E_ARG           # null planes
        assert call(sg=None, work_args=wa) == E_ARG
        assert call(nr=None, work_args=wa) == E_ARG           # null norms / mins
        assert call(mn=None, work_args=wa) == E_ARG
        assert call(wsp=None, work_args=wa) == E_ARG          # null workspace
        for bits in (0, 17, -1):
            assert call(bits=bits, work_args=wa) == E_BITS
        assert call(nchunks=0, work_args=wa) == E_ARG
        assert call(nchunks=-1, work_args=wa) == E_ARG
        assert call(nchunks=1 << 31, wsb=1 << 40, work_args=wa) == E_ARG   # above INT32_MAX
        assert call(wsb=ws - 1, work_args=wa) == E_WORKSPACE
        assert call(nchunks=3, wsb=2 * ws, work_args=wa) == E_WORKSPACE
        assert call(wsp=24, work_args=wa) == E_ALIGN           # workspace base
        assert call(lv=20, work_args=wa) == E_ALIGN            # plane bases
        assert call(sg=8, work_args=wa) == E_ALIGN
        assert call(unif=4, work_args=wa) == E_ALIGN           # injected uniforms' base
    assert call(work_args=(None, 1)) == E_ARG                  # null work list
    assert call(work_args=(p, -1)) == E_ARG                    # nwork < 0
    assert call(work_args=(p, 2)) == E_ARG                     # nwork > nchunks


def test_qsgd_update_argument_errors_return_codes_without_launching():
    f = _lib.load().adfl_qsgd_quantize_update_batched
    p = 16

    def call(x=p, chunks=p, nchunks=1, bits=8, nr=p, unif=None, lv=p, sg=p, hidden=p, ntensors=1):
        return f(x, chunks, nchunks, bits, nr, unif, 1, 2, lv, sg, hidden, ntensors, None)

    assert call(x=None) == E_ARG
    assert call(chunks=None) == E_ARG
    assert call(nr=None) == E_ARG
    assert call(lv=None) == E_ARG
    assert call(sg=None) == E_ARG
    assert call(hidden=None) == E_ARG
    assert call(ntensors=0) == E_ARG
    assert call(nchunks=0) == E_ARG
    assert call(nchunks=-1) == E_ARG
    assert call(nchunks=1 << 31) == E_ARG
    for bits in (0, 17, -1):
        assert call(bits=bits) == E_BITS
    assert call(x=20) == E_ALIGN
    assert call(lv=20) == E_ALIGN
    assert call(sg=8) == E_ALIGN
    assert call(unif=4) == E_ALIGN


def test_custom_op_registered_in_adfl_apply_mutating_hidden_with_a_fake():
    A = torch.ops.adfl_apply
    assert hasattr(A, "stoch_encode_delta_update_batched")
    assert not hasattr(torch.ops.adfl, "stoch_encode_delta_update_batched")   # torch.ops.adfl.* is the codec proper
    schema = str(A.stoch_encode_delta_update_batched.default._schema)
    # torch prints an `int` argument of a Python-registered op as SymInt, a mutated argument as Tensor(a!)
    assert re.search(r"\(Tensor new, Tensor\(\w+!\) hidden, Tensor offsets, Tensor sizes, str codec, (Sym)?[Ii]nt bits, "
                     r"(Sym)?[Ii]nt seed, (Sym)?[Ii]nt counter\) -> \(Tensor, Tensor, Tensor, Tensor\)", schema), schema
    off, siz = torch.tensor([0, 100, 50]), torch.tensor([40, 7, 50])
    with FakeTensorMode(allow_non_fake_inputs=True) as mode:
        new = mode.from_tensor(torch.empty(107))
        hidden = mode.from_tensor(torch.empty(107))
        for codec in ("qsgd", "rqsgd", "cnat"):
            got = A.stoch_encode_delta_update_batched(new, hidden, off, siz, codec, 8, 1, 2)
            want = torch.ops.adfl.stoch_encode_delta_batched(new, hidden, off, siz, codec, 8, 1, 2)
            assert [(t.shape, t.dtype, t.device) for t in got] == [(t.shape, t.dtype, t.device) for t in want]
            assert got[0].shape == (107,) and got[0].dtype == (torch.int8 if codec == "cnat" else torch.uint8)
            assert got[2].shape == (3,) and got[3].dtype == torch.float32
    names = {n.split(".")[0] for n in torch._C._dispatch_get_all_op_names() if n.startswith("adfl::")}
    assert len(names) == 19, sorted(names)                      # the codec namespace is unchanged


def test_host_layers_expose_the_broadcast():
    assert callable(sops.rqsgd_encode_delta_update_batched) and callable(sops.qsgd_quantize_update_batched)
    assert {"rqsgd_encode_delta_update_batched", "qsgd_quantize_update_batched"} <= set(sops.__all__)
    # the stochastic channels share one fused override; the uni-directional classes keep the identity route
    for cls in (QSGDChannel, RQSGDChannel, CNATChannel):
        assert cls.broadcast_delta_ is not _CodecChannel.broadcast_delta_, cls.__name__
        assert cls.broadcast_delta_ is QSGDChannel.broadcast_delta_ is not SLQChannel.broadcast_delta_
    for cls in (UQSGDChannel, URQSGDChannel, UCNATChannel):
        assert cls.broadcast_delta_ is not QSGDChannel.broadcast_delta_, cls.__name__
