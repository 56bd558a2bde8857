"""CPU: the stochastic delta encode's C ABI, binding table, header constant, argument checks (nothing is launched
by any call here) and the custom op's registration and fake implementation."""

import ctypes
import re

import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import adfl_amd  # noqa: F401  registers torch.ops.adfl.*
from adfl_amd import _lib
from adfl_amd._build import LIB_PATH
import delta_cases

NEW = ["adfl_rqsgd_encode_delta_batched", "adfl_rqsgd_encode_delta_batched_work", "adfl_bucket_diff"]
E_ARG, E_BITS, E_ALIGN, E_WORKSPACE = -1, -2, -3, -4


def test_symbols_bound_and_exported():
    raw = ctypes.CDLL(LIB_PATH)
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert hasattr(raw, name), name
    # the non-delta counterparts with one more source pointer and the per-tensor uniform shifts
    assert len(_lib.SIGNATURES[NEW[0]][1]) == len(_lib.SIGNATURES["adfl_rqsgd_encode_batched"][1]) + 2
    assert len(_lib.SIGNATURES[NEW[1]][1]) == len(_lib.SIGNATURES["adfl_rqsgd_encode_batched_work"][1]) + 2
    assert len(_lib.SIGNATURES[NEW[1]][1]) == len(_lib.SIGNATURES[NEW[0]][1]) + 2   # work list, nwork


def test_abi_version_is_still_3():
    assert delta_cases.header_constant("ADFL_SLQ_ABI_VERSION") == _lib.ABI_VERSION == 3
    assert _lib.load().adfl_slq_abi_version() == 3


def test_rqsgd_delta_argument_errors_return_codes_without_launching():
    lib = _lib.load()
    two, work = lib.adfl_rqsgd_encode_delta_batched, lib.adfl_rqsgd_encode_delta_batched_work
    p = 16   # any non-null, aligned value: no call below gets as far as a launch
    ws = 16  # adfl_stoch_workspace_bytes(1)
    assert lib.adfl_stoch_workspace_bytes(1) == ws

    def call(new=p, prev=p, chunks=p, nchunks=1, bits=8, unif=None, ushift=None, wsp=p, wsb=ws, lv=p, sg=p, nr=p,
             mn=p, work_args=None):
        args = (bits, unif, ushift, 1, 2, wsp, wsb, lv, sg, nr, mn, None)
        if work_args is None:
            return two(new, prev, chunks, nchunks, *args)
        return work(new, prev, chunks, nchunks, *work_args, *args)

    for wa in (None, (p, 0), (p, 1)):   # the two-pass entry, the _work entry as two-pass, with a work list
        assert call(new=None, work_args=wa) == E_ARG          # null tables
        assert call(prev=None, work_args=wa) == E_ARG
        assert call(chunks=None, work_args=wa) == E_ARG
        assert call(lv=None, work_args=wa) == E_ARG           # null planes
        assert call(sg=None, work_args=wa) == E_ARG
        assert call(nr=None, work_args=wa) == E_ARG           # null norms / mins
        assert call(mn=None, work_args=wa) == E_ARG
        assert call(wsp=None, work_args=wa) == E_ARG          # null workspace
        assert call(bits=0, work_args=wa) == E_BITS
        assert call(bits=17, work_args=wa) == E_BITS
        assert call(nchunks=0, work_args=wa) == E_ARG
        assert call(nchunks=-1, work_args=wa) == E_ARG
        assert call(nchunks=1 << 31, wsb=1 << 40, work_args=wa) == E_ARG   # oversized
        assert call(wsb=ws - 1, work_args=wa) == E_WORKSPACE
        assert call(nchunks=3, wsb=2 * ws, work_args=wa) == E_WORKSPACE
        assert call(wsp=24, work_args=wa) == E_ALIGN           # workspace base
        assert call(lv=20, work_args=wa) == E_ALIGN            # plane bases
        assert call(sg=8, work_args=wa) == E_ALIGN
        assert call(unif=4, work_args=wa) == E_ALIGN           # injected uniforms' base
    assert call(work_args=(None, 1)) == E_ARG                  # null work list
    assert call(work_args=(p, -1)) == E_ARG                    # nwork < 0
    assert call(work_args=(p, 2)) == E_ARG                     # nwork > nchunks


def test_bucket_diff_argument_errors():
    f = _lib.load().adfl_bucket_diff
    p = 16
    assert f(None, p, 1, p, p, None) == E_ARG
    assert f(p, None, 1, p, p, None) == E_ARG
    assert f(p, p, 1, None, p, None) == E_ARG
    assert f(p, p, 1, p, None, None) == E_ARG
    assert f(p, p, 0, p, p, None) == E_ARG
    assert f(p, p, -1, p, p, None) == E_ARG
    assert f(p, p, 1 << 31, p, p, None) == E_ARG


def test_custom_op_registered_with_the_non_delta_ops_schema_and_fake():
    A = torch.ops.adfl
    assert hasattr(A, "stoch_encode_delta_batched")
    schema = str(A.stoch_encode_delta_batched.default._schema)
    base = str(A.stoch_encode_batched.default._schema)
    # the same schema with two sources in place of one
    assert schema.replace("stoch_encode_delta_batched(Tensor new, Tensor prev,", "stoch_encode_batched(Tensor flat,") == base
    assert re.search(r"\(Tensor new, Tensor prev, Tensor offsets, Tensor sizes, str codec, (Sym)?[Ii]nt bits, "
                     r"(Sym)?[Ii]nt seed, (Sym)?[Ii]nt counter\) -> \(Tensor, Tensor, Tensor, Tensor\)", schema), schema
    off, siz = torch.tensor([0, 100, 50]), torch.tensor([40, 7, 50])
    with FakeTensorMode(allow_non_fake_inputs=True) as mode:
        new = mode.from_tensor(torch.empty(107))
        prev = mode.from_tensor(torch.empty(107))
        for codec in ("qsgd", "rqsgd", "cnat"):
            got = A.stoch_encode_delta_batched(new, prev, off, siz, codec, 8, 1, 2)
            want = A.stoch_encode_batched(new, off, siz, codec, 8, 1, 2)
            assert [(t.shape, t.dtype, t.device) for t in got] == [(t.shape, t.dtype, t.device) for t in want]
            assert got[0].shape == (107,) and got[0].dtype == (torch.int8 if codec == "cnat" else torch.uint8)
            assert got[2].shape == (3,) and got[3].dtype == torch.float32


def test_there_are_19_custom_ops():
    names = {n.split(".")[0] for n in torch._C._dispatch_get_all_op_names() if n.startswith("adfl::")}
    assert "adfl::stoch_encode_delta_batched" in names
    assert len(names) == 19, sorted(names)
