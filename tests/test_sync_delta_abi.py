"""CPU: the fused decode-mean + axpby entries' C ABI (the synchronous DELTA server step) — declared in
include/adfl_slq.h / adfl_stoch.h, bound in _lib.SIGNATURES, exported by the library, the ABI version unchanged, and
every argument error answered with ADFL_E_ARG before anything is launched (no call here reaches a kernel) — and the
three custom ops' registration and fakes."""

import ctypes
import os
import re

import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import adfl_amd  # noqa: F401  registers the custom ops
from adfl_amd import _lib
from adfl_amd._build import LIB_PATH

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
SLQ8, SLQ4 = "adfl_slq_dequantize_mean_axpby_batched", "adfl_slq_dequantize_mean_axpby_batched_int4"
STOCH = "adfl_stoch_dequantize_mean_axpby_batched"
HEADERS = {SLQ8: "adfl_slq.h", SLQ4: "adfl_slq.h", STOCH: "adfl_stoch.h"}
E_ARG = -1
MAX_ROWS = 1 << 19


def _params(name):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, HEADERS[name])).read(), flags=re.S)
    m = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)", header)
    assert m, name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_declared_bound_and_exported_with_the_declared_signatures():
    raw = ctypes.CDLL(LIB_PATH)
    for name in HEADERS:
        assert name in _lib.SIGNATURES and hasattr(raw, name), name
        res, args = _lib.SIGNATURES[name]
        params = _params(name)
        assert res is ctypes.c_int and len(params) == len(args), name
        for p, a in zip(params, args):   # each declared parameter against its binding
            want = (ctypes.c_void_p if "*" in p else ctypes.c_float if p.startswith("float ")
                    else ctypes.c_int64 if p.startswith("int64_t ") else ctypes.c_int32 if p.startswith("int32_t ")
                    else ctypes.c_int)
            assert a is want, (name, p)
        # what replaces self_row / d_self_x: one base and one output pointer table, ntensors, alpha, beta
        tail = params[-6:]
        assert tail == ["const float* const* d_base", "float* const* d_out", "int32_t ntensors", "float alpha",
                        "float beta", "void* stream"], name
        assert not any("self" in p for p in params), name


def test_abi_version_is_still_3():
    assert "#define ADFL_SLQ_ABI_VERSION 3" in open(os.path.join(INCLUDE, "adfl_slq.h")).read()
    assert _lib.ABI_VERSION == 3 and _lib.load().adfl_slq_abi_version() == 3


def test_slq_argument_errors_return_codes_without_launching():
    p = 16   # any non-null, 16-byte aligned value: no call below gets as far as a launch
    for name in (SLQ8, SLQ4):
        fn = getattr(_lib.load(), name)
        # (q, row_stride, k, chunks, nchunks, scales, scale_stride, base, out, ntensors, alpha, beta, stream)
        ok = [p, 64, 5, p, 1, p, 3, p, p, 3, 1.0, 1.0, None]
        for null in (0, 3, 5, 7, 8):                             # payload, chunk table, scales, base and out tables
            args = list(ok)
            args[null] = None
            assert fn(*args) == E_ARG, (name, null)
        for idx, bad in ((9, 0), (9, -2),                        # ntensors < 1
                         (2, 0), (2, -1), (2, MAX_ROWS + 1),     # k < 1 or above adfl_sum::kMaxRows
                         (1, 0), (1, 24), (1, -16),              # row stride: not a positive multiple of 16
                         (4, 0), (4, -1), (4, 1 << 31),          # nchunks outside [1, INT32_MAX]
                         (6, 0)):                                # scale stride
            args = list(ok)
            args[idx] = bad
            assert fn(*args) == E_ARG, (name, idx, bad)


def test_stoch_argument_errors_return_codes_without_launching():
    fn = _lib.load().adfl_stoch_dequantize_mean_axpby_batched
    p = 16
    # (codec, levels, signs, row_stride, k, chunks, nchunks, bits, norms, mins, norm_stride, base, out, ntensors,
    #  alpha, beta, stream)
    for codec in (0, 1, 2):
        ok = [codec, p, p, 64, 5, p, 1, 8, p, p, 3, p, p, 3, 1.0, 1.0, None]
        for null in (1, 2, 5, 8, 11, 12):                        # planes, chunk table, norms, base and out tables
            args = list(ok)
            args[null] = None
            assert fn(*args) == E_ARG, (codec, null)
        for idx, bad in ((13, 0), (13, -1), (4, 0), (4, MAX_ROWS + 1), (3, 24), (3, 0), (6, 0), (6, 1 << 31),
                         (10, 0)):
            args = list(ok)
            args[idx] = bad
            assert fn(*args) == E_ARG, (codec, idx, bad)
    ok = [1, p, p, 64, 5, p, 1, 8, p, None, 3, p, p, 3, 1.0, 1.0, None]
    assert fn(*ok) == E_ARG                                      # RQSGD without its minima
    ok[0] = 7
    assert fn(*ok) == E_ARG                                      # unknown codec


def test_custom_ops_registered_with_fakes():
    A = torch.ops.adfl_apply
    ops_ = ("slq_decode_mean_axpby_batched", "slq_decode_mean_axpby_batched_int4", "stoch_decode_mean_axpby_batched")
    names = {n.split(".")[0] for n in torch._C._dispatch_get_all_op_names()}
    for name in ops_:
        assert hasattr(A, name) and f"adfl_apply::{name}" in names, name
        assert not any(a.is_write for a in getattr(A, name).default._schema.arguments), name   # functional
    assert len([n for n in names if n.startswith("adfl::")]) == 19   # the codec's namespace is left as it was
    off, siz = torch.tensor([0, 100, 50]), torch.tensor([40, 7, 50])
    with FakeTensorMode(allow_non_fake_inputs=True) as mode:
        base = mode.from_tensor(torch.empty(107))
        q = mode.from_tensor(torch.empty((4, 112), dtype=torch.int8))
        p = mode.from_tensor(torch.empty((4, 64), dtype=torch.uint8))
        sg = mode.from_tensor(torch.empty((4, 112), dtype=torch.int8))
        sc = mode.from_tensor(torch.empty((4, 3)))
        for out in (A.slq_decode_mean_axpby_batched(q, sc, base, off, siz, 1.0, 1.0),
                    A.slq_decode_mean_axpby_batched_int4(p, sc, base, off, siz, 0.4, 0.6),
                    A.stoch_decode_mean_axpby_batched(q, sg, sc, sc, base, off, siz, "rqsgd", 8, 1.0, 1.0)):
            assert out.shape == (107,) and out.dtype == torch.float32
