"""CPU: the buffered servers' flush entries' C ABI — declared in include/adfl_slq.h, bound in _lib.SIGNATURES,
exported by the library, the ABI version unchanged, and every argument error answered with ADFL_E_ARG before
anything is launched (no call here reaches a kernel) — and the two custom ops' registration and fakes."""

import ctypes
import os
import re

import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import adfl_amd  # noqa: F401  registers the custom ops
from adfl_amd import _lib, flush
from adfl_amd._build import LIB_PATH

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
FEDBUFF, FADAS = "adfl_fedbuff_flush_batched", "adfl_fadas_flush_batched"
E_ARG = -1


def test_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, "adfl_slq.h")).read(), flags=re.S)
    raw = ctypes.CDLL(LIB_PATH)
    for name in (FEDBUFF, FADAS):
        assert re.search(rf"\bint\s+{name}\s*\(", header), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(raw, name), name
    # three / six pointer tables + the chunk table + the stream; one / seven float scalars after K
    P, F = ctypes.c_void_p, ctypes.c_float
    assert _lib.SIGNATURES[FEDBUFF][1].count(P) == 5 and _lib.SIGNATURES[FEDBUFF][1].count(F) == 1
    assert _lib.SIGNATURES[FADAS][1].count(P) == 8 and _lib.SIGNATURES[FADAS][1].count(F) == 7
    # the declaration's parameter count equals the binding's
    for name in (FEDBUFF, FADAS):
        params = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)", header).group(1)
        assert len(params.split(",")) == len(_lib.SIGNATURES[name][1]), name


def test_abi_version_is_still_3():
    assert "#define ADFL_SLQ_ABI_VERSION 3" in open(os.path.join(INCLUDE, "adfl_slq.h")).read()
    assert _lib.ABI_VERSION == 3 and _lib.load().adfl_slq_abi_version() == 3


def test_fedbuff_argument_errors_return_codes_without_launching():
    fn = _lib.load().adfl_fedbuff_flush_batched
    p = 16   # any non-null value: no call below gets as far as a launch
    # (buf, g, out, chunks, nchunks, ntensors, K, lr, stream)
    assert fn(None, p, p, p, 1, 1, 3, 0.05, None) == E_ARG       # null buffer table
    assert fn(p, None, p, p, 1, 1, 3, 0.05, None) == E_ARG       # null g table
    assert fn(p, p, None, p, 1, 1, 3, 0.05, None) == E_ARG       # null output table
    assert fn(p, p, p, None, 1, 1, 3, 0.05, None) == E_ARG       # null chunk table
    assert fn(p, p, p, p, 0, 1, 3, 0.05, None) == E_ARG          # nchunks 0
    assert fn(p, p, p, p, -1, 1, 3, 0.05, None) == E_ARG
    assert fn(p, p, p, p, 1 << 31, 1, 3, 0.05, None) == E_ARG    # oversized
    assert fn(p, p, p, p, 1, 0, 3, 0.05, None) == E_ARG          # ntensors 0
    assert fn(p, p, p, p, 1, -2, 3, 0.05, None) == E_ARG
    assert fn(p, p, p, p, 1, 1, 0, 0.05, None) == E_ARG          # K 0
    assert fn(p, p, p, p, 1, 1, -3, 0.05, None) == E_ARG


def test_fadas_argument_errors_return_codes_without_launching():
    fn = _lib.load().adfl_fadas_flush_batched
    p = 16
    s = (0.9, 0.1, 0.999, 0.001, 0.03, 1e-8, 0.5)
    # (buf, g, m, v, v_hat, out, chunks, nchunks, ntensors, K, 7 scalars, stream)
    for null in range(7):                                        # each of the six tables, then the chunk table
        tables = [None if i == null else p for i in range(7)]
        assert fn(*tables, 1, 1, 3, *s, None) == E_ARG, null
    assert fn(*[p] * 7, 0, 1, 3, *s, None) == E_ARG              # nchunks 0
    assert fn(*[p] * 7, -1, 1, 3, *s, None) == E_ARG
    assert fn(*[p] * 7, 1 << 31, 1, 3, *s, None) == E_ARG        # oversized
    assert fn(*[p] * 7, 1, 0, 3, *s, None) == E_ARG              # ntensors 0
    assert fn(*[p] * 7, 1, 1, 0, *s, None) == E_ARG              # K 0
    assert fn(*[p] * 7, 1, 1, -1, *s, None) == E_ARG


def test_custom_ops_registered_with_fakes():
    A = torch.ops.adfl_apply
    for name in ("fedbuff_flush_batched", "fadas_flush_batched"):
        assert hasattr(A, name), name
    names = {n.split(".")[0] for n in torch._C._dispatch_get_all_op_names()}
    assert {"adfl_apply::fedbuff_flush_batched", "adfl_apply::fadas_flush_batched"} <= names
    assert len([n for n in names if n.startswith("adfl::")]) == 19   # the codec's namespace is left as it was
    mutated = [a.name for a in A.fadas_flush_batched.default._schema.arguments if a.is_write]
    assert mutated == ["m", "v", "v_hat"]
    assert not any(a.is_write for a in A.fedbuff_flush_batched.default._schema.arguments)
    off, siz = torch.tensor([0, 100, 50]), torch.tensor([40, 7, 50])
    sc = flush.fadas_scalars(0.9, 0.999, 1e-8, 0.05, 2)
    with FakeTensorMode(allow_non_fake_inputs=True) as mode:
        buf, g, m, v, h = (mode.from_tensor(torch.empty(107)) for _ in range(5))
        for out in (A.fedbuff_flush_batched(buf, g, off, siz, 3, 0.05),
                    A.fadas_flush_batched(buf, g, m, v, h, off, siz, 3, *sc)):
            assert out.shape == (107,) and out.dtype == torch.float32


def test_scalars_are_the_references_doubles():
    """fadas_scalars: fadas.py:97-101,127-128 in Python doubles (each rounded to fp32 once, at the call)."""
    import math
    b1, omb1, b2, omb2, sq, eps, step = flush.fadas_scalars(0.9, 0.999, 1e-8, 0.05 / 25, 3)
    assert (b1, omb1, b2, omb2, eps) == (0.9, 1 - 0.9, 0.999, 1 - 0.999, 1e-8)
    assert sq == math.sqrt(1 - 0.999 ** 3) and step == (0.05 / 25) / (1 - 0.9 ** 3)
