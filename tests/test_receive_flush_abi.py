"""CPU: the fused decode + accumulate + flush entries' C ABI (the buffered servers' K-th client update) — declared in
include/adfl_slq.h / adfl_stoch.h, bound in _lib.SIGNATURES, exported by the library, the ABI version unchanged,
every argument error answered with ADFL_E_ARG before anything is launched (no call here reaches a kernel: the
well-formed calls with a null d_buf are stopped by their last check, the payload's alignment) — and the six custom
ops' registration, schemas and fakes."""

import ctypes
import os
import re

import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import adfl_amd  # noqa: F401  registers the custom ops
from adfl_amd import _lib, flush
from adfl_amd._build import LIB_PATH

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
SLQ_FEDBUFF = ("adfl_slq_dequantize_fedbuff_flush_batched", "adfl_slq_dequantize_fedbuff_flush_batched_int4")
SLQ_FADAS = ("adfl_slq_dequantize_fadas_flush_batched", "adfl_slq_dequantize_fadas_flush_batched_int4")
STOCH_FEDBUFF, STOCH_FADAS = "adfl_stoch_dequantize_fedbuff_flush_batched", "adfl_stoch_dequantize_fadas_flush_batched"
E_ARG, E_ALIGN = -1, -3
SC = (0.9, 0.1, 0.999, 0.001, 0.03, 1e-8, 0.5)
P16, P4 = 16, 4      # a 16-byte aligned non-null pointer value, and one that is not


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, name)).read(), flags=re.S)


def test_declared_bound_and_exported():
    raw = ctypes.CDLL(LIB_PATH)
    for header, names in (("adfl_slq.h", SLQ_FEDBUFF + SLQ_FADAS), ("adfl_stoch.h", (STOCH_FEDBUFF, STOCH_FADAS))):
        text = _header(header)
        for name in names:
            assert re.search(rf"\bint\s+{name}\s*\(", text), name
            assert name in _lib.SIGNATURES, name
            assert hasattr(raw, name), name
            params = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)", text).group(1)
            assert len(params.split(",")) == len(_lib.SIGNATURES[name][1]), name
    P, F = ctypes.c_void_p, ctypes.c_float
    for name in SLQ_FEDBUFF:     # payload, chunks, scales, buf, g, out, stream; factor and lr
        assert _lib.SIGNATURES[name][1].count(P) == 7 and _lib.SIGNATURES[name][1].count(F) == 2
    for name in SLQ_FADAS:       # ... m, v, v_hat as well; the seven FADAS scalars
        assert _lib.SIGNATURES[name][1].count(P) == 10 and _lib.SIGNATURES[name][1].count(F) == 7
    # two planes, chunks, norms, mins, tables, stream; s beside the scalars
    assert _lib.SIGNATURES[STOCH_FEDBUFF][1].count(P) == 9 and _lib.SIGNATURES[STOCH_FEDBUFF][1].count(F) == 3
    assert _lib.SIGNATURES[STOCH_FADAS][1].count(P) == 12 and _lib.SIGNATURES[STOCH_FADAS][1].count(F) == 8


def test_abi_version_is_still_3():
    assert "#define ADFL_SLQ_ABI_VERSION 3" in open(os.path.join(INCLUDE, "adfl_slq.h")).read()
    assert _lib.ABI_VERSION == 3 and _lib.load().adfl_slq_abi_version() == 3


def _slq_fedbuff(fn, q=P16, chunks=P16, nchunks=1, scales=P16, buf=P16, g=P16, out=P16, ntensors=1, K=3):
    return fn(q, chunks, nchunks, scales, buf, g, out, ntensors, K, 0.5, 0.05, None)


def _slq_fadas(fn, q=P16, chunks=P16, nchunks=1, scales=P16, buf=P16, g=P16, m=P16, v=P16, h=P16, out=P16,
               ntensors=1, K=3):
    return fn(q, chunks, nchunks, scales, buf, g, m, v, h, out, ntensors, K, *SC, None)


def _stoch_fedbuff(codec=0, lv=P16, sg=P16, chunks=P16, nchunks=1, norms=P16, mins=P16, buf=P16, g=P16, out=P16,
                   ntensors=1, K=3):
    return _lib.load().adfl_stoch_dequantize_fedbuff_flush_batched(codec, lv, sg, chunks, nchunks, norms, mins, 255.0,
                                                                  buf, g, out, ntensors, K, 0.5, 0.05, None)


def _stoch_fadas(codec=0, lv=P16, sg=P16, chunks=P16, nchunks=1, norms=P16, mins=P16, buf=P16, g=P16, m=P16, v=P16,
                 h=P16, out=P16, ntensors=1, K=3):
    return _lib.load().adfl_stoch_dequantize_fadas_flush_batched(codec, lv, sg, chunks, nchunks, norms, mins, 255.0, buf,
                                                                g, m, v, h, out, ntensors, K, *SC, None)


COUNTS = [dict(nchunks=0), dict(nchunks=-1), dict(nchunks=1 << 31), dict(ntensors=0), dict(ntensors=-2), dict(K=0),
          dict(K=-3)]


def test_slq_argument_errors_return_codes_without_launching():
    lib = _lib.load()
    for name in SLQ_FEDBUFF:
        fn = getattr(lib, name)
        for null in ("q", "chunks", "scales", "g", "out"):
            assert _slq_fedbuff(fn, **{null: None}) == E_ARG, (name, null)
        for bad in COUNTS:
            assert _slq_fedbuff(fn, **bad) == E_ARG, (name, bad)
    for name in SLQ_FADAS:
        fn = getattr(lib, name)
        for null in ("q", "chunks", "scales", "g", "m", "v", "h", "out"):
            assert _slq_fadas(fn, **{null: None}) == E_ARG, (name, null)
        for bad in COUNTS:
            assert _slq_fadas(fn, **bad) == E_ARG, (name, bad)


def test_stoch_argument_errors_return_codes_without_launching():
    for call, tables in ((_stoch_fedbuff, ("g", "out")), (_stoch_fadas, ("g", "m", "v", "h", "out"))):
        for null in ("lv", "sg", "chunks", "norms") + tables:
            assert call(**{null: None}) == E_ARG, (call.__name__, null)
        for bad in COUNTS:
            assert call(**bad) == E_ARG, (call.__name__, bad)
        for codec in (-1, 3, 99):                                  # an unknown codec
            assert call(codec=codec) == E_ARG, (call.__name__, codec)
        assert call(codec=1, mins=None) == E_ARG                    # RQSGD needs its minima
        # ... and only RQSGD does: QSGD / CNAT with null mins pass every argument check (stopped at the alignment)
        assert call(codec=0, mins=None, lv=P4) == E_ALIGN
        assert call(codec=2, mins=None, sg=P4) == E_ALIGN


def test_a_null_buffer_table_is_accepted():
    """d_buf == NULL is "no buffer", not an argument error: with every other argument well-formed the call gets
    past the argument checks and is answered by the last one before the launch, the payload's alignment."""
    lib = _lib.load()
    for name in SLQ_FEDBUFF:
        assert _slq_fedbuff(getattr(lib, name), buf=None, q=P4) == E_ALIGN, name
        assert _slq_fedbuff(getattr(lib, name), buf=None, q=P4, K=0) == E_ARG, name   # the other checks still apply
    for name in SLQ_FADAS:
        assert _slq_fadas(getattr(lib, name), buf=None, q=P4) == E_ALIGN, name
        assert _slq_fadas(getattr(lib, name), buf=None, q=P4, m=None) == E_ARG, name
    for call in (_stoch_fedbuff, _stoch_fadas):
        assert call(buf=None, lv=P4) == E_ALIGN, call.__name__
        assert call(buf=None, lv=P4, g=None) == E_ARG, call.__name__


OPS = {
    "slq_dequantize_fedbuff_flush_batched": [], "slq_dequantize_fedbuff_flush_batched_int4": [],
    "stoch_dequantize_fedbuff_flush_batched": [],
    "slq_dequantize_fadas_flush_batched": ["m", "v", "v_hat"], "slq_dequantize_fadas_flush_batched_int4": ["m", "v", "v_hat"],
    "stoch_dequantize_fadas_flush_batched": ["m", "v", "v_hat"],
}


def test_custom_ops_registered_with_schemas_and_fakes():
    A = torch.ops.adfl_apply
    names = {n.split(".")[0] for n in torch._C._dispatch_get_all_op_names()}
    for name, mutated in OPS.items():
        assert hasattr(A, name) and f"adfl_apply::{name}" in names, name
        args = getattr(A, name).default._schema.arguments
        assert [a.name for a in args if a.is_write] == mutated, name
        assert "Tensor? buf" in str(getattr(A, name).default._schema), name    # the buffer is optional
    assert len([n for n in names if n.startswith("adfl::")]) == 19   # the codec's namespace is left as it was
    off, siz = torch.tensor([0, 100, 50]), torch.tensor([40, 7, 50])
    sc = flush.fadas_scalars(0.9, 0.999, 1e-8, 0.05, 2)
    with FakeTensorMode(allow_non_fake_inputs=True) as mode:
        buf, g, m, v, h = (mode.from_tensor(torch.empty(107)) for _ in range(5))
        q = mode.from_tensor(torch.empty(107, dtype=torch.int8))
        p4 = mode.from_tensor(torch.empty(54, dtype=torch.uint8))
        lv = mode.from_tensor(torch.empty(107, dtype=torch.uint8))
        s3 = mode.from_tensor(torch.empty(3))
        outs = [A.slq_dequantize_fedbuff_flush_batched(q, s3, buf, g, off, siz, 3, 0.5, 0.05),
                A.slq_dequantize_fedbuff_flush_batched(q, s3, None, g, off, siz, 1, 0.5, 0.05),
                A.slq_dequantize_fedbuff_flush_batched_int4(p4, s3, buf, g, off, siz, 3, 0.5, 0.05),
                A.stoch_dequantize_fedbuff_flush_batched(lv, q, s3, s3, buf, g, off, siz, "rqsgd", 8, 3, 0.5, 0.05),
                A.slq_dequantize_fadas_flush_batched(q, s3, buf, g, m, v, h, off, siz, 3, *sc),
                A.slq_dequantize_fadas_flush_batched_int4(p4, s3, None, g, m, v, h, off, siz, 1, *sc),
                A.stoch_dequantize_fadas_flush_batched(lv, q, s3, s3, buf, g, m, v, h, off, siz, "cnat", 8, 3, *sc)]
        for out in outs:
            assert out.shape == (107,) and out.dtype == torch.float32


def test_python_surface():
    """The wrappers, the channels' method and FadasMoments' exist on the modules and classes that document them."""
    from adfl_amd import ops, stoch
    from adfl_amd.Channel._base import _CodecChannel
    for mod in (ops, stoch):
        assert callable(mod.dequantize_fedbuff_flush_batched) and callable(mod.dequantize_fadas_flush_batched)
    assert callable(_CodecChannel.receive_scaled_flush) and callable(adfl_amd.FadasMoments.receive_flush)
    for cls in (adfl_amd.SLQChannel, adfl_amd.PackedSLQChannel, adfl_amd.QSGDChannel, adfl_amd.RQSGDChannel,
                adfl_amd.CNATChannel, adfl_amd.USLQChannel, adfl_amd.UCNATChannel):
        assert cls._flush_payload is not _CodecChannel._flush_payload, cls
