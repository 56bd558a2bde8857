"""Access to tests/golden/apply_small.npz (make_golden_apply.py) for test_apply_golden.py and
test_gpu_channel_apply.py: the reference's payloads decoded by the oracles, the coefficients its strategies used,
and the numpy restatement of the arithmetic the kernels implement."""

import numpy as np

import apply_cases as ac
import slq_oracle
import stoch_oracle as so

F32 = np.float32


def f32_of_bits(rec) -> np.float32:
    return np.array([rec["bits"]], np.uint32).view(np.float32)[0]


def slq_scale(rec) -> float:
    """The payload's q_scale(), a double."""
    return float(np.array([rec["f64_bits"]], np.uint64).view(np.float64)[0])


def passthrough(run: str, name: str) -> np.ndarray:
    return ac.fixture()[0][f"{run}__pass__{name}"]


def oracle_decode(run: str, name: str) -> np.ndarray:
    """The decode of one coded entry of a run, by the CPU oracle, from the stored payload."""
    z, m = ac.fixture()
    rec = m["runs"][run]
    q = z[f"{run}__q__{name}"]
    if run.startswith("slq"):
        return slq_oracle.np_decode(q, F32(slq_scale(rec["scale"][name])))   # fbgemm uses the scale as fp32
    signs = z[f"{run}__signs__{name}"]
    norm = f32_of_bits(rec["scale"][name])
    levels = 2 ** rec["bits"] - 1
    if run.startswith("qsgd"):
        return so.qsgd_dequantize(q, signs, levels, norm)
    if run.startswith("rqsgd"):
        return so.rqsgd_dequantize(q, signs, levels, norm, f32_of_bits(rec["scale_2"][name]))
    return so.cnat_dequantize(q.view(np.int8) if rec["q_dtype"][name] == "int8" else q, signs, norm)


def decoded(run: str):
    """D(c) of a run as numpy arrays in the dict's order (passthrough entries as stored)."""
    _, m = ac.fixture()
    return {n: oracle_decode(run, n) if n in ac.CODED else passthrough(run, n) for n in m["order"]}


def coef(run: str, case: str):
    _, m = ac.fixture()
    return [float.fromhex(h) for h in m["runs"][run]["coef"][case]]


def np_axpby(y: np.ndarray, d: np.ndarray, alpha: float, beta: float) -> np.ndarray:
    """fp32(fp32(af * y) + fp32(bf * d)), af / bf the Python doubles rounded to fp32 first: three separately
    rounded fp32 operations (numpy never contracts)."""
    with np.errstate(all="ignore"):
        a = (F32(alpha) * y.astype(F32)).astype(F32)
        b = (F32(beta) * d.astype(F32)).astype(F32)
        return (a + b).astype(F32)


def np_scale(d: np.ndarray, factor: float) -> np.ndarray:
    with np.errstate(all="ignore"):
        return (F32(factor) * d.astype(F32)).astype(F32)
