"""The runs, updates and strategy settings of the fused decode + accumulate + flush golden fixture
(receive_flush_small.npz), listed once: the generator (make_golden_receive_flush.py) and the tests
(test_receive_flush_golden.py, test_gpu_receive_flush_golden.py) take them from here, with access to the stored
payloads and their decode by the CPU oracles.

The dict, the seeds, lr and the staleness values are flush_cases'. Six updates are encoded per run: updates 0-2 are
FedBuff's one buffer and FADAS's first, updates 3-5 FADAS's second, update 0 alone FedBuff(1)'s. The inputs are
regenerated from the seeds and are not stored (the fixture pins their digests); the passthrough entries of a payload
are the update's own ndim <= 1 entries and are not stored either."""

import json
import os

import numpy as np

import flush_cases as fc
import slq_oracle
import stoch_oracle as so

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "receive_flush_small.npz")
MAX_BYTES = 400 * 1000                   # the flush fixture's own limit

F32 = np.float32
# run name -> (the reference channel's class, bits)
RUNS = {"slq_b8": ("SLQChannel", 8), "slq_b4": ("SLQChannel", 4), "qsgd_b8": ("QSGDChannel", 8),
        "rqsgd_b8": ("RQSGDChannel", 8), "cnat_b8": ("CNATChannel", 8)}
FULL_PRIME = ("slq_b8", "qsgd_b8")       # the runs whose FADAS params_prime is stored in full
CODED = [n for n, s, _ in fc.DICT_SHAPES if len(s) > 1]
ORDER = [n for n, _, _ in fc.DICT_SHAPES]

K = fc.K
LR = fc.LR
UPDATES = [("fedbuff", 0, 0), ("fedbuff", 0, 1), ("fedbuff", 0, 2), ("fadas", 1, 0), ("fadas", 1, 1), ("fadas", 1, 2)]
FEDBUFF_UPDATES, FEDBUFF_STALENESS = (0, 1, 2), fc.FEDBUFF_STALENESS        # FedBuff(3, 0.05, True): one flush
FADAS_UPDATES = ((0, 1, 2), (3, 4, 5))                                       # FADAS(3, 0.05): two flushes
FADAS_STALENESS = fc.FADAS_STALENESS[:2]                                     # the second has 25 > max_delay
FEDBUFF1_UPDATE, FEDBUFF1_STALENESS = 0, 0                                   # FedBuff(1, 0.05, True): no buffer


def update(j: int):
    return fc.update(*UPDATES[j])


def fedbuff_g():
    return fc.g_params("fedbuff", 0)


def fadas_g(r: int):
    return fc.g_params("fadas", r)


_cache = {}


def fixture():
    if "z" not in _cache:
        z = np.load(FIXTURE)
        _cache["z"] = z
        _cache["m"] = json.loads(str(z["manifest"]))
    return _cache["z"], _cache["m"]


def f32_of_bits(rec) -> np.float32:
    return np.array([rec["bits"]], np.uint32).view(np.float32)[0]


def slq_scale(rec) -> float:
    """The payload's q_scale(), a double."""
    return float(np.array([rec["f64_bits"]], np.uint64).view(np.float64)[0])


def oracle_decode(run: str, j: int, name: str) -> np.ndarray:
    """The decode of one coded entry of update j of a run, by the CPU oracle, from the stored payload."""
    z, m = fixture()
    rec = m["runs"][run]["payloads"][j]
    q = z[f"{run}__u{j}__q__{name}"]
    if run.startswith("slq"):
        return slq_oracle.np_decode(q, F32(slq_scale(rec["scale"][name])))   # fbgemm uses the scale as fp32
    signs = z[f"{run}__u{j}__signs__{name}"]
    norm = f32_of_bits(rec["scale"][name])
    levels = 2 ** m["runs"][run]["bits"] - 1
    if run.startswith("qsgd"):
        return so.qsgd_dequantize(q, signs, levels, norm)
    if run.startswith("rqsgd"):
        return so.rqsgd_dequantize(q, signs, levels, norm, f32_of_bits(rec["scale_2"][name]))
    return so.cnat_dequantize(q.view(np.int8) if rec["q_dtype"][name] == "int8" else q, signs, norm)


def decoded(run: str, j: int):
    """D(c) of update j of a run as numpy arrays in the dict's order (passthrough entries: the update's own)."""
    u = update(j)
    return {n: oracle_decode(run, j, n) if n in CODED else u[n] for n in ORDER}
