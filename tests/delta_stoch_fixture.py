"""Access to tests/golden/delta_stoch_small.npz + delta_stoch_manifest.json (made by executing the reference,
tests/golden/make_golden_delta_stoch.py), shared by test_delta_stoch_golden.py and test_gpu_stoch_channel_delta.py.
The main pair's inputs are delta_small.npz's (not stored twice)."""

import json
import os

import numpy as np

from conftest import GOLDEN

MANIFEST = json.load(open(os.path.join(GOLDEN, "delta_stoch_manifest.json")))
ARR = np.load(os.path.join(GOLDEN, "delta_stoch_small.npz"))
_MAIN = np.load(os.path.join(GOLDEN, "delta_small.npz"))
PAIRS = list(MANIFEST["pairs"])                     # main, zero, nan
RUNS = [(c, b) for c in ("qsgd", "rqsgd", "cnat") for b in (8, 4)]


def pair(pname: str):
    """(prev, new) as name -> numpy array dicts, each in the key order the reference was given."""
    rec = MANIFEST["pairs"][pname]
    if pname == "main":
        get = lambda side, n: _MAIN[f"{side}__{n}"]              # noqa: E731
    else:
        get = lambda side, n: ARR[f"{side}__{pname}__{n}"]       # noqa: E731
    return ({n: get("prev", n) for n in rec["prev_order"]}, {n: get("new", n) for n in rec["new_order"]})


def run(pname: str, codec: str, bits: int) -> dict:
    return MANIFEST["pairs"][pname]["runs"][f"{codec}_b{bits}"]


def arr(pname: str, codec: str, bits: int, kind: str, name: str) -> np.ndarray:
    return ARR[f"{pname}__{codec}_b{bits}__{kind}__{name}"]


def uniforms(pname: str, name: str) -> np.ndarray:
    return ARR[f"u__{pname}__{name}"]


def scale_value(rec):
    """A scale record as (fp32 value, is the 0-dim tensor of the zero branch, is the int 0)."""
    if "int" in rec:
        return np.float32(rec["int"]), False, True
    return np.array([rec["bits"]], np.uint32).view(np.float32)[0], bool(rec.get("tensor")), False
