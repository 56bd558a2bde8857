"""CPU: bench.py's --dump-outputs writer and the --full switch, without a device (host tensors stand in for
the timed path's buffers; the GPU run is tests/test_gpu_bench_contract.py)."""

import os
import sys

import numpy as np
import torch

import bench


def _args(monkeypatch, argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    return bench.parse()


def test_full_and_dump_outputs_are_off_by_default(monkeypatch):
    a = _args(monkeypatch, ["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = _args(monkeypatch, ["--full", "--dump-outputs", "somewhere"])
    assert a.full is True and a.dump_outputs == "somewhere"


def test_dump_outputs_writes_a_fixed_float32_sample(tmp_path):
    n = 1 << 16
    g = torch.Generator().manual_seed(1)
    q = torch.randint(-127, 128, (64, n // 64), generator=g, dtype=torch.int8)
    scale = torch.tensor([3.0e-5])
    out = q.float() * scale
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), q, scale, out)
    assert sorted(os.listdir(tmp_path / "a")) == ["dequantized.npy", "payload.npy", "scale.npy"]
    got = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in ("payload", "dequantized", "scale")}
    m = 2 * bench.DUMP_EDGE + bench.DUMP_SAMPLE
    assert all(v.dtype == np.float32 for v in got.values())
    assert got["payload"].shape == got["dequantized"].shape == (m,)
    # at the real size (2^28 elements) the files stay under the 64 MB a dump may take: 4 bytes per position, twice
    assert 2 * 4 * m + 4 + 3 * 128 <= 64 * 10 ** 6
    qf, of = q.reshape(-1).numpy(), out.reshape(-1).numpy()
    e = bench.DUMP_EDGE
    assert np.array_equal(got["payload"][:e], qf[:e]) and np.array_equal(got["payload"][e:2 * e], qf[-e:])
    assert np.array_equal(got["dequantized"][:e], of[:e]) and np.array_equal(got["dequantized"][e:2 * e], of[-e:])
    assert np.array_equal(got["dequantized"], got["payload"] * np.float32(3.0e-5))   # the same positions in both
    assert np.array_equal(got["scale"], scale.numpy())
    for k, v in got.items():      # the positions do not change from call to call
        assert np.array_equal(v, np.load(tmp_path / "b" / f"{k}.npy")), k
