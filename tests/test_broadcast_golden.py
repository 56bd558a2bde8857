"""CPU: QAFeL's broadcast arithmetic as the executed reference computes it. The numpy restatement
(tests/broadcast_ref.py: the oracle's SLQ encode of fp32(g - h), then h + fp32(scale * q)) reproduces every step
of tests/golden/broadcast_small.npz — the reference's diff_parameters, SLQChannel(bits).on_server_send,
on_client_receive and add_parameters_inpace, three broadcasts in a row — bit for bit; and the packed variant's
nibble read-back is what adfl_amd.compression.unpack_4bit reads from pack_4bit's bytes."""

import os

import numpy as np
import pytest

import broadcast_cases as bc
import broadcast_ref as br
import delta_cases
import slq_oracle as so
from golden_util import GOLDEN, bits_of, same_f32

PATH = os.path.join(GOLDEN, "broadcast_small.npz")


def same_bytes(a, b) -> bool:
    a, b = np.atleast_1d(np.asarray(a)), np.atleast_1d(np.asarray(b))
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def matches(g, prefix: str, name: str, a: np.ndarray) -> bool:
    """a against prefix__<name>, or its SHA-256 against prefixsha__<name>."""
    if f"{prefix}__{name}" in g.files:
        return same_bytes(a, g[f"{prefix}__{name}"])
    return bc.sha(a) == str(g[f"{prefix}sha__{name}"])


@pytest.fixture(scope="module")
def g():
    return np.load(PATH)


@pytest.fixture(scope="module")
def inputs():
    return bc.inputs()


def test_fixture_is_small_and_the_recipe_reproduces_its_inputs(g, inputs):
    assert os.path.getsize(PATH) <= 256 * 1024
    order = [str(n) for n in g["order"]]
    assert order == [name for name, _, _ in delta_cases.DICT_SHAPES]
    assert [str(n) for n in g["new_order"]] == order[::-1]
    h0, news = inputs
    assert len(news) == bc.STEPS == 3
    for name in order:
        assert matches(g, "h0", name, h0[name]), name
        for k, new in enumerate(news, 1):
            if k == bc.STEPS and name == bc.FROZEN:
                continue
            assert matches(g, f"s{k}__new", name, new[name]), (k, name)
            if k > 1 and new[name].dtype == np.float32:
                assert not same_bytes(new[name], news[k - 2][name]), (k, name)   # g moves at every step
    assert h0["big.weight"].size == delta_cases.R + 1


@pytest.mark.parametrize("bits", [8, 4])
def test_restatement_reproduces_every_step_of_the_reference(g, inputs, bits):
    h0, news = inputs
    order = [str(n) for n in g["order"]]
    qnames = [str(n) for n in g[f"b{bits}__qnames"]]
    assert qnames == [n for n in order if h0[n].ndim > 1]
    hidden = {n: h0[n].copy() for n in order}
    for k, new in enumerate(news, 1):
        pre = f"b{bits}__s{k}"
        assert [str(n) for n in g[f"{pre}__order"]] == order          # diff_parameters iterates hidden_state
        size = 0
        for name in order:
            gn = new[name]
            if k == bc.STEPS and name == bc.FROZEN:
                gn = g[f"{pre}__new__{name}"]
                assert same_bytes(gn, hidden[name])                   # the frozen layer: g is the hidden state
            if name in qnames:
                q, scale, h2 = br.step(hidden[name], gn, bits)
                q_c, scale_c = so.encode((gn - hidden[name]).astype(np.float32), bits)   # the compiled oracle agrees
                assert np.array_equal(q, np.asarray(q_c).reshape(q.shape)) and bits_of(scale) == bits_of(scale_c)
                assert matches(g, f"{pre}__q", name, q), (k, name)
                assert bits_of(scale) == int(g[f"{pre}__scale_bits"][qnames.index(name)]), (k, name)
                size += q.size
            else:
                d = gn - hidden[name]
                assert same_bytes(d, g[f"{pre}__pass__{name}"]), (k, name)
                h2 = hidden[name] + d
                size += d.nbytes
            assert h2.dtype == hidden[name].dtype
            assert matches(g, f"{pre}__h", name, h2), (k, name)
            hidden[name] = h2
        assert size == int(g[f"{pre}__size"])
    k = qnames.index(bc.FROZEN)
    assert int(g[f"b{bits}__s3__scale_bits"][k]) == 0                 # scale +0, every code 127, h + 0
    assert (g[f"b{bits}__s3__q__{bc.FROZEN}"] == 127).all()
    assert same_bytes(g[f"b{bits}__s3__h__{bc.FROZEN}"], g[f"b{bits}__s2__h__{bc.FROZEN}"])


def _unpack(q: np.ndarray) -> np.ndarray:
    import torch
    from adfl_amd import compression
    if not torch.cuda.is_available():   # compression.py packs on the device: the oracle's pack / unpack restate it
        return so.np_unpack_int4(so.np_pack_int4(q.reshape(-1)), q.size).reshape(q.shape)
    packed = compression.pack_4bit(torch.from_numpy(q.copy()))
    return compression.unpack_4bit(packed, torch.Size(q.shape)).numpy().astype(np.int8)


@pytest.mark.parametrize("n", [1, 2, 33, 1024, 2049])
@pytest.mark.parametrize("case", ["random", "equal", "nan"])
def test_packed_update_reads_the_nibbles_back(n, case):
    rng = np.random.default_rng(n)
    h = rng.standard_normal(n, dtype=np.float32)
    h[0] = np.float32(-0.0)
    g = (h + np.float32(1e-2) * rng.standard_normal(n, dtype=np.float32)).astype(np.float32)
    if case == "equal":
        g = h.copy()
    elif case == "nan":
        g[n // 2] = np.nan
    q, scale, h2 = br.step(h, g, 4, packed=True)
    codes = br.readback_int4(q)
    assert np.array_equal(codes, _unpack(q))                          # the rule is unpack_4bit(pack_4bit(q))
    assert same_f32(h2, br.update(h, scale, codes))
    if case == "random":
        assert np.array_equal(codes, q) and bits_of(scale) != 0
    elif case == "equal":       # codes 127 alias: high nibble 7 (with its partner's carry, -1), low nibble -1
        assert (q == 127).all() and bits_of(scale) == 0
        assert set(np.unique(codes).tolist()) <= {7, -1} and not np.array_equal(codes, q)
        assert same_bytes(h2[1:], h[1:])                              # h + (+-0) = h ...
        assert bits_of(h2[0]) == bits_of(np.float32(-0.0) + np.float32(scale) * np.float32(codes[0]))  # ... IEEE
    else:
        assert np.isnan(scale) and np.isnan(h2).all()                 # the whole hidden tensor becomes NaN
