"""GPU: the executed reference's payloads (tests/golden/receive_flush_small.npz) through the channels' calls — the
first K - 1 updates through ``receive_scaled`` / ``receive_scaled_add_``, the K-th through ``receive_scaled_flush`` /
``FadasMoments.receive_flush`` — reproduce what the reference's own FedBuff(3), FedBuff(1) and FADAS(3) computed from
them, under test_receive_flush_golden.py's rules: FedBuff's params_prime and FADAS's m, v, v_hat bit for bit;
FADAS's params_prime through ``flush_cases.explained_by_sqrt`` on every stored element (and ours equal to the
restatement with the correctly rounded root)."""

import numpy as np
import pytest
import torch

import flush_cases as fc
import receive_flush_cases as rc
import slq_oracle

pytestmark = pytest.mark.gpu

from adfl_amd import FadasMoments  # noqa: E402
from adfl_amd.Channel import CNATChannel, PackedSLQChannel, QSGDChannel, RQSGDChannel, SLQChannel  # noqa: E402
from adfl_amd.model import QuantParameter, QuantParameters  # noqa: E402

DEVICES = ["cuda", "cpu"]
CHANNELS = {"slq8": (lambda: SLQChannel(8), "slq_b8"), "slq4": (lambda: SLQChannel(4), "slq_b4"),
            "packed4": (lambda: PackedSLQChannel(4), "slq_b4"), "qsgd8": (lambda: QSGDChannel(8), "qsgd_b8"),
            "rqsgd8": (lambda: RQSGDChannel(8), "rqsgd_b8"), "cnat8": (lambda: CNATChannel(8), "cnat_b8")}


def golden_payload(name, j):
    """Update j of the channel's run as the channel's own payload objects (fresh tensors on every call)."""
    run = CHANNELS[name][1]
    z, m = rc.fixture()
    rec, bits = m["runs"][run]["payloads"][j], m["runs"][run]["bits"]
    unused = torch.zeros(1, dtype=torch.uint8)
    upd = rc.update(j)
    out = {}
    for n in m["order"]:
        if n not in rc.CODED:
            t = torch.from_numpy(np.array(upd[n]))
            out[n] = QuantParameter(t, bits, 1, unused, t.shape, t.dtype, t.dtype)
            continue
        q = z[f"{run}__u{j}__q__{n}"]
        shape = torch.Size(q.shape)
        if name == "packed4":
            data = torch.from_numpy(slq_oracle.np_pack_int4(q)).view(torch.int8)
            out[n] = QuantParameter(data, bits, float(np.float32(rc.slq_scale(rec["scale"][n]))), unused, shape,
                                    torch.float32, torch.int8)
        elif run.startswith("slq"):
            scale = rc.slq_scale(rec["scale"][n])
            data = torch._make_per_tensor_quantized_tensor(torch.from_numpy(q.copy()), scale, 0)
            out[n] = QuantParameter(data, bits, scale, unused, shape, torch.float32, torch.qint8)
        else:
            data = torch.from_numpy(q.copy())
            if rec["q_dtype"][n] == "int8":
                data = data.view(torch.int8)
            signs = torch.from_numpy(z[f"{run}__u{j}__signs__{n}"].copy())
            s2 = rec["scale_2"][n]
            out[n] = QuantParameter(data, bits, float(rc.f32_of_bits(rec["scale"][n])), signs, shape, torch.float32,
                                    data.dtype, s2["int"] if "int" in s2 else float(rc.f32_of_bits(s2)))
    return QuantParameters(out, 0)


def _digests(params):
    return {n: fc.digest(t.detach().cpu().numpy()) for n, t in params.items()}


def _on(device, d):
    return {n: torch.from_numpy(np.array(a)).to(device) for n, a in d.items()}


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("name", list(CHANNELS))
def test_fedbuff_reproduces_the_reference(name, device):
    ch, run = CHANNELS[name][0](), CHANNELS[name][1]
    z, man = rc.fixture()
    g = _on(device, rc.fedbuff_g())
    fs = [fc.staleness_factor(s) for s in rc.FEDBUFF_STALENESS]
    js = rc.FEDBUFF_UPDATES
    buf = {n: t.to(device) for n, t in ch.receive_scaled(golden_payload(name, js[0]), fs[0])[0].items()}
    for j, f in zip(js[1:-1], fs[1:-1]):
        ch.receive_scaled_add_(golden_payload(name, j), [buf], f)
    got, _ = ch.receive_scaled_flush(golden_payload(name, js[-1]), buf, g, fs[-1], rc.K, rc.LR)
    assert _digests(got) == man["runs"][run]["fedbuff"]["params_prime"], (name, device)
    assert all(t.device.type == device for t in got.values())
    # FedBuff(1): no buffer
    for empty in (None, {}):
        got, _ = ch.receive_scaled_flush(golden_payload(name, rc.FEDBUFF1_UPDATE), empty, g,
                                         fc.staleness_factor(rc.FEDBUFF1_STALENESS), 1, rc.LR)
        assert _digests(got) == man["runs"][run]["fedbuff1"]["params_prime"], (name, device, "K = 1")


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("name", list(CHANNELS))
def test_fadas_reproduces_the_reference(name, device):
    ch, run = CHANNELS[name][0](), CHANNELS[name][1]
    z, man = rc.fixture()
    mom = FadasMoments(fc.BETA_1, fc.BETA_2, fc.EPS)
    before = {n: (np.zeros(s, np.float32),) * 3 for n, s, _ in fc.DICT_SHAPES if n in fc.FLOAT_NAMES}
    for r, (js, stale) in enumerate(zip(rc.FADAS_UPDATES, rc.FADAS_STALENESS)):
        rec = man["runs"][run]["fadas"][r]
        g_np = rc.fadas_g(r)
        g = _on(device, g_np)
        lr_t = fc.delay_lr(rc.LR, max(stale))
        assert lr_t == float.fromhex(rec["lr_t"])
        # fadas.py:60-63 as INTEGRATION.md writes it: to_float=True leaves the non-fp32 entries alone
        buf = {n: t.to(device) for n, t in ch.receive_scaled(golden_payload(name, js[0]), 1.0)[0].items()}
        for j in js[1:-1]:
            keep = {k: t.clone() for k, t in buf.items() if t.dtype != torch.float32}
            ch.receive_scaled_add_(golden_payload(name, j), [buf], 1.0)
            buf.update(keep)
        got = mom.receive_flush(ch, golden_payload(name, js[-1]), buf, g, rc.K, lr_t, r + 1, keep_non_fp32=True)
        assert list(got) == rc.ORDER
        for which in ("m", "v", "v_hat"):                      # the counter included: its moments are the reference's
            assert _digests(getattr(mom, which)) == rec[which], (name, device, r, which)
        assert {n: str(t.dtype) for n, t in got.items()} == rec["dtypes"]
        sc = fc.fadas_scalars(fc.BETA_1, fc.BETA_2, fc.EPS, lr_t, r + 1)
        decs = [rc.decoded(run, j) for j in js]
        for n in fc.FLOAT_NAMES:
            full = fc.fadas_buffer([d[n] for d in decs])
            ours = got[n].detach().cpu().numpy()
            want = fc.fadas_flush(full, g_np[n], *before[n], rc.K, sc)
            assert fc.same_bits(ours, want["out"]).all(), (name, device, r, n)
            key = f"{run}__fadas_r{r}__params_prime__{n}"
            if key in z.files:
                assert fc.explained_by_sqrt(z[key], full, g_np[n], *before[n], rc.K, sc).all(), (name, device, r, n)
                # ... and ours is one of the values that criterion allows the reference
                assert fc.explained_by_sqrt(ours, full, g_np[n], *before[n], rc.K, sc).all()
            before[n] = (want["m"], want["v"], want["v_hat"])
