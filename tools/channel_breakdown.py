"""Per-phase wall time of SLQChannel's host-to-host path on the C3 dict (256 weights + 256 biases, CPU
tensors): where the milliseconds of on_client_send / on_server_receive go. Each phase is synchronised
separately, so the phases add up to more than the real (overlapped) call. Phases follow the current code
(Channel/_staging.py: _stage_in / _stage_out over the native copy pool, csrc/host_copy.cpp).

    python tools/channel_breakdown.py
"""
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "ad-federatedlearning_amd"))
from adfl_amd import hostcopy, ops  # noqa: E402
from adfl_amd.Channel import SLQChannel  # noqa: E402
from adfl_amd.Channel._staging import _int8_view, _stage_out, _staging  # noqa: E402


def main():
    base, rem = divmod(11_689_512, 256)
    params = {}
    for i in range(256):
        params[f"layer{i}.weight"] = torch.randn(1, base + (1 if i < rem else 0)) * 1e-3
        params[f"layer{i}.bias"] = torch.randn(64)
    names = [n for n, p in params.items() if p.ndim > 1]
    tensors = [params[n] for n in names]
    ch = SLQChannel(8)
    for _ in range(3):
        qp, _ = ch.on_client_send(params)
        ch.on_server_receive(qp)
    st = _staging()
    dev = st.device
    lay = st.layout(tuple(int(t.numel()) for t in tensors))
    offs = lay.offsets.tolist()
    res = {"host_copy_threads": hostcopy.threads(), "torch_threads": torch.get_num_threads(),
           "bucket_MB": round(lay.total * 4 / 1e6, 1)}

    def t(name, fn, reps=10):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        res[name] = round((time.perf_counter() - t0) / reps * 1e3, 3)

    host = st.buf("x_host", lay.total, torch.float32, pinned=True)
    devb = st.buf("x", lay.total, torch.float32)
    q = st.buf("q", lay.total, torch.int8)
    t("encode.native_gather_into_pinned", lambda: hostcopy.gather(tensors, host, offs))
    t("encode.h2d", lambda: devb.copy_(host, non_blocking=True))
    t("encode.kernels", lambda: ops.encode_batched(devb, lay, 8, q=q))
    t("encode.alloc_qint8_outputs", lambda: [torch._empty_affine_quantized(tt.shape, scale=0.01, zero_point=0,
                                                                           dtype=torch.qint8) for tt in tensors])
    qs = [torch._empty_affine_quantized(tt.shape, scale=0.01, zero_point=0, dtype=torch.qint8) for tt in tensors]
    t("encode.d2h_plus_scatter_reused_outputs", lambda: _stage_out(q, lay, st, "q", qs))
    t("encode.d2h_plus_scatter_fresh_outputs", lambda: _stage_out(
        q, lay, st, "q", [torch._empty_affine_quantized(tt.shape, scale=0.01, zero_point=0, dtype=torch.qint8)
                          for tt in tensors]))
    t("encode.total_on_client_send", lambda: ch.on_client_send(params))
    items = [(n, qp.params[n].data) for n in names]
    views = [_int8_view(x) for _, x in items]
    dq_host = st.buf("dq_host", lay.total, torch.int8, pinned=True)
    t("decode.native_gather_into_pinned", lambda: hostcopy.gather([x for _, x in items], dq_host, offs))
    dq = st.buf("dq", lay.total, torch.int8)
    t("decode.h2d_payload", lambda: dq.copy_(dq_host, non_blocking=True))
    s = torch.full((lay.ntensors,), 0.01, device=dev)
    out = torch.empty(lay.total, device=dev)
    t("decode.kernel", lambda: ops.decode_batched(dq, s, lay, out=out))
    oh = st.buf("d_out_host", lay.total, torch.float32, pinned=True)
    t("decode.d2h_out_one_copy", lambda: oh.copy_(out, non_blocking=True))
    t("decode.alloc_fp32_outputs", lambda: [torch.empty(tt.shape) for tt in tensors])
    outs = [torch.empty(tt.shape) for tt in tensors]
    t("decode.scatter_reused_outputs", lambda: hostcopy.scatter(oh, outs, offs))
    t("decode.alloc_plus_scatter_fresh_outputs", lambda: hostcopy.scatter(oh, [torch.empty(tt.shape) for tt in tensors],
                                                                          offs))
    t("decode.d2h_plus_scatter_reused_outputs", lambda: _stage_out(out, lay, st, "d_out", outs))
    t("decode.total_on_server_receive", lambda: ch.on_server_receive(qp))
    del views
    print(json.dumps(res))


if __name__ == "__main__":
    main()
