"""Secondary measurements for BASELINE.json's other configs (one JSON line each).

bench.py measures the headline (C2). This tool measures the rest on the same codec:

  c3        ResNet-18-sized update: 11,689,512 fp32 in 256 tensors, per-tensor scales, bucketed
            (one launch per pass), device-resident; with and without an Infinity-Cache flush
  c5_int4   4 GiB fp32 gradient per GPU (2^30 elements), SLQ bits=4 with pack_4bit layout,
            device-resident round trip (13 B/element algorithmic)
  exchange  one simulated client per GPU: encode -> RCCL all-gather -> fused decode+mean
            (--packed --chunks 8 --elems 1073741824 for C5's int4 pipelined variant). torchrun N>1.
  pcie      the same 1 GiB round trip starting and ending in pinned host memory
            (H2D 4N, D2H N, H2D N, D2H 4N), the rate DESIGN.md reports next to the device-resident one
  stoch     QSGD / RQSGD / CNAT (bits=8) device-resident encode + decode on the C2 tensor (2^28 fp32) and on
            the C3 bucket, in-kernel Philox uniforms; algorithmic bytes: QSGD/RQSGD encode 10N (norm pass
            4N + quantize 4N read, 2N levels+signs write), CNAT encode 6N (one pass), every decode 6N;
            plus the reference's ATen op sequence timed on a 2^22-element host sample
  delta     the send side of a DELTA round on a C3-shaped dict pair (256 x 45,662 fp32 weights + 256 biases):
            SLQChannel.send_delta(prev, new) against on_client_send(diff_parameters(prev, new)) with the
            difference taken by torch on the device, in one process, Infinity Cache flushed before every call;
            the delta encode alone against torch._foreach_sub + gather + encode_batched alone (HIP events);
            the same for a log-uniform layout (the two-pass form) and, wall time only, for CPU dicts
  delta_stoch  the same protocol for QSGDChannel / RQSGDChannel / CNATChannel(8).send_delta, and in HIP events the
            two-source RQSGD encode and bucket_diff against torch._foreach_sub + gather (+ rqsgd_encode_batched)
  apply     the asynchronous server's update step (FedAsync's coefficients at staleness 1), SLQChannel(8), on the C3
            dict and on one 2^28-element tensor: the fused decode + axpby over a device-resident base against the
            decode launch followed by torch's alpha * g + beta * d on the device (HIP events, Infinity Cache
            flushed); and host to host, receive_axpby against on_server_receive + the reference's CPU
            add_parameters (wall). A parity flag per leg; no threshold
  flush     the buffered servers' flush on a C3-shaped device dict (256 x 45,662 weights + 256 biases) and on one
            2^28-element tensor: flush.fedbuff_flush_batched / fadas_flush_batched (one launch) against the
            reference's statements run by torch on the same device tensors in the same process (FedBuff 4 launches
            per tensor, FADAS 10); HIP events, Infinity Cache read-flushed before every call, medians of --steps
            calls, three repeats; parity against the numpy restatement (tests/flush_cases.py); no threshold
  broadcast_stoch  QAFeL's broadcast through the stochastic channels on the C3 layouts and one 2^28-element tensor
            (the protocol of `broadcast`): per codec broadcast_delta_ against send_delta + receive_add_ (wall), and in
            HIP events each fused kernel against the kernels it replaces over planes that stay on the device
  packed_stoch  the packed QSGD wire format (bits + 1 bits per weight) against the unpacked channel and kernels in
            one process, at 8 and 4 bits, on the C3-shaped dict and one 2^26-element tensor: device-resident
            quantize, decode and decode + axpby (HIP events, Infinity Cache flushed, medians of --steps calls) and
            the host-to-host encode + decode round trip (wall); a parity flag per leg
  receive_add  receive_add_ into a device-resident model from a CPU payload, per channel (SLQ 8, PackedSLQ 4, QSGD 8,
            RQSGD 8, CNAT 8, PackedQSGD 8; wall), and ops.dequantize_add_batched alone into K = 1 and 4 models (HIP
            events), on the C3-shaped dict and one 2^26-element tensor; public calls only, so a worktree of the
            parent commit runs the same file and --baseline <its JSON line> judges every leg against it

    python tools/bench_configs.py --mode c3
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 tools/bench_configs.py --mode exchange
"""

import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "ad-federatedlearning_amd"))

from bench import GIB, HBM_PEAK_GBS, barrier, dist_setup, free_port, max_over_ranks, maybe_launch  # noqa: E402

RESNET18 = 11_689_512


def events(k):
    return [[torch.cuda.Event(enable_timing=True) for _ in range(k)] for _ in range(2)]


def timed(step, steps, warmup, world, nev):
    """Run `step(ev)` (ev: list of nev events to record, or None) warmup+steps times; return
    (max-over-ranks wall seconds for `steps`, per-step event lists)."""
    for _ in range(warmup):
        step(None)
    torch.cuda.synchronize()
    evs = [[torch.cuda.Event(enable_timing=True) for _ in range(nev)] for _ in range(steps)]
    barrier(world)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(steps):
        step(evs[k])
    torch.cuda.synchronize()
    barrier(world)
    return max_over_ranks(time.perf_counter() - t0, world), evs


def seg_ms(evs, i, j):
    return sum(e[i].elapsed_time(e[j]) for e in evs) / len(evs)


def c3_round_trip(lay, packed, args, world, rank, dev, lib, sh, junk, mode="auto"):
    """Device-resident encode + decode of one bucket (per-tensor scales), Infinity Cache warm and
    flushed. packed: the int4 nibble layout (PackedSLQChannel's kernels, 13 B/element). mode: the int8
    encode as ops.encode_batched picks it ("auto": resident when every tensor fits a block, else the
    two passes) or forced ("twopass")."""
    from adfl_amd import _lib
    g = torch.Generator(device=dev).manual_seed(rank)
    x = torch.randn(lay.total, device=dev, generator=g) * 1e-3
    q = torch.empty(lay.total // 2 if packed else lay.total, dtype=torch.int8, device=dev)
    scales = torch.empty(lay.ntensors, device=dev)
    partials = torch.empty(lay.nchunks, dtype=torch.int32, device=dev)
    out = torch.empty(lay.total, device=dev)
    chunks = lay.device_chunks(dev)
    work = lay.device_work(dev)
    bits = 4 if packed else 8
    n = int(lay.sizes.sum())
    nwork = 0 if mode == "twopass" else lay.nwork

    def enc():
        if packed:
            _lib.check(lib.adfl_slq_encode_batched_int4_work(x.data_ptr(), chunks.data_ptr(), lay.nchunks,
                                                             work.data_ptr(), lay.nwork, bits, q.data_ptr(),
                                                             scales.data_ptr(), partials.data_ptr(), sh))
        else:  # resident one-launch encode when every tensor fits a block (nwork > 0), else the two passes
            _lib.check(lib.adfl_slq_encode_batched_work(x.data_ptr(), chunks.data_ptr(), lay.nchunks, work.data_ptr(),
                                                        nwork, bits, q.data_ptr(), scales.data_ptr(),
                                                        partials.data_ptr(), sh))

    dec_fn = lib.adfl_slq_dequantize_batched_int4 if packed else lib.adfl_slq_dequantize_batched

    def dec():
        _lib.check(dec_fn(q.data_ptr(), chunks.data_ptr(), lay.nchunks, scales.data_ptr(), out.data_ptr(), sh))

    res = {"encode": "resident" if nwork else "twopass", "encode_launches": 1 if nwork else 2}
    resident = bool(lay.nwork if packed else nwork)
    # bytes per element the kernels that ran must move: the one-launch encode reads x
    # once (int8: 4 + 1, int4: 4 + 0.5), the two passes twice; decode 1 + 4 (int4: 0.5 + 4)
    enc_moved = (4.5 if packed else 5.0) if resident else (8.5 if packed else 9.0)
    dec_moved = 4.5 if packed else 5.0
    for flush in (False, True):
        def flush_cache():
            if flush:
                junk.amax()  # READS 512 MiB: the Infinity Cache (256 MiB) holds clean junk lines, nothing of
                             # the codec's buffers, and no dirty lines drain during the timed region

        def step_rt(ev):  # the round trip as one span: no event between the launches
            flush_cache()
            if ev is not None:
                ev[0].record()
            enc()
            dec()
            if ev is not None:
                ev[1].record()

        def step_split(ev):  # encode and decode apart (an event between them perturbs the span)
            flush_cache()
            if ev is not None:
                ev[0].record()
            enc()
            if ev is not None:
                ev[1].record()
            dec()
            if ev is not None:
                ev[2].record()
        _, evs = timed(step_rt, args.steps, args.warmup, world, 2)
        rt = seg_ms(evs, 0, 1)
        _, evs = timed(step_split, args.steps, args.warmup, world, 3)
        e, d = seg_ms(evs, 0, 1), seg_ms(evs, 1, 2)
        res["flushed" if flush else "cache_resident"] = {
            "round_trip_ms": round(rt, 4), "GiB_per_s": round(n * 4 / GIB / (rt * 1e-3), 1),
            "hbm_frac": round((13 if packed else 14) * n / (rt * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
            "hbm_frac_moved": round((enc_moved + dec_moved) * n / (rt * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
            "encode_frac_moved": round(enc_moved * n / (e * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
            "encode_ms": round(e, 4), "decode_ms": round(d, 4), "split_round_trip_ms": round(e + d, 4)}
    return res


def mode_c3(args, world, rank, dev):
    """C3: ResNet-18's 11,689,512 parameters in 256 tensors. The headline layout is equal sizes; the
    log-uniform layout (sizes drawn in [64, 2.4 M] and scaled to the total: 64 .. 350,191 elements,
    tests/golden/recipes.py) and the packed int4 variant are
    reported beside it."""
    sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
    import recipes
    from adfl_amd import _lib, ops
    lib = _lib.load()
    sh = torch.cuda.current_stream(dev).cuda_stream
    junk = torch.zeros(128 << 20, dtype=torch.float32, device=dev)
    lay = ops.BucketLayout(recipes.bucket_sizes("equal"))
    res = c3_round_trip(lay, False, args, world, rank, dev, lib, sh, junk)
    lay_log = ops.BucketLayout(recipes.bucket_sizes("loguniform", 0))
    return {"metric": "C3 bucketed round trip, 11,689,512 fp32 in 256 tensors (per-tensor scales)", "unit": "GiB/s",
            "value": res["flushed"]["GiB_per_s"], "chunks": lay.nchunks, **res,
            "loguniform_layout": {"chunks": lay_log.nchunks,
                                  **c3_round_trip(lay_log, False, args, world, rank, dev, lib, sh, junk)},
            "int4_packed": c3_round_trip(lay, True, args, world, rank, dev, lib, sh, junk)}


def mode_c5_int4(args, world, rank, dev):
    from adfl_amd import _lib, ops
    lib = _lib.load()
    sh = torch.cuda.current_stream(dev).cuda_stream
    n = args.elems or (1 << 30)
    g = torch.Generator(device=dev).manual_seed(rank)
    x = torch.randn(n, device=dev, generator=g) * 1e-3
    packed = torch.empty((n + 1) // 2, dtype=torch.uint8, device=dev)
    scale = torch.empty(1, device=dev)
    ws = ops.new_workspace(dev)
    out = torch.empty(n, device=dev)

    def step(ev):
        if ev is not None:
            ev[0].record()
        _lib.check(lib.adfl_slq_absmax(x.data_ptr(), n, ws.data_ptr(), ws.numel(), sh))
        if ev is not None:
            ev[1].record()
        _lib.check(lib.adfl_slq_quantize_int4(x.data_ptr(), n, 4, ws.data_ptr(), packed.data_ptr(),
                                              scale.data_ptr(), sh))
        if ev is not None:
            ev[2].record()
        _lib.check(lib.adfl_slq_dequantize_int4(packed.data_ptr(), n, scale.data_ptr(), out.data_ptr(), sh))
        if ev is not None:
            ev[3].record()
    elapsed, evs = timed(step, args.steps, args.warmup, world, 4)
    ms = {k: round(seg_ms(evs, i, i + 1), 4) for i, k in enumerate(("absmax", "quantize_int4", "dequantize_int4"))}
    t = elapsed / args.steps
    return {"metric": "C5 int4 device-resident round trip, 4 GiB fp32 per GPU", "unit": "GiB/s",
            "value": round(world * n * 4 / GIB / t, 2), "n_gpus": world, "ms_per_step": round(t * 1e3, 4),
            "kernels_ms": ms, "hbm_frac": round(13 * n / (sum(ms.values()) * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}


def mode_exchange(args, world, rank, dev):
    from adfl_amd.exchange import PeerExchange
    import torch.distributed as dist
    if world == 1 and not dist.is_initialized():
        dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{free_port()}", rank=0, world_size=1,
                                device_id=dev)
    bits = 4 if args.packed else 8
    layout = None
    if args.layout != "flat":   # a whole C3 state dict per client, SLQChannel's per-tensor scales
        sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
        import recipes
        from adfl_amd import ops
        name = args.layout.split("_", 1)[1]
        layout = ops.BucketLayout(recipes.bucket_sizes(name) if name == "equal" else recipes.bucket_sizes(name, 0))
        n = layout.total
    else:
        n = args.elems or (1 << 28)
    ex = PeerExchange(n, bits=bits, packed=args.packed, chunks=args.chunks, device=dev, layout=layout,
                      side_stream=False if args.serial else None)
    g = torch.Generator(device=dev).manual_seed(rank)
    x = torch.randn(n, device=dev, generator=g) * 1e-3
    out = torch.empty(n, device=dev)

    if args.graph:   # the whole step captured once (PeerExchange.graph), replayed with one host call
        gx = ex.graph(x, out)

        def step(ev):
            gx.replay()
    else:
        def step(ev):
            ex.exchange_mean(x, out)
    elapsed, _ = timed(step, args.steps, args.warmup, world, 1)
    t = elapsed / args.steps
    moved = ex.bytes_per_rank * (world - 1)  # bytes each rank receives over xGMI
    what = (f"bucketed {args.layout} state dict, per-tensor scales, bits={bits}{' packed' if args.packed else ''}"
            if layout is not None else
            f"bits={bits}{' packed' if args.packed else ''}, chunks={args.chunks}"
            f"{', side stream' if ex.side_stream else ', in order'}") + (", HIP graph replay" if args.graph else "")
    return {"metric": f"peer exchange: SLQ encode + RCCL all-gather + fused decode-mean, {what}", "unit": "GiB/s",
            "value": round(world * n * 4 / GIB / t, 2), "n_gpus": world, "ms_per_step": round(t * 1e3, 4),
            "elements_per_rank": n, "bytes_per_rank_on_wire": ex.bytes_per_rank,
            "allgather_algbw_GBs": round(moved / t / 1e9, 1) if world > 1 else None}


def mode_pcie(args, world, rank, dev):
    from adfl_amd import _lib, ops
    lib = _lib.load()
    sh = torch.cuda.current_stream(dev).cuda_stream
    n = args.elems or (1 << 28)
    x_h = (torch.randn(n) * 1e-3).pin_memory()
    q_h = torch.empty(n, dtype=torch.int8).pin_memory()
    out_h = torch.empty(n).pin_memory()
    s_h = torch.empty(1).pin_memory()
    x = torch.empty(n, device=dev)
    q = torch.empty(n, dtype=torch.int8, device=dev)
    q2 = torch.empty(n, dtype=torch.int8, device=dev)
    s = torch.empty(1, device=dev)
    out = torch.empty(n, device=dev)
    ws = ops.new_workspace(dev)

    def step(ev):
        if ev is not None:
            ev[0].record()
        x.copy_(x_h, non_blocking=True)
        if ev is not None:
            ev[1].record()
        _lib.check(lib.adfl_slq_encode(x.data_ptr(), n, 8, q.data_ptr(), s.data_ptr(), ws.data_ptr(), ws.numel(), sh))
        if ev is not None:
            ev[2].record()
        q_h.copy_(q, non_blocking=True)
        s_h.copy_(s, non_blocking=True)
        q2.copy_(q_h, non_blocking=True)   # the payload comes back over the host "wire"
        if ev is not None:
            ev[3].record()
        _lib.check(lib.adfl_slq_dequantize(q2.data_ptr(), n, s.data_ptr(), out.data_ptr(), sh))
        if ev is not None:
            ev[4].record()
        out_h.copy_(out, non_blocking=True)
        if ev is not None:
            ev[5].record()
    elapsed, evs = timed(step, args.steps, args.warmup, world, 6)
    t = elapsed / args.steps
    segs = {k: round(seg_ms(evs, i, i + 1), 4) for i, k in
            enumerate(("h2d_x", "encode", "d2h_h2d_payload", "decode", "d2h_out"))}
    pcie_ms = segs["h2d_x"] + segs["d2h_h2d_payload"] + segs["d2h_out"]
    stream = _pcie_stream(lib, n, x_h, dev, args)
    del x, q, q2, out, x_h, q_h, out_h
    # The same 1 GiB as ADFL hands it over: a pageable CPU state dict through SLQChannel (host to host). The
    # channel stages in element ranges (gather || H2D, D2H || scatter) and allocates its outputs while the
    # D2H runs (Channel/quant.py); encode returns an owned qint8 tensor, decode an owned fp32 tensor.
    from adfl_amd.Channel import SLQChannel
    ch = SLQChannel(8)
    params = {"w": (torch.randn(n) * 1e-3).view(-1, 1024)}
    enc_t, dec_t = [], []
    for k in range(args.warmup + min(args.steps, 10)):
        t0 = time.perf_counter()
        qp, _ = ch.on_client_send(params)
        t1 = time.perf_counter()
        ch.on_server_receive(qp)
        t2 = time.perf_counter()
        if k >= args.warmup:
            enc_t.append(t1 - t0)
            dec_t.append(t2 - t1)
    enc_ms, dec_ms = min(enc_t) * 1e3, min(dec_t) * 1e3
    return {"metric": "PCIe-inclusive SLQ round trip, 1 GiB fp32 from and to pinned host memory", "unit": "GiB/s",
            "value": round(n * 4 / GIB / t, 2), "ms_per_step": round(t * 1e3, 4), "segments_ms": segs,
            "pcie_GBs": round(10 * n / (pcie_ms * 1e-3) / 1e9, 1),
            "stream_of_updates": stream,
            "channel_pageable_dict": {"encode_ms": round(enc_ms, 3), "decode_ms": round(dec_ms, 3),
                                      "round_trip_GiB_per_s": round(n * 4 / GIB / ((enc_ms + dec_ms) * 1e-3), 2),
                                      "best_of": len(enc_t)}}


def _pcie_stream(lib, n, x_h, dev, args, updates: int = 8):
    """The same host-to-host round trip for a STREAM of 1 GiB updates (what a server decoding update after
    update sees): three copy streams and one compute stream ordered only by events, device and pinned
    buffers double-buffered. PCIe is full duplex, so update i+1's
    H2D of x runs under update i's D2H of the output; per update each direction carries 5N bytes."""
    from adfl_amd import _lib, ops
    # four streams (the box runs 4 hardware queues per process; more streams would share them): x in, the
    # payload's hop out and back in (sequential by nature), output out, compute
    streams = {k: torch.cuda.Stream(dev) for k in ("x_in", "q_path", "o_out", "comp")}
    streams["q_out"] = streams["q_in"] = streams["q_path"]
    xs = [torch.empty(n, device=dev) for _ in range(2)]
    qs = [torch.empty(n, dtype=torch.int8, device=dev) for _ in range(2)]
    q2s = [torch.empty(n, dtype=torch.int8, device=dev) for _ in range(2)]
    outs = [torch.empty(n, device=dev) for _ in range(2)]
    ss = [torch.empty(1, device=dev) for _ in range(2)]
    wss = [ops.new_workspace(dev) for _ in range(2)]
    q_hs = [torch.empty(n, dtype=torch.int8).pin_memory() for _ in range(2)]
    o_hs = [torch.empty(n).pin_memory() for _ in range(2)]
    ev = lambda: torch.cuda.Event()  # noqa: E731
    last = {}  # per buffer slot: events of the previous use, so a slot is reused only when free

    def issue(i):
        b = i % 2
        e_x, e_enc, e_qo, e_qi, e_dec, e_oo = ev(), ev(), ev(), ev(), ev(), ev()
        prev = last.get(b)
        with torch.cuda.stream(streams["x_in"]):
            if prev:
                streams["x_in"].wait_event(prev["enc"])          # x[b] free once its encode has read it
            xs[b].copy_(x_h, non_blocking=True)
            e_x.record()
        with torch.cuda.stream(streams["comp"]):
            streams["comp"].wait_event(e_x)
            if prev:
                streams["comp"].wait_event(prev["qo"])           # q[b] free once sent
            _lib.check(lib.adfl_slq_encode(xs[b].data_ptr(), n, 8, qs[b].data_ptr(), ss[b].data_ptr(),
                                           wss[b].data_ptr(), wss[b].numel(), streams["comp"].cuda_stream))
            e_enc.record()
        with torch.cuda.stream(streams["q_out"]):
            streams["q_out"].wait_event(e_enc)
            if prev:
                streams["q_out"].wait_event(prev["qi"])          # q_h[b] free once received
            q_hs[b].copy_(qs[b], non_blocking=True)
            e_qo.record()
        with torch.cuda.stream(streams["q_in"]):
            streams["q_in"].wait_event(e_qo)
            if prev:
                streams["q_in"].wait_event(prev["dec"])          # q2[b] free once decoded
            q2s[b].copy_(q_hs[b], non_blocking=True)
            e_qi.record()
        with torch.cuda.stream(streams["comp"]):
            streams["comp"].wait_event(e_qi)
            if prev:
                streams["comp"].wait_event(prev["oo"])           # out[b] free once sent
            _lib.check(lib.adfl_slq_dequantize(q2s[b].data_ptr(), n, ss[b].data_ptr(), outs[b].data_ptr(),
                                               streams["comp"].cuda_stream))
            e_dec.record()
        with torch.cuda.stream(streams["o_out"]):
            streams["o_out"].wait_event(e_dec)
            o_hs[b].copy_(outs[b], non_blocking=True)
            e_oo.record()
        last[b] = {"enc": e_enc, "qo": e_qo, "qi": e_qi, "dec": e_dec, "oo": e_oo}

    for i in range(2):  # warmup
        issue(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(updates):
        issue(i)
    torch.cuda.synchronize()
    t = (time.perf_counter() - t0) / updates
    ok = bool(torch.equal(o_hs[(updates - 1) % 2], o_hs[(updates - 2) % 2]))  # same input, same output
    # the duplex ceiling on this box: 1 GiB H2D and 1 GiB D2H at the same time, alone and together
    def copy_ms(h2d, d2h, reps=3):
        best = 1e9
        for _ in range(reps):
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if h2d:
                with torch.cuda.stream(streams["x_in"]):
                    xs[0].copy_(x_h, non_blocking=True)
            if d2h:
                with torch.cuda.stream(streams["o_out"]):
                    o_hs[0].copy_(outs[0], non_blocking=True)
            torch.cuda.synchronize()
            best = min(best, time.perf_counter() - t1)
        return round(best * 1e3, 3)
    duplex = {"h2d_1GiB_ms": copy_ms(True, False), "d2h_1GiB_ms": copy_ms(False, True),
              "both_at_once_ms": copy_ms(True, True)}
    return {"updates": updates, "ms_per_update": round(t * 1e3, 3), "GiB_per_s": round(n * 4 / GIB / t, 2),
            "pcie_GBs_per_direction": round(5 * n / t / 1e9, 1), "outputs_consistent": ok, "duplex_probe": duplex}


def mode_channel(args, world, rank, dev):
    """ADFL's own call pattern: a CPU state dict through SLQChannel.on_client_send / on_server_receive
    (what Src/ADFL/Client/worker.py:176 and Src/ADFL/Server/async_sc.py:209 do), against the reference's
    per-tensor ATen loop (quant.py:74-112) on the same host and dict."""
    from adfl_amd.Channel import SLQChannel
    base, rem = divmod(RESNET18, 256)
    g = torch.Generator().manual_seed(0)
    params = {}
    for i in range(256):
        params[f"layer{i}.weight"] = torch.randn(1, base + (1 if i < rem else 0), generator=g) * 1e-3
        params[f"layer{i}.bias"] = torch.randn(64, generator=g) * 1e-3
    ch = SLQChannel(bits=8)

    def ours():
        t0 = time.perf_counter()
        qp, _ = ch.on_client_send(params)
        t1 = time.perf_counter()
        d, _ = ch.on_server_receive(qp)
        return t1 - t0, time.perf_counter() - t1, qp, d

    def reference():  # quant.py:74-104 then :67-71,107-112 — the reference's loop, ATen CPU ops
        t0 = time.perf_counter()
        enc = {}
        for name, t in params.items():
            if t.ndim > 1:
                scale = torch.max(torch.abs(t)) / 127
                enc[name] = torch.quantize_per_tensor(t, float(scale), 0, dtype=torch.qint8)
            else:
                enc[name] = t
        t1 = time.perf_counter()
        dec = {name: (q.dequantize() if q.ndim > 1 else q.data) for name, q in enc.items()}
        return t1 - t0, time.perf_counter() - t1, enc, dec

    for _ in range(args.warmup):
        ours()
        reference()
    o = [ours()[:2] for _ in range(args.steps)]
    r = [reference()[:2] for _ in range(max(3, args.steps // 4))]
    _, _, qp, d = ours()
    _, _, enc, dec = reference()
    same = all(torch.equal(qp.params[k].data.int_repr(), enc[k].int_repr()) and torch.equal(d[k], dec[k])
               for k in params if params[k].ndim > 1)
    best = lambda xs, i: min(x[i] for x in xs) * 1e3  # noqa: E731
    gib = sum(t.numel() for t in params.values()) * 4 / GIB

    # synchronous server aggregate of K = 4 client updates (Src/ADFL/Strategy/simple.py:83-89): ours
    # receive_mean (one fused decode-mean launch) vs the reference's K decodes + simple_aggregate
    # (Src/ADFL/model.py:221-234) on the host
    ups = []
    for ci in range(4):
        gr = torch.Generator().manual_seed(10 + ci)
        ups.append(ch.on_client_send({k: torch.randn(v.shape, generator=gr) * 1e-3 for k, v in params.items()})[0])

    def ref_aggregate():
        t0 = time.perf_counter()
        dec = [{k: (p.data.dequantize() if p.data.ndim > 1 else p.data.data) for k, p in u.params.items()}
               for u in ups]
        agg = {k: torch.sum(torch.stack([d[k] for d in dec], dim=0), dim=0) / len(dec) for k in dec[0]}
        return time.perf_counter() - t0, agg

    for _ in range(args.warmup):
        ch.receive_mean(ups)
        ref_aggregate()
    om = min(ch.receive_mean(ups)[1] for _ in range(args.steps))
    rm = min(ref_aggregate()[0] for _ in range(max(3, args.steps // 4)))
    mine, want = ch.receive_mean(ups)[0], ref_aggregate()[1]
    agg_same = all(torch.equal(mine[k], want[k]) for k in want)
    return {"metric": "SLQChannel on a CPU ResNet-18-sized state dict (256 weights + 256 biases), host to host",
            "unit": "ms", "ours_encode_ms": round(best(o, 0), 3), "ours_decode_ms": round(best(o, 1), 3),
            "reference_encode_ms": round(best(r, 0), 3), "reference_decode_ms": round(best(r, 1), 3),
            "ours_GiB_s": round(gib / ((best(o, 0) + best(o, 1)) * 1e-3), 2),
            "reference_GiB_s": round(gib / ((best(r, 0) + best(r, 1)) * 1e-3), 2),
            "reference_threads": torch.get_num_threads(), "identical_output": same,
            "aggregate_k4": {"ours_receive_mean_ms": round(om * 1e3, 3),
                             "reference_decode_simple_aggregate_ms": round(rm * 1e3, 3),
                             "identical_output": agg_same}}


def _ref_stoch_cpu(codec, x, bits=8):
    """The reference's op sequence (quant.py:223-252 / 364-398 / 509-545) on a host tensor, in seconds."""
    s = 2 ** bits - 1
    t0 = time.perf_counter()
    if codec == "cnat":
        norm = torch.linalg.vector_norm(x, ord=2)
        signs = torch.sign(x).to(torch.int8)
        xa = torch.abs(x)
        lg = torch.log2(xa + torch.finfo(x.dtype).eps)
        f, c = torch.floor(lg), torch.ceil(lg)
        prob = (2 ** c - xa) / 2 ** f
        e = torch.where(torch.rand_like(prob) < prob, f, c).clamp_(-128, 127)
        e[x == 0] = -128
        e = e.to(torch.int8)
        t1 = time.perf_counter()
        _ = norm.item() * signs.float() * (2 ** e.float())
    else:
        norm = torch.linalg.vector_norm(x, ord=2 if codec == "qsgd" else float("inf"))
        scaled = s * torch.abs(x) / norm
        lo = torch.floor(scaled)
        q = (lo + (torch.rand_like(scaled) < scaled - lo).float()).to(torch.uint8)
        signs = torch.sign(x).to(torch.int8)
        if codec == "rqsgd":
            mf = torch.linalg.vector_norm(x, ord=-float("inf")).item()
        t1 = time.perf_counter()
        r = norm.item() * signs.float() * q.float() / s
        if codec == "rqsgd":
            z = q == 0
            r[z] = mf * signs[z].float()
    return t1 - t0, time.perf_counter() - t1


def mode_channel_stoch(args, world, rank, dev):
    """The stochastic channels on ADFL's call pattern: the C3 CPU state dict through QSGDChannel /
    RQSGDChannel / CNATChannel(8).on_client_send + on_server_receive, against the reference's per-tensor op
    sequence (quant.py:223-252, 364-398, 509-545; restated in _ref_stoch_cpu) on the same host and dict.
    Outputs are not compared here (the uniforms differ by design; tests/test_gpu_stoch.py pins parity)."""
    from adfl_amd.Channel import CNATChannel, QSGDChannel, RQSGDChannel
    base, rem = divmod(RESNET18, 256)
    g = torch.Generator().manual_seed(0)
    params = {}
    for i in range(256):
        params[f"layer{i}.weight"] = torch.randn(1, base + (1 if i < rem else 0), generator=g) * 1e-3
        params[f"layer{i}.bias"] = torch.randn(64, generator=g) * 1e-3
    weights = [t for t in params.values() if t.ndim > 1]
    gib = sum(t.numel() for t in params.values()) * 4 / GIB
    res = {"metric": "stochastic channels on a CPU ResNet-18-sized state dict (256 weights + 256 biases), host "
                     "to host", "unit": "ms", "reference_threads": torch.get_num_threads()}
    for name, cls in (("qsgd", QSGDChannel), ("rqsgd", RQSGDChannel), ("cnat", CNATChannel)):
        ch = cls(8)

        def ours():
            t0 = time.perf_counter()
            qp, _ = ch.on_client_send(params)
            t1 = time.perf_counter()
            ch.on_server_receive(qp)
            return t1 - t0, time.perf_counter() - t1

        def reference():
            e = d = 0.0
            for t in weights:
                a, b = _ref_stoch_cpu(name, t)
                e += a
                d += b
            return e, d

        for _ in range(args.warmup):
            ours()
        reference()
        o = [ours() for _ in range(args.steps)]
        r = [reference() for _ in range(3)]
        best = lambda xs, i: min(x[i] for x in xs) * 1e3  # noqa: E731
        res[name] = {"ours_encode_ms": round(best(o, 0), 3), "ours_decode_ms": round(best(o, 1), 3),
                     "reference_encode_ms": round(best(r, 0), 3), "reference_decode_ms": round(best(r, 1), 3),
                     "ours_GiB_s": round(gib / ((best(o, 0) + best(o, 1)) * 1e-3), 2),
                     "reference_GiB_s": round(gib / ((best(r, 0) + best(r, 1)) * 1e-3), 3)}
        res[name]["aggregate_k4"] = _stoch_aggregate_k4(name, ch, params, args)
    return res


def _stoch_aggregate_k4(codec, ch, params, args):
    """Synchronous server aggregate of K = 4 updates (Src/ADFL/Strategy/simple.py:83-89): receive_mean (one
    decode-mean launch) against the reference's per-tensor decode ops (quant.py:243-252 / 385-398 / 537-545)
    + simple_aggregate (Src/ADFL/model.py:221-234) on the host, over the same payloads; the output is checked
    against simple_aggregate of the channel's own decodes (bit-identical for K <= 4)."""
    s = float(2 ** ch.bits - 1)
    ups = []
    for ci in range(4):
        gr = torch.Generator().manual_seed(10 + ci)
        ups.append(ch.on_client_send({k: torch.randn(v.shape, generator=gr) * 1e-3 for k, v in params.items()})[0])

    def ref_decode(p):
        if p.data.ndim <= 1:
            return p.data.data
        norm, sf = float(p.scale), p.signs.float()
        if codec == "qsgd":
            return (norm * p.data.float()) / s * sf
        if codec == "rqsgd":
            r = ((norm * sf) * p.data.float()) / s
            z = p.data == 0
            r[z] = float(p.scale_2) * sf[z]
            return r
        return (norm * sf) * (2 ** p.data.float())

    def aggregate(dec):
        return {k: torch.sum(torch.stack([d[k] for d in dec], dim=0), dim=0) / len(dec) for k in dec[0]}

    def ref_aggregate():
        t0 = time.perf_counter()
        agg = aggregate([{k: ref_decode(p) for k, p in u.params.items()} for u in ups])
        return time.perf_counter() - t0, agg

    for _ in range(args.warmup):
        ch.receive_mean(ups)
        ref_aggregate()
    om = min(ch.receive_mean(ups)[1] for _ in range(args.steps))
    rm = min(ref_aggregate()[0] for _ in range(max(3, args.steps // 4)))
    mine = ch.receive_mean(ups)[0]
    want = aggregate([ch.on_server_receive(u)[0] for u in ups])
    return {"ours_receive_mean_ms": round(om * 1e3, 3), "reference_decode_simple_aggregate_ms": round(rm * 1e3, 3),
            "identical_to_own_decodes_aggregated": all(torch.equal(mine[k], want[k]) for k in want)}


def mode_stoch(args, world, rank, dev):
    """Stochastic codecs (QSGD / RQSGD / CNAT, bits = 8, in-kernel Philox) on C2 (one 2^28 tensor) and C3
    (256 tensors: one-launch resident encodes). Each timed span starts behind GPU work (a 512 MiB read that
    flushes the Infinity Cache, or a short spin when warm), so the Python enqueue cost stays off the span.
    encode_frac counts the algorithmic bytes of the multi-launch design (QSGD / RQSGD read x twice:
    10 B/element; CNAT 6), encode_frac_moved the bytes the kernels that ran must move (6 B/element for every
    codec when the resident encode runs)."""
    from adfl_amd import ops, stoch
    n_flat = args.elems or (1 << 28)
    base, rem = divmod(RESNET18, 256)
    workloads = {"c2_flat": [n_flat], "c3_bucket": [base + (1 if i < rem else 0) for i in range(256)]}
    junk = torch.ones(128 << 20, dtype=torch.float32, device=dev)
    res = {}
    for wname, sizes in workloads.items():
        lay = ops.BucketLayout(sizes, align=1)
        g = torch.Generator(device=dev).manual_seed(rank)
        x = torch.randn(lay.total, device=dev, generator=g) * 1e-3
        lv = torch.empty(lay.total, dtype=torch.uint8, device=dev)
        sg = torch.empty(lay.total, dtype=torch.int8, device=dev)
        nr = torch.empty(lay.ntensors, device=dev)
        mn = torch.empty(lay.ntensors, device=dev)
        out = torch.empty(lay.total, device=dev)
        ws = stoch.workspace(lay, dev)
        n = lay.total
        resident = lay.nwork > 0 and os.environ.get("ADFL_STOCH_RESIDENT", "1") != "0"
        for codec in ("qsgd", "rqsgd", "cnat"):
            for flush in (False, True):
                def step(ev, codec=codec, flush=flush):
                    if flush:
                        junk.amax()
                    else:
                        torch.cuda._sleep(100000)   # ~50 us of GPU spin: the host enqueues behind it
                    if ev is not None:
                        ev[0].record()
                    if codec == "qsgd":
                        stoch.qsgd_encode_batched(x, lay, 8, seed=7, counter=0, levels=lv, signs=sg, norms=nr, ws=ws)
                    elif codec == "rqsgd":
                        stoch.rqsgd_encode_batched(x, lay, 8, seed=7, counter=0, levels=lv, signs=sg, norms=nr,
                                                   mins=mn, ws=ws)
                    else:
                        stoch.cnat_encode_batched(x, lay, 8, seed=7, counter=0, exps=lv.view(torch.int8), signs=sg,
                                                  norms=nr, ws=ws)
                    if ev is not None:
                        ev[1].record()
                    if codec == "qsgd":
                        stoch.qsgd_decode_batched(lv, sg, nr, lay, 8, out=out)
                    elif codec == "rqsgd":
                        stoch.rqsgd_decode_batched(lv, sg, nr, mn, lay, 8, out=out)
                    else:
                        stoch.cnat_decode_batched(lv.view(torch.int8), sg, nr, lay, out=out)
                    if ev is not None:
                        ev[2].record()
                wall, evs = timed(step, args.steps, args.warmup, world, 3)
                enc, dec = seg_ms(evs, 0, 1), seg_ms(evs, 1, 2)
                enc_bytes = (6 if codec == "cnat" else 10) * n
                moved = 6 * n if (resident or codec == "cnat") else 10 * n
                res[f"{wname}_{codec}" + ("_flushed" if flush else "")] = {
                    "encode_ms": round(enc, 4), "decode_ms": round(dec, 4),
                    "encode_launches": 1 if resident else 3,
                    "encode_GBs": round(enc_bytes / enc / 1e6, 1), "decode_GBs": round(6 * n / dec / 1e6, 1),
                    "encode_frac": round(enc_bytes / enc / 1e6 / HBM_PEAK_GBS, 3),
                    "encode_frac_moved": round(moved / enc / 1e6 / HBM_PEAK_GBS, 3),
                    "decode_frac": round(6 * n / dec / 1e6 / HBM_PEAK_GBS, 3),
                    "round_trip_GiBs": round(4 * n / GIB / ((enc + dec) / 1e3), 1)}
    # fp16 / bf16 / fp64 C3 buckets (the *_dt kernels: the reference's arithmetic in each dtype), encode only
    # (decode is the fp32 kernels'); flushed
    lay = ops.BucketLayout(workloads["c3_bucket"], align=1)
    for dtype in (torch.float16, torch.bfloat16, torch.float64):
        xd = (torch.randn(lay.total, device=dev) * 1e-3).to(dtype)
        lvd = torch.empty(lay.total, dtype=torch.uint8, device=dev)
        sgd = torch.empty(lay.total, dtype=torch.int8, device=dev)
        wsd = stoch.workspace(lay, dev)
        for codec in ("qsgd", "cnat"):
            def step_dt(ev, codec=codec):
                junk.amax()
                if ev is not None:
                    ev[0].record()
                stoch.encode_batched_dt(codec, xd, lay, 8, seed=7, counter=0,
                                        levels=lvd.view(torch.int8) if codec == "cnat" else lvd, signs=sgd, ws=wsd)
                if ev is not None:
                    ev[1].record()
            _, evs = timed(step_dt, args.steps, args.warmup, world, 2)
            enc = seg_ms(evs, 0, 1)
            # QSGD: x read twice (norm pass, quantize) + 2 planes; CNAT: x once (exponents + partials) + 2 planes
            eb = ((1 if codec == "cnat" else 2) * xd.element_size() + 2) * lay.total
            res[f"c3_bucket_{str(dtype).replace('torch.', '')}_{codec}_flushed"] = {
                "encode_ms": round(enc, 4), "encode_GBs": round(eb / enc / 1e6, 1),
                "encode_frac": round(eb / enc / 1e6 / HBM_PEAK_GBS, 3)}
        del xd, lvd, sgd
    del junk
    # calibration on the same box: the SLQ flat round trip of bench.py's headline kernels
    from adfl_amd import _lib
    lib = _lib.load()
    sh = torch.cuda.current_stream(dev).cuda_stream
    x = torch.randn(n_flat, device=dev) * 1e-3
    q = torch.empty(n_flat, dtype=torch.int8, device=dev)
    sc = torch.empty(1, device=dev)
    wsl = ops.new_workspace(dev)
    outf = torch.empty(n_flat, device=dev)

    def slq_step(ev):
        if ev is not None:
            ev[0].record()
        lib.adfl_slq_encode(x.data_ptr(), n_flat, 8, q.data_ptr(), sc.data_ptr(), wsl.data_ptr(), wsl.numel(), sh)
        if ev is not None:
            ev[1].record()
        lib.adfl_slq_dequantize(q.data_ptr(), n_flat, sc.data_ptr(), outf.data_ptr(), sh)
        if ev is not None:
            ev[2].record()
    _, evs = timed(slq_step, args.steps, args.warmup, world, 3)
    res["c2_flat_slq_calibration"] = {"encode_ms": round(seg_ms(evs, 0, 1), 4), "decode_ms": round(seg_ms(evs, 1, 2), 4)}
    del x, q, outf
    if rank == 0 and not args.no_cpu:
        m = 1 << 22
        xs = torch.randn(m) * 1e-3
        torch.set_num_threads(os.cpu_count() if os.cpu_count() <= 16 else 16)
        for codec in ("qsgd", "rqsgd", "cnat"):
            best = min((_ref_stoch_cpu(codec, xs) for _ in range(3)), key=lambda t: t[0] + t[1])
            res[f"cpu_reference_{codec}"] = {"sample_elems": m, "threads": torch.get_num_threads(),
                                             "encode_ms": round(best[0] * 1e3, 2), "decode_ms": round(best[1] * 1e3, 2),
                                             "round_trip_GiBs": round(4 * m / GIB / (best[0] + best[1]), 3)}
    return {"mode": "stoch", "n_gpus": world, "steps": args.steps, **res}


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def _delta_same(a, b) -> bool:
    """Two QuantParameters equal field for field (the parity flag of the delta leg)."""
    if list(a.params) != list(b.params) or a.size != b.size:
        return False
    for n, p in a.params.items():
        o = b.params[n]
        if (p.bits, tuple(p.shape), p.dtype, p.q_dtype, p.data.dtype, p.data.shape, p.data.device) != \
                (o.bits, tuple(o.shape), o.dtype, o.q_dtype, o.data.dtype, o.data.shape, o.data.device):
            return False
        if p.scale != o.scale and not (p.scale != p.scale and o.scale != o.scale):
            return False
        pd, od = (p.data.int_repr(), o.data.int_repr()) if p.data.is_quantized else (p.data, o.data)
        if not torch.equal(pd, od):
            return False
    return True


def _delta_leg(sizes, args, dev, junk, repeats=5):
    """One layout of the delta leg. Wall medians are per repeat (`repeats` medians of args.steps calls each): the
    fused route counts as faster when its worst repeat beats the unfused route's best by more than nothing, i.e.
    the gap exceeds the unfused route's run-to-run spread (max - min of its medians)."""
    from adfl_amd import _lib, ops
    from adfl_amd.Channel import SLQChannel
    lib = _lib.load()
    sh = torch.cuda.current_stream(dev).cuda_stream
    g = torch.Generator(device=dev).manual_seed(0)
    prev, new = {}, {}
    for i, n in enumerate(sizes):
        for name, shape in ((f"layer{i:03d}.weight", (1, n)), (f"layer{i:03d}.bias", (64,))):
            new[name] = torch.randn(shape, device=dev, generator=g) * 1e-2
            prev[name] = new[name] + torch.randn(shape, device=dev, generator=g) * 1e-5
    ch = SLQChannel(8)

    def fused(a=prev, b=new):
        return ch.send_delta(a, b)[0]

    def unfused(a=prev, b=new):
        with torch.no_grad():
            diff = {k: b[k] - a[k] for k in a}   # diff_parameters (model.py:350-358), torch on the dict's device
        return ch.on_client_send(diff)[0]

    def wall(fn, steps):
        out = []
        for _ in range(steps):
            junk.amax()   # read-flush of the Infinity Cache, as the C3 leg's
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return _median(out)

    parity = _delta_same(fused(), unfused())
    for _ in range(args.warmup):
        fused(), unfused()
    f_ms = [wall(fused, args.steps) for _ in range(repeats)]
    u_ms = [wall(unfused, args.steps) for _ in range(repeats)]
    spread = max(u_ms) - min(u_ms)
    res = {"tensors": len(sizes), "elements": int(sum(sizes)), "parity": parity,
           "send_delta_ms": round(_median(f_ms), 4), "send_delta_ms_repeats": [round(v, 4) for v in f_ms],
           "unfused_ms": round(_median(u_ms), 4), "unfused_ms_repeats": [round(v, 4) for v in u_ms],
           "unfused_spread_ms": round(spread, 4),
           "fused_faster_than_spread": bool(_median(u_ms) - _median(f_ms) > spread)}

    # the kernels alone, HIP events: the delta encode over prebuilt pointer tables against
    # torch._foreach_sub + bucket gather + encode_batched (the difference, the bucket of it, its encode)
    names = [k for k in prev if prev[k].ndim > 1]
    news, prevs = [new[k] for k in names], [prev[k] for k in names]
    lay = ops.BucketLayout(list(sizes))             # 64-aligned payload, as send_delta's device route
    lay_c = ops.BucketLayout(list(sizes), align=1)  # the compact bucket _encode_dict stages a device dict in
    n_tab = torch.tensor([t.data_ptr() for t in news], dtype=torch.int64).to(dev)
    p_tab = torch.tensor([t.data_ptr() for t in prevs], dtype=torch.int64).to(dev)
    q = torch.empty(lay.total, dtype=torch.int8, device=dev)
    x = torch.empty(lay_c.total, dtype=torch.float32, device=dev)
    scales = torch.empty(lay.ntensors, device=dev)
    partials = torch.empty(lay.nchunks, dtype=torch.int32, device=dev)
    nwork = lay.nwork if lay.max_tensor_chunks <= _lib.DELTA_RESIDENT_CHUNKS else 0
    chunks, work = lay.device_chunks(dev), lay.device_work(dev)

    def k_fused(ev):
        junk.amax()
        if ev is not None:
            ev[0].record()
        _lib.check(lib.adfl_slq_encode_delta_batched_work(n_tab.data_ptr(), p_tab.data_ptr(), chunks.data_ptr(),
                                                          lay.nchunks, work.data_ptr(), nwork, 8, q.data_ptr(),
                                                          scales.data_ptr(), partials.data_ptr(), sh))
        if ev is not None:
            ev[1].record()

    def k_unfused(ev):
        junk.amax()
        if ev is not None:
            ev[0].record()
        d = torch._foreach_sub(news, prevs)
        ops.bucket_gather(d, lay_c, x, checked=False)
        ops.encode_batched(x, lay_c, 8, q=q, scales=scales, partials=partials)
        if ev is not None:
            ev[1].record()

    _, evs = timed(k_fused, args.steps, args.warmup, 1, 2)
    kf = _median([e[0].elapsed_time(e[1]) for e in evs])
    _, evs = timed(k_unfused, args.steps, args.warmup, 1, 2)
    ku = _median([e[0].elapsed_time(e[1]) for e in evs])
    n = int(sum(sizes))
    res.update({"encode_form": "resident" if nwork else "twopass",
                "delta_encode_alone_ms": round(kf, 4), "foreach_sub_gather_encode_alone_ms": round(ku, 4),
                # bytes the delta encode must move: read new + prev (twice in the two passes), write the payload
                "delta_encode_frac_moved": round((9 if nwork else 17) * n / (kf * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)})

    # CPU dicts: two H2D copies against a host difference and one H2D (reported, no criterion)
    prev_h, new_h = {k: v.cpu() for k, v in prev.items()}, {k: v.cpu() for k, v in new.items()}
    steps = max(3, min(args.steps, 7))
    res["cpu_dict_parity"] = _delta_same(fused(prev_h, new_h), unfused(prev_h, new_h))
    res["cpu_dict_send_delta_ms"] = round(wall(lambda: fused(prev_h, new_h), steps), 4)
    res["cpu_dict_unfused_ms"] = round(wall(lambda: unfused(prev_h, new_h), steps), 4)
    return res


def mode_delta(args, world, rank, dev):
    """The send side of a DELTA round (FedBuff, FADAS, QAFeL, the simple delta modes): fused against unfused."""
    sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
    import recipes
    junk = torch.zeros(128 << 20, dtype=torch.float32, device=dev)
    eq = _delta_leg(recipes.bucket_sizes("equal"), args, dev, junk)
    log = _delta_leg(recipes.bucket_sizes("loguniform", 0), args, dev, junk)
    return {"mode": "delta", "metric": "send_delta on a C3-shaped device dict pair (256 weights + 256 biases), "
            "Infinity Cache flushed", "unit": "ms", "value": eq["send_delta_ms"], "parity": eq["parity"] and
            log["parity"] and eq["cpu_dict_parity"] and log["cpu_dict_parity"], "steps": args.steps,
            "c3_equal": eq, "c3_loguniform": log}


def _stoch_same(a, b) -> bool:
    """Two stochastic QuantParameters equal field for field (the parity flag of the delta_stoch leg)."""
    def same_scale(x, y):
        if isinstance(x, torch.Tensor) or isinstance(y, torch.Tensor):
            return isinstance(x, torch.Tensor) and isinstance(y, torch.Tensor) and x.dtype == y.dtype and torch.equal(x, y)
        return type(x) is type(y) and (x == y or (x != x and y != y))
    if list(a.params) != list(b.params) or a.size != b.size:
        return False
    for n, p in a.params.items():
        o = b.params[n]
        if (p.bits, tuple(p.shape), p.dtype, p.q_dtype) != (o.bits, tuple(o.shape), o.dtype, o.q_dtype):
            return False
        if not (same_scale(p.scale, o.scale) and same_scale(p.scale_2, o.scale_2)):
            return False
        for x, y in ((p.data, o.data), (p.signs, o.signs)):
            if (x.dtype, x.shape, x.device) != (y.dtype, y.shape, y.device) or not torch.equal(x, y):
                return False
    return True


def _delta_stoch_leg(sizes, args, dev, junk, repeats=5):
    """One layout of the delta_stoch leg, _delta_leg's protocol per stochastic codec: send_delta against
    on_client_send of torch's difference on the device (a route this library has not changed), both under one
    torch.manual_seed for the parity flag; then the kernels alone in HIP events."""
    from adfl_amd import ops, stoch
    from adfl_amd.Channel import CNATChannel, QSGDChannel, RQSGDChannel
    g = torch.Generator(device=dev).manual_seed(0)
    prev, new = {}, {}
    for i, n in enumerate(sizes):
        for name, shape in ((f"layer{i:03d}.weight", (1, n)), (f"layer{i:03d}.bias", (64,))):
            new[name] = torch.randn(shape, device=dev, generator=g) * 1e-2
            prev[name] = new[name] + torch.randn(shape, device=dev, generator=g) * 1e-5
    prev_h, new_h = {k: v.cpu() for k, v in prev.items()}, {k: v.cpu() for k, v in new.items()}

    def wall(fn, steps):
        out = []
        for _ in range(steps):
            junk.amax()   # read-flush of the Infinity Cache
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return _median(out)

    res = {"tensors": len(sizes), "elements": int(sum(sizes))}
    for codec, cls in (("qsgd", QSGDChannel), ("rqsgd", RQSGDChannel), ("cnat", CNATChannel)):
        ch = cls(8)

        def fused(a=prev, b=new):
            return ch.send_delta(a, b)[0]

        def unfused(a=prev, b=new):
            with torch.no_grad():
                diff = {k: b[k] - a[k] for k in a}   # diff_parameters (model.py:350-358), torch on the dict's device
            return ch.on_client_send(diff)[0]

        def seeded(fn, *a):
            torch.manual_seed(1234)
            return fn(*a)

        parity = _stoch_same(seeded(fused), seeded(unfused))
        for _ in range(args.warmup):
            fused(), unfused()
        f_ms = [wall(fused, args.steps) for _ in range(repeats)]
        u_ms = [wall(unfused, args.steps) for _ in range(repeats)]
        spread = max(u_ms) - min(u_ms)
        steps = max(3, min(args.steps, 7))
        res[codec] = {"parity": parity, "send_delta_ms": round(_median(f_ms), 4),
                      "send_delta_ms_repeats": [round(v, 4) for v in f_ms], "unfused_ms": round(_median(u_ms), 4),
                      "unfused_ms_repeats": [round(v, 4) for v in u_ms], "unfused_spread_ms": round(spread, 4),
                      "fused_faster_than_spread": bool(_median(u_ms) - _median(f_ms) > spread),
                      # CPU dicts: two H2D copies against a host difference and one H2D (reported, no criterion)
                      "cpu_dict_parity": _stoch_same(seeded(fused, prev_h, new_h), seeded(unfused, prev_h, new_h)),
                      "cpu_dict_send_delta_ms": round(wall(lambda: fused(prev_h, new_h), steps), 4),
                      "cpu_dict_unfused_ms": round(wall(lambda: unfused(prev_h, new_h), steps), 4)}

    # the kernels alone, HIP events
    names = [k for k in prev if prev[k].ndim > 1]
    news, prevs = [new[k] for k in names], [prev[k] for k in names]
    lay = ops.BucketLayout(list(sizes))             # 64-aligned planes, as send_delta's device route
    lay_c = ops.BucketLayout(list(sizes), align=1)  # the compact bucket of the two-step route
    ptrs = (torch.tensor([t.data_ptr() for t in news], dtype=torch.int64).to(dev),
            torch.tensor([t.data_ptr() for t in prevs], dtype=torch.int64).to(dev))   # prebuilt device tables
    ushift = lay_c.offsets - lay.offsets
    x = torch.empty(lay_c.total, dtype=torch.float32, device=dev)
    bufs = {k: torch.empty(lay.total, dtype=dt, device=dev) for k, dt in (("levels", torch.uint8), ("signs", torch.int8))}
    nm = {k: torch.empty(lay.ntensors, device=dev) for k in ("norms", "mins")}
    ws = stoch.workspace(lay, dev)

    def event_ms(body):
        def run(ev):
            junk.amax()
            if ev is not None:
                ev[0].record()
            body()
            if ev is not None:
                ev[1].record()
        _, evs = timed(run, args.steps, args.warmup, 1, 2)
        return round(_median([e[0].elapsed_time(e[1]) for e in evs]), 4)

    def sub_gather():
        ops.bucket_gather(torch._foreach_sub(news, prevs), lay_c, x, checked=False)

    def two_step_rqsgd():
        sub_gather()
        stoch.rqsgd_encode_batched(x, lay_c, 8, seed=1, **bufs, **nm, ws=ws)

    n = int(sum(sizes))
    phases = (ushift % 4 != 0)
    res["kernels"] = {
        "rqsgd_delta_encode_ms": event_ms(lambda: stoch.rqsgd_encode_delta_batched(
            news, prevs, lay, 8, ptrs=ptrs, ushift=ushift, seed=1, **bufs, **nm, ws=ws)),
        "rqsgd_delta_encode_twopass_ms": event_ms(lambda: stoch.rqsgd_encode_delta_batched(
            news, prevs, lay, 8, ptrs=ptrs, ushift=ushift, seed=1, **bufs, **nm, ws=ws, resident=False)),
        # every tensor on the one-block-per-group path: what the straddling tensors cost
        "rqsgd_delta_encode_ushift0_ms": event_ms(lambda: stoch.rqsgd_encode_delta_batched(
            news, prevs, lay, 8, ptrs=ptrs, seed=1, **bufs, **nm, ws=ws)),
        "rqsgd_foreach_sub_gather_encode_ms": event_ms(two_step_rqsgd),
        "bucket_diff_ms": event_ms(lambda: ops.bucket_diff(news, prevs, lay_c, out=x, ptrs=ptrs)),
        "foreach_sub_gather_ms": event_ms(sub_gather),
        "rqsgd_delta_form": "resident" if lay.nwork else "twopass", "tensors_on_the_straddling_path": int(phases.sum()),
        "rqsgd_delta_frac_moved": None, "bucket_diff_frac_moved": None}
    k = res["kernels"]
    k["rqsgd_delta_frac_moved"] = round((10 if lay.nwork else 18) * n / (k["rqsgd_delta_encode_ms"] * 1e-3) / 1e9
                                        / HBM_PEAK_GBS, 4)
    k["bucket_diff_frac_moved"] = round(12 * n / (k["bucket_diff_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
    return res


def mode_delta_stoch(args, world, rank, dev):
    """The send side of a DELTA round through QSGD / RQSGD / CNAT: send_delta against the two steps."""
    sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
    import recipes
    junk = torch.zeros(128 << 20, dtype=torch.float32, device=dev)
    eq = _delta_stoch_leg(recipes.bucket_sizes("equal"), args, dev, junk)
    log = _delta_stoch_leg(recipes.bucket_sizes("loguniform", 0), args, dev, junk)
    codecs = ("qsgd", "rqsgd", "cnat")
    return {"mode": "delta_stoch", "metric": "QSGDChannel(8).send_delta on a C3-shaped device dict pair (256 weights "
            "+ 256 biases), Infinity Cache flushed", "unit": "ms", "value": eq["qsgd"]["send_delta_ms"],
            "parity": all(leg[c][f] for leg in (eq, log) for c in codecs for f in ("parity", "cpu_dict_parity")),
            "steps": args.steps, "c3_equal": eq, "c3_loguniform": log}


def _bits_equal(a, b) -> bool:
    a, b = a.detach().cpu().reshape(-1), b.detach().cpu().reshape(-1)
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _apply_leg(sizes, args, dev, junk, host_steps):
    """One layout of the apply leg, SLQChannel(8), FedAsync's coefficients at staleness 1.
    device: ops.dequantize_axpby_batched over a device-resident base (new outputs) against the route without it —
            the decode launch, then torch's (alpha * g) + (beta * d) on the device, over the flat bucket (torch's
            best case: three launches, not three per tensor). HIP events, Infinity Cache flushed before each.
    host:   receive_axpby on a CPU base against on_server_receive + the reference's CPU add_parameters, wall."""
    from adfl_amd import ops
    from adfl_amd.Channel import SLQChannel
    alpha_t = 0.6 * 2 ** -0.5
    alpha, beta = 1 - alpha_t, alpha_t
    lay = ops.BucketLayout(list(sizes))
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(lay.total, device=dev, generator=g) * 1e-2
    base = torch.randn(lay.total, device=dev, generator=g)
    q, s = ops.encode_batched(x, lay, 8)
    del x
    out = torch.empty(lay.total, device=dev)
    dec = torch.empty(lay.total, device=dev)

    def k_fused(ev):
        junk.amax()
        if ev is not None:
            ev[0].record()
        ops.dequantize_axpby_batched(q, s, lay, base, out, alpha, beta)
        if ev is not None:
            ev[1].record()

    res2 = []

    def k_two_step(ev):
        junk.amax()
        if ev is not None:
            ev[0].record()
        d = ops.decode_batched(q, s, lay, out=dec)
        r = (alpha * base) + (beta * d)
        if ev is not None:
            ev[1].record()
        res2[:] = [r]

    k_fused(None), k_two_step(None)
    torch.cuda.synchronize()
    own = torch.zeros(lay.total, dtype=torch.bool)
    for o, n in zip(lay.offsets.tolist(), lay.sizes.tolist()):
        own[o:o + n] = True
    own = own.to(dev)
    parity = _bits_equal(out[own], res2[0][own])
    _, evs = timed(k_fused, args.steps, args.warmup, 1, 2)
    kf = _median([e[0].elapsed_time(e[1]) for e in evs])
    _, evs = timed(k_two_step, args.steps, args.warmup, 1, 2)
    ku = _median([e[0].elapsed_time(e[1]) for e in evs])
    n = int(sum(sizes))
    res = {"tensors": len(sizes), "elements": n, "device_parity": parity, "fused_ms": round(kf, 4),
           "decode_then_torch_ms": round(ku, 4), "device_ratio": round(ku / kf, 3),
           # bytes the fused kernel must move: payload 1, base 4, result 4
           "fused_frac_moved": round(9 * n / (kf * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
    del out, dec, res2[:]

    # host to host: ADFL's own pattern (a CPU g_params, a CPU payload, a CPU result)
    ch = SLQChannel(8)
    shapes = [(1, m) for m in sizes]
    upd = {f"layer{i:03d}.weight": (torch.randn(sh) * 1e-2) for i, sh in enumerate(shapes)}
    g_cpu = {k: torch.randn(v.shape) for k, v in upd.items()}
    for i in range(len(sizes) if len(sizes) > 1 else 0):
        upd[f"layer{i:03d}.bias"], g_cpu[f"layer{i:03d}.bias"] = torch.randn(64) * 1e-2, torch.randn(64)
    c, _ = ch.on_client_send(upd)
    del upd

    def fused():
        return ch.receive_axpby(c, g_cpu, alpha, beta)[0]

    def two_step():
        d, _ = ch.on_server_receive(c)
        with torch.no_grad():   # add_parameters (model.py:326-334) on the same box
            return {k: (alpha * g_cpu[k]) + (beta * d[k]) for k in d}

    def wall(fn, steps):
        ts = []
        for _ in range(steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return _median(ts)

    a, b = fused(), two_step()
    res["host_parity"] = list(a) == list(b) and all(_bits_equal(a[k], b[k]) for k in a)
    del a, b
    res["host_receive_axpby_ms"] = round(wall(fused, host_steps), 3)
    res["host_receive_then_add_parameters_ms"] = round(wall(two_step, host_steps), 3)
    res["host_ratio"] = round(res["host_receive_then_add_parameters_ms"] / res["host_receive_axpby_ms"], 3)
    return res


def mode_apply(args, world, rank, dev):
    """The asynchronous server's update step (FedAsync / Simple DELTA / FedBuff): fused decode + axpby against
    decode, then torch. No threshold: both times and their ratio are reported with a parity flag per leg."""
    sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
    import recipes
    junk = torch.zeros(128 << 20, dtype=torch.float32, device=dev)
    c3 = _apply_leg(recipes.bucket_sizes("equal"), args, dev, junk, host_steps=max(3, min(args.steps, 7)))
    big = _apply_leg([args.elems or 1 << 28], args, dev, junk, host_steps=3)
    return {"mode": "apply", "metric": "SLQChannel(8) decode + axpby, device-resident base, C3 dict "
            "(fused kernel, Infinity Cache flushed)", "unit": "ms", "value": c3["fused_ms"],
            "parity": all(leg[f] for leg in (c3, big) for f in ("device_parity", "host_parity")),
            "steps": args.steps, "c3_equal": c3, "one_tensor": big}


def _flush_leg(sizes, args, dev, junk, repeats=3, sample=1 << 20):
    """One dict of the flush leg: `sizes` separately allocated device tensors. Fused: one launch over pointer
    tables. Torch: the reference's statements (fed_buff.py:88-92; fadas.py:69-70,105-106,127-129) per tensor on
    the same device tensors; its in-place `div_` works on a copy of the buffer refreshed before every call, outside
    the timed span. The moments are updated in place by both legs, each on its own copy. Parity: the fused results
    of one call from known moments against tests/flush_cases.py, on every element of a tensor of at most `sample`
    elements and on the first, middle and last `sample` elements of a longer one."""
    import numpy as np

    sys.path.insert(0, os.path.join(REPO, "tests"))
    import flush_cases as fc
    from adfl_amd import flush, ops
    K, lr, rnd = 10, 0.05, 3
    lay = ops.BucketLayout(list(sizes))
    g = torch.Generator(device=dev).manual_seed(0)

    def make(scale, positive=False):
        ts = [torch.randn(n, device=dev, generator=g) * scale for n in sizes]
        return [t.abs_() for t in ts] if positive else ts

    buf, gp = make(1e-2), make(1.0)
    m0, v0 = make(1e-3), make(1e-5, positive=True)
    h0 = [t * 1.5 for t in v0]
    out = [torch.empty_like(t) for t in gp]
    sc = flush.fadas_scalars(0.9, 0.999, 1e-8, lr, rnd)

    def windows(n):
        if n <= sample:
            return [(0, n)]
        return [(0, sample), ((n - sample) // 2, (n - sample) // 2 + sample), (n - sample, n)]

    def host(ts):
        return [[t[a:b].cpu().numpy() for a, b in windows(t.numel())] for t in ts]

    # parity from known moments
    mf, vf, hf = ([t.clone() for t in x] for x in (m0, v0, h0))
    flush.fedbuff_flush_batched(buf, gp, out, lay, K, lr)
    fb = host(out)
    flush.fadas_flush_batched(buf, gp, mf, vf, hf, out, lay, K, sc)
    torch.cuda.synchronize()
    got = {"m": host(mf), "v": host(vf), "v_hat": host(hf), "out": host(out)}
    hb, hg, hm, hv, hh = (host(x) for x in (buf, gp, m0, v0, h0))
    parity_fedbuff = parity_fadas = True
    checked = 0
    for t in range(len(sizes)):
        for w in range(len(hb[t])):
            parity_fedbuff &= bool(fc.same_bits(fb[t][w], fc.fedbuff_flush(hb[t][w], hg[t][w], K, lr)).all())
            want = fc.fadas_flush(hb[t][w], hg[t][w], hm[t][w], hv[t][w], hh[t][w], K, sc)
            parity_fadas &= all(bool(fc.same_bits(got[k][t][w], want[k]).all()) for k in got)
            checked += hb[t][w].size
    del fb, got, hb, hg, hm, hv, hh

    work = [torch.empty_like(t) for t in buf]
    mt, vt, ht = ([t.clone() for t in x] for x in (m0, v0, h0))
    sqrt_bc2, step = sc[4], sc[6]

    def span(body, refresh=False):
        def run(ev):
            if refresh:
                torch._foreach_copy_(work, buf)
            junk.amax()
            if ev is not None:
                ev[0].record()
            body()
            if ev is not None:
                ev[1].record()
        return run

    keep = []

    def torch_fedbuff():
        with torch.no_grad():
            for t in work:
                t.float().div_(K)
            keep[:] = [(1.0 * a) + (lr * b) for a, b in zip(gp, work)]

    def torch_fadas():
        with torch.no_grad():
            for t in work:
                t.float().div_(K)
            for b, m, v, h in zip(work, mt, vt, ht):
                m.mul_(0.9).add_(b, alpha=(1 - 0.9))
                v.mul_(0.999).addcmul_(b, b, value=(1 - 0.999))
                torch.maximum(h, v, out=h)
            res = []
            for a, m, h in zip(gp, mt, ht):
                denom = (h.sqrt() / sqrt_bc2).add_(1e-8)
                res.append(torch.addcdiv(a, m, denom, value=step))
            keep[:] = res

    legs = {"fedbuff_fused": span(lambda: flush.fedbuff_flush_batched(buf, gp, out, lay, K, lr)),
            "fedbuff_torch": span(torch_fedbuff, refresh=True),
            "fadas_fused": span(lambda: flush.fadas_flush_batched(buf, gp, mf, vf, hf, out, lay, K, sc)),
            "fadas_torch": span(torch_fadas, refresh=True)}
    ms = {k: [] for k in legs}
    for _ in range(repeats):   # the four legs alternate within a repeat
        for k, step_fn in legs.items():
            _, evs = timed(step_fn, args.steps, args.warmup, 1, 2)
            ms[k].append(_median([e[0].elapsed_time(e[1]) for e in evs]))
    del keep[:]
    n = int(sum(sizes))
    res = {"tensors": len(sizes), "elements": n, "parity_elements": checked, "parity_fedbuff": parity_fedbuff,
           "parity_fadas": parity_fadas, "K": K, "round": rnd}
    for k, v in ms.items():
        res[k + "_ms"] = [round(x, 4) for x in v]
    for name, nbytes in (("fedbuff", 12), ("fadas", 36)):
        f, t = _median(ms[name + "_fused"]), _median(ms[name + "_torch"])
        res[name + "_ratio"] = round(t / f, 3)
        res[name + "_fused_frac_moved"] = round(nbytes * n / (f * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
    return res


def mode_flush(args, world, rank, dev):
    """The buffered servers' flush: one fused launch against the reference's statements run by torch on the same
    device tensors. No threshold and no parent-commit number (the path is new): times, ratios, parity flags."""
    sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
    import recipes
    junk = torch.zeros(128 << 20, dtype=torch.float32, device=dev)
    c3 = _flush_leg(list(recipes.bucket_sizes("equal")) + [64] * 256, args, dev, junk)
    big = _flush_leg([args.elems or 1 << 28], args, dev, junk)
    return {"mode": "flush", "metric": "FADAS flush (m, v, v_hat in place + params_prime), C3-shaped device dict, one "
            "launch, Infinity Cache flushed", "unit": "ms", "value": _median(c3["fadas_fused_ms"]),
            "parity": all(leg[f] for leg in (c3, big) for f in ("parity_fedbuff", "parity_fadas")),
            "steps": args.steps, "repeats": 3, "c3_dict": c3, "one_tensor": big}


def _broadcast_leg(sizes, args, dev, junk, repeats=3):
    """One layout of the broadcast leg, hidden state and g both device-resident. Kernels alone (HIP events, the
    Infinity Cache read-flushed before every call): ops.encode_delta_batched followed by ops.dequantize_add_batched
    (the pair the fused launch replaces) against ops.encode_delta_update_batched in its two-pass form and, where
    the layout allows it, its resident form. Whole call (wall): broadcast_delta_ against send_delta + receive_add_.
    Every figure is `repeats` medians of args.steps calls, all listed; a fused form counts as faster when its
    worst repeat is below the pair's best repeat (the gap exceeds the spread of the repeats)."""
    from adfl_amd import _lib, ops
    from adfl_amd.Channel import SLQChannel
    gen = torch.Generator(device=dev).manual_seed(0)
    hidden, new = {}, {}
    for i, n in enumerate(sizes):
        for name, shape in ((f"layer{i:03d}.weight", (1, n)), (f"layer{i:03d}.bias", (64,))):
            new[name] = torch.randn(shape, device=dev, generator=gen) * 1e-2
            hidden[name] = new[name] + torch.randn(shape, device=dev, generator=gen) * 1e-5
    names = [k for k in hidden if hidden[k].ndim > 1]
    gs, hs = [new[k] for k in names], [hidden[k] for k in names]
    lay = ops.BucketLayout(list(sizes))
    ptrs = tuple(torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64) for ts in (gs, hs))
    q = torch.empty(lay.total, dtype=torch.int8, device=dev)
    scales = torch.empty(lay.ntensors, device=dev)
    partials = torch.empty(lay.nchunks, dtype=torch.int32, device=dev)
    resident_ok = lay.nwork > 0 and lay.max_tensor_chunks <= _lib.DELTA_RESIDENT_CHUNKS
    n = int(sum(sizes))

    # parity of each fused form against the pair, on copies
    def pair_on(h):
        qq, ss = ops.encode_delta_batched(gs, h, lay, 8)
        ops.dequantize_add_batched(qq, ss, lay, [h])
        return qq, ss
    want_h = [t.clone() for t in hs]
    want_q, want_s = pair_on(want_h)
    parity = {}
    for form in (("twopass", "resident") if resident_ok else ("twopass",)):
        ops._UPDATE_RESIDENT_FORM = form
        got_h = [t.clone() for t in hs]
        got_q, got_s = ops.encode_delta_update_batched(gs, got_h, lay, 8)
        owned = torch.zeros(lay.total, dtype=torch.bool, device=dev)
        for o, m in zip(lay.offsets.tolist(), sizes):
            owned[o:o + m] = True
        parity[form] = bool(torch.equal(got_q[owned], want_q[owned])
                            and torch.equal(got_s.view(torch.int32), want_s.view(torch.int32))
                            and all(torch.equal(a.view(torch.int32), b.view(torch.int32))
                                    for a, b in zip(got_h, want_h)))
    del want_h, want_q, got_h, got_q

    def k_pair(ev):
        junk.amax()   # read-flush of the Infinity Cache
        if ev is not None:
            ev[0].record()
        ops.encode_delta_batched(gs, hs, lay, 8, q=q, scales=scales, partials=partials, ptrs=ptrs)
        ops.dequantize_add_batched(q, scales, lay, [hs])
        if ev is not None:
            ev[1].record()

    def k_fused(ev):
        junk.amax()
        if ev is not None:
            ev[0].record()
        ops.encode_delta_update_batched(gs, hs, lay, 8, q=q, scales=scales, partials=partials, ptrs=ptrs)
        if ev is not None:
            ev[1].record()

    def events(step):
        out = []
        for _ in range(repeats):
            _, evs = timed(step, args.steps, args.warmup, 1, 2)
            out.append(_median([e[0].elapsed_time(e[1]) for e in evs]))
        return out

    res = {"tensors": len(sizes), "elements": n, "parity": parity}
    pair = events(k_pair)
    res["pair_alone_ms"] = round(_median(pair), 4)
    res["pair_alone_ms_repeats"] = [round(v, 4) for v in pair]
    for form in parity:
        ops._UPDATE_RESIDENT_FORM = form
        f = events(k_fused)
        res[f"fused_{form}_alone_ms"] = round(_median(f), 4)
        res[f"fused_{form}_alone_ms_repeats"] = [round(v, 4) for v in f]
        res[f"fused_{form}_below_pair_by_more_than_spread"] = bool(max(f) < min(pair))
        res[f"fused_{form}_over_pair"] = round(_median(f) / _median(pair), 4)
        # 13 B per element: read g, read h, write the payload, write h (the two passes read g and h once more)
        res[f"fused_{form}_frac_of_peak_on_13B"] = round(13 * n / (_median(f) * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
    ops._UPDATE_RESIDENT_FORM = "resident"

    # the whole call, wall clock
    ch = SLQChannel(8)

    def wall(fn):
        out = []
        for _ in range(args.steps):
            junk.amax()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return _median(out)

    def two_calls(h):
        c = ch.send_delta(h, new)[0]
        ch.receive_add_(c, [h])
        return c
    h_a, h_b = ({k: v.clone() for k, v in hidden.items()} for _ in range(2))
    c_a, c_b = ch.broadcast_delta_(h_a, new)[0], two_calls(h_b)
    res["call_parity"] = bool(_delta_same(c_a, c_b) and all(
        torch.equal(h_a[k].view(torch.int32), h_b[k].view(torch.int32)) for k in h_a))
    del c_a, c_b
    for _ in range(args.warmup):
        ch.broadcast_delta_(h_a, new), two_calls(h_b)
    f_ms = [wall(lambda: ch.broadcast_delta_(h_a, new)) for _ in range(repeats)]
    u_ms = [wall(lambda: two_calls(h_b)) for _ in range(repeats)]
    res.update({"broadcast_delta_ms": round(_median(f_ms), 4), "broadcast_delta_ms_repeats": [round(v, 4) for v in f_ms],
                "send_delta_receive_add_ms": round(_median(u_ms), 4),
                "send_delta_receive_add_ms_repeats": [round(v, 4) for v in u_ms],
                "call_below_two_calls_by_more_than_spread": bool(max(f_ms) < min(u_ms))})
    return res


def mode_broadcast(args, world, rank, dev):
    """QAFeL's broadcast (delta encode + hidden-state update in one launch) against the two calls it replaces, on
    the C3 layouts and one 2^28-element tensor; written to profiles/broadcast/broadcast.json (an A/B library
    selected with ADFL_LIB_VARIANT writes broadcast_<its name>.json)."""
    sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
    import recipes
    junk = torch.zeros(128 << 20, dtype=torch.float32, device=dev)
    legs = {"c3_equal": _broadcast_leg(recipes.bucket_sizes("equal"), args, dev, junk),
            "c3_loguniform": _broadcast_leg(recipes.bucket_sizes("loguniform", 0), args, dev, junk),
            "one_tensor_2p28": _broadcast_leg([1 << 28], args, dev, junk)}
    variant = os.environ.get("ADFL_LIB_VARIANT")
    line = {"mode": "broadcast", "metric": "fused delta encode + hidden-state update, kernels alone, C3 equal layout, "
            "Infinity Cache flushed", "unit": "ms", "library": os.path.basename(variant) if variant else "product",
            "value": min(v for k, v in legs["c3_equal"].items() if k.startswith("fused_") and k.endswith("_alone_ms")),
            "parity": all(all(leg["parity"].values()) and leg["call_parity"] for leg in legs.values()),
            "steps": args.steps, "repeats": 3, **legs}
    out_dir = os.path.join(REPO, "profiles", "broadcast")
    os.makedirs(out_dir, exist_ok=True)
    tag = "" if not variant else "_" + os.path.splitext(os.path.basename(variant))[0].replace("libadfl_", "")
    with open(os.path.join(out_dir, f"broadcast{tag}.json"), "w") as f:
        json.dump(line, f, indent=1)
        f.write("\n")
    return line


def _broadcast_stoch_leg(sizes, args, dev, junk, repeats=3):
    """One layout of the broadcast_stoch leg (mode_broadcast's protocol per stochastic codec), hidden state and g
    both device-resident, bits 8.

    Kernels alone (HIP events, the Infinity Cache read-flushed before every call), each new kernel against the sum
    of the kernels it replaces over planes that stay on the device: rqsgd_encode_delta_update_batched (two passes
    and, where the layout allows it, one launch) against rqsgd_encode_delta_batched + dequantize_axpby_batched;
    qsgd_quantize_update_batched against qsgd_quantize_batched + dequantize_axpby_batched (the difference bucket
    and its norms made once: that part is unchanged code). Whole call (wall), per codec: broadcast_delta_ against
    send_delta + receive_add_; the fused route counts as faster when its median lies below the two calls' median
    by more than the two calls' own spread across the repeats (max - min of their `repeats` medians).

    A broadcast pulls h onto g, and a tensor whose difference has become exactly zero takes the codecs' norm == 0
    branch, which reads less: successive calls therefore alternate between two g (as the server's model moves
    between two flushes), so every timed call encodes a difference of the magnitude of the step between them."""
    import numpy as np
    from adfl_amd import _lib, ops
    from adfl_amd import stoch as sops
    from adfl_amd.Channel import CNATChannel, QSGDChannel, RQSGDChannel
    gen = torch.Generator(device=dev).manual_seed(0)
    hidden, new = {}, {}
    for i, n in enumerate(sizes):
        for name, shape in ((f"layer{i:03d}.weight", (1, n)), (f"layer{i:03d}.bias", (64,))):
            new[name] = torch.randn(shape, device=dev, generator=gen) * 1e-2
            hidden[name] = new[name] + torch.randn(shape, device=dev, generator=gen) * 1e-5
    new2 = {k: v + torch.randn(v.shape, device=dev, generator=gen) * 1e-5 for k, v in new.items()}
    news = (new, new2)
    names = [k for k in hidden if hidden[k].ndim > 1]
    gs, gs2, hs = [new[k] for k in names], [new2[k] for k in names], [hidden[k].clone() for k in names]
    comp, lay = ops.BucketLayout(list(sizes), align=1), ops.BucketLayout(list(sizes))
    ushift = np.ascontiguousarray(comp.offsets - lay.offsets, dtype=np.int64)
    table = lambda ts: torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64)   # noqa: E731
    h_tab = table(hs)
    g_alt = ((gs, (table(gs), h_tab)), (gs2, (table(gs2), h_tab)))   # (g, its pointer tables) of even / odd calls
    calls = [0]

    def next_g():
        calls[0] += 1
        return g_alt[calls[0] & 1]
    n = int(sum(sizes))
    resident_ok = lay.nwork > 0 and lay.max_tensor_chunks <= _lib.DELTA_RESIDENT_CHUNKS
    same = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))   # noqa: E731

    def owned(L):
        m = torch.zeros(L.total, dtype=torch.bool, device=dev)
        for o, k in zip(L.offsets.tolist(), sizes):
            m[o:o + k] = True
        return m

    def events(step):
        out = []
        for _ in range(repeats):
            _, evs = timed(step, args.steps, args.warmup, 1, 2)
            out.append(_median([e[0].elapsed_time(e[1]) for e in evs]))
        return out

    def kernel(fn):
        def step(ev):
            junk.amax()   # read-flush of the Infinity Cache
            if ev is not None:
                ev[0].record()
            fn()
            if ev is not None:
                ev[1].record()
        return step

    def record(res, key, f, pair, nbytes):
        res[f"{key}_alone_ms"] = round(_median(f), 4)
        res[f"{key}_alone_ms_repeats"] = [round(v, 4) for v in f]
        res[f"{key}_below_pair_by_more_than_spread"] = bool(_median(pair) - _median(f) > max(pair) - min(pair))
        res[f"{key}_over_pair"] = round(_median(f) / _median(pair), 4)
        res[f"{key}_frac_of_peak_on_{nbytes}B"] = round(nbytes * n / (_median(f) * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)

    res = {"tensors": len(sizes), "elements": n}
    # ---- RQSGD: planes in the aligned bucket, the compact draws kept by ushift (the channel's layout)
    lv, sg = torch.empty(lay.total, dtype=torch.uint8, device=dev), torch.empty(lay.total, dtype=torch.int8, device=dev)
    norms, mins = torch.empty(lay.ntensors, device=dev), torch.empty(lay.ntensors, device=dev)
    ws = sops.workspace(lay, dev)
    kw = dict(ushift=ushift, seed=11, counter=0, levels=lv, signs=sg, norms=norms, mins=mins, ws=ws)

    def rq_pair(h, g=gs, **k):
        out = sops.rqsgd_encode_delta_batched(g, h, lay, 8, **k)
        sops.dequantize_axpby_batched("rqsgd", out[0], out[1], out[2], lay, 8, [h], [h], 1.0, 1.0, mins=out[3])
        return out
    x = ops.bucket_diff(gs, hs, comp)   # QSGD's difference bucket, before the timed calls move hs
    want_h = [t.clone() for t in hs]
    want = [t.clone() for t in rq_pair(want_h, ushift=ushift, seed=11, counter=0)]
    m = owned(lay)
    rq = {"parity": {}}
    forms = (("twopass", False), ("resident", True)) if resident_ok else (("twopass", False),)
    for form, resident in forms:
        got_h = [t.clone() for t in hs]
        got = sops.rqsgd_encode_delta_update_batched(gs, got_h, lay, 8, ushift=ushift, seed=11, counter=0,
                                                     resident=resident)
        rq["parity"][form] = bool(torch.equal(got[0][m], want[0][m]) and torch.equal(got[1][m], want[1][m])
                                  and same(got[2], want[2]) and same(got[3], want[3])
                                  and all(same(a, b) for a, b in zip(got_h, want_h)))
    del want_h, want, got_h, got
    def rq_pair_step():
        g, tabs = next_g()
        rq_pair(hs, g, ptrs=tabs, **kw)

    def rq_fused_step(resident):
        g, tabs = next_g()
        sops.rqsgd_encode_delta_update_batched(g, hs, lay, 8, resident=resident, ptrs=tabs, **kw)
    pair = events(kernel(rq_pair_step))
    rq["pair_alone_ms"], rq["pair_alone_ms_repeats"] = round(_median(pair), 4), [round(v, 4) for v in pair]
    for form, resident in forms:
        f = events(kernel(lambda: rq_fused_step(resident)))
        record(rq, f"fused_{form}", f, pair, 18 if resident else 22)
    rq["zero_norm_tensors_after_timing"] = int((norms == 0).sum())
    res["rqsgd"] = rq
    # ---- QSGD under the reference norm: the compact difference bucket and its norms made once
    qn = sops.torch_norms(x, comp)
    lvc, sgc = lv[:comp.total], sg[:comp.total]
    qkw = dict(seed=11, counter=0, levels=lvc, signs=sgc)

    def qs_pair(h, **k):
        a, b = sops.qsgd_quantize_batched(x, comp, 8, qn, **k)
        sops.dequantize_axpby_batched("qsgd", a, b, qn, comp, 8, [h], [h], 1.0, 1.0)
        return a, b
    hs = [hidden[k].clone() for k in names]   # (x and its norms do not move: neither do the kernels' paths)
    h_tab = table(hs)
    want_h, got_h = [t.clone() for t in hs], [t.clone() for t in hs]
    want = [t.clone() for t in qs_pair(want_h, seed=11, counter=0)]
    got = sops.qsgd_quantize_update_batched(x, comp, 8, qn, got_h, seed=11, counter=0)
    qs = {"parity": bool(torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
                         and all(same(a, b) for a, b in zip(got_h, want_h))),
          "zero_norm_tensors": int((qn == 0).sum())}
    del want_h, want, got_h, got
    pair = events(kernel(lambda: qs_pair(hs, **qkw)))
    qs["pair_alone_ms"], qs["pair_alone_ms_repeats"] = round(_median(pair), 4), [round(v, 4) for v in pair]
    f = events(kernel(lambda: sops.qsgd_quantize_update_batched(x, comp, 8, qn, hs, ptrs=h_tab, **qkw)))
    record(qs, "fused", f, pair, 14)
    res["qsgd"] = qs
    del x, lv, sg

    # ---- the whole call, wall clock, per codec
    def wall(fn):
        out = []
        for _ in range(args.steps):
            junk.amax()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return _median(out)

    for codec, cls in (("qsgd", QSGDChannel), ("rqsgd", RQSGDChannel), ("cnat", CNATChannel)):
        ch = cls(8)

        def two_calls(h, g):
            c = ch.send_delta(h, g)[0]
            ch.receive_add_(c, [h])
            return c

        def next_new():
            calls[0] += 1
            return news[calls[0] & 1]
        h_a, h_b = ({k: v.clone() for k, v in hidden.items()} for _ in range(2))
        torch.manual_seed(3)
        c_a = ch.broadcast_delta_(h_a, new)[0]
        torch.manual_seed(3)
        c_b = two_calls(h_b, new)
        call = {"call_parity": bool(_stoch_same(c_a, c_b) and all(same(h_a[k], h_b[k]) for k in h_a))}
        del c_a, c_b
        for _ in range(args.warmup):
            ch.broadcast_delta_(h_a, next_new()), two_calls(h_b, next_new())
        f_ms = [wall(lambda: ch.broadcast_delta_(h_a, next_new())) for _ in range(repeats)]
        u_ms = [wall(lambda: two_calls(h_b, next_new())) for _ in range(repeats)]
        call["zero_norm_payloads_in_last_call"] = sum(
            isinstance(p.scale, torch.Tensor) for p in ch.broadcast_delta_(h_a, next_new())[0].params.values())
        call.update({"broadcast_delta_ms": round(_median(f_ms), 4),
                     "broadcast_delta_ms_repeats": [round(v, 4) for v in f_ms],
                     "send_delta_receive_add_ms": round(_median(u_ms), 4),
                     "send_delta_receive_add_ms_repeats": [round(v, 4) for v in u_ms],
                     "two_calls_spread_ms": round(max(u_ms) - min(u_ms), 4),
                     "call_below_two_calls_by_more_than_spread":
                         bool(_median(u_ms) - _median(f_ms) > max(u_ms) - min(u_ms))})
        res.setdefault(codec, {}).update(call)
        del h_a, h_b
    return res


def mode_broadcast_stoch(args, world, rank, dev):
    """QAFeL's broadcast through QSGDChannel / RQSGDChannel / CNATChannel(8) (the hidden-state update fused into
    the delta encode) against the two calls it replaces, on the C3 layouts and one 2^28-element tensor; written to
    profiles/broadcast/broadcast_stoch.json (an A/B library selected with ADFL_LIB_VARIANT writes
    broadcast_stoch_<its name>.json: the h' store flavour)."""
    sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
    import recipes
    junk = torch.zeros(128 << 20, dtype=torch.float32, device=dev)
    legs = {"c3_equal": _broadcast_stoch_leg(recipes.bucket_sizes("equal"), args, dev, junk),
            "c3_loguniform": _broadcast_stoch_leg(recipes.bucket_sizes("loguniform", 0), args, dev, junk),
            "one_tensor_2p28": _broadcast_stoch_leg([1 << 28], args, dev, junk)}
    variant = os.environ.get("ADFL_LIB_VARIANT")
    parity = all(all(leg["rqsgd"]["parity"].values()) and leg["qsgd"]["parity"]
                 and all(leg[c]["call_parity"] for c in ("qsgd", "rqsgd", "cnat")) for leg in legs.values())
    line = {"mode": "broadcast_stoch", "metric": "RQSGD fused delta encode + hidden-state update, kernels alone, C3 "
            "equal layout, Infinity Cache flushed", "unit": "ms",
            "library": os.path.basename(variant) if variant else "product",
            "value": min(v for k, v in legs["c3_equal"]["rqsgd"].items()
                         if k.startswith("fused_") and k.endswith("_alone_ms")),
            "parity": parity, "steps": args.steps, "repeats": 3, **legs}
    out_dir = os.path.join(REPO, "profiles", "broadcast")
    os.makedirs(out_dir, exist_ok=True)
    tag = "" if not variant else "_" + os.path.splitext(os.path.basename(variant))[0].replace("libadfl_", "")
    with open(os.path.join(out_dir, f"broadcast_stoch{tag}.json"), "w") as f:
        json.dump(line, f, indent=1)
        f.write("\n")
    return line


def _sync_delta_rows(codec, lay, k, dev, gen):
    """K random bucket payloads of `codec` on the device (bytes drawn directly: the kernels' time does not depend
    on the values) and the two launches over them: (mean(out), fused(base, out, alpha, beta), bytes per element)."""
    from adfl_amd import ops, stoch
    row = (lay.total + 15) // 16 * 16
    t = lay.ntensors
    sc = (torch.rand((k, t), device=dev, generator=gen) + 0.5) * 1e-3
    if codec in ("slq8", "slq4"):
        packed = codec == "slq4"
        width = (row // 2 + 15) // 16 * 16 if packed else row
        q = torch.randint(0, 256, (k, width), device=dev, generator=gen, dtype=torch.uint8)
        q = q if packed else q.view(torch.int8)
        return (lambda out: ops.dequantize_mean_batched(q, sc, lay, out=out, packed=packed),
                lambda base, out, a, b: ops.dequantize_mean_axpby_batched(q, sc, lay, base, out, a, b, packed=packed),
                0.5 if packed else 1.0)
    if codec == "cnat":
        lv = (-torch.randint(0, 21, (k, row), device=dev, generator=gen, dtype=torch.int8)).view(torch.uint8)
    else:
        lv = torch.randint(0, 256, (k, row), device=dev, generator=gen, dtype=torch.uint8)
    sg = (torch.randint(0, 2, (k, row), device=dev, generator=gen, dtype=torch.int8) * 2 - 1).to(torch.int8)
    mins = (torch.rand((k, t), device=dev, generator=gen) - 0.5) * 1e-3 if codec == "rqsgd" else None
    return (lambda out: stoch.dequantize_mean_batched(codec, lv, sg, sc, lay, 8, mins=mins, out=out),
            lambda base, out, a, b: stoch.dequantize_mean_axpby_batched(codec, lv, sg, sc, mins, lay, 8, base, out, a,
                                                                        b),
            2.0)


SYNC_DELTA_CODECS = ("slq8", "slq4", "qsgd", "rqsgd", "cnat")


def _sync_delta_leg(sizes, k, args, dev, junk, repeats=3):
    """One layout and K of the sync_delta leg, per codec: the fused decode-mean + axpby launch over a device-resident
    base bucket (new output) against the route without it on the same device tensors in this process — the existing
    decode-mean launch, then torch's (alpha * g) + (beta * m) over the flat bucket (torch's best case: three
    launches, not three per tensor). HIP events, Infinity Cache read-flushed before every call, medians of
    args.steps calls, `repeats` repeats, all listed. Criterion: the fused medians lie below the two-step medians by
    more than the two-step leg's spread (max - min over its repeats)."""
    from adfl_amd import ops
    alpha, beta = 1.0, 1.0
    res = {"tensors": len(sizes), "elements": int(sum(sizes)), "k": k}
    for codec in SYNC_DELTA_CODECS:
        lay = ops.BucketLayout(list(sizes), align=2 if codec == "slq4" else 1)   # receive_mean's compact layouts
        gen = torch.Generator(device=dev).manual_seed(k)
        mean, fused, row_bytes = _sync_delta_rows(codec, lay, k, dev, gen)
        base = torch.randn(lay.total, device=dev, generator=gen)
        out = torch.empty(lay.total, device=dev)
        m = torch.zeros(lay.total, device=dev)
        res2 = []

        def k_fused(ev):
            junk.amax()
            if ev is not None:
                ev[0].record()
            fused(base, out, alpha, beta)
            if ev is not None:
                ev[1].record()

        def k_two_step(ev):
            junk.amax()
            if ev is not None:
                ev[0].record()
            mean(m)
            r = (alpha * base) + (beta * m)
            if ev is not None:
                ev[1].record()
            res2[:] = [r]

        k_fused(None), k_two_step(None)
        torch.cuda.synchronize()
        own = torch.zeros(lay.total, dtype=torch.bool)
        for o, n in zip(lay.offsets.tolist(), lay.sizes.tolist()):
            own[o:o + n] = True
        own = own.to(dev)
        parity = _bits_equal(out[own], res2[0][own])
        f_ms, u_ms = [], []
        for _ in range(repeats):
            _, evs = timed(k_fused, args.steps, args.warmup, 1, 2)
            f_ms.append(_median([e[0].elapsed_time(e[1]) for e in evs]))
            _, evs = timed(k_two_step, args.steps, args.warmup, 1, 2)
            u_ms.append(_median([e[0].elapsed_time(e[1]) for e in evs]))
        spread = max(u_ms) - min(u_ms)
        n = int(sum(sizes))
        res[codec] = {"parity": parity, "fused_ms_repeats": [round(v, 4) for v in f_ms],
                      "two_step_ms_repeats": [round(v, 4) for v in u_ms], "fused_ms": round(_median(f_ms), 4),
                      "two_step_ms": round(_median(u_ms), 4), "two_step_spread_ms": round(spread, 4),
                      "ratio": round(_median(u_ms) / _median(f_ms), 3),
                      "fused_below_two_step_by_more_than_spread": bool(_median(u_ms) - _median(f_ms) > spread),
                      # bytes the fused kernel must move per element: K payload rows, g 4, result 4
                      "fused_frac_of_hbm_peak": round((k * row_bytes + 8) * n / (_median(f_ms) * 1e-3) / 1e9
                                                      / HBM_PEAK_GBS, 4)}
        del base, out, m, res2[:], mean, fused
    return res


def _sync_delta_host(sizes, k, steps):
    """The whole channel call host to host on a CPU dict (ADFL's own pattern): receive_mean_axpby against
    receive_mean followed by the reference's CPU add_parameters, wall clock, per channel class."""
    from adfl_amd.Channel import CNATChannel, PackedSLQChannel, QSGDChannel, RQSGDChannel, SLQChannel
    shapes = [(1, m) for m in sizes]
    g_cpu = {f"layer{i:03d}.weight": torch.randn(sh) for i, sh in enumerate(shapes)}
    for i in range(len(sizes)):
        g_cpu[f"layer{i:03d}.bias"] = torch.randn(64)
    res = {"k": k, "tensors": len(sizes)}

    def wall(fn):
        ts = []
        for _ in range(steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return _median(ts)

    for name, ch in (("slq8", SLQChannel(8)), ("slq4", PackedSLQChannel(4)), ("qsgd", QSGDChannel(8)),
                     ("rqsgd", RQSGDChannel(8)), ("cnat", CNATChannel(8))):
        torch.manual_seed(1)
        ups = [ch.on_client_send({n: torch.randn(t.shape) * 1e-2 for n, t in g_cpu.items()})[0] for _ in range(k)]

        def fused():
            return ch.receive_mean_axpby(ups, g_cpu, 1.0, 1.0)[0]

        def two_step():
            agg, _ = ch.receive_mean(ups)
            with torch.no_grad():   # add_parameters (model.py:326-334) on the same box
                return {n: (1.0 * g_cpu[n]) + (1.0 * agg[n]) for n in agg}

        a, b = fused(), two_step()
        rec = {"parity": list(a) == list(b) and all(_bits_equal(a[n], b[n]) for n in a)}
        del a, b
        rec["receive_mean_axpby_ms"] = round(wall(fused), 3)
        rec["receive_mean_then_add_parameters_ms"] = round(wall(two_step), 3)
        rec["ratio"] = round(rec["receive_mean_then_add_parameters_ms"] / rec["receive_mean_axpby_ms"], 3)
        res[name] = rec
        del ups
    return res


def mode_sync_delta(args, world, rank, dev):
    """The synchronous DELTA server step (Simple(CommType.DELTA, sync=True)._sync_update): the fused decode-mean +
    axpby launch against the decode-mean launch followed by torch's statement, per codec, on the C3 layouts at
    K = 4 and 16 and one 2^26-element tensor at K = 4, plus the whole channel call host to host on the C3 dict;
    written to profiles/sync_delta/sync_delta.json. A leg that misses the criterion is reported as such."""
    sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
    import recipes
    junk = torch.zeros(128 << 20, dtype=torch.float32, device=dev)
    eq, lu = recipes.bucket_sizes("equal"), recipes.bucket_sizes("loguniform", 0)
    legs = {"c3_equal_k4": _sync_delta_leg(eq, 4, args, dev, junk),
            "c3_equal_k16": _sync_delta_leg(eq, 16, args, dev, junk),
            "c3_loguniform_k4": _sync_delta_leg(lu, 4, args, dev, junk),
            "c3_loguniform_k16": _sync_delta_leg(lu, 16, args, dev, junk),
            "one_tensor_2p26_k4": _sync_delta_leg([args.elems or 1 << 26], 4, args, dev, junk)}
    host = _sync_delta_host(eq, 4, max(3, min(args.steps, 5)))
    flags = [leg[c]["fused_below_two_step_by_more_than_spread"] for leg in legs.values() for c in SYNC_DELTA_CODECS]
    line = {"mode": "sync_delta", "metric": "SLQ 8 fused decode-mean + axpby, kernel alone, C3 equal layout, K = 4, "
            "Infinity Cache flushed", "unit": "ms", "value": legs["c3_equal_k4"]["slq8"]["fused_ms"],
            "parity": all(leg[c]["parity"] for leg in legs.values() for c in SYNC_DELTA_CODECS)
            and all(host[c]["parity"] for c in SYNC_DELTA_CODECS),
            "legs_meeting_criterion": f"{sum(flags)} of {len(flags)}", "steps": args.steps, "repeats": 3, **legs,
            "host_c3_equal_k4": host}
    out_dir = os.path.join(REPO, "profiles", "sync_delta")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "sync_delta.json"), "w") as f:
        json.dump(line, f, indent=1)
        f.write("\n")
    return line


RECEIVE_FLUSH_CODECS = ("slq8", "qsgd")


def _receive_flush_leg(sizes, args, dev, junk, repeats=3):
    """One layout of the receive_flush leg, kernels alone: every operand one flat device bucket of the payload's
    64-aligned layout (what the channels' host route stages; pointer tables to separate tensors run the same kernels
    after a host-side table build, which HIP events around two launches would count against the two-call route). The
    fused decode + accumulate + flush launch against today's two launches on the same buckets in this process — the
    decode + axpby in place on the buffer, then the flush — for SLQ(8) and QSGD(8), FedBuff and FADAS. HIP events,
    Infinity Cache read-flushed before every call as _flush_leg does, medians of args.steps calls, `repeats`
    repeats, all listed. Parity: one call of each route from the same buffer and moments, `out` and the three
    moments compared bit for bit."""
    from adfl_amd import flush, ops, stoch
    K, lr, factor, rnd = 10, 0.05, 6 ** -0.5, 3
    lay = ops.BucketLayout(list(sizes), align=64)
    gen = torch.Generator(device=dev).manual_seed(0)

    def make(scale, positive=False):
        t = torch.randn(lay.total, device=dev, generator=gen) * scale
        return t.abs_() if positive else t

    buf0, gp = make(1e-2), make(1.0)
    m0, v0 = make(1e-3), make(1e-5, positive=True)
    h0 = v0 * 1.5
    sc = flush.fadas_scalars(0.9, 0.999, 1e-8, lr, rnd)
    x = make(1e-2)
    n_el = int(sum(sizes))
    res = {"tensors": len(sizes), "elements": n_el, "K": K, "round": rnd}
    for codec in RECEIVE_FLUSH_CODECS:
        if codec == "slq8":
            q, s = ops.encode_batched(x, lay, 8)
            fed = lambda b, o: ops.dequantize_fedbuff_flush_batched(q, s, lay, b, gp, o, K, factor, lr)   # noqa: E731
            fad = lambda b, m, v, h, o: ops.dequantize_fadas_flush_batched(q, s, lay, b, gp, m, v, h, o, K, sc)  # noqa: E731
            add = lambda b, f: ops.dequantize_axpby_batched(q, s, lay, b, b, 1.0, f)   # noqa: E731
            payload_bytes = 1
        else:
            lv, sg, nr = stoch.qsgd_encode_batched(x, lay, 8, seed=5, counter=0)[:3]
            fed = lambda b, o: stoch.dequantize_fedbuff_flush_batched("qsgd", lv, sg, nr, lay, 8, b, gp, o, K, factor,   # noqa: E731
                                                                      lr)
            fad = lambda b, m, v, h, o: stoch.dequantize_fadas_flush_batched("qsgd", lv, sg, nr, lay, 8, b, gp, m, v, h,   # noqa: E731
                                                                             o, K, sc)
            add = lambda b, f: stoch.dequantize_axpby_batched("qsgd", lv, sg, nr, lay, 8, b, b, 1.0, f)   # noqa: E731
            payload_bytes = 2
        out_f, out_t = torch.zeros_like(gp), torch.zeros_like(gp)
        for strategy, moved in (("fedbuff", payload_bytes + 12), ("fadas", payload_bytes + 36)):
            fadas = strategy == "fadas"
            bt = buf0.clone()                                    # the two-call route writes its buffer
            mf, vf, hf = (y.clone() for y in (m0, v0, h0))
            mt, vt, ht = (y.clone() for y in (m0, v0, h0))

            def fused():
                if fadas:
                    fad(buf0, mf, vf, hf, out_f)
                else:
                    fed(buf0, out_f)

            def two_calls():
                if fadas:
                    add(bt, 1.0)
                    flush.fadas_flush_batched(bt, gp, mt, vt, ht, out_t, lay, K, sc)
                else:
                    add(bt, factor)
                    flush.fedbuff_flush_batched(bt, gp, out_t, lay, K, lr)

            fused(), two_calls()
            torch.cuda.synchronize()
            pairs = [(out_f, out_t)] + ([(mf, mt), (vf, vt), (hf, ht)] if fadas else [])
            parity = all(_bits_equal(a, b) for a, b in pairs)

            def span(body, refresh):
                def run(ev):
                    if refresh:   # the same buffer for every timed call, restored outside the timed span
                        bt.copy_(buf0)
                    junk.amax()
                    if ev is not None:
                        ev[0].record()
                    body()
                    if ev is not None:
                        ev[1].record()
                return run

            f_ms, t_ms = [], []
            for _ in range(repeats):
                _, evs = timed(span(fused, False), args.steps, args.warmup, 1, 2)
                f_ms.append(_median([e[0].elapsed_time(e[1]) for e in evs]))
                _, evs = timed(span(two_calls, True), args.steps, args.warmup, 1, 2)
                t_ms.append(_median([e[0].elapsed_time(e[1]) for e in evs]))
            f, t = _median(f_ms), _median(t_ms)
            res[f"{codec}_{strategy}"] = {
                "parity": parity, "fused_ms_repeats": [round(v, 4) for v in f_ms],
                "two_calls_ms_repeats": [round(v, 4) for v in t_ms], "fused_ms": round(f, 4),
                "two_calls_ms": round(t, 4), "ratio": round(t / f, 3), "fused_faster": bool(f < t),
                "fused_bytes_per_element": moved, "two_calls_bytes_per_element": moved + 8,
                "fused_frac_of_hbm_peak": round(moved * n_el / (f * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
            del bt, mf, vf, hf, mt, vt, ht
        del out_f, out_t
    return res


def _receive_flush_host(sizes, steps, repeats=3):
    """The whole channel call host to host on a CPU dict (ADFL's own pattern), wall clock: receive_scaled_flush /
    FadasMoments.receive_flush against receive_scaled_add_ followed by fedbuff_flush / FadasMoments.flush, each route
    on its own copy of the buffer and its own moments, for SLQChannel(8) and QSGDChannel(8)."""
    import copy

    from adfl_amd import FadasMoments, fedbuff_flush
    from adfl_amd.Channel import QSGDChannel, SLQChannel
    K, lr, factor = 10, 0.05, 6 ** -0.5
    g_cpu = {f"layer{i:03d}.weight": torch.randn(1, m) for i, m in enumerate(sizes)}
    for i in range(len(sizes)):
        g_cpu[f"layer{i:03d}.bias"] = torch.randn(64)
    res = {"tensors": len(sizes), "K": K}

    def wall(fn):
        ts = []
        for _ in range(steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return _median(ts)

    for name, ch in (("slq8", SLQChannel(8)), ("qsgd", QSGDChannel(8))):
        torch.manual_seed(1)
        c = ch.on_client_send({n: torch.randn(t.shape) * 1e-2 for n, t in g_cpu.items()})[0]
        buf0 = {n: torch.randn(t.shape) * 1e-2 for n, t in g_cpu.items()}
        for strategy in ("fedbuff", "fadas"):
            buf_f, buf_t = copy.deepcopy(buf0), copy.deepcopy(buf0)
            mom_f, mom_t = FadasMoments(), FadasMoments()
            rnd = [1, 1]

            def fused(c=c):
                if strategy == "fedbuff":
                    return ch.receive_scaled_flush(c, buf_f, g_cpu, factor, K, lr)[0]
                rnd[0] += 1
                return mom_f.receive_flush(ch, c, buf_f, g_cpu, K, lr, rnd[0] - 1)

            def two_calls(c=c):
                if strategy == "fedbuff":
                    ch.receive_scaled_add_(c, [buf_t], factor)
                    return fedbuff_flush(buf_t, g_cpu, K, lr)
                ch.receive_scaled_add_(c, [buf_t], 1.0)
                rnd[1] += 1
                return mom_t.flush(buf_t, g_cpu, K, lr, rnd[1] - 1)

            # parity on copies of the payload: the reference's scaling writes a passthrough entry's own tensor
            a, b = fused(copy.deepcopy(c)), two_calls(copy.deepcopy(c))
            parity = list(a) == list(b) and all(_bits_equal(a[n], b[n]) for n in a)
            if strategy == "fadas":
                parity = parity and all(_bits_equal(x[n], y[n]) for x, y in ((mom_f.m, mom_t.m), (mom_f.v, mom_t.v),
                                                                           (mom_f.v_hat, mom_t.v_hat)) for n in x)
            del a, b
            f_ms, t_ms = [], []
            for _ in range(repeats):
                f_ms.append(wall(fused))
                t_ms.append(wall(two_calls))
            f, t = _median(f_ms), _median(t_ms)
            res[f"{name}_{strategy}"] = {"parity": parity, "fused_ms_repeats": [round(v, 3) for v in f_ms],
                                         "two_calls_ms_repeats": [round(v, 3) for v in t_ms], "fused_ms": round(f, 3),
                                         "two_calls_ms": round(t, 3), "ratio": round(t / f, 3),
                                         "fused_faster": bool(f < t)}
        del c, buf0
    return res


def mode_receive_flush(args, world, rank, dev):
    """The buffered servers' K-th client update: the fused decode + accumulate + flush against today's two calls
    (decode + axpby into the buffer, then the flush), which this change leaves untouched and which are therefore the
    baseline, timed in this process. Kernels alone on the C3-shaped device dict and on one 2^26-element tensor, the
    whole channel call host to host on the C3-shaped CPU dict; SLQ(8) and QSGD(8), FedBuff and FADAS; medians of 3
    repeats. No ratio is fixed in advance: times, ratios and a parity flag per leg, written to
    profiles/receive_flush/receive_flush.json."""
    sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
    import recipes
    junk = torch.zeros(128 << 20, dtype=torch.float32, device=dev)
    eq = list(recipes.bucket_sizes("equal"))
    legs = {"c3_dict_device": _receive_flush_leg(eq + [64] * 256, args, dev, junk),
            "one_tensor_2p26": _receive_flush_leg([args.elems or 1 << 26], args, dev, junk),
            "c3_dict_host": _receive_flush_host(eq, max(3, min(args.steps, 5)))}
    cases = [f"{c}_{s}" for c in RECEIVE_FLUSH_CODECS for s in ("fedbuff", "fadas")]
    faster = [leg[c]["fused_faster"] for leg in legs.values() for c in cases]
    line = {"mode": "receive_flush", "metric": "SLQ 8 fused decode + accumulate + FedBuff flush, kernel alone, "
            "C3-shaped device dict, Infinity Cache flushed", "unit": "ms",
            "value": legs["c3_dict_device"]["slq8_fedbuff"]["fused_ms"],
            "parity": all(leg[c]["parity"] for leg in legs.values() for c in cases),
            "legs_where_fused_is_faster": f"{sum(faster)} of {len(faster)}", "steps": args.steps, "repeats": 3, **legs}
    out_dir = os.path.join(REPO, "profiles", "receive_flush")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "receive_flush.json"), "w") as f:
        json.dump(line, f, indent=1)
        f.write("\n")
    return line


def _unpack_planes(lv, sb, total, bits):
    """(level bytes, `sign byte == -1` mask) of a packed bucket's planes, by torch on the device (the format of
    include/adfl_stoch.h, "packed planes")."""
    idx = torch.arange(total, device=lv.device)
    neg = ((sb[idx >> 3].to(torch.int32) >> (idx & 7).to(torch.int32)) & 1).bool()
    if bits > 4:
        return lv[:total], neg
    b = lv[idx >> 1]
    return torch.where((idx & 1) == 0, b >> 4, b & 15), neg


def _packed_stoch_leg(sizes, bits, args, dev, junk, host_steps, repeats=3):
    """One layout and bit width of the packed_stoch leg, QSGD: the packed kernels against the unpacked ones they
    restate (this change leaves those untouched: they are the baseline), alternating, in one process.
    device: quantize given norms, decode, decode + axpby over planes that stay on the device; HIP events, the
            Infinity Cache read-flushed before every call, medians of --steps calls, the median of `repeats` rounds.
    host:   PackedQSGDChannel against QSGDChannel, on_client_send + on_server_receive of a CPU dict, wall."""
    from adfl_amd import ops, stoch
    from adfl_amd.Channel import PackedQSGDChannel, QSGDChannel
    alpha_t = 0.6 * 2 ** -0.5
    alpha, beta = 1 - alpha_t, alpha_t
    lay = ops.BucketLayout(list(sizes))
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(lay.total, device=dev, generator=g) * 1e-2
    base = torch.randn(lay.total, device=dev, generator=g)
    norms = stoch.torch_norms(x, lay)
    nl, ns = stoch.packed_plane_bytes(lay.total, bits)
    p_lv, p_sb = torch.empty(nl, dtype=torch.uint8, device=dev), torch.empty(ns, dtype=torch.uint8, device=dev)
    u_lv, u_sg = torch.empty(lay.total, dtype=torch.uint8, device=dev), torch.empty(lay.total, dtype=torch.int8, device=dev)
    out_p, out_u = torch.empty(lay.total, device=dev), torch.empty(lay.total, device=dev)
    own = torch.zeros(lay.total, dtype=torch.bool)
    for o, m in zip(lay.offsets.tolist(), lay.sizes.tolist()):
        own[o:o + m] = True
    own = own.to(dev)
    legs = {
        "quantize": (lambda: stoch.quantize_packed_batched("qsgd", x, lay, bits, norms, seed=7, levels=p_lv, signbits=p_sb),
                     lambda: stoch.qsgd_quantize_batched(x, lay, bits, norms, seed=7, levels=u_lv, signs=u_sg)),
        "decode": (lambda: stoch.dequantize_packed_batched("qsgd", p_lv, p_sb, norms, lay, bits, out=out_p),
                   lambda: stoch.qsgd_decode_batched(u_lv, u_sg, norms, lay, bits, out=out_u)),
        "decode_axpby": (lambda: stoch.dequantize_axpby_packed_batched("qsgd", p_lv, p_sb, norms, lay, bits, base, out_p,
                                                                       alpha, beta),
                         lambda: stoch.dequantize_axpby_batched("qsgd", u_lv, u_sg, norms, lay, bits, base, out_u,
                                                                alpha, beta)),
    }

    def ev_ms(fn):
        def step(ev):
            junk.amax()
            if ev is not None:
                ev[0].record()
            fn()
            if ev is not None:
                ev[1].record()
        _, evs = timed(step, args.steps, args.warmup, 1, 2)
        return _median([e[0].elapsed_time(e[1]) for e in evs])

    n = int(sum(sizes))
    lvb = 1.0 if bits > 4 else 0.5
    moved = {"quantize": (4 + lvb + 0.125, 6), "decode": (lvb + 0.125 + 4, 6), "decode_axpby": (lvb + 0.125 + 8, 10)}
    res = {"tensors": len(sizes), "elements": n, "bits": bits}
    for name, (packed, unpacked) in legs.items():
        packed(), unpacked()
        torch.cuda.synchronize()
        if name == "quantize":
            lv, neg = _unpack_planes(p_lv, p_sb, lay.total, bits)
            parity = bool(torch.equal(lv[own], u_lv[own]) and torch.equal(neg[own], (u_sg < 0)[own]))
            del lv, neg
        else:
            parity = _bits_equal(out_p[own], out_u[own])
        tp, tu = [], []
        for _ in range(repeats):
            tp.append(ev_ms(packed))
            tu.append(ev_ms(unpacked))
        mp, mu = _median(tp), _median(tu)
        res[name] = {"parity": parity, "packed_ms": round(mp, 4), "unpacked_ms": round(mu, 4),
                     "packed_over_unpacked": round(mp / mu, 3), "within_1_05": bool(mp <= 1.05 * mu),
                     "packed_bytes_per_element": moved[name][0], "unpacked_bytes_per_element": moved[name][1],
                     "packed_frac_moved": round(moved[name][0] * n / (mp * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                     "unpacked_frac_moved": round(moved[name][1] * n / (mu * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
    del x, base, p_lv, p_sb, u_lv, u_sg, out_p, out_u, own

    # host to host: ADFL's own pattern (a CPU update in, a CPU payload over the wire, CPU tensors out)
    shapes = [(1, m) for m in sizes]
    upd = {f"layer{i:03d}.weight": (torch.randn(sh) * 1e-2) for i, sh in enumerate(shapes)}
    for i in range(len(sizes) if len(sizes) > 1 else 0):
        upd[f"layer{i:03d}.bias"] = torch.randn(64) * 1e-2
    chans = {"packed": PackedQSGDChannel(bits), "unpacked": QSGDChannel(bits)}
    wire = {}

    def round_trip(ch):
        c, _ = ch.on_client_send(upd)
        wire[ch.__class__.__name__] = sum(p.data.nbytes + (p.signs.nbytes if p.data.ndim > 1 or p.signs.numel() > 1 else 0)
                                          for p in c.params.values())
        return ch.on_server_receive(c)[0]

    def wall(fn, steps):
        ts = []
        for _ in range(steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return _median(ts)

    torch.manual_seed(3)
    a = round_trip(chans["packed"])
    torch.manual_seed(3)
    b = round_trip(chans["unpacked"])
    host = {"parity": list(a) == list(b) and all(_bits_equal(a[k], b[k]) for k in a)}
    del a, b
    tp, tu = [], []
    for _ in range(repeats):
        tp.append(wall(lambda: round_trip(chans["packed"]), host_steps))
        tu.append(wall(lambda: round_trip(chans["unpacked"]), host_steps))
    mp, mu = _median(tp), _median(tu)
    host.update({"packed_ms": round(mp, 3), "unpacked_ms": round(mu, 3), "packed_over_unpacked": round(mp / mu, 3),
                 "packed_faster": bool(mp < mu), "packed_wire_bytes": wire["PackedQSGDChannel"],
                 "unpacked_wire_bytes": wire["QSGDChannel"]})
    res["host_round_trip"] = host
    return res


def mode_packed_stoch(args, world, rank, dev):
    """The packed QSGD wire format (bits + 1 bits per weight) against the unpacked channel and kernels, which this
    change leaves untouched and which are therefore the baseline, timed in this process: device-resident quantize,
    decode and decode + axpby, and the host-to-host encode + decode round trip, at 8 and 4 bits, on the C3-shaped
    dict and on one 2^26-element tensor. Expectation: every device leg within 1.05 x its unpacked counterpart, the
    host round trip faster; a miss is reported as such. Written to profiles/packed_stoch/packed_stoch.json."""
    sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
    import recipes
    junk = torch.zeros(128 << 20, dtype=torch.float32, device=dev)
    eq = list(recipes.bucket_sizes("equal"))
    legs = {}
    for bits in (8, 4):
        legs[f"c3_dict_qsgd{bits}"] = _packed_stoch_leg(eq, bits, args, dev, junk, max(3, min(args.steps, 7)))
        legs[f"one_tensor_2p26_qsgd{bits}"] = _packed_stoch_leg([args.elems or 1 << 26], bits, args, dev, junk, 3)
    kernels = ("quantize", "decode", "decode_axpby")
    within = [leg[k]["within_1_05"] for leg in legs.values() for k in kernels]
    faster = [leg["host_round_trip"]["packed_faster"] for leg in legs.values()]
    line = {"mode": "packed_stoch", "metric": "QSGD 8 packed decode, C3-shaped device dict, Infinity Cache flushed",
            "unit": "ms", "value": legs["c3_dict_qsgd8"]["decode"]["packed_ms"],
            "parity": all(leg[k]["parity"] for leg in legs.values() for k in kernels + ("host_round_trip",)),
            "device_legs_within_1_05": f"{sum(within)} of {len(within)}",
            "host_round_trips_faster": f"{sum(faster)} of {len(faster)}", "steps": args.steps, "repeats": 3, **legs}
    out_dir = os.path.join(REPO, "profiles", "packed_stoch")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "packed_stoch.json"), "w") as f:
        json.dump(line, f, indent=1)
        f.write("\n")
    return line


def _receive_add_leg(sizes, args, dev, junk, repeats=3):
    """One layout of the receive_add mode. Whole call (wall, Infinity Cache read-flushed before every call):
    ch.receive_add_(c, [model]) with a device-resident model and the CPU payload a client sent, per channel.
    Kernel alone (HIP events, flushed likewise): ops.dequantize_add_batched into K = 1 and K = 4 device models.
    Every figure is `repeats` medians of args.steps calls, all listed. "digest": sha256 over the model after one
    call from a fixed start, so two commits' runs can be compared bit for bit. Only public calls."""
    import hashlib

    from adfl_amd import ops
    from adfl_amd.Channel import (CNATChannel, PackedQSGDChannel, PackedSLQChannel, QSGDChannel, RQSGDChannel,
                                  SLQChannel)
    gen = torch.Generator().manual_seed(0)
    update, start = {}, {}
    for i, n in enumerate(sizes):
        for name, shape in ((f"layer{i:03d}.weight", (1, n)), (f"layer{i:03d}.bias", (64,))):
            update[name] = torch.randn(shape, generator=gen) * 1e-2
            start[name] = torch.randn(shape, generator=gen)

    def digest(tensors):
        h = hashlib.sha256()
        for t in tensors:
            h.update(t.detach().cpu().contiguous().numpy().tobytes())
        return h.hexdigest()[:16]

    def medians(fn, sync_wall):
        out = []
        for _ in range(repeats):
            if sync_wall:
                ms = []
                for _ in range(args.steps):
                    junk.amax()   # read-flush of the Infinity Cache
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    ms.append((time.perf_counter() - t0) * 1e3)
            else:
                _, evs = timed(fn, args.steps, args.warmup, 1, 2)
                ms = [e[0].elapsed_time(e[1]) for e in evs]
            out.append(round(_median(ms), 4))
        return out

    res = {"tensors": len(sizes), "elements": int(sum(sizes))}
    channels = {"slq8": SLQChannel(8), "packed_slq4": PackedSLQChannel(4), "qsgd8": QSGDChannel(8),
                "rqsgd8": RQSGDChannel(8), "cnat8": CNATChannel(8), "packed_qsgd8": PackedQSGDChannel(8)}
    for key, ch in channels.items():
        torch.manual_seed(1)   # the stochastic encodes draw their Philox seed from torch's CPU generator
        c = ch.on_client_send(update)[0]
        model = {k: v.to(dev) for k, v in start.items()}
        ch.receive_add_(c, [model])
        leg = {"digest": digest(model.values())}
        for _ in range(args.warmup):
            ch.receive_add_(c, [model])
        leg["ms_repeats"] = medians(lambda: ch.receive_add_(c, [model]), True)
        leg["ms"] = _median(leg["ms_repeats"])
        res[f"receive_add_{key}"] = leg
        del c, model

    lay = ops.BucketLayout(list(sizes))
    x = torch.cat([update[k].reshape(-1) for k in update if update[k].ndim > 1]).to(dev)
    flat = torch.zeros(lay.total, device=dev)
    for o, n, s in zip(lay.offsets.tolist(), lay.sizes.tolist(), torch.split(x, list(sizes))):
        flat[o:o + n] = s
    q, scales = ops.encode_batched(flat, lay, 8)
    del x, flat
    for k in (1, 4):
        targets = [[start[n].reshape(-1).to(dev) for n in start if start[n].ndim > 1] for _ in range(k)]
        ops.dequantize_add_batched(q, scales, lay, targets)
        leg = {"digest": digest(t for m in targets for t in m)}

        def step(ev):
            junk.amax()
            if ev is not None:
                ev[0].record()
            ops.dequantize_add_batched(q, scales, lay, targets)
            if ev is not None:
                ev[1].record()
        leg["ms_repeats"] = medians(step, False)
        leg["ms"] = _median(leg["ms_repeats"])
        res[f"kernel_alone_k{k}"] = leg
        del targets
    return res


def mode_receive_add(args, world, rank, dev):
    """receive_add_ (decode a payload and add it into device-resident models in place) on the C3-shaped dict and on
    one 2^26-element tensor: the whole call per channel (wall) and ops.dequantize_add_batched alone (HIP events), see
    _receive_add_leg. The mode uses only public calls, so the same file measures any commit: run it from a git
    worktree of the parent commit with its own build, keep that run's JSON line, and give it to the run on this
    commit as --baseline. That run then judges every leg as the broadcast mode judges its own (this commit's median
    of repeats not above the parent's worst repeat: the margin is the parent's own spread), compares the digests,
    and writes both commits' figures to profiles/receive_add/receive_add.json."""
    sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
    import recipes
    junk = torch.zeros(128 << 20, dtype=torch.float32, device=dev)
    legs = {"c3_dict": _receive_add_leg(list(recipes.bucket_sizes("equal")), args, dev, junk),
            "one_tensor_2p26": _receive_add_leg([args.elems or 1 << 26], args, dev, junk)}
    line = {"mode": "receive_add", "metric": "SLQChannel(8).receive_add_ into one device-resident model, CPU payload, "
            "C3-shaped dict, Infinity Cache flushed", "unit": "ms", "value": legs["c3_dict"]["receive_add_slq8"]["ms"],
            "steps": args.steps, "repeats": 3, **legs}
    if not args.baseline:
        return line
    with open(args.baseline) as f:
        parent = json.loads([ln for ln in f.read().splitlines() if ln.startswith("{")][-1])
    verdicts = {}
    for layout, new in legs.items():
        for key, leg in new.items():
            if not isinstance(leg, dict):
                continue
            old = parent[layout][key]
            verdicts[f"{layout}.{key}"] = {
                "parent_ms": old["ms"], "parent_ms_repeats": old["ms_repeats"], "ms": leg["ms"],
                "ms_repeats": leg["ms_repeats"], "over_parent": round(leg["ms"] / old["ms"], 4),
                "not_above_parent_worst_repeat": bool(leg["ms"] <= max(old["ms_repeats"])),
                "same_bits_as_parent": leg["digest"] == old["digest"]}
    doc = {"mode": "receive_add", "unit": "ms", "steps": args.steps, "repeats": 3,
           "parity": all(v["same_bits_as_parent"] for v in verdicts.values()),
           "legs_not_above_parent_worst_repeat": f"{sum(v['not_above_parent_worst_repeat'] for v in verdicts.values())} "
                                                 f"of {len(verdicts)}", "legs": verdicts}
    out_dir = os.path.join(REPO, "profiles", "receive_add")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "receive_add.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return {**line, "parity": doc["parity"],
            "legs_not_above_parent_worst_repeat": doc["legs_not_above_parent_worst_repeat"]}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--serial", action="store_true", help="exchange: no side stream (quantize + all-gather in order)")
    p.add_argument("--graph", action="store_true", help="exchange: time PeerExchange.graph replays")
    p.add_argument("--layout", choices=["flat", "c3_equal", "c3_loguniform"], default="flat",
                   help="exchange: one flat update per rank, or a C3 state dict with per-tensor scales")
    p.add_argument("--mode", choices=["c3", "c5_int4", "exchange", "pcie", "channel", "channel_stoch", "stoch",
                                      "delta", "delta_stoch", "apply", "flush", "broadcast", "broadcast_stoch",
                                      "sync_delta", "receive_flush", "packed_stoch", "receive_add"],
                   required=True)
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--elems", type=int, default=0)
    p.add_argument("--packed", action="store_true")
    p.add_argument("--chunks", type=int, default=1)
    p.add_argument("--no-cpu", action="store_true", help="stoch: skip the host reference timing")
    p.add_argument("--baseline", default="", help="receive_add: the JSON line of this mode run on the parent commit")
    args = p.parse_args()
    rc = maybe_launch(args.gpus, os.path.abspath(__file__), sys.argv[1:])
    if rc is not None:
        sys.exit(rc)
    world, rank, local = dist_setup(args)
    assert world == args.gpus, (world, args.gpus)
    dev = torch.device("cuda", local)
    line = {"c3": mode_c3, "c5_int4": mode_c5_int4, "exchange": mode_exchange, "pcie": mode_pcie,
            "channel": mode_channel, "channel_stoch": mode_channel_stoch, "stoch": mode_stoch,
            "delta": mode_delta, "delta_stoch": mode_delta_stoch, "apply": mode_apply,
            "flush": mode_flush, "broadcast": mode_broadcast, "broadcast_stoch": mode_broadcast_stoch,
            "sync_delta": mode_sync_delta, "receive_flush": mode_receive_flush,
            "packed_stoch": mode_packed_stoch, "receive_add": mode_receive_add}[args.mode](
        args, world, rank, dev)
    if rank == 0:
        print(json.dumps(line), flush=True)
    if torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
