// stoch_delta.hip — MI355X (gfx950, CDNA4) kernels for the send side of a DELTA round with the stochastic
// codecs: RQSGD encode of new - prev without ever writing the difference (include/adfl_stoch.h,
// adfl_rqsgd_encode_delta_batched*). QSGD / CNAT take their scale from the torch-order L2 norm, which reads one
// flat bucket: for them the difference is written once (adfl_bucket_diff, bucket_copy.hip) and the existing
// encode runs over it. The same RQSGD kernels with UPD also leave h' = fp32(h + decode(stored bytes)) in `prev`,
// QAFeL's hidden state (adfl_rqsgd_encode_delta_update_batched*; Src/ADFL/Server/qafel.py:156-180).
//
// Reference behaviour restated here (bit-exact given the same uniforms):
//   diff    Src/ADFL/model.py:350-358            diff_parameters: params_b[k] - params_a[k] per tensor
//   encode  Src/ADFL/Channel/quant.py:364-382    max|x| norm, min|x| factor, stochastic level rounding
//
// The element source is x[e] = new_t[e - t0] - prev_t[e - t0]: one fp32 subtraction (exact IEEE, no
// contraction: the build uses -ffp-contract=off). max / min |x| are order-free, and everything downstream of
// x is stoch_codec.hip's arithmetic taken from stoch_device.h unchanged, so the planes, norms and mins are
// those of the two-step route (torch's b - a, then adfl_rqsgd_encode_batched) bit for bit. Two passes over
// both sources: 18 bytes per element (2 x 8 read, 2 written) against 8 + 4 (sub) + 4 + 4 (gather) + 4 + 4 + 2
// (two-pass encode) = 30 for the two steps; the one-launch form for buckets of small tensors reads both sources
// once: 10 bytes per element.
//
// Sources: two device pointer tables, one base pointer per tensor, addressed through the bucket's chunk
// table as slq_delta.hip does: ptrs[c.tensor] + (c.start - the tensor's first element).
//
// Alignment: the sources have no precondition. A block takes the 4-element-group path (a 16-byte load per
// source and a 4-byte store per plane and lane) when, at the chunk's head (where the planes reach a 4-byte
// boundary), both source addresses are 16-byte aligned; otherwise it goes element by element with the exact
// element rule, which gives the same bytes (block-uniform decision).
//
// Uniform index. The element at chunk-table index g of tensor t draws uniform g + ushift[t] (that Philox word,
// or that entry of the injected plane): the planes may sit in a 64-element-aligned layout while the draws stay
// those of the compact layout. ushift[t] % 4 == 0 keeps one Philox block per 4-element group (quantize_regs
// unchanged, its group index shifted); otherwise a group straddles two blocks and the lane takes the second
// from the next lane (quantize_regs_straddle). The branch is per tensor, hence block-uniform. Injected uniforms with a
// straddling shift take the element-wise path (a test hook: no 16-byte load of the plane is possible there).
//
// Cache policy: both sources are read non-temporally (dead after the second pass); plane stores allocate.

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "adfl_stoch.h"
#include "stoch_device.h"

namespace {

typedef const float* const* __restrict__ PtrTable;

struct DeltaSrc {
  const float* nw;  // the chunk's first element of `new`
  const float* pv;  // ... and of `prev`
};

__device__ __forceinline__ DeltaSrc delta_src(PtrTable nws, PtrTable pvs, const adfl_slq_chunk* __restrict__ chunks,
                                              const adfl_slq_chunk& c) {
  const int64_t off = c.start - chunks[c.first_chunk].start;
  DeltaSrc s;
  s.nw = nws[c.tensor] + off;
  s.pv = pvs[c.tensor] + off;
  return s;
}

__device__ __forceinline__ bool dev_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

__device__ __forceinline__ float ld_nt(const float* p) { return __builtin_nontemporal_load(p); }

__device__ __forceinline__ float delta1(const float* __restrict__ nw, const float* __restrict__ pv, int i) {
  return ld_nt(nw + i) - ld_nt(pv + i);
}

__device__ __forceinline__ float4 sub4(float4 a, float4 b) {
  return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w);
}

// All of a chunk's float4 groups of both sources issued before the first use (k_quantize_delta_batched's
// schedule: 64 registers of loads in flight), then subtracted into v.
__device__ __forceinline__ void load_delta_regs(const float4* __restrict__ n4p, const float4* __restrict__ p4p, int n4,
                                                float4 (&v)[kPer], int tg = threadIdx.x) {
  float4 b[kPer];
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int k = tg + j * kBlock;
    if (k < n4) v[j] = load4_nt(n4p + k);
  }
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int k = tg + j * kBlock;
    if (k < n4) b[j] = load4_nt(p4p + k);
  }
#pragma unroll
  for (int j = 0; j < kPer; ++j)
    if (tg + j * kBlock < n4) v[j] = sub4(v[j], b[j]);
}

// Pass 1: one {max, min} |new - prev| bit pair per chunk (NaN patterns compare above inf, so a NaN wins the
// max and the finalize turns both outputs into NaN), in the 8-byte slots k_norm_finalize<ADFL_NORM_LINF> reads.
// The planes are not touched here: the float4 path needs only both sources 16-byte aligned at the same element.
__global__ __launch_bounds__(kBlock) void k_maxmin_delta_partials(PtrTable nws, PtrTable pvs,
                                                                  const adfl_slq_chunk* __restrict__ chunks,
                                                                  uint2* __restrict__ partials) {
  const adfl_slq_chunk c = chunks[blockIdx.x];
  const DeltaSrc s = delta_src(nws, pvs, chunks, c);
  const int tid = (int)threadIdx.x;
  uint32_t mx = 0u, mn = 0xffffffffu;
  if (((reinterpret_cast<uintptr_t>(s.nw) ^ reinterpret_cast<uintptr_t>(s.pv)) & 15u) == 0) {  // block-uniform
    const int h = (int)(((16u - (reinterpret_cast<uintptr_t>(s.nw) & 15u)) & 15u) >> 2);
    const int head = h < c.len ? h : c.len;
    const int n4 = (c.len - head) >> 2;
    float4 v[kPer];
    load_delta_regs(reinterpret_cast<const float4*>(s.nw + head), reinterpret_cast<const float4*>(s.pv + head), n4, v);
    const int i = edge_elem(head, head + (n4 << 2), c.len);
    if (i >= 0) mx = mn = abs_bits(delta1(s.nw, s.pv, i));
#pragma unroll
    for (int j = 0; j < kPer; ++j)
      if (tid + j * kBlock < n4) {
        const uint32_t a = abs_bits(v[j].x), b = abs_bits(v[j].y), d = abs_bits(v[j].z), e = abs_bits(v[j].w);
        mx = max(mx, max(max(a, b), max(d, e)));
        mn = min(mn, min(min(a, b), min(d, e)));
      }
  } else {
    for (int i = tid; i < c.len; i += kBlock) {
      const uint32_t a = abs_bits(delta1(s.nw, s.pv, i));
      mx = max(mx, a);
      mn = min(mn, a);
    }
  }
  const uint2 r = block_maxmin(mx, mn);
  if (tid == 0) partials[blockIdx.x] = r;
}

struct NoAcc {
  __device__ __forceinline__ void add4(float4) {}
};

// quantize_regs for a tensor whose uniform index is not a multiple of 4 at its 4-element groups: element e of
// the group at uniform index u0 + 4k (u0 % 4 = p in 1..3) draws word (p + e) % 4 of Philox block
// (u0 + 4k) / 4 + (p + e) / 4: words p..3 of the group's own block `a` and words 0..p-1 of the next block `b`.
// Same element rules, ballot and stores as quantize_regs; Philox uniforms only. Two forms of getting `b`:
//  * both blocks made by the lane (PB groups = 2 PB interleaved chains per batch);
//  * ADFL_STRADDLE_NEIGHBOUR: `b` of group k is `a` of group k + 1, the next lane's — three cross-lane moves per
//    group; a wave's last lane has no next lane, so lanes 0 .. kPer - 1 make, in one more chain per chunk, the
//    block after the wave's last group for each of the chunk's kPer rows (9 chains per chunk instead of 16).
// Measured A/B on C3 (tools/build_variant.py -DADFL_STRADDLE_NEIGHBOUR=0 against the product, alternating runs of
// tools/bench_configs.py --mode delta_stoch; profiles/delta/straddle_ab.json): the neighbour's block is faster
// in every leg — two passes 58.9 against 64.5 us (equal layout) and 83.0 against 89.9 us (log-uniform), one launch
// 54.2 against 55.5 us — so it is the product; the other form stays behind the switch. (In this form the compiler
// places 64 bytes per thread in LDS, 16 KiB per 256-thread block and 64 KiB per resident block: within the CU's
// 160 KiB at the kernels' register-bound occupancy of 5 and 4 waves per SIMD, and part of what was measured.)
#ifndef ADFL_STRADDLE_NEIGHBOUR
#define ADFL_STRADDLE_NEIGHBOUR 1
#endif
constexpr bool kStraddleNeighbour = ADFL_STRADDLE_NEIGHBOUR != 0;

template <class F, class E, class P>
__device__ __forceinline__ void straddle_group(const float4& vj, const uint4& a, const uint4& b, int p, int j, int k,
                                               bool live, uint32_t* __restrict__ l4, uint32_t* __restrict__ s4, F fast,
                                               E exact, bool all_exact, P post) {
  const float4 uj = make_float4(u24(p == 1 ? a.y : p == 2 ? a.z : a.w), u24(p == 1 ? a.z : p == 2 ? a.w : b.x),
                                u24(p == 1 ? a.w : p == 2 ? b.x : b.y), u24(p == 1 ? b.x : p == 2 ? b.y : b.z));
  bool bad = all_exact;
  uint32_t q = pack4(fast(vj.x, uj.x, bad), fast(vj.y, uj.y, bad), fast(vj.z, uj.z, bad), fast(vj.w, uj.w, bad));
  if (wave_any(bad && live))
    q = pack4(exact(vj.x, uj.x), exact(vj.y, uj.y), exact(vj.z, uj.z), exact(vj.w, uj.w));
  if (live) {
    l4[k] = q;
    s4[k] = pack4(sign_byte(vj.x), sign_byte(vj.y), sign_byte(vj.z), sign_byte(vj.w));
  }
  post(j, k, live, q);  // every lane (quantize_regs' hook)
}

template <int PB, class F, class E, class P = NoPost>
__device__ __forceinline__ void quantize_regs_straddle(const float4 (&v)[kPer], int tg, int n4, int64_t u0,
                                                       const Uniforms& U, uint32_t* __restrict__ l4,
                                                       uint32_t* __restrict__ s4, F fast, E exact, bool all_exact,
                                                       P post = P{}) {
  static_assert(kPer % PB == 0, "batches tile a chunk's groups");
  const int p = (int)(u0 & 3);  // block-uniform
  if (kStraddleNeighbour) {
    static_assert(kPer <= 64, "one lane per row makes the wave's extra block");
    const int lane = tg & 63;
    uint4 extra;  // lane r < kPer: the block after the wave's last group of row r
    {
      const uint64_t c1[1] = {U.counter + (uint64_t)((u0 >> 2) + (tg - lane) + 64 + (lane % kPer) * kBlock)};
      uint4 w1[1];
      philox4x32_batch(c1, U.seed, w1);
      extra = w1[0];
    }
#pragma unroll
    for (int jb = 0; jb < kPer; jb += 2 * PB) {  // 2 PB groups per batch: as many chains as the other form
      if (jb * kBlock >= n4) break;  // group-uniform
      uint64_t ctr[2 * PB];
      uint4 w[2 * PB];
#pragma unroll
      for (int i = 0; i < 2 * PB; ++i) ctr[i] = U.counter + (uint64_t)((u0 >> 2) + tg + (jb + i) * kBlock);
      philox4x32_batch(ctr, U.seed, w);
#pragma unroll
      for (int i = 0; i < 2 * PB; ++i) {
        const int j = jb + i;
        const int k = tg + j * kBlock;
        if (j * kBlock >= n4) break;  // group-uniform
        const bool last = lane == 63;
        // every cross-lane move is made by the whole wave, then selected: a move inside a lane-dependent branch
        // would read lanes that are switched off there
        const uint32_t nx = __shfl_down(w[i].x, 1, 64), ny = __shfl_down(w[i].y, 1, 64), nz = __shfl_down(w[i].z, 1, 64);
        const uint32_t ex = __shfl(extra.x, j, 64), ey = __shfl(extra.y, j, 64), ez = __shfl(extra.z, j, 64);
        const uint4 b = make_uint4(last ? ex : nx, last ? ey : ny, last ? ez : nz, 0u);  // word 3 is never drawn (p <= 3)
        straddle_group(v[j], w[i], b, p, j, k, k < n4, l4, s4, fast, exact, all_exact, post);
      }
    }
    return;
  }
#pragma unroll
  for (int jb = 0; jb < kPer; jb += PB) {
    if (jb * kBlock >= n4) break;  // group-uniform
    uint64_t ctr[2 * PB];
    uint4 w[2 * PB];
#pragma unroll
    for (int i = 0; i < PB; ++i) {
      ctr[2 * i] = U.counter + (uint64_t)((u0 >> 2) + tg + (jb + i) * kBlock);
      ctr[2 * i + 1] = ctr[2 * i] + 1;
    }
    philox4x32_batch(ctr, U.seed, w);
#pragma unroll
    for (int i = 0; i < PB; ++i) {
      const int j = jb + i;
      if (j * kBlock >= n4) break;  // group-uniform
      const int k = tg + j * kBlock;
      straddle_group(v[j], w[2 * i], w[2 * i + 1], p, j, k, k < n4, l4, s4, fast, exact, all_exact, post);
    }
  }
}

constexpr int kPbDelta = 4;          // Philox blocks per batch, as k_qsgd_quantize's kPbQuantize
constexpr int kPbDeltaStraddle = 2;  // groups per batch on the straddling path (4 chains as well)

// Pass 2: the two sources again, levels and signs from the finalized max / min. norm == 0 (every difference
// +-0) gives the reference's zero branch, levels 0 and signs 1 (quant.py:368-369).
//
// UPD (QAFeL's broadcast, Src/ADFL/Server/qafel.py:156-180): `prev` is the server's hidden state h, and the pass
// also leaves h' = fp32(h + d) in place, d being k_stoch_dequantize<1>'s decode (decode4 / decode_exact) of the
// level and sign bytes this thread has just stored, under the finalized max and min: what on_client_receive then
// add_parameters_inpace(h, d, 1, 1) leave. A zero norm decodes to +0, which is still added (-0 becomes +0).
// Holding h's groups from the difference's loads to the store costs 31 VGPRs and an occupancy step (124 VGPRs, 4
// waves per SIMD against 5), so a group of h is re-read where it is updated, by the thread that read it for the
// difference, and an edge element is read before the quantize: every element of h is read for the last time before
// the same thread writes it.
template <bool UPD>
__global__ __launch_bounds__(kBlock) void k_rqsgd_quantize_delta(PtrTable nws, PtrTable pvs,
                                                                 const adfl_slq_chunk* __restrict__ chunks, float s,
                                                                 const float* __restrict__ norms,
                                                                 const float* __restrict__ mins,
                                                                 const int64_t* __restrict__ ushift, Uniforms U,
                                                                 uint8_t* __restrict__ levels,
                                                                 int8_t* __restrict__ signs) {
  const adfl_slq_chunk c = chunks[blockIdx.x];
  const float norm = norms[c.tensor];
  uint8_t* lv = levels + c.start;
  int8_t* sg = signs + c.start;
  const DeltaSrc src = delta_src(nws, pvs, chunks, c);
  float* hw = const_cast<float*>(src.pv);  // UPD: the hidden tensor's chunk, written in place
  const int tid = (int)threadIdx.x;
  if (norm == 0.0f) {
    fill_zero_norm(lv, sg, c.len);
    if (UPD)
      for (int i = tid; i < c.len; i += kBlock) hw[i] = hw[i] + 0.0f;
    return;
  }
  const float mn = UPD ? mins[c.tensor] : 0.0f;
  const int64_t ug = c.start + (ushift ? ushift[c.tensor] : 0);  // the chunk's first uniform index (>= 0)
  const Div d = make_div(norm);
  const Div ds = make_div(s);  // the decode divides by the level count
  const auto fast = [&](float xv, float uv, bool& bad) { return qsgd_level_fast(xv, s, d, uv, bad); };
  const auto exact = [&](float xv, float uv) { return qsgd_level_exact(xv, s, norm, uv); };
  const int head = chunk_head4(c.start, c.len);
  const int phase = (int)((ug + head) & 3);
  if (!(dev_aligned16(src.nw + head) && dev_aligned16(src.pv + head)) || (U.inj && phase)) {  // block-uniform
    for (int i = tid; i < c.len; i += kBlock) {
      const float h = ld_nt(src.pv + i);
      const float x = ld_nt(src.nw + i) - h;
      const uint32_t l = exact(x, U.one(ug + i)), g = sign_byte(x);
      lv[i] = (uint8_t)l;
      sg[i] = (int8_t)g;
      if (UPD) hw[i] = h + decode_exact<1>(l, g, norm, mn, s);
    }
    return;
  }
  const int n4 = (c.len - head) >> 2;
  float4 v[kPer];
  load_delta_regs(reinterpret_cast<const float4*>(src.nw + head), reinterpret_cast<const float4*>(src.pv + head), n4, v);
  const int i = edge_elem(head, head + (n4 << 2), c.len);
  const float eh = i >= 0 ? ld_nt(src.pv + i) : 0.0f;
  const float ev = i >= 0 ? ld_nt(src.nw + i) - eh : 0.0f;
  uint32_t* l4 = reinterpret_cast<uint32_t*>(lv + head);
  uint32_t* s4 = reinterpret_cast<uint32_t*>(sg + head);
  const auto update = [&](int j, int k, bool live, uint32_t q) {  // every lane: decode4 holds a ballot
    const float4 dv = decode4<1>(q, sign4(v[j]), norm, mn, ds, s, live);
    if (live) store_sum_h4(hw + head + 4 * k, true, load_h4(hw + head + 4 * k, true), dv);
  };
  if (UPD) {
    if (phase == 0)
      quantize_regs<kPbDelta>(v, tid, n4, ug + head, U, l4, s4, fast, exact, !d.fast, (NoAcc*)nullptr, nullptr, 0,
                              update);
    else
      quantize_regs_straddle<kPbDeltaStraddle>(v, tid, n4, ug + head, U, l4, s4, fast, exact, !d.fast, update);
  } else {
    if (phase == 0)
      quantize_regs<kPbDelta>(v, tid, n4, ug + head, U, l4, s4, fast, exact, !d.fast, (NoAcc*)nullptr);
    else
      quantize_regs_straddle<kPbDeltaStraddle>(v, tid, n4, ug + head, U, l4, s4, fast, exact, !d.fast);
  }
  if (i >= 0) {
    const uint32_t l = exact(ev, U.one(ug + i)), g = sign_byte(ev);
    lv[i] = (uint8_t)l;
    sg[i] = (int8_t)g;
    if (UPD) hw[i] = eh + decode_exact<1>(l, g, norm, mn, s);
  }
}

// ---- one launch for a bucket of small tensors (a whole tensor per 1024-thread block) -----------------------
// k_qsgd_encode_resident<ADFL_NORM_LINF>'s walk over the work list of adfl_slq_build_encode_work with two
// sources: 4 groups of 256 threads, group g takes chunks g and g + 4, the difference held in VGPRs (16 float4
// per lane) between the block's max / min reduction and the quantize: both sources read once, 10 bytes per
// element. A 1024-thread block has 128 VGPRs per lane, so the loads go in two stages (one chunk of both
// sources each: 64 registers in flight), each subtracted into the difference's registers as it lands — the
// scheme of k_encode_delta_resident. No LDS Philox prefetch: the words are made after the reduction.
// The alignment and the uniform phase are the tensor's (every chunk of a tensor starts 8192 elements after the
// last): block-uniform. Element-wise path: the sources are read twice, for the max / min and for the levels.
constexpr int kResBlock = 1024;
constexpr int kResGroups = kResBlock / kBlock;                              // 4
constexpr int kResPerGroup = ADFL_SLQ_DELTA_RESIDENT_CHUNKS / kResGroups;  // 2
constexpr int kResWaves = kResBlock / 64;
static_assert(kResPerGroup * kResGroups == ADFL_SLQ_DELTA_RESIDENT_CHUNKS, "groups cover a resident tensor");
constexpr int kPbDeltaResident = 2;  // Philox blocks per batch: the registers hold two chunks per lane

__device__ __forceinline__ uint2 block_maxmin_res(uint32_t mx, uint32_t mn, uint32_t* red_mx, uint32_t* red_mn) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mx = max(mx, (uint32_t)__shfl_xor((int)mx, o, 64));
    mn = min(mn, (uint32_t)__shfl_xor((int)mn, o, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    red_mx[threadIdx.x >> 6] = mx;
    red_mn[threadIdx.x >> 6] = mn;
  }
  __syncthreads();
  mx = red_mx[0];
  mn = red_mn[0];
#pragma unroll
  for (int w = 1; w < kResWaves; ++w) {
    mx = max(mx, red_mx[w]);
    mn = min(mn, red_mn[w]);
  }
  return make_uint2(mx, mn);
}

//
// UPD: k_rqsgd_quantize_delta<true>'s update in the one launch. The difference fills the registers (124 VGPRs), so
// a stage re-reads its groups of h after quantizing them and stores h' = fp32(h + d): the thread that writes a
// group is the one that read it for the difference, after the block's reduction (every read for the max / min
// precedes every write), and an edge element's h is re-read by the thread that holds its difference.
template <bool UPD>
__global__ __launch_bounds__(kResBlock) void k_rqsgd_encode_delta_resident(
    PtrTable nws, PtrTable pvs, const adfl_slq_chunk* __restrict__ chunks, const int32_t* __restrict__ work, float lev,
    const int64_t* __restrict__ ushift, Uniforms U, uint8_t* __restrict__ levels, int8_t* __restrict__ signs,
    float* __restrict__ norms, float* __restrict__ mins) {
  __shared__ uint32_t red_mx[kResWaves], red_mn[kResWaves];
  const int64_t ci = work[blockIdx.x];
  const adfl_slq_chunk ct = chunks[ci];
  if (ct.nchunks > ADFL_SLQ_DELTA_RESIDENT_CHUNKS) {  // not a resident work list: NaN norm and min, nothing written
    if (threadIdx.x == 0) norms[ct.tensor] = mins[ct.tensor] = __builtin_nanf("");
    return;
  }
  const int grp = __builtin_amdgcn_readfirstlane(threadIdx.x / kBlock);
  const int tg = threadIdx.x % kBlock;
  const float* nw = nws[ct.tensor];  // ci is the tensor's first chunk
  const float* pv = pvs[ct.tensor];
  float* hw = const_cast<float*>(pv);  // UPD: the hidden tensor, written in place
  const int64_t ut = ct.start + (ushift ? ushift[ct.tensor] : 0);  // the tensor's first uniform index (>= 0)
  const int head0 = (int)((4 - (ct.start & 3)) & 3);                // every chunk's head (its len permitting)
  const int phase = (int)((ut + head0) & 3);
  uint32_t mx = 0u, mi = 0xffffffffu;
  if (!(dev_aligned16(nw + head0) && dev_aligned16(pv + head0)) || (U.inj && phase)) {  // block-uniform
    const int len = (ct.nchunks - 1) * ADFL_SLQ_CHUNK_ELEMS + chunks[ci + ct.nchunks - 1].len;
    for (int i = threadIdx.x; i < len; i += kResBlock) {
      const uint32_t a = abs_bits(delta1(nw, pv, i));
      mx = max(mx, a);
      mi = min(mi, a);
    }
    const uint2 r = block_maxmin_res(mx, mi, red_mx, red_mn);
    const bool nan = r.x > 0x7f800000u;
    const float norm = nan ? __builtin_nanf("") : __uint_as_float(r.x);
    const float mn = nan ? __builtin_nanf("") : __uint_as_float(r.y);
    if (threadIdx.x == 0) {
      norms[ct.tensor] = norm;
      mins[ct.tensor] = mn;
    }
    uint8_t* lv = levels + ct.start;
    int8_t* sg = signs + ct.start;
    for (int i = threadIdx.x; i < len; i += kResBlock) {  // the indices this thread read above
      if (norm == 0.0f) {
        lv[i] = 0;
        sg[i] = 1;
        if (UPD) hw[i] = hw[i] + 0.0f;
      } else {
        const float h = pv[i];
        const float x = nw[i] - h;
        const uint32_t l = qsgd_level_exact(x, lev, norm, U.one(ut + i)), g = sign_byte(x);
        lv[i] = (uint8_t)l;
        sg[i] = (int8_t)g;
        if (UPD) hw[i] = h + decode_exact<1>(l, g, norm, mn, lev);
      }
    }
    return;
  }
  float4 v[kResPerGroup][kPer];
  float ev[kResPerGroup];
  int ei[kResPerGroup], n4s[kResPerGroup];
#pragma unroll
  for (int r = 0; r < kResPerGroup; ++r) {  // one stage per chunk: both sources' loads, then the subtraction
    const int kc = grp + r * kResGroups;
    ei[r] = -1;
    n4s[r] = 0;
    ev[r] = 0.0f;
    if (kc < ct.nchunks) {  // group-uniform
      const adfl_slq_chunk c = chunks[ci + kc];
      const int off = (int)(c.start - ct.start);
      const int head = chunk_head4(c.start, c.len);
      n4s[r] = (c.len - head) >> 2;
      ei[r] = edge_elem_t(tg, head, head + (n4s[r] << 2), c.len);
      const float en = ei[r] >= 0 ? ld_nt(nw + off + ei[r]) : 0.0f, ep = ei[r] >= 0 ? ld_nt(pv + off + ei[r]) : 0.0f;
      load_delta_regs(reinterpret_cast<const float4*>(nw + off + head), reinterpret_cast<const float4*>(pv + off + head),
                      n4s[r], v[r], tg);
      ev[r] = en - ep;
    }
  }
#pragma unroll
  for (int r = 0; r < kResPerGroup; ++r) {
    if (ei[r] >= 0) {
      mx = max(mx, abs_bits(ev[r]));
      mi = min(mi, abs_bits(ev[r]));
    }
#pragma unroll
    for (int j = 0; j < kPer; ++j)
      if (tg + j * kBlock < n4s[r]) {
        const float4 a = v[r][j];
        mx = max(mx, max(max(abs_bits(a.x), abs_bits(a.y)), max(abs_bits(a.z), abs_bits(a.w))));
        mi = min(mi, min(min(abs_bits(a.x), abs_bits(a.y)), min(abs_bits(a.z), abs_bits(a.w))));
      }
  }
  const uint2 red = block_maxmin_res(mx, mi, red_mx, red_mn);
  const bool nan = red.x > 0x7f800000u;
  const float norm = nan ? __builtin_nanf("") : __uint_as_float(red.x);
  const float mn = nan ? __builtin_nanf("") : __uint_as_float(red.y);
  if (threadIdx.x == 0) {
    norms[ct.tensor] = norm;
    mins[ct.tensor] = mn;
  }
  const Div d = make_div(norm);
  const Div ds = make_div(lev);  // the decode divides by the level count
  const auto fast = [&](float xv, float uv, bool& bad) { return qsgd_level_fast(xv, lev, d, uv, bad); };
  const auto exact = [&](float xv, float uv) { return qsgd_level_exact(xv, lev, norm, uv); };
  // Stage r's quantize with r a compile-time constant: as a loop over r the compiler declined to unroll this body
  // and indexed v dynamically, which put the 64 registers of the difference in scratch (288 bytes per lane).
  const auto quantize_stage = [&](auto stage) {
    constexpr int r = decltype(stage)::value;
    const int kc = grp + r * kResGroups;
    if (kc >= ct.nchunks) return;  // group-uniform
    const adfl_slq_chunk c = chunks[ci + kc];
    uint8_t* lv = levels + c.start;
    int8_t* sg = signs + c.start;
    float* hc = hw + (c.start - ct.start);
    if (norm == 0.0f) {
      fill_zero_norm(lv, sg, c.len, tg);
      if (UPD)
        for (int i = tg; i < c.len; i += kBlock) hc[i] = hc[i] + 0.0f;
      return;
    }
    const int head = chunk_head4(c.start, c.len);
    const int64_t ug = ut + (c.start - ct.start);
    uint32_t* l4 = reinterpret_cast<uint32_t*>(lv + head);
    uint32_t* s4 = reinterpret_cast<uint32_t*>(sg + head);
    const auto update = [&](int j, int k, bool live, uint32_t q) {  // every lane: decode4 holds a ballot
      const float4 dv = decode4<1>(q, sign4(v[r][j]), norm, mn, ds, lev, live);
      if (live) store_sum_h4(hc + head + 4 * k, true, load_h4(hc + head + 4 * k, true), dv);
    };
    if (UPD) {
      if (phase == 0)
        quantize_regs<kPbDeltaResident>(v[r], tg, n4s[r], ug + head, U, l4, s4, fast, exact, !d.fast, (NoAcc*)nullptr,
                                        nullptr, 0, update);
      else
        quantize_regs_straddle<kPbDeltaResident / 2>(v[r], tg, n4s[r], ug + head, U, l4, s4, fast, exact, !d.fast,
                                                     update);
    } else {
      if (phase == 0)
        quantize_regs<kPbDeltaResident>(v[r], tg, n4s[r], ug + head, U, l4, s4, fast, exact, !d.fast, (NoAcc*)nullptr);
      else
        quantize_regs_straddle<kPbDeltaResident / 2>(v[r], tg, n4s[r], ug + head, U, l4, s4, fast, exact, !d.fast);
    }
    if (ei[r] >= 0) {
      const uint32_t l = exact(ev[r], U.one(ug + ei[r])), g = sign_byte(ev[r]);
      lv[ei[r]] = (uint8_t)l;
      sg[ei[r]] = (int8_t)g;
      if (UPD) hc[ei[r]] = hc[ei[r]] + decode_exact<1>(l, g, norm, mn, lev);
    }
  };
  static_assert(kResPerGroup == 2, "two stages");
  quantize_stage(std::integral_constant<int, 0>{});
  quantize_stage(std::integral_constant<int, 1>{});
}

// ------------------------------------------------------------------------------------------------
// host helpers
// ------------------------------------------------------------------------------------------------
inline bool host_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

inline int launch_status() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? ADFL_OK : (int)e;
}

// The delta entries' argument checks, in the order of the non-delta RQSGD entries: null pointers and counts
// (ADFL_E_ARG), bits (ADFL_E_BITS), the workspace (ADFL_E_ARG / ADFL_E_ALIGN / ADFL_E_WORKSPACE), then the
// 16-byte alignment of the plane and uniform bases (ADFL_E_ALIGN).
inline int check_delta_args(const void* d_new, const void* d_prev, const void* d_chunks, int64_t nchunks, int bits,
                            const void* d_uniforms, const void* d_ws, int64_t ws_bytes, const void* d_levels,
                            const void* d_signs, const void* d_norms, const void* d_mins) {
  if (!d_new || !d_prev || !d_chunks || !d_levels || !d_signs || !d_norms || !d_mins || nchunks < 1 ||
      nchunks > INT32_MAX)
    return ADFL_E_ARG;
  if (bits < 1 || bits > 16) return ADFL_E_BITS;
  if (!d_ws) return ADFL_E_ARG;
  if (!host_aligned16(d_ws)) return ADFL_E_ALIGN;
  if (ws_bytes < nchunks * kPartialBytes) return ADFL_E_WORKSPACE;
  if (!host_aligned16(d_levels) || !host_aligned16(d_signs) || (d_uniforms && !host_aligned16(d_uniforms)))
    return ADFL_E_ALIGN;
  return ADFL_OK;
}

// The two passes and the one launch, without (UPD false: d_prev is read only) or with the hidden-state update.
template <bool UPD>
int rqsgd_delta_twopass(const float* const* d_new, const float* const* d_prev, const adfl_slq_chunk* d_chunks,
                        int64_t nchunks, int bits, const float* d_uniforms, const int64_t* d_ushift, uint64_t seed,
                        uint64_t counter, void* d_workspace, int64_t workspace_bytes, uint8_t* d_levels,
                        int8_t* d_signs, float* d_norms, float* d_mins, void* stream) {
  if (int s = check_delta_args(d_new, d_prev, d_chunks, nchunks, bits, d_uniforms, d_workspace, workspace_bytes,
                               d_levels, d_signs, d_norms, d_mins))
    return s;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)nchunks), block(kBlock);
  hipLaunchKernelGGL(k_maxmin_delta_partials, grid, block, 0, st, d_new, d_prev, d_chunks,
                     reinterpret_cast<uint2*>(d_workspace));
  if (int s = launch_status()) return s;
  if (int s = adfl_stoch_detail::launch_finalize_linf(d_chunks, nchunks, d_workspace, d_norms, d_mins, st)) return s;
  const Uniforms U{d_uniforms, seed, counter};
  hipLaunchKernelGGL(k_rqsgd_quantize_delta<UPD>, grid, block, 0, st, d_new, d_prev, d_chunks,
                     (float)((1LL << bits) - 1), (const float*)d_norms, (const float*)d_mins, d_ushift, U, d_levels,
                     d_signs);
  return launch_status();
}

template <bool UPD>
int rqsgd_delta_work(const float* const* d_new, const float* const* d_prev, const adfl_slq_chunk* d_chunks,
                     int64_t nchunks, const int32_t* d_work, int64_t nwork, int bits, const float* d_uniforms,
                     const int64_t* d_ushift, uint64_t seed, uint64_t counter, void* d_workspace,
                     int64_t workspace_bytes, uint8_t* d_levels, int8_t* d_signs, float* d_norms, float* d_mins,
                     void* stream) {
  if (nwork == 0)
    return rqsgd_delta_twopass<UPD>(d_new, d_prev, d_chunks, nchunks, bits, d_uniforms, d_ushift, seed, counter,
                                    d_workspace, workspace_bytes, d_levels, d_signs, d_norms, d_mins, stream);
  if (!d_work || nwork < 0 || nwork > nchunks) return ADFL_E_ARG;
  if (int s = check_delta_args(d_new, d_prev, d_chunks, nchunks, bits, d_uniforms, d_workspace, workspace_bytes,
                               d_levels, d_signs, d_norms, d_mins))
    return s;
  const Uniforms U{d_uniforms, seed, counter};
  hipLaunchKernelGGL(k_rqsgd_encode_delta_resident<UPD>, dim3((unsigned)nwork), dim3(kResBlock), 0,
                     (hipStream_t)stream, d_new, d_prev, d_chunks, d_work, (float)((1LL << bits) - 1), d_ushift, U, d_levels,
                     d_signs, d_norms, d_mins);
  return launch_status();
}

}  // namespace

extern "C" {

int adfl_rqsgd_encode_delta_batched(const float* const* d_new, const float* const* d_prev,
                                    const adfl_slq_chunk* d_chunks, int64_t nchunks, int bits,
                                    const float* d_uniforms, const int64_t* d_ushift, uint64_t seed, uint64_t counter,
                                    void* d_workspace, int64_t workspace_bytes, uint8_t* d_levels, int8_t* d_signs,
                                    float* d_norms, float* d_mins, void* stream) {
  return rqsgd_delta_twopass<false>(d_new, d_prev, d_chunks, nchunks, bits, d_uniforms, d_ushift, seed, counter,
                                    d_workspace, workspace_bytes, d_levels, d_signs, d_norms, d_mins, stream);
}

int adfl_rqsgd_encode_delta_batched_work(const float* const* d_new, const float* const* d_prev,
                                         const adfl_slq_chunk* d_chunks, int64_t nchunks, const int32_t* d_work,
                                         int64_t nwork, int bits, const float* d_uniforms, const int64_t* d_ushift,
                                         uint64_t seed, uint64_t counter, void* d_workspace, int64_t workspace_bytes,
                                         uint8_t* d_levels, int8_t* d_signs, float* d_norms, float* d_mins,
                                         void* stream) {
  return rqsgd_delta_work<false>(d_new, d_prev, d_chunks, nchunks, d_work, nwork, bits, d_uniforms, d_ushift, seed,
                                 counter, d_workspace, workspace_bytes, d_levels, d_signs, d_norms, d_mins, stream);
}

// The same encodes with d_hidden in prev's place, updated in place: h' = fp32(h + decode(stored bytes)).
int adfl_rqsgd_encode_delta_update_batched(const float* const* d_new, float* const* d_hidden,
                                           const adfl_slq_chunk* d_chunks, int64_t nchunks, int bits,
                                           const float* d_uniforms, const int64_t* d_ushift, uint64_t seed,
                                           uint64_t counter, void* d_workspace, int64_t workspace_bytes,
                                           uint8_t* d_levels, int8_t* d_signs, float* d_norms, float* d_mins,
                                           void* stream) {
  return rqsgd_delta_twopass<true>(d_new, d_hidden, d_chunks, nchunks, bits, d_uniforms, d_ushift, seed, counter,
                                   d_workspace, workspace_bytes, d_levels, d_signs, d_norms, d_mins, stream);
}

int adfl_rqsgd_encode_delta_update_batched_work(const float* const* d_new, float* const* d_hidden,
                                                const adfl_slq_chunk* d_chunks, int64_t nchunks, const int32_t* d_work,
                                                int64_t nwork, int bits, const float* d_uniforms,
                                                const int64_t* d_ushift, uint64_t seed, uint64_t counter,
                                                void* d_workspace, int64_t workspace_bytes, uint8_t* d_levels,
                                                int8_t* d_signs, float* d_norms, float* d_mins, void* stream) {
  return rqsgd_delta_work<true>(d_new, d_hidden, d_chunks, nchunks, d_work, nwork, bits, d_uniforms, d_ushift, seed,
                                counter, d_workspace, workspace_bytes, d_levels, d_signs, d_norms, d_mins, stream);
}

}  // extern "C"
