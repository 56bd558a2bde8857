// slq_delta.hip — MI355X (gfx950, CDNA4) kernels for the send side of a DELTA round: SLQ encode of
// new - prev without ever writing the difference (include/adfl_slq.h, adfl_slq_encode_delta_batched*), and
// QAFeL's broadcast, the same encode fused with the hidden-state update (adfl_slq_encode_delta_update_batched*;
// its section below states the arithmetic and the in-place invariant).
//
// Reference behaviour restated here (bit-exact, pinned by tests/golden/delta_small.npz):
//   diff    Src/ADFL/model.py:350-358          diff_parameters: params_b[k] - params_a[k] per tensor
//   encode  Src/ADFL/Channel/quant.py:74-104   per-tensor scale = max|x| / q_max ; quantize_per_tensor
//   callers Src/ADFL/Client/async_sc.py:106-114,318-324 (clients), Src/ADFL/Server/qafel.py:160-161
//
// The element source is x[e] = new_t[e - t0] - prev_t[e - t0]: one fp32 subtraction (exact IEEE, no
// contraction: the build uses -ffp-contract=off). Everything downstream of x is slq_codec.hip's arithmetic,
// taken from slq_device.h unchanged, so the payload and scales are those of the two-step route
// (torch's b - a, then adfl_slq_encode_batched) bit for bit. Per element the two-step route moves 25 bytes
// (sub 8 + 4, gather 4 + 4, resident encode 4 + 1); this one 9 (read new, read prev, write the payload).
//
// Sources: two device pointer tables, one base pointer per tensor, addressed through the bucket's chunk
// table as bucket_copy.hip does: ptrs[c.tensor] + (c.start - the tensor's first element). Two flat buckets
// are the case ptr[t] = base + offset[t]. The payload and scales go to a bucket at the layout's offsets.
//
// Alignment: the sources have no precondition. The 16-byte-per-lane wave-tile path needs, at the element where
// the payload reaches a 16-byte boundary, both source addresses 16-byte aligned; each block decides this from
// the three addresses (block-uniform, as k_bucket_copy decides its word size) and otherwise takes an
// element-wise path with the same results.
//
// Cache policy: both sources are read non-temporally (dead after the read); payload stores allocate (the
// decode or the scatter that follows reads them from the Infinity Cache), as measured for k_encode_resident.

#include <hip/hip_runtime.h>

#include <cstdint>

#include "adfl_slq.h"
#include "slq_device.h"

namespace {

constexpr int kDeltaSegChunks = ADFL_SLQ_DELTA_RESIDENT_CHUNKS;
static_assert(kDeltaSegChunks >= 1 && kDeltaSegChunks <= kSegChunks, "the delta resident form walks the resident work list");

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

// x[i] of the chunk / tensor whose sources start at nw, pv
__device__ __forceinline__ float delta1(const float* __restrict__ nw, const float* __restrict__ pv, int i) {
  return ld_nt(nw + i) - ld_nt(pv + i);
}

__device__ __forceinline__ float4 sub4(float4 a, float4 b) {
  return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w);
}

__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// ------------------------------------------------------------------------------------------------
// two passes, any layout (one 256-thread block per chunk)
// ------------------------------------------------------------------------------------------------
// Pass 1: one max|new - prev| partial per chunk, all of the chunk's loads of both sources in flight. The
// float4 path needs only the two sources at the same phase mod 16 bytes (the payload is not touched here).
__global__ __launch_bounds__(kBlock) void k_absmax_delta_batched(PtrTable nws, PtrTable pvs,
                                                                 const adfl_slq_chunk* __restrict__ chunks,
                                                                 uint32_t* __restrict__ partials) {
  const adfl_slq_chunk c = chunks[blockIdx.x];
  const DeltaSrc s = delta_src(nws, pvs, chunks, c);
  const int tid = (int)threadIdx.x;
  uint32_t m = 0;
  if (((reinterpret_cast<uintptr_t>(s.nw) ^ reinterpret_cast<uintptr_t>(s.pv)) & 15u) == 0) {  // block-uniform
    const int h = (int)(((16u - (reinterpret_cast<uintptr_t>(s.nw) & 15u)) & 15u) >> 2);
    const int head = h < c.len ? h : c.len;
    const float4* n4p = reinterpret_cast<const float4*>(s.nw + head);
    const float4* p4p = reinterpret_cast<const float4*>(s.pv + head);
    const int n4 = (c.len - head) >> 2;
    constexpr int U = ADFL_SLQ_CHUNK_ELEMS / 4 / kBlock;  // 8 float4 per thread and source
    float4 a[U], b[U];
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const int i = tid + k * kBlock;
      a[k] = i < n4 ? load4<true>(n4p + i) : zero4();
    }
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const int i = tid + k * kBlock;
      b[k] = i < n4 ? load4<true>(p4p + i) : zero4();
    }
    if (tid < head) m = abs_bits(delta1(s.nw, s.pv, tid));
    const int tail = head + (n4 << 2);
    if (tid < c.len - tail) m = max(m, abs_bits(delta1(s.nw, s.pv, tail + tid)));
#pragma unroll
    for (int k = 0; k < U; ++k) m = max(m, abs_bits4(sub4(a[k], b[k])));
  } else {
    for (int i = tid; i < c.len; i += kBlock) m = max(m, abs_bits(delta1(s.nw, s.pv, i)));
  }
  m = block_max(m);
  if (tid == 0) partials[blockIdx.x] = m;
}

// Pass 2: all of the chunk's loads of both sources are issued before the partial reduction, whose latency
// they hide (k_quantize_batched's schedule); the difference lands in the chunk's quantize-tile registers and
// chunk_store writes the payload. Element-wise path: the sources are read after the reduction.
__global__ __launch_bounds__(kBlock) void k_quantize_delta_batched(PtrTable nws, PtrTable pvs,
                                                                   const adfl_slq_chunk* __restrict__ chunks,
                                                                   float qmax, const uint32_t* __restrict__ partials,
                                                                   int8_t* __restrict__ q, float* __restrict__ scales) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kWaves][kTile / 4];
  const int64_t ci = blockIdx.x;
  const adfl_slq_chunk c = chunks[ci];
  const DeltaSrc s = delta_src(nws, pvs, chunks, c);
  const int tid = (int)threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int head = chunk_head(c.start, c.len, 16);  // where the payload reaches a 16-byte boundary
  if (!(dev_aligned16(s.nw + head) && dev_aligned16(s.pv + head))) {  // block-uniform
    const ScaleInv si = make_scale(reduce_partials(partials + c.first_chunk, c.nchunks), qmax);
    if (ci == c.first_chunk && tid == 0) scales[c.tensor] = si.scale;
    int8_t* qc = q + c.start;
    for (int i = tid; i < c.len; i += kBlock) qc[i] = (int8_t)quant1(delta1(s.nw, s.pv, i), si.inv);
    return;
  }
  const int ntiles = (c.len - head) / kTile;
  const float4* n4p = reinterpret_cast<const float4*>(s.nw + head);
  const float4* p4p = reinterpret_cast<const float4*>(s.pv + head);
  ChunkRegs r;
  float4 b[kChunkTilesPerWave][4];
#pragma unroll
  for (int k = 0; k < kChunkTilesPerWave; ++k) {
    const int t = wave + k * kWaves;
    if (t < ntiles) {
      load_tile(n4p + t * (kTile / 4), r.v[k], lane);
      load_tile(p4p + t * (kTile / 4), b[k], lane);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) r.v[k][j] = b[k][j] = zero4();
    }
  }
  r.head = tid < head ? delta1(s.nw, s.pv, tid) : 0.0f;
  const int t0 = head + ntiles * kTile;
#pragma unroll
  for (int k = 0; k < kChunkTailPerThread; ++k) {
    const int i = t0 + k * kBlock + tid;
    r.tail[k] = i < c.len ? delta1(s.nw, s.pv, i) : 0.0f;
  }
#pragma unroll
  for (int k = 0; k < kChunkTilesPerWave; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j) r.v[k][j] = sub4(r.v[k][j], b[k][j]);
  const ScaleInv si = make_scale(reduce_partials(partials + c.first_chunk, c.nchunks), qmax);
  if (ci == c.first_chunk && tid == 0) scales[c.tensor] = si.scale;
  chunk_store(c, r, si.inv, q, lds[wave], lane, wave);
}

// int4 pairs of [a, b) of a chunk (a even), element-wise: the pad of an odd tensor's last pair is a zero CODE
// (compression.py:42-43). pc: the chunk's first packed byte.
template <int BLOCK>
__device__ __forceinline__ void quantize_pairs_delta_int4(const float* __restrict__ nw, const float* __restrict__ pv,
                                                          uint8_t* __restrict__ pc, int a, int b, int len,
                                                          float inv) {
  for (int i = a + 2 * (int)threadIdx.x; i < b; i += 2 * BLOCK) {
    const int hi = quant1(delta1(nw, pv, i), inv);
    const int lo = (i + 1 < len) ? quant1(delta1(nw, pv, i + 1), inv) : 0;
    pc[i >> 1] = (uint8_t)pack_pair(hi, lo);
  }
}

// int4 pass 2 (pass 1 is k_absmax_delta_batched): every tensor offset even, flat element e in packed byte e/2.
// One int4 wave tile per wave per chunk, loaded from both sources before the partial reduction.
__global__ __launch_bounds__(kBlock) void k_quantize_delta_batched_int4(PtrTable nws, PtrTable pvs,
                                                                        const adfl_slq_chunk* __restrict__ chunks,
                                                                        float qmax,
                                                                        const uint32_t* __restrict__ partials,
                                                                        uint8_t* __restrict__ packed,
                                                                        float* __restrict__ scales) {
  static_assert(ADFL_SLQ_CHUNK_ELEMS == kTile4 * kWaves, "one int4 tile per wave per chunk");
  __shared__ __attribute__((aligned(16))) uint16_t lds[kWaves][kTile4 / 4];
  const int64_t ci = blockIdx.x;
  const adfl_slq_chunk c = chunks[ci];
  const DeltaSrc s = delta_src(nws, pvs, chunks, c);
  const int tid = (int)threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  uint8_t* pc = packed + (c.start >> 1);
  const int head = chunk_head(c.start, c.len, 32);  // even; where the packed bytes reach a 16-byte boundary
  const bool vec = dev_aligned16(s.nw + head) && dev_aligned16(s.pv + head);  // block-uniform
  const int ntiles = vec ? (c.len - head) / kTile4 : 0;
  float4 v[8], b[8];
  if (wave < ntiles) {
    load_tile_int4(reinterpret_cast<const float4*>(s.nw + head) + wave * (kTile4 / 4), v, lane);
    load_tile_int4(reinterpret_cast<const float4*>(s.pv + head) + wave * (kTile4 / 4), b, lane);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = sub4(v[j], b[j]);
  }
  const ScaleInv si = make_scale(reduce_partials(partials + c.first_chunk, c.nchunks), qmax);
  if (ci == c.first_chunk && tid == 0) scales[c.tensor] = si.scale;
  if (!vec) {
    quantize_pairs_delta_int4<kBlock>(s.nw, s.pv, pc, 0, c.len, c.len, si.inv);
    return;
  }
  quantize_pairs_delta_int4<kBlock>(s.nw, s.pv, pc, 0, head, c.len, si.inv);
  if (wave < ntiles)
    quantize_tile_int4_regs(v, reinterpret_cast<uint4*>(pc + (head >> 1)) + wave * 64, si.inv, lds[wave], lane);
  quantize_pairs_delta_int4<kBlock>(s.nw, s.pv, pc, head + ntiles * kTile4, c.len, c.len, si.inv);
}

// ------------------------------------------------------------------------------------------------
// resident, one launch (every tensor <= ADFL_SLQ_DELTA_RESIDENT_CHUNKS chunks: a tensor per 1024-thread block)
// ------------------------------------------------------------------------------------------------
// k_encode_resident's walk over the work list (work[b] = the first chunk of tensor b), the tensor's difference
// held in registers between the in-block max and the quantize. A 1024-thread block leaves 128 VGPRs per lane
// (4 waves per SIMD of the 512-entry file), so the 64 registers of the difference and both sources' loads do
// not fit in flight at once. The loads go in two stages of kDeltaStageTiles wave tiles of BOTH sources (64
// registers in flight), each subtracted into new's registers as it lands, the second stage issued behind the
// first's 32 registers of difference: 96 registers of data at the peak, 128 VGPRs and no scratch in all
// (DESIGN.md §9 has the compiler's resource usage; the head and tail elements are loaded first and subtracted
// last, so no wait stands between the stages' loads).
// Element-wise path (sources not 16-byte aligned where the payload is): the sources are read twice, for the
// max and for the quantize.
constexpr int kDeltaStageTiles = 2;
static_assert(kSegTilesPerWave % kDeltaStageTiles == 0, "whole stages");

template <bool ST_NT>
__global__ __launch_bounds__(kSegBlock) void k_encode_delta_resident(PtrTable nws, PtrTable pvs,
                                                                     const adfl_slq_chunk* __restrict__ chunks,
                                                                     const int32_t* __restrict__ work, float qmax,
                                                                     int8_t* __restrict__ q,
                                                                     float* __restrict__ scales) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kSegWaves][kTile / 4];
  const int64_t ci = work[blockIdx.x];
  const adfl_slq_chunk c = chunks[ci];
  const int tid = (int)threadIdx.x;
  if (c.nchunks > kDeltaSegChunks) {  // not a resident work list (a direct C caller's): NaN scale, nothing written
    if (tid == 0) scales[c.tensor] = __builtin_nanf("");
    return;
  }
  const int lane = tid & 63, wave = tid >> 6;
  const int len = (c.nchunks - 1) * ADFL_SLQ_CHUNK_ELEMS + chunks[ci + c.nchunks - 1].len;
  const float* nw = nws[c.tensor];  // ci is the tensor's first chunk
  const float* pv = pvs[c.tensor];
  int8_t* qt = q + c.start;
  const int head = chunk_head(c.start, len, 16);
  if (!(dev_aligned16(nw + head) && dev_aligned16(pv + head))) {  // block-uniform
    uint32_t m = 0;
    for (int i = tid; i < len; i += kSegBlock) m = max(m, abs_bits(delta1(nw, pv, i)));
    const ScaleInv si = make_scale(block_max_seg(m), qmax);
    if (tid == 0) scales[c.tensor] = si.scale;
    for (int i = tid; i < len; i += kSegBlock) qt[i] = (int8_t)quant1(nw[i] - pv[i], si.inv);
    return;
  }
  const int ntiles = (len - head) / kTile;
  const float4* n4p = reinterpret_cast<const float4*>(nw + head);
  const float4* p4p = reinterpret_cast<const float4*>(pv + head);
  float4 v[kSegTilesPerWave][4];
  const float hn = tid < head ? ld_nt(nw + tid) : 0.0f, hp = tid < head ? ld_nt(pv + tid) : 0.0f;
  const int ti = head + ntiles * kTile + tid;  // < 1024 tail elements: one per thread
  const float tn = ti < len ? ld_nt(nw + ti) : 0.0f, tp = ti < len ? ld_nt(pv + ti) : 0.0f;
#pragma unroll
  for (int s = 0; s < kSegTilesPerWave / kDeltaStageTiles; ++s) {
    float4 b[kDeltaStageTiles][4];
#pragma unroll
    for (int d = 0; d < kDeltaStageTiles; ++d) {
      const int k = s * kDeltaStageTiles + d;
      const int t = wave + k * kSegWaves;
      if (t < ntiles) {
        load_tile(n4p + t * (kTile / 4), v[k], lane);
        load_tile(p4p + t * (kTile / 4), b[d], lane);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[k][j] = b[d][j] = zero4();
      }
    }
#pragma unroll
    for (int d = 0; d < kDeltaStageTiles; ++d)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        v[s * kDeltaStageTiles + d][j] = sub4(v[s * kDeltaStageTiles + d][j], b[d][j]);
  }
  const float hv = hn - hp, tv = tn - tp;
  uint32_t m = max(abs_bits(hv), abs_bits(tv));
#pragma unroll
  for (int k = 0; k < kSegTilesPerWave; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j) m = max(m, abs_bits4(v[k][j]));
  const ScaleInv si = make_scale(block_max_seg(m), qmax);
  if (tid == 0) scales[c.tensor] = si.scale;
  uint4* q16 = reinterpret_cast<uint4*>(qt + head);
#pragma unroll
  for (int k = 0; k < kSegTilesPerWave; ++k) {
    const int t = wave + k * kSegWaves;
    if (t < ntiles) quantize_tile_regs<ST_NT>(v[k], q16 + t * (kTile / 16), si.inv, lds[wave], lane);
  }
  if (tid < head) qt[tid] = (int8_t)quant1(hv, si.inv);
  if (ti < len) qt[ti] = (int8_t)quant1(tv, si.inv);
}
constexpr bool kDeltaResidentNtStores = false;  // allocating payload stores, as k_encode_resident's

// int4 variant (PackedSLQChannel's buckets): 2048-element int4 wave tiles, 2 per wave (16 float4 per lane);
// one tile of both sources per stage (the same 64 registers in flight). The < 32-element head and the
// < 2048-element tail go pairwise, one pair per thread.
constexpr int kSegTiles4PerWave = (int)(kSegMaxElems / kTile4 / kSegWaves);  // 2
static_assert(kSegTiles4PerWave * kTile4 * kSegWaves == kSegMaxElems, "int4 tiles cover a segment");
static_assert(2 * kSegBlock == kTile4, "int4 tail: one pair per thread");

__global__ __launch_bounds__(kSegBlock) void k_encode_delta_resident_int4(PtrTable nws, PtrTable pvs,
                                                                          const adfl_slq_chunk* __restrict__ chunks,
                                                                          const int32_t* __restrict__ work,
                                                                          float qmax, uint8_t* __restrict__ packed,
                                                                          float* __restrict__ scales) {
  __shared__ __attribute__((aligned(16))) uint16_t lds[kSegWaves][kTile4 / 4];
  const int64_t ci = work[blockIdx.x];
  const adfl_slq_chunk c = chunks[ci];
  const int tid = (int)threadIdx.x;
  if (c.nchunks > kDeltaSegChunks) {  // not a resident work list (a direct C caller's): NaN scale, nothing written
    if (tid == 0) scales[c.tensor] = __builtin_nanf("");
    return;
  }
  const int lane = tid & 63, wave = tid >> 6;
  const int len = (c.nchunks - 1) * ADFL_SLQ_CHUNK_ELEMS + chunks[ci + c.nchunks - 1].len;
  const float* nw = nws[c.tensor];
  const float* pv = pvs[c.tensor];
  uint8_t* pt = packed + (c.start >> 1);
  const int head = chunk_head(c.start, len, 32);  // even: tensor offsets are even
  if (!(dev_aligned16(nw + head) && dev_aligned16(pv + head))) {  // block-uniform
    uint32_t m = 0;
    for (int i = tid; i < len; i += kSegBlock) m = max(m, abs_bits(delta1(nw, pv, i)));
    const ScaleInv si = make_scale(block_max_seg(m), qmax);
    if (tid == 0) scales[c.tensor] = si.scale;
    for (int i = 2 * tid; i < len; i += 2 * kSegBlock) {
      const int hi = quant1(nw[i] - pv[i], si.inv);
      const int lo = (i + 1 < len) ? quant1(nw[i + 1] - pv[i + 1], si.inv) : 0;
      pt[i >> 1] = (uint8_t)pack_pair(hi, lo);
    }
    return;
  }
  const int ntiles = (len - head) / kTile4;
  const float4* n4p = reinterpret_cast<const float4*>(nw + head);
  const float4* p4p = reinterpret_cast<const float4*>(pv + head);
  float4 v[kSegTiles4PerWave][8];
  // head pair (element 2*tid of [0, head)) and tail pair (t0 + 2*tid of [t0, len))
  const int hi = 2 * tid;
  const bool has_h = hi < head, has_h1 = has_h && hi + 1 < len;
  const float h0n = has_h ? ld_nt(nw + hi) : 0.0f, h0p = has_h ? ld_nt(pv + hi) : 0.0f;
  const float h1n = has_h1 ? ld_nt(nw + hi + 1) : 0.0f, h1p = has_h1 ? ld_nt(pv + hi + 1) : 0.0f;
  const int ti = head + ntiles * kTile4 + 2 * tid;
  const bool has_t = ti < len, has_t1 = has_t && ti + 1 < len;
  const float t0n = has_t ? ld_nt(nw + ti) : 0.0f, t0p = has_t ? ld_nt(pv + ti) : 0.0f;
  const float t1n = has_t1 ? ld_nt(nw + ti + 1) : 0.0f, t1p = has_t1 ? ld_nt(pv + ti + 1) : 0.0f;
#pragma unroll
  for (int k = 0; k < kSegTiles4PerWave; ++k) {
    const int t = wave + k * kSegWaves;
    float4 b[8];
    if (t < ntiles) {
      load_tile_int4(n4p + t * (kTile4 / 4), v[k], lane);
      load_tile_int4(p4p + t * (kTile4 / 4), b, lane);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[k][j] = b[j] = zero4();
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) v[k][j] = sub4(v[k][j], b[j]);
  }
  const float h0 = h0n - h0p, h1 = h1n - h1p, t0v = t0n - t0p, t1v = t1n - t1p;
  uint32_t m = max(max(abs_bits(h0), abs_bits(h1)), max(abs_bits(t0v), abs_bits(t1v)));
#pragma unroll
  for (int k = 0; k < kSegTiles4PerWave; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) m = max(m, abs_bits4(v[k][j]));
  const ScaleInv si = make_scale(block_max_seg(m), qmax);
  if (tid == 0) scales[c.tensor] = si.scale;
#pragma unroll
  for (int k = 0; k < kSegTiles4PerWave; ++k) {
    const int t = wave + k * kSegWaves;
    if (t < ntiles)
      quantize_tile_int4_regs(v[k], reinterpret_cast<uint4*>(pt + (head >> 1)) + t * 64, si.inv, lds[wave], lane);
  }
  // the pad of an odd tensor's last pair is a zero CODE (compression.py:42-43), not quant1(0)
  if (has_h) pt[hi >> 1] = (uint8_t)pack_pair(quant1(h0, si.inv), hi + 1 < len ? quant1(h1, si.inv) : 0);
  if (has_t) pt[ti >> 1] = (uint8_t)pack_pair(quant1(t0v, si.inv), ti + 1 < len ? quant1(t1v, si.inv) : 0);
}

// ------------------------------------------------------------------------------------------------
// QAFeL's broadcast: delta encode + hidden-state update (adfl_slq_encode_delta_update_batched*)
// ------------------------------------------------------------------------------------------------
// Src/ADFL/Server/qafel.py:156-180 runs, back to back, q = encode(g - h) and h += decode(q). The encode kernels
// above hold everything the update needs once the scale is known, so these forms write the payload AND
//   h'[i] = fp32(h[i] + fp32(scale * c[i]))          c: the code the channel's decode reads back from q
// in the same launch: two separately rounded operations (__fmul_rn, __fadd_rn; never an FMA), what
// k_dequantize_add_batched computes for mul_(1).add_(d, alpha=1). int8: c is the stored code. int4: c is
// nibble - 8 of the PACKED byte (dequant_byte_int4), so a code 127 (all-zero or NaN tensor) aliases into both
// nibbles exactly as the decode sees it, and an odd tensor's pad is a zero code. No special cases: a scale of
// 0, NaN or inf flows through the two operations as it does through the reference's.
// Per element 13 bytes (read g, read h, write the payload, write h) against the 18 of send_delta then
// receive_add_.
//
// In-place invariant: every element of h is read only by the block that writes it, and read before it is
// written. Pass 1 (k_absmax_delta_batched) finishes at a kernel boundary; pass 2 loads its own chunk of h
// before it stores any of it; the resident form reads its own tensor first, then each wave re-reads a tile of
// its own and stores that tile; the element-wise paths read an element, then write it. g is never written and
// nothing outside the tensors' elements is. Overlap of g[t] with h[t], or of two tensors of h, is undefined.
//
// Cache policy: g is read non-temporally (dead after the read); h is read with plain loads (it is rewritten;
// the resident form re-reads it from L2 / the Infinity Cache); h' is stored non-temporally when kUpdateHiddenNt
// (the next broadcast reads h only after a whole buffer of client updates; DESIGN.md §9 has the A/B).
#ifndef ADFL_UPDATE_H_NT
#define ADFL_UPDATE_H_NT 1
#endif
constexpr bool kUpdateHiddenNt = ADFL_UPDATE_H_NT != 0;

typedef float* const* __restrict__ MutPtrTable;

__device__ __forceinline__ float nib(uint32_t n) { return (float)((int)(n & 0xfu) - 8); }

__device__ __forceinline__ float upd1(float h, float scale, float code) { return __fadd_rn(h, __fmul_rn(scale, code)); }

__device__ __forceinline__ float4 upd4(float4 h, float4 d) {
  return make_float4(__fadd_rn(h.x, d.x), __fadd_rn(h.y, d.y), __fadd_rn(h.z, d.z), __fadd_rn(h.w, d.w));
}

// fp32(scale * code) of the 4 int8 codes of payload dword w
__device__ __forceinline__ float4 dq4(uint32_t w, float s) {
  return make_float4(__fmul_rn(s, (float)(int8_t)(w & 0xffu)), __fmul_rn(s, (float)(int8_t)((w >> 8) & 0xffu)),
                     __fmul_rn(s, (float)(int8_t)((w >> 16) & 0xffu)), __fmul_rn(s, (float)(int8_t)(w >> 24)));
}

// fp32(scale * (nibble - 8)) of the 4 nibbles of 2 packed bytes (high nibble = even element)
__device__ __forceinline__ float4 dq4_int4(uint32_t h, float s) {
  return make_float4(__fmul_rn(s, nib(h >> 4)), __fmul_rn(s, nib(h)), __fmul_rn(s, nib(h >> 12)),
                     __fmul_rn(s, nib(h >> 8)));
}

__device__ __forceinline__ void store_h4(float4* p, float4 d) {
  if (kUpdateHiddenNt) store4_nt(p, d);
  else *p = d;
}

__device__ __forceinline__ void store_h1(float* p, float d) {
  if (kUpdateHiddenNt) __builtin_nontemporal_store(d, p);
  else *p = d;
}

// One element: the payload byte and h'. hv: the h value already read.
__device__ __forceinline__ void update1(float x, float hv, ScaleInv si, int8_t* q, float* h) {
  const int8_t c = (int8_t)quant1(x, si.inv);
  *q = c;
  store_h1(h, upd1(hv, si.scale, (float)c));
}

// One int4 pair whose h values a0, a1 are already read: the packed byte b, then h' of both from its nibbles.
__device__ __forceinline__ void update_pair_store(uint32_t b, float a0, float a1, bool two, float scale, uint8_t* pb,
                                                  float* h) {
  *pb = (uint8_t)b;
  store_h1(h, upd1(a0, scale, nib(b >> 4)));
  if (two) store_h1(h + 1, upd1(a1, scale, nib(b)));
}

// One int8 wave tile: hb the tile's h, v its g (SUB: the two-pass form, which needs no difference before the
// scale and so forms it here, group by group, instead of holding a third set of registers) or the difference
// itself, all in the load layout. The payload goes through the LDS transpose; h' goes out in the load layout
// with 16-byte stores, group by group as its codes are formed.
template <bool SUB>
__device__ __forceinline__ void update_tile_regs(const float4 (&v)[4], const float4 (&hb)[4], uint4* __restrict__ q16,
                                                 float4* h4, ScaleInv si, uint32_t* __restrict__ lds, int lane) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t w = quant4(SUB ? sub4(v[j], hb[j]) : v[j], si.inv);
    lds[j * 64 + lane] = w;
    store_h4(h4 + j * 64 + lane, upd4(hb[j], dq4(w, si.scale)));
  }
  __builtin_amdgcn_wave_barrier();
  const uint4 o = reinterpret_cast<const uint4*>(lds)[lane];
  __builtin_amdgcn_wave_barrier();
  q16[lane] = o;
}

// One int4 wave tile (2048 elements, 8 float4 per lane).
template <bool SUB>
__device__ __forceinline__ void update_tile_int4_regs(const float4 (&v)[8], const float4 (&hb)[8],
                                                      uint4* __restrict__ p16, float4* h4, ScaleInv si,
                                                      uint16_t* __restrict__ lds, int lane) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const uint32_t w = quant4_int4(SUB ? sub4(v[j], hb[j]) : v[j], si.inv);
    lds[j * 64 + lane] = (uint16_t)w;
    store_h4(h4 + j * 64 + lane, upd4(hb[j], dq4_int4(w, si.scale)));
  }
  __builtin_amdgcn_wave_barrier();
  const uint4 o = reinterpret_cast<const uint4*>(lds)[lane];
  __builtin_amdgcn_wave_barrier();
  p16[lane] = o;
}

// int4 pairs of [a, b) of a chunk / tensor of `len` (a even), element-wise: each pair's h is read, then its
// packed byte and h' are written. The pad of an odd tensor's last pair is a zero CODE and updates nothing.
template <int BLOCK>
__device__ __forceinline__ void update_pairs_int4(const float* __restrict__ nw, float* hd, uint8_t* __restrict__ pc,
                                                  int a, int b, int len, ScaleInv si) {
  for (int i = a + 2 * (int)threadIdx.x; i < b; i += 2 * BLOCK) {
    const bool two = i + 1 < len;
    const float h0 = hd[i], h1 = two ? hd[i + 1] : 0.0f;
    const int hi = quant1(ld_nt(nw + i) - h0, si.inv);
    const int lo = two ? quant1(ld_nt(nw + i + 1) - h1, si.inv) : 0;
    update_pair_store(pack_pair(hi, lo), h0, h1, two, si.scale, pc + (i >> 1), hd + i);
  }
}

// Pass 2 of the two-pass form (pass 1: k_absmax_delta_batched, unchanged): k_quantize_delta_batched's schedule
// with the h registers kept. All of the chunk's loads of both sources are issued before the partial reduction;
// after it every 16-byte group is quantized, its payload goes out through the LDS transpose, and the same
// codes are dequantized in the load layout, added to the kept h and stored.
__global__ __launch_bounds__(kBlock) void k_quantize_delta_update_batched(PtrTable nws, MutPtrTable hds,
                                                                          const adfl_slq_chunk* __restrict__ chunks,
                                                                          float qmax,
                                                                          const uint32_t* __restrict__ partials,
                                                                          int8_t* __restrict__ q,
                                                                          float* __restrict__ scales) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kWaves][kTile / 4];
  const int64_t ci = blockIdx.x;
  const adfl_slq_chunk c = chunks[ci];
  const int64_t off = c.start - chunks[c.first_chunk].start;
  const float* nw = nws[c.tensor] + off;
  float* hd = hds[c.tensor] + off;
  const int tid = (int)threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  int8_t* qc = q + c.start;
  const int head = chunk_head(c.start, c.len, 16);  // where the payload reaches a 16-byte boundary
  if (!(dev_aligned16(nw + head) && dev_aligned16(hd + head))) {  // block-uniform
    const ScaleInv si = make_scale(reduce_partials(partials + c.first_chunk, c.nchunks), qmax);
    if (ci == c.first_chunk && tid == 0) scales[c.tensor] = si.scale;
    for (int i = tid; i < c.len; i += kBlock) {
      const float hv = hd[i];
      update1(ld_nt(nw + i) - hv, hv, si, qc + i, hd + i);
    }
    return;
  }
  const int ntiles = (c.len - head) / kTile;
  const float4* n4p = reinterpret_cast<const float4*>(nw + head);
  float4* h4p = reinterpret_cast<float4*>(hd + head);
  float4 v[kChunkTilesPerWave][4], b[kChunkTilesPerWave][4];
#pragma unroll
  for (int k = 0; k < kChunkTilesPerWave; ++k) {
    const int t = wave + k * kWaves;
    if (t < ntiles) {
      load_tile(n4p + t * (kTile / 4), v[k], lane);
#pragma unroll
      for (int j = 0; j < 4; ++j) b[k][j] = h4p[t * (kTile / 4) + j * 64 + lane];
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[k][j] = b[k][j] = zero4();
    }
  }
  // head and tail elements: the difference is kept, their h is read again for the update
  const float hx = tid < head ? ld_nt(nw + tid) - hd[tid] : 0.0f;
  const int t0 = head + ntiles * kTile;
  float tx[kChunkTailPerThread];
#pragma unroll
  for (int k = 0; k < kChunkTailPerThread; ++k) {
    const int i = t0 + k * kBlock + tid;
    tx[k] = i < c.len ? ld_nt(nw + i) - hd[i] : 0.0f;
  }
  const ScaleInv si = make_scale(reduce_partials(partials + c.first_chunk, c.nchunks), qmax);
  if (ci == c.first_chunk && tid == 0) scales[c.tensor] = si.scale;
  uint4* q16 = reinterpret_cast<uint4*>(qc + head);
#pragma unroll
  for (int k = 0; k < kChunkTilesPerWave; ++k) {
    const int t = wave + k * kWaves;
    if (t < ntiles) update_tile_regs<true>(v[k], b[k], q16 + t * (kTile / 16), h4p + t * (kTile / 4), si, lds[wave], lane);
  }
  if (tid < head) update1(hx, hd[tid], si, qc + tid, hd + tid);
#pragma unroll
  for (int k = 0; k < kChunkTailPerThread; ++k) {
    const int i = t0 + k * kBlock + tid;
    if (i < c.len) update1(tx[k], hd[i], si, qc + i, hd + i);
  }
}

// reduce_partials without the loop interleaving: its second address pair and load would sit on top of the 64
// registers of both sources that the int4 pass 2 holds across it (84 VGPRs, one wave per SIMD fewer).
__device__ __forceinline__ uint32_t reduce_partials_rolled(const uint32_t* __restrict__ p, int count) {
  uint32_t m = 0;
  for (int k = threadIdx.x; k < count; k += kBlock) {
    m = max(m, p[k]);
    asm volatile("" ::: "memory");  // one load at a time, whatever the loop passes decide
  }
  return block_max(m);
}

// int4 pass 2: k_quantize_delta_batched_int4 with the h tile kept.
__global__ __launch_bounds__(kBlock) void k_quantize_delta_update_batched_int4(
    PtrTable nws, MutPtrTable hds, const adfl_slq_chunk* __restrict__ chunks, float qmax,
    const uint32_t* __restrict__ partials, uint8_t* __restrict__ packed, float* __restrict__ scales) {
  __shared__ __attribute__((aligned(16))) uint16_t lds[kWaves][kTile4 / 4];
  const int64_t ci = blockIdx.x;
  const adfl_slq_chunk c = chunks[ci];
  const int64_t off = c.start - chunks[c.first_chunk].start;
  const float* nw = nws[c.tensor] + off;
  float* hd = hds[c.tensor] + off;
  const int tid = (int)threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  uint8_t* pc = packed + (c.start >> 1);
  const int head = chunk_head(c.start, c.len, 32);  // even; where the packed bytes reach a 16-byte boundary
  if (!(dev_aligned16(nw + head) && dev_aligned16(hd + head))) {  // block-uniform
    const ScaleInv si = make_scale(reduce_partials(partials + c.first_chunk, c.nchunks), qmax);
    if (ci == c.first_chunk && tid == 0) scales[c.tensor] = si.scale;
    update_pairs_int4<kBlock>(nw, hd, pc, 0, c.len, c.len, si);
    return;
  }
  const int ntiles = (c.len - head) / kTile4;
  float4 v[8], b[8];
  float4* h4 = reinterpret_cast<float4*>(hd + head) + wave * (kTile4 / 4);
  if (wave < ntiles) {
    load_tile_int4(reinterpret_cast<const float4*>(nw + head) + wave * (kTile4 / 4), v, lane);
#pragma unroll
    for (int j = 0; j < 8; ++j) b[j] = h4[j * 64 + lane];
  }
  const ScaleInv si = make_scale(reduce_partials_rolled(partials + c.first_chunk, c.nchunks), qmax);
  if (ci == c.first_chunk && tid == 0) scales[c.tensor] = si.scale;
  // the tile first: the pair loops' temporaries then do not sit on top of its 64 registers
  if (wave < ntiles)
    update_tile_int4_regs<true>(v, b, reinterpret_cast<uint4*>(pc + (head >> 1)) + wave * 64, h4, si, lds[wave], lane);
  update_pairs_int4<kBlock>(nw, hd, pc, 0, head, c.len, si);
  update_pairs_int4<kBlock>(nw, hd, pc, head + ntiles * kTile4, c.len, c.len, si);
}

// Resident one-launch form: k_encode_delta_resident's load stages and in-block max, h read with allocating
// loads. The 128 VGPRs of a 1024-thread block hold the 64 registers of the difference, so h does not stay:
// the quantize phase re-reads it tile by tile (L2 / Infinity Cache hits of the first read), the next tile's
// reload issued half way through the current tile — at most two tiles, 32 registers, on top of the difference,
// whose registers die as the tiles are consumed. The head and tail elements of h are re-read likewise. A missing
// tile's h registers are left undefined, not zeroed (they are never read): zero-filling them cost 28 bytes of
// scratch per lane.
__global__ __launch_bounds__(kSegBlock) void k_encode_delta_update_resident(PtrTable nws, MutPtrTable hds,
                                                                            const adfl_slq_chunk* __restrict__ chunks,
                                                                            const int32_t* __restrict__ work,
                                                                            float qmax, int8_t* __restrict__ q,
                                                                            float* __restrict__ scales) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kSegWaves][kTile / 4];
  const int64_t ci = work[blockIdx.x];
  const adfl_slq_chunk c = chunks[ci];
  const int tid = (int)threadIdx.x;
  if (c.nchunks > kDeltaSegChunks) {  // not a resident work list: NaN scale, no payload, h untouched
    if (tid == 0) scales[c.tensor] = __builtin_nanf("");
    return;
  }
  const int lane = tid & 63, wave = tid >> 6;
  const int len = (c.nchunks - 1) * ADFL_SLQ_CHUNK_ELEMS + chunks[ci + c.nchunks - 1].len;
  const float* nw = nws[c.tensor];  // ci is the tensor's first chunk
  float* hd = hds[c.tensor];
  int8_t* qt = q + c.start;
  const int head = chunk_head(c.start, len, 16);
  if (!(dev_aligned16(nw + head) && dev_aligned16(hd + head))) {  // block-uniform
    uint32_t m = 0;
    for (int i = tid; i < len; i += kSegBlock) m = max(m, abs_bits(ld_nt(nw + i) - hd[i]));
    const ScaleInv si = make_scale(block_max_seg(m), qmax);
    if (tid == 0) scales[c.tensor] = si.scale;
    for (int i = tid; i < len; i += kSegBlock) {
      const float hv = hd[i];
      update1(nw[i] - hv, hv, si, qt + i, hd + i);
    }
    return;
  }
  const int ntiles = (len - head) / kTile;
  const float4* n4p = reinterpret_cast<const float4*>(nw + head);
  float4* h4p = reinterpret_cast<float4*>(hd + head);
  float4 v[kSegTilesPerWave][4];
  const float hn = tid < head ? ld_nt(nw + tid) : 0.0f, hp = tid < head ? hd[tid] : 0.0f;
  const int ti = head + ntiles * kTile + tid;  // < 1024 tail elements: one per thread
  const float tn = ti < len ? ld_nt(nw + ti) : 0.0f, tp = ti < len ? hd[ti] : 0.0f;
#pragma unroll
  for (int s = 0; s < kSegTilesPerWave / kDeltaStageTiles; ++s) {
    float4 b[kDeltaStageTiles][4];
#pragma unroll
    for (int d = 0; d < kDeltaStageTiles; ++d) {
      const int k = s * kDeltaStageTiles + d;
      const int t = wave + k * kSegWaves;
      if (t < ntiles) {
        load_tile(n4p + t * (kTile / 4), v[k], lane);
#pragma unroll
        for (int j = 0; j < 4; ++j) b[d][j] = h4p[t * (kTile / 4) + j * 64 + lane];
      }
    }
#pragma unroll
    for (int d = 0; d < kDeltaStageTiles; ++d) {
      const int k = s * kDeltaStageTiles + d;
      const bool have = wave + k * kSegWaves < ntiles;  // wave-uniform; a missing tile is zeros, its b never read
#pragma unroll
      for (int j = 0; j < 4; ++j) v[k][j] = have ? sub4(v[k][j], b[d][j]) : zero4();
    }
  }
  const float hv = hn - hp, tv = tn - tp;
  uint32_t m = max(abs_bits(hv), abs_bits(tv));
#pragma unroll
  for (int k = 0; k < kSegTilesPerWave; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j) m = max(m, abs_bits4(v[k][j]));
  const ScaleInv si = make_scale(block_max_seg(m), qmax);
  if (tid == 0) scales[c.tensor] = si.scale;
  uint4* q16 = reinterpret_cast<uint4*>(qt + head);
  float4 hb[2][4];
  if (wave < ntiles) {
#pragma unroll
    for (int j = 0; j < 4; ++j) hb[0][j] = h4p[wave * (kTile / 4) + j * 64 + lane];
  }
  // update_tile_regs' body with the next tile's reload issued half way through the current tile, when two of
  // its four groups (16 registers of difference and h) are dead
#pragma unroll
  for (int k = 0; k < kSegTilesPerWave; ++k) {
    const int t = wave + k * kSegWaves;
    const bool cur = t < ntiles, nxt = k + 1 < kSegTilesPerWave && t + kSegWaves < ntiles;  // wave-uniform
    float4* h4 = h4p + t * (kTile / 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (cur) {
        const uint32_t w = quant4(v[k][j], si.inv);
        lds[wave][j * 64 + lane] = w;
        store_h4(h4 + j * 64 + lane, upd4(hb[k & 1][j], dq4(w, si.scale)));
      }
      if (j == 1 && nxt) {
#pragma unroll
        for (int i = 0; i < 4; ++i) hb[(k + 1) & 1][i] = h4[kSegWaves * (kTile / 4) + i * 64 + lane];
      }
    }
    if (cur) {
      __builtin_amdgcn_wave_barrier();
      const uint4 o = reinterpret_cast<const uint4*>(lds[wave])[lane];
      __builtin_amdgcn_wave_barrier();
      q16[t * (kTile / 16) + lane] = o;
    }
  }
  if (tid < head) update1(hv, hd[tid], si, qt + tid, hd + tid);
  if (ti < len) update1(tv, hd[ti], si, qt + ti, hd + ti);
}

// int4 resident form: 2 int4 wave tiles per wave; the quantize phase re-reads one tile of h (32 registers) at
// a time on top of the 64 of the difference. Head and tail pairs: one per thread, h re-read.
__global__ __launch_bounds__(kSegBlock) void k_encode_delta_update_resident_int4(
    PtrTable nws, MutPtrTable hds, const adfl_slq_chunk* __restrict__ chunks, const int32_t* __restrict__ work,
    float qmax, uint8_t* __restrict__ packed, float* __restrict__ scales) {
  __shared__ __attribute__((aligned(16))) uint16_t lds[kSegWaves][kTile4 / 4];
  const int64_t ci = work[blockIdx.x];
  const adfl_slq_chunk c = chunks[ci];
  const int tid = (int)threadIdx.x;
  if (c.nchunks > kDeltaSegChunks) {  // not a resident work list: NaN scale, no payload, h untouched
    if (tid == 0) scales[c.tensor] = __builtin_nanf("");
    return;
  }
  const int lane = tid & 63, wave = tid >> 6;
  const int len = (c.nchunks - 1) * ADFL_SLQ_CHUNK_ELEMS + chunks[ci + c.nchunks - 1].len;
  const float* nw = nws[c.tensor];
  float* hd = hds[c.tensor];
  uint8_t* pt = packed + (c.start >> 1);
  const int head = chunk_head(c.start, len, 32);  // even: tensor offsets are even
  if (!(dev_aligned16(nw + head) && dev_aligned16(hd + head))) {  // block-uniform
    uint32_t m = 0;
    for (int i = tid; i < len; i += kSegBlock) m = max(m, abs_bits(ld_nt(nw + i) - hd[i]));
    const ScaleInv si = make_scale(block_max_seg(m), qmax);
    if (tid == 0) scales[c.tensor] = si.scale;
    update_pairs_int4<kSegBlock>(nw, hd, pt, 0, len, len, si);
    return;
  }
  const int ntiles = (len - head) / kTile4;
  const float4* n4p = reinterpret_cast<const float4*>(nw + head);
  float4* h4p = reinterpret_cast<float4*>(hd + head);
  float4 v[kSegTiles4PerWave][8];
  // head pair (element 2*tid of [0, head)) and tail pair (t0 + 2*tid of [t0, len))
  const int hi = 2 * tid;
  const bool has_h = hi < head, has_h1 = has_h && hi + 1 < len;
  const float h0n = has_h ? ld_nt(nw + hi) : 0.0f, h0p = has_h ? hd[hi] : 0.0f;
  const float h1n = has_h1 ? ld_nt(nw + hi + 1) : 0.0f, h1p = has_h1 ? hd[hi + 1] : 0.0f;
  const int ti = head + ntiles * kTile4 + 2 * tid;
  const bool has_t = ti < len, has_t1 = has_t && ti + 1 < len;
  const float t0n = has_t ? ld_nt(nw + ti) : 0.0f, t0p = has_t ? hd[ti] : 0.0f;
  const float t1n = has_t1 ? ld_nt(nw + ti + 1) : 0.0f, t1p = has_t1 ? hd[ti + 1] : 0.0f;
#pragma unroll
  for (int k = 0; k < kSegTiles4PerWave; ++k) {
    const int t = wave + k * kSegWaves;
    float4 b[8];
    if (t < ntiles) {
      load_tile_int4(n4p + t * (kTile4 / 4), v[k], lane);
#pragma unroll
      for (int j = 0; j < 8; ++j) b[j] = h4p[t * (kTile4 / 4) + j * 64 + lane];
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[k][j] = b[j] = zero4();
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) v[k][j] = sub4(v[k][j], b[j]);
  }
  const float h0 = h0n - h0p, h1 = h1n - h1p, t0v = t0n - t0p, t1v = t1n - t1p;
  uint32_t m = max(max(abs_bits(h0), abs_bits(h1)), max(abs_bits(t0v), abs_bits(t1v)));
#pragma unroll
  for (int k = 0; k < kSegTiles4PerWave; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) m = max(m, abs_bits4(v[k][j]));
  const ScaleInv si = make_scale(block_max_seg(m), qmax);
  if (tid == 0) scales[c.tensor] = si.scale;
#pragma unroll
  for (int k = 0; k < kSegTiles4PerWave; ++k) {
    const int t = wave + k * kSegWaves;
    if (t < ntiles) {
      float4 hb[8];
      float4* h4 = h4p + t * (kTile4 / 4);
#pragma unroll
      for (int j = 0; j < 8; ++j) hb[j] = h4[j * 64 + lane];
      update_tile_int4_regs<false>(v[k], hb, reinterpret_cast<uint4*>(pt + (head >> 1)) + t * 64, h4, si, lds[wave], lane);
    }
  }
  // the pad of an odd tensor's last pair is a zero CODE (compression.py:42-43), not quant1(0)
  if (has_h)
    update_pair_store(pack_pair(quant1(h0, si.inv), has_h1 ? quant1(h1, si.inv) : 0), hd[hi], has_h1 ? hd[hi + 1] : 0.0f,
                      has_h1, si.scale, pt + (hi >> 1), hd + hi);
  if (has_t)
    update_pair_store(pack_pair(quant1(t0v, si.inv), has_t1 ? quant1(t1v, si.inv) : 0), hd[ti], has_t1 ? hd[ti + 1] : 0.0f,
                      has_t1, si.scale, pt + (ti >> 1), hd + ti);
}

// ------------------------------------------------------------------------------------------------
// host helpers
// ------------------------------------------------------------------------------------------------
inline bool host_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// Argument errors of the delta entries are all ADFL_E_ARG: null tables or outputs, a chunk count outside
// [1, INT32_MAX], bits outside [1, max_bits] (a code must fit the int8 payload, or the nibble).
inline bool bad_delta_args(const void* d_new, const void* d_prev, const void* d_chunks, int64_t nchunks, int bits,
                           int max_bits, const void* d_out, const void* d_scales) {
  return !d_new || !d_prev || !d_chunks || !d_out || !d_scales || nchunks < 1 || nchunks > INT32_MAX || bits < 1 ||
         bits > max_bits;
}

}  // namespace

extern "C" {

int adfl_slq_encode_delta_batched(const float* const* d_new, const float* const* d_prev, const adfl_slq_chunk* d_chunks,
                                  int64_t nchunks, int bits, int8_t* d_q, float* d_scales, uint32_t* d_partials,
                                  void* stream) {
  if (bad_delta_args(d_new, d_prev, d_chunks, nchunks, bits, 8, d_q, d_scales) || !d_partials) return ADFL_E_ARG;
  if (!host_aligned16(d_q)) return ADFL_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_absmax_delta_batched, dim3((unsigned)nchunks), dim3(kBlock), 0, st, d_new, d_prev, d_chunks,
                     d_partials);
  if (int s = launch_status()) return s;
  hipLaunchKernelGGL(k_quantize_delta_batched, dim3((unsigned)nchunks), dim3(kBlock), 0, st, d_new, d_prev, d_chunks,
                     qmax_f(bits), (const uint32_t*)d_partials, d_q, d_scales);
  return launch_status();
}

int adfl_slq_encode_delta_batched_work(const float* const* d_new, const float* const* d_prev,
                                       const adfl_slq_chunk* d_chunks, int64_t nchunks, const int32_t* d_work,
                                       int64_t nwork, int bits, int8_t* d_q, float* d_scales, uint32_t* d_partials,
                                       void* stream) {
  if (nwork == 0)
    return adfl_slq_encode_delta_batched(d_new, d_prev, d_chunks, nchunks, bits, d_q, d_scales, d_partials, stream);
  if (bad_delta_args(d_new, d_prev, d_chunks, nchunks, bits, 8, d_q, d_scales) || !d_work || nwork < 0 ||
      nwork > nchunks)
    return ADFL_E_ARG;
  if (!host_aligned16(d_q)) return ADFL_E_ALIGN;
  hipLaunchKernelGGL(k_encode_delta_resident<kDeltaResidentNtStores>, dim3((unsigned)nwork), dim3(kSegBlock), 0,
                     (hipStream_t)stream, d_new, d_prev, d_chunks, d_work, qmax_f(bits), d_q, d_scales);
  return launch_status();
}

int adfl_slq_encode_delta_batched_int4(const float* const* d_new, const float* const* d_prev,
                                       const adfl_slq_chunk* d_chunks, int64_t nchunks, int bits, uint8_t* d_packed,
                                       float* d_scales, uint32_t* d_partials, void* stream) {
  if (bad_delta_args(d_new, d_prev, d_chunks, nchunks, bits, 4, d_packed, d_scales) || !d_partials) return ADFL_E_ARG;
  if (!host_aligned16(d_packed)) return ADFL_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_absmax_delta_batched, dim3((unsigned)nchunks), dim3(kBlock), 0, st, d_new, d_prev, d_chunks,
                     d_partials);
  if (int s = launch_status()) return s;
  hipLaunchKernelGGL(k_quantize_delta_batched_int4, dim3((unsigned)nchunks), dim3(kBlock), 0, st, d_new, d_prev,
                     d_chunks, qmax_f(bits), (const uint32_t*)d_partials, d_packed, d_scales);
  return launch_status();
}

int adfl_slq_encode_delta_batched_int4_work(const float* const* d_new, const float* const* d_prev,
                                            const adfl_slq_chunk* d_chunks, int64_t nchunks, const int32_t* d_work,
                                            int64_t nwork, int bits, uint8_t* d_packed, float* d_scales,
                                            uint32_t* d_partials, void* stream) {
  if (nwork == 0)
    return adfl_slq_encode_delta_batched_int4(d_new, d_prev, d_chunks, nchunks, bits, d_packed, d_scales, d_partials,
                                              stream);
  if (bad_delta_args(d_new, d_prev, d_chunks, nchunks, bits, 4, d_packed, d_scales) || !d_work || nwork < 0 ||
      nwork > nchunks)
    return ADFL_E_ARG;
  if (!host_aligned16(d_packed)) return ADFL_E_ALIGN;
  hipLaunchKernelGGL(k_encode_delta_resident_int4, dim3((unsigned)nwork), dim3(kSegBlock), 0, (hipStream_t)stream,
                     d_new, d_prev, d_chunks, d_work, qmax_f(bits), d_packed, d_scales);
  return launch_status();
}

// The broadcast forms: the delta entries' checks and codes; d_hidden is read and written in place.
int adfl_slq_encode_delta_update_batched(const float* const* d_new, float* const* d_hidden,
                                         const adfl_slq_chunk* d_chunks, int64_t nchunks, int bits, int8_t* d_q,
                                         float* d_scales, uint32_t* d_partials, void* stream) {
  if (bad_delta_args(d_new, d_hidden, d_chunks, nchunks, bits, 8, d_q, d_scales) || !d_partials) return ADFL_E_ARG;
  if (!host_aligned16(d_q)) return ADFL_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_absmax_delta_batched, dim3((unsigned)nchunks), dim3(kBlock), 0, st, d_new,
                     (const float* const*)d_hidden, d_chunks, d_partials);
  if (int s = launch_status()) return s;
  hipLaunchKernelGGL(k_quantize_delta_update_batched, dim3((unsigned)nchunks), dim3(kBlock), 0, st, d_new, d_hidden,
                     d_chunks, qmax_f(bits), (const uint32_t*)d_partials, d_q, d_scales);
  return launch_status();
}

int adfl_slq_encode_delta_update_batched_work(const float* const* d_new, float* const* d_hidden,
                                              const adfl_slq_chunk* d_chunks, int64_t nchunks, const int32_t* d_work,
                                              int64_t nwork, int bits, int8_t* d_q, float* d_scales,
                                              uint32_t* d_partials, void* stream) {
  if (nwork == 0)
    return adfl_slq_encode_delta_update_batched(d_new, d_hidden, d_chunks, nchunks, bits, d_q, d_scales, d_partials,
                                                stream);
  if (bad_delta_args(d_new, d_hidden, d_chunks, nchunks, bits, 8, d_q, d_scales) || !d_work || nwork < 0 ||
      nwork > nchunks)
    return ADFL_E_ARG;
  if (!host_aligned16(d_q)) return ADFL_E_ALIGN;
  hipLaunchKernelGGL(k_encode_delta_update_resident, dim3((unsigned)nwork), dim3(kSegBlock), 0, (hipStream_t)stream,
                     d_new, d_hidden, d_chunks, d_work, qmax_f(bits), d_q, d_scales);
  return launch_status();
}

int adfl_slq_encode_delta_update_batched_int4(const float* const* d_new, float* const* d_hidden,
                                              const adfl_slq_chunk* d_chunks, int64_t nchunks, int bits,
                                              uint8_t* d_packed, float* d_scales, uint32_t* d_partials, void* stream) {
  if (bad_delta_args(d_new, d_hidden, d_chunks, nchunks, bits, 4, d_packed, d_scales) || !d_partials)
    return ADFL_E_ARG;
  if (!host_aligned16(d_packed)) return ADFL_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_absmax_delta_batched, dim3((unsigned)nchunks), dim3(kBlock), 0, st, d_new,
                     (const float* const*)d_hidden, d_chunks, d_partials);
  if (int s = launch_status()) return s;
  hipLaunchKernelGGL(k_quantize_delta_update_batched_int4, dim3((unsigned)nchunks), dim3(kBlock), 0, st, d_new,
                     d_hidden, d_chunks, qmax_f(bits), (const uint32_t*)d_partials, d_packed, d_scales);
  return launch_status();
}

int adfl_slq_encode_delta_update_batched_int4_work(const float* const* d_new, float* const* d_hidden,
                                                   const adfl_slq_chunk* d_chunks, int64_t nchunks,
                                                   const int32_t* d_work, int64_t nwork, int bits, uint8_t* d_packed,
                                                   float* d_scales, uint32_t* d_partials, void* stream) {
  if (nwork == 0)
    return adfl_slq_encode_delta_update_batched_int4(d_new, d_hidden, d_chunks, nchunks, bits, d_packed, d_scales,
                                                     d_partials, stream);
  if (bad_delta_args(d_new, d_hidden, d_chunks, nchunks, bits, 4, d_packed, d_scales) || !d_work || nwork < 0 ||
      nwork > nchunks)
    return ADFL_E_ARG;
  if (!host_aligned16(d_packed)) return ADFL_E_ALIGN;
  hipLaunchKernelGGL(k_encode_delta_update_resident_int4, dim3((unsigned)nwork), dim3(kSegBlock), 0,
                     (hipStream_t)stream, d_new, d_hidden, d_chunks, d_work, qmax_f(bits), d_packed, d_scales);
  return launch_status();
}

}  // extern "C"
