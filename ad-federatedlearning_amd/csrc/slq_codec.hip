// slq_codec.hip — MI355X (gfx950, CDNA4) kernels for ADFL's SLQ gradient codec + the C ABI of
// include/adfl_slq.h.
//
// Reference behaviour restated here (bit-exact, pinned by tests/golden):
//   encode  Src/ADFL/Channel/quant.py:97-104   scale = max|x| / q_max ; torch.quantize_per_tensor
//   decode  Src/ADFL/Channel/quant.py:107-112  q.dequantize()
//   loop    Src/ADFL/Channel/quant.py:74-94    per-tensor scales over a whole state dict (bucketed)
//   int4    Src/ADFL/compression.py:35-66      pack_4bit / unpack_4bit nibble layout
//   mean    Examples/ray_ad.py:188             stack(updates).mean(0) after the peer exchange
//
// Design (DESIGN.md has the byte accounting and the measurements behind every choice): the codec is a
// pure HBM stream with ~6 VALU ops per element, so every kernel is built for bandwidth.
//  * Wave tiles. A wave owns a tile of 1024 elements (int4: 2048). Every global access is a 16-byte
//    per-lane access that is contiguous across the wave (1 KiB per wave-instruction). Where the natural
//    per-lane shape differs between input and output (4 floats in, 4 bytes out), the wave transposes
//    through 1 KiB of LDS, so both the loads and the stores stay fully coalesced.
//  * The one grid-wide dependency (scale needs max|x| over the whole tensor) is a kernel boundary:
//    pass 1 writes one absmax partial per block, pass 2 re-reduces them (<= 8 KiB, L2) in every block's
//    prologue. No atomics, no in-launch hand-off, deterministic.
//  * Cache policy per stream (MI355X 256 MiB Infinity Cache): pass 1 reads x block-contiguously with
//    non-temporal loads (kCacheKeepBytes = 0: keeping x's tail on-die for pass 2 measured slower).
//    Pass 2 reads x non-temporally (x is dead afterwards) and writes the payload backwards with
//    allocating stores; decode reads the payload forwards, starting on the bytes pass 2 wrote last,
//    which are still in the Infinity Cache. Decode writes its fp32 output with non-temporal stores
//    (nothing re-reads it soon; it must not evict the next pass's lines). No output bit depends on it.
//
// Numerics: no fast-math, fp32 denormals preserved (gfx950 default), -ffp-contract=off. Scale and
// reciprocal are fp64 quotients rounded once to fp32 = the correctly rounded fp32 quotient (53 >= 2*24+2),
// independent of the compiler's fp32 division lowering.

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "adfl_slq.h"
#include "apply_device.h"  // the axpby / scale tail shared with stoch_codec.hip
#include "flush_device.h"  // the buffered servers' per-element flush and the fused kernels' tail
#include "slq_device.h"  // the device helpers shared with slq_delta.hip
#include "torch_sum_order.h"

namespace {

constexpr int kMaxFlatBlocks = 2048;               // 256 CUs x 8 resident 256-thread blocks
constexpr int kAbsmaxBlocks = 1024;                // pass-1 grid (block-contiguous ranges)
constexpr int kCountSlot = kMaxFlatBlocks;         // workspace word holding pass 1's partial count
constexpr int64_t kWorkspaceBytes = 16384;         // >= (kMaxFlatBlocks + 1) * 4, padded
constexpr int64_t kCacheKeepBytes = 0;             // tail of x pass 1 leaves in the Infinity Cache

template <bool ST_NT = false>
__device__ __forceinline__ void quantize_tile(const float4* __restrict__ x4, uint4* __restrict__ q16, float inv,
                                              uint32_t* __restrict__ lds, int lane) {
  float4 v[4];
  load_tile(x4, v, lane);
  quantize_tile_regs<ST_NT>(v, q16, inv, lds, lane);
}

template <bool LD_NT = false>
__device__ __forceinline__ void dequantize_tile(const uint4* __restrict__ q16, float4* __restrict__ o4, float s,
                                                uint32_t* __restrict__ lds, int lane) {
  reinterpret_cast<uint4*>(lds)[lane] = load16<LD_NT>(q16 + lane);
  __builtin_amdgcn_wave_barrier();
  uint32_t w[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) w[j] = lds[j * 64 + lane];
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int j = 0; j < 4; ++j) store4_nt(o4 + j * 64 + lane, dequant4(w[j], s));
}

// ------------------------------------------------------------------------------------------------
// flat kernels (one tensor)
// ------------------------------------------------------------------------------------------------
template <int U, bool NT>
__device__ __forceinline__ uint32_t absmax_range(const float4* __restrict__ x4, int64_t b0, int64_t b1) {
  uint32_t m = 0;
  int64_t i = b0 + threadIdx.x;
  for (; i + (U - 1) * kBlock < b1; i += U * kBlock) {
    float4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = load4<NT>(x4 + i + u * kBlock);
#pragma unroll
    for (int u = 0; u < U; ++u) m = max(m, abs_bits4(v[u]));
  }
  for (; i < b1; i += kBlock) m = max(m, abs_bits4(load4<NT>(x4 + i)));
  return m;
}

// Pass 1: block b owns float4s [b*per, (b+1)*per). Blocks wholly before the last keep4 float4s read
// non-temporally; the rest with allocating loads (they stay in the Infinity Cache for pass 2). The
// product uses keep4 = 0 (kCacheKeepBytes): measured, the non-temporal read's speed-up outweighs what
// pass 2 gains from finding x's tail on-die (profiles/r01/microbench_keep_sweep.txt).
template <int U>
__global__ __launch_bounds__(kBlock) void k_absmax_flat(const float* __restrict__ x, int64_t n, int64_t keep4,
                                                        uint32_t* __restrict__ partials) {
  const float4* x4 = reinterpret_cast<const float4*>(x);
  const int64_t n4 = n >> 2;
  const int64_t per = ((n4 + gridDim.x - 1) / gridDim.x + kBlock - 1) / kBlock * kBlock;
  const int64_t b0 = (int64_t)blockIdx.x * per;
  const int64_t b1 = min(n4, b0 + per);
  uint32_t m = (b1 <= n4 - keep4) ? absmax_range<U, true>(x4, b0, b1) : absmax_range<U, false>(x4, b0, b1);
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) m = max(m, abs_bits(x[(n4 << 2) + threadIdx.x]));
  m = block_max(m);
  if (threadIdx.x == 0) partials[blockIdx.x] = m;
  if (blockIdx.x == 0 && threadIdx.x == 0) partials[kCountSlot] = gridDim.x;  // self-describing workspace
}

// Pass 2: tiles walked from the END of x, so decode (which walks forwards) starts on the payload bytes
// written last. Template knobs exist for tools/microbench.hip; the ABI uses <true, false>.
template <bool REVERSE, bool ST_NT>
__global__ __launch_bounds__(kBlock) void k_quantize_flat(const float* __restrict__ x, int64_t n, float qmax,
                                                          const uint32_t* __restrict__ partials,
                                                          int8_t* __restrict__ q, float* __restrict__ scale_out) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kWaves][kTile / 4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float4* x4 = reinterpret_cast<const float4*>(x);
  uint4* q16 = reinterpret_cast<uint4*>(q);
  const int64_t ntiles = n / kTile;
  const int64_t wstride = (int64_t)gridDim.x * kWaves;
  int64_t t0 = (int64_t)blockIdx.x * kWaves + wave;
  // The first tile's loads do not need the scale: issue them before the partial reduction, whose
  // latency they then hide.
  float4 v[4];
  if (t0 < ntiles) load_tile(x4 + (REVERSE ? ntiles - 1 - t0 : t0) * (kTile / 4), v, lane);
  const ScaleInv si = make_scale(reduce_partials(partials, (int)partials[kCountSlot]), qmax);
  if (blockIdx.x == 0 && threadIdx.x == 0) *scale_out = si.scale;
  for (; t0 < ntiles; t0 += wstride) {
    const int64_t t = REVERSE ? ntiles - 1 - t0 : t0;
    if (t0 != (int64_t)blockIdx.x * kWaves + wave) load_tile(x4 + t * (kTile / 4), v, lane);
    quantize_tile_regs<ST_NT>(v, q16 + t * (kTile / 16), si.inv, lds[wave], lane);
  }
  if (blockIdx.x == gridDim.x - 1)
    for (int64_t i = ntiles * kTile + threadIdx.x; i < n; i += kBlock) q[i] = (int8_t)quant1(x[i], si.inv);
}

// max|x| as a value (torch.max(torch.abs(t)), quant.py:100): pass 1's partials reduced by one block. The
// abs bit patterns order like the magnitudes, and a NaN's pattern exceeds +inf's, so NaN propagates.
__global__ __launch_bounds__(kBlock) void k_absmax_value(const uint32_t* __restrict__ partials,
                                                         float* __restrict__ out) {
  const uint32_t m = reduce_partials(partials, (int)partials[kCountSlot]);
  if (threadIdx.x == 0) *out = __uint_as_float(m);
}

// Decode: tiles walked forwards (pass 2 wrote the head of the payload last). ABI: <false, false>.
template <bool REVERSE, bool LD_NT>
__global__ __launch_bounds__(kBlock) void k_dequantize_flat(const int8_t* __restrict__ q, int64_t n,
                                                            const float* __restrict__ scale_p,
                                                            float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kWaves][kTile / 4];
  const float s = *scale_p;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint4* q16 = reinterpret_cast<const uint4*>(q);
  float4* o4 = reinterpret_cast<float4*>(out);
  const int64_t ntiles = n / kTile;
  const int64_t wstride = (int64_t)gridDim.x * kWaves;
  for (int64_t t0 = (int64_t)blockIdx.x * kWaves + wave; t0 < ntiles; t0 += wstride) {
    const int64_t t = REVERSE ? ntiles - 1 - t0 : t0;
    dequantize_tile<LD_NT>(q16 + t * (kTile / 16), o4 + t * (kTile / 4), s, lds[wave], lane);
  }
  if (blockIdx.x == gridDim.x - 1)
    for (int64_t i = ntiles * kTile + threadIdx.x; i < n; i += kBlock) out[i] = s * (float)q[i];
}

// int4 decode tile: one coalesced 16-byte load per lane, LDS transpose, 8 coalesced float4 NT stores.
__device__ __forceinline__ void dequantize_tile_int4(const uint4* __restrict__ p16, float4* __restrict__ o4, float s,
                                                     uint16_t* __restrict__ lds, int lane) {
  reinterpret_cast<uint4*>(lds)[lane] = p16[lane];
  __builtin_amdgcn_wave_barrier();
  uint32_t h[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) h[j] = lds[j * 64 + lane];
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int j = 0; j < 8; ++j) store4_nt(o4 + j * 64 + lane, dequant2_int4(h[j], s));
}

// int4 pass 2 (flat).
__global__ __launch_bounds__(kBlock) void k_quantize_int4_flat(const float* __restrict__ x, int64_t n, float qmax,
                                                               const uint32_t* __restrict__ partials,
                                                               uint8_t* __restrict__ packed,
                                                               float* __restrict__ scale_out) {
  __shared__ __attribute__((aligned(16))) uint16_t lds[kWaves][kTile4 / 4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float4* x4 = reinterpret_cast<const float4*>(x);
  uint4* p16 = reinterpret_cast<uint4*>(packed);
  const int64_t ntiles = n / kTile4;
  const int64_t wstride = (int64_t)gridDim.x * kWaves;
  const int64_t first = (int64_t)blockIdx.x * kWaves + wave;
  // the first tile's loads do not need the scale: issued before the partial reduction they hide
  float4 v[8];
  if (first < ntiles) load_tile_int4(x4 + (ntiles - 1 - first) * (kTile4 / 4), v, lane);
  const ScaleInv si = make_scale(reduce_partials(partials, (int)partials[kCountSlot]), qmax);
  if (blockIdx.x == 0 && threadIdx.x == 0) *scale_out = si.scale;
  for (int64_t t0 = first; t0 < ntiles; t0 += wstride) {
    const int64_t t = ntiles - 1 - t0;
    if (t0 != first) load_tile_int4(x4 + t * (kTile4 / 4), v, lane);
    quantize_tile_int4_regs(v, p16 + t * 64, si.inv, lds[wave], lane);
  }
  if (blockIdx.x == gridDim.x - 1) {
    const int64_t np = (n + 1) >> 1;
    for (int64_t j = ntiles * (kTile4 / 2) + threadIdx.x; j < np; j += kBlock) {
      const int hi = quant1(x[2 * j], si.inv);
      const int lo = (2 * j + 1 < n) ? quant1(x[2 * j + 1], si.inv) : 0;  // pad one zero (compression.py:42-43)
      packed[j] = (uint8_t)pack_pair(hi, lo);
    }
  }
}

// int4 decode (flat).
__global__ __launch_bounds__(kBlock) void k_dequantize_int4_flat(const uint8_t* __restrict__ packed, int64_t n,
                                                                 const float* __restrict__ scale_p,
                                                                 float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint16_t lds[kWaves][kTile4 / 4];
  const float s = *scale_p;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint4* p16 = reinterpret_cast<const uint4*>(packed);
  float4* o4 = reinterpret_cast<float4*>(out);
  const int64_t ntiles = n / kTile4;
  const int64_t wstride = (int64_t)gridDim.x * kWaves;
  for (int64_t t = (int64_t)blockIdx.x * kWaves + wave; t < ntiles; t += wstride)
    dequantize_tile_int4(p16 + t * 64, o4 + t * (kTile4 / 4), s, lds[wave], lane);
  if (blockIdx.x == gridDim.x - 1)
    for (int64_t i = ntiles * kTile4 + threadIdx.x; i < n; i += kBlock) {
      float e0, e1;
      dequant_byte_int4(packed[i >> 1], s, e0, e1);
      out[i] = (i & 1) ? e1 : e0;
    }
}

// Standalone pack_4bit / unpack_4bit over int8 payloads (compression.py:35-66).
__global__ __launch_bounds__(kBlock) void k_pack_int4(const int8_t* __restrict__ q, int64_t n,
                                                      uint8_t* __restrict__ packed) {
  const int64_t np = (n + 1) >> 1;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < np; j += stride) {
    const int hi = q[2 * j];
    const int lo = (2 * j + 1 < n) ? (int)q[2 * j + 1] : 0;
    packed[j] = (uint8_t)pack_pair(hi, lo);
  }
}

__global__ __launch_bounds__(kBlock) void k_unpack_int4(const uint8_t* __restrict__ packed, int64_t n,
                                                        int8_t* __restrict__ q) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    const uint32_t b = packed[i >> 1];
    q[i] = (int8_t)((i & 1) ? (int)(b & 0xfu) - 8 : (int)((b >> 4) & 0xfu) - 8);
  }
}

// Peer-exchange epilogue / synchronous aggregate: mean of K dequantized rows in torch's summation order
// (torch_sum_order.h: the CPU sum(stack(rows), dim=0) that stack(...).mean(0) at ray_ad.py:188 and
// simple_aggregate at model.py:229-231 compute), then a correctly rounded division by K. The row sequence is
// rows r != self_row in r order, then (self_row >= 0) the rank's own fp32 update self_x, exactly, LAST
// (async_peer.py:170-174 / ray_ad.py:183-188 append the local parameters after the received updates).
// Vector tiles are SEQ-order columns of the one tensor (a tile ends below n & ~31); the < 1024 tail elements
// take each element's own order. Per row: one coalesced 16-byte load per lane + LDS transpose; output:
// coalesced NT float4 stores. DEEP: K >= 256 (the cascade's levels 2-3).
__device__ __forceinline__ int seq_row(int s, int self_row) { return (self_row >= 0 && s >= self_row) ? s + 1 : s; }

// Element e of the rows, summed in torch's order for tensor-relative index j of an n-element tensor.
template <class Dequant>
__device__ __forceinline__ float mean_elem_torch(const Dequant& dq, int k, int self_row,
                                                 const float* __restrict__ self_x, int64_t e, int64_t j, int64_t n,
                                                 double dk) {
  auto get = [&](int s) -> float {
    if (self_row >= 0 && s == k - 1) return self_x[e];
    return dq(seq_row(s, self_row), e);
  };
  return (float)((double)adfl_sum::sum_elem(get, k, adfl_sum::mode_of(j, n, k)) / dk);
}

template <bool DEEP>
__global__ __launch_bounds__(kBlock) void k_dequantize_mean(const int8_t* __restrict__ q, int64_t row_stride, int k,
                                                            int64_t n, const float* __restrict__ scales,
                                                            int64_t scale_stride, int self_row,
                                                            const float* __restrict__ self_x,
                                                            float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kWaves][kTile / 4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t ntiles = n / kTile;
  const int64_t wstride = (int64_t)gridDim.x * kWaves;
  const double dk = (double)k;
  for (int64_t t = (int64_t)blockIdx.x * kWaves + wave; t < ntiles; t += wstride) {
    adfl_sum::SeqTile<4, DEEP> acc;
    acc.init();
    for (int r = 0; r < k; ++r) {
      if (r == self_row) continue;
      const uint4* q16 = reinterpret_cast<const uint4*>(q + r * row_stride) + t * (kTile / 16);
      const float s = scales[r * scale_stride];
      reinterpret_cast<uint4*>(lds[wave])[lane] = q16[lane];
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int j = 0; j < 4; ++j) acc.add(j, dequant4(lds[wave][j * 64 + lane], s));
      __builtin_amdgcn_wave_barrier();
      acc.step();
    }
    if (self_row >= 0) {
      const float4* xs = reinterpret_cast<const float4*>(self_x) + t * (kTile / 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc.add(j, xs[j * 64 + lane]);
      acc.step();
    }
    float4* o4 = reinterpret_cast<float4*>(out) + t * (kTile / 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) store4_nt(o4 + j * 64 + lane, div4(acc.result(j), dk));
  }
  if (blockIdx.x == gridDim.x - 1) {
    auto dq = [&](int r, int64_t e) -> float { return scales[r * scale_stride] * (float)q[r * row_stride + e]; };
    for (int64_t i = ntiles * kTile + threadIdx.x; i < n; i += kBlock)
      out[i] = mean_elem_torch(dq, k, self_row, self_x, i, i, n, dk);
  }
}

// Same over K int4-packed rows (2048-element wave tiles, 1 KiB of packed bytes per row per tile).
template <bool DEEP>
__global__ __launch_bounds__(kBlock) void k_dequantize_mean_int4(const uint8_t* __restrict__ p, int64_t row_stride,
                                                                 int k, int64_t n, const float* __restrict__ scales,
                                                                 int64_t scale_stride, int self_row,
                                                                 const float* __restrict__ self_x,
                                                                 float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint16_t lds[kWaves][kTile4 / 4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t ntiles = n / kTile4;
  const int64_t wstride = (int64_t)gridDim.x * kWaves;
  const double dk = (double)k;
  for (int64_t t = (int64_t)blockIdx.x * kWaves + wave; t < ntiles; t += wstride) {
    adfl_sum::SeqTile<8, DEEP> acc;
    acc.init();
    for (int r = 0; r < k; ++r) {
      if (r == self_row) continue;
      const uint4* p16 = reinterpret_cast<const uint4*>(p + r * row_stride) + t * 64;
      const float s = scales[r * scale_stride];
      reinterpret_cast<uint4*>(lds[wave])[lane] = p16[lane];
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int j = 0; j < 8; ++j) acc.add(j, dequant2_int4(lds[wave][j * 64 + lane], s));
      __builtin_amdgcn_wave_barrier();
      acc.step();
    }
    if (self_row >= 0) {
      const float4* xs = reinterpret_cast<const float4*>(self_x) + t * (kTile4 / 4);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc.add(j, xs[j * 64 + lane]);
      acc.step();
    }
    float4* o4 = reinterpret_cast<float4*>(out) + t * (kTile4 / 4);
#pragma unroll
    for (int j = 0; j < 8; ++j) store4_nt(o4 + j * 64 + lane, div4(acc.result(j), dk));
  }
  if (blockIdx.x == gridDim.x - 1) {
    auto dq = [&](int r, int64_t e) -> float {
      float e0, e1;
      dequant_byte_int4(p[r * row_stride + (e >> 1)], scales[r * scale_stride], e0, e1);
      return (e & 1) ? e1 : e0;
    };
    for (int64_t i = ntiles * kTile4 + threadIdx.x; i < n; i += kBlock)
      out[i] = mean_elem_torch(dq, k, self_row, self_x, i, i, n, dk);
  }
}

// ------------------------------------------------------------------------------------------------
// Pass 1: one partial per chunk, all of the chunk's loads in flight. Non-temporal: in the C3 config
// bench, allocating loads (x left in the Infinity Cache for pass 2) measured the same (A/B in
// profiles/r01/c3_absmax_policy.txt), and NT leaves the cache to the payload.
// chunk_base: the first chunk of the launch (adfl_slq_absmax_batched_range; 0 for the whole table).
__global__ __launch_bounds__(kBlock) void k_absmax_batched(const float* __restrict__ x,
                                                           const adfl_slq_chunk* __restrict__ chunks,
                                                           uint32_t* __restrict__ partials,
                                                           int64_t chunk_base = 0) {
  const int64_t ci = chunk_base + blockIdx.x;
  const adfl_slq_chunk c = chunks[ci];
  const float* xc = x + c.start;
  const int head = chunk_head(c.start, c.len, 4);
  const float4* x4 = reinterpret_cast<const float4*>(xc + head);
  const int n4 = (c.len - head) >> 2;
  constexpr int U = ADFL_SLQ_CHUNK_ELEMS / 4 / kBlock;  // 8 float4 per thread
  float4 v[U];
#pragma unroll
  for (int k = 0; k < U; ++k) {
    const int i = (int)threadIdx.x + k * kBlock;
    v[k] = i < n4 ? load4<true>(x4 + i) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  uint32_t m = 0;
  if (threadIdx.x < head) m = abs_bits(xc[threadIdx.x]);
  const int tail = head + (n4 << 2);
  if (threadIdx.x < c.len - tail) m = max(m, abs_bits(xc[tail + threadIdx.x]));
#pragma unroll
  for (int k = 0; k < U; ++k) m = max(m, abs_bits4(v[k]));
  m = block_max(m);
  if (threadIdx.x == 0) partials[ci] = m;
}

// Pass 2: the chunk's loads are issued before the partial reduction, whose latency they hide.
// chunk_base: the first chunk of the launch (adfl_slq_quantize_batched_range; 0 for the whole table).
__global__ __launch_bounds__(kBlock) void k_quantize_batched(const float* __restrict__ x,
                                                             const adfl_slq_chunk* __restrict__ chunks,
                                                             float qmax, const uint32_t* __restrict__ partials,
                                                             int8_t* __restrict__ q, float* __restrict__ scales,
                                                             int64_t chunk_base = 0) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kWaves][kTile / 4];
  const int64_t ci = chunk_base + blockIdx.x;
  const adfl_slq_chunk c = chunks[ci];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  ChunkRegs r;
  chunk_load(x, c, r, lane, wave);
  const ScaleInv si = make_scale(reduce_partials(partials + c.first_chunk, c.nchunks), qmax);
  if (ci == c.first_chunk && threadIdx.x == 0) scales[c.tensor] = si.scale;
  chunk_store(c, r, si.inv, q, lds[wave], lane, wave);
}

// A one-launch encode for tensors of any size (chunk blocks meeting per tensor in a cooperative launch) was
// measured in round 2 and removed in round 3: the cooperative launch cost ~20 us more than an ordinary
// one on C3 (log-uniform 43 vs 24.7 us two-pass; equal 38 vs 17 us resident; profiles/r02/coop/).


// ---- one-launch encode of a bucket of small tensors (a whole tensor per block, x read once) -------
// A tensor of up to kSegChunks chunks (<= 65536 elements) fits the VGPRs of one 1024-thread block
// (16 waves x 4 wave tiles x 4 float4 per lane = 64 VGPRs). When EVERY tensor of the bucket does, the
// encode is one launch: each block loads its whole tensor, reduces max|x| in-block, forms the scale and
// quantizes from registers — no cross-block dependency, no second pass, x read once (5 B/element
// instead of 9). C3's 256 x 45,662 layout: encode 22.8 -> 16.4 us, round trip 0.63 -> 0.78 of 8 TB/s
// with the Infinity Cache flushed (profiles/r02/microbench_c3.txt).
// Blocks walk a host-built work list (adfl_slq_build_encode_work: the first chunk of every tensor), so no
// block is launched only to exit: a 1024-thread block takes a whole CU's wave slots, and idle ones queued
// behind the working blocks (27.6 us with the chunk table as the grid).
// With any larger tensor the two-pass encode runs instead: big blocks pay off only while there are about
// as many of them as CUs, and segmenting the large tensors (one absmax per 65,536-element segment, then
// a segment quantize launch) measured slower than the two passes (log-uniform layout: 28.4 vs 23.9 us).
// work[b] = the first chunk of tensor b (every tensor <= kSegChunks chunks).
// ST_NT: non-temporal payload stores. The block's stores are the tail of a launch in which every CU loads,
// reduces and stores in lockstep (tools/microbench_resident_timeline.hip: entry spread 0.6 us, block max
// at 8.5 us, stores acknowledged at 11.5-12 us); streaming them past the L2 shortens the encode (15.7 vs
// 16.6 us, profiles/r03/c3_resident/timeline.txt) but the decode that follows then reads the payload from
// HBM: C3 round trip 30.3 vs 27.0 us (profiles/r03/c3_resident/c3_nt_stores.json). kResidentNtStores = false.
template <bool ST_NT>
__global__ __launch_bounds__(kSegBlock) void k_encode_resident(const float* __restrict__ x,
                                                               const adfl_slq_chunk* __restrict__ chunks,
                                                               const int32_t* __restrict__ work, float qmax,
                                                               int8_t* __restrict__ q, float* __restrict__ scales) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kSegWaves][kTile / 4];
  const int64_t ci = work[blockIdx.x];
  const adfl_slq_chunk c = chunks[ci];
  if (c.nchunks > kSegChunks) {  // not a resident work list (a direct C caller's): NaN scale, nothing written
    if (threadIdx.x == 0) scales[c.tensor] = __builtin_nanf("");
    return;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int len = (c.nchunks - 1) * ADFL_SLQ_CHUNK_ELEMS + chunks[ci + c.nchunks - 1].len;
  const float* xt = x + c.start;
  // all of the tensor's loads in flight at once (x non-temporal: dead after this pass)
  const int head = chunk_head(c.start, len, 16);
  const int ntiles = (len - head) / kTile;
  const float4* x4 = reinterpret_cast<const float4*>(xt + head);
  float4 v[kSegTilesPerWave][4];
#pragma unroll
  for (int k = 0; k < kSegTilesPerWave; ++k) {
    const int t = wave + k * kSegWaves;
    if (t < ntiles) {
      load_tile(x4 + t * (kTile / 4), v[k], lane);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[k][j] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  const float hv = (int)threadIdx.x < head ? xt[threadIdx.x] : 0.0f;
  const int ti = head + ntiles * kTile + (int)threadIdx.x;  // < 1024 tail elements: one per thread
  const float tv = ti < len ? __builtin_nontemporal_load(xt + ti) : 0.0f;
  uint32_t m = max(abs_bits(hv), abs_bits(tv));
#pragma unroll
  for (int k = 0; k < kSegTilesPerWave; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j) m = max(m, abs_bits4(v[k][j]));
  const ScaleInv si = make_scale(block_max_seg(m), qmax);
  if (threadIdx.x == 0) scales[c.tensor] = si.scale;
  int8_t* qt = q + c.start;
  uint4* q16 = reinterpret_cast<uint4*>(qt + head);
#pragma unroll
  for (int k = 0; k < kSegTilesPerWave; ++k) {
    const int t = wave + k * kSegWaves;
    if (t < ntiles) quantize_tile_regs<ST_NT>(v[k], q16 + t * (kTile / 16), si.inv, lds[wave], lane);
  }
  if ((int)threadIdx.x < head) qt[threadIdx.x] = (int8_t)quant1(hv, si.inv);
  if (ti < len) qt[ti] = (int8_t)quant1(tv, si.inv);
}
constexpr bool kResidentNtStores = false;

// int4 variant (PackedSLQChannel's buckets: even tensor offsets, packed byte e/2 = flat elements e, e+1):
// 2048-element int4 wave tiles, 2 per wave (16 float4 per lane); the < 32-element head and the < 2048-
// element tail go pairwise, one pair per thread, an odd tensor's last element paired with pack_4bit's
// zero pad (compression.py:42-43).
constexpr int kSegTiles4PerWave = (int)(kSegMaxElems / kTile4 / kSegWaves);  // 2
static_assert(kSegTiles4PerWave * kTile4 * kSegWaves == kSegMaxElems, "int4 tiles cover a segment");
static_assert(2 * kSegBlock == kTile4, "int4 tail: one pair per thread");

__global__ __launch_bounds__(kSegBlock) void k_encode_resident_int4(const float* __restrict__ x,
                                                                    const adfl_slq_chunk* __restrict__ chunks,
                                                                    const int32_t* __restrict__ work, float qmax,
                                                                    uint8_t* __restrict__ packed,
                                                                    float* __restrict__ scales) {
  __shared__ __attribute__((aligned(16))) uint16_t lds[kSegWaves][kTile4 / 4];
  const int64_t ci = work[blockIdx.x];
  const adfl_slq_chunk c = chunks[ci];
  if (c.nchunks > kSegChunks) {  // not a resident work list (a direct C caller's): NaN scale, nothing written
    if (threadIdx.x == 0) scales[c.tensor] = __builtin_nanf("");
    return;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int len = (c.nchunks - 1) * ADFL_SLQ_CHUNK_ELEMS + chunks[ci + c.nchunks - 1].len;
  const float* xt = x + c.start;
  const int head = chunk_head(c.start, len, 32);  // even: tensor offsets are even
  const int ntiles = (len - head) / kTile4;
  const float4* x4 = reinterpret_cast<const float4*>(xt + head);
  float4 v[kSegTiles4PerWave][8];
#pragma unroll
  for (int k = 0; k < kSegTiles4PerWave; ++k) {
    const int t = wave + k * kSegWaves;
    if (t < ntiles) {
      load_tile_int4(x4 + t * (kTile4 / 4), v[k], lane);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[k][j] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  // head pair (element 2*tid of [0, head)) and tail pair (t0 + 2*tid of [t0, len))
  const int hi = 2 * (int)threadIdx.x;
  const bool has_h = hi < head;
  const float h0 = has_h ? xt[hi] : 0.0f, h1 = (has_h && hi + 1 < len) ? xt[hi + 1] : 0.0f;
  const int ti = head + ntiles * kTile4 + 2 * (int)threadIdx.x;
  const bool has_t = ti < len;
  const float t0v = has_t ? __builtin_nontemporal_load(xt + ti) : 0.0f;
  const float t1v = (has_t && ti + 1 < len) ? __builtin_nontemporal_load(xt + ti + 1) : 0.0f;
  uint32_t m = max(max(abs_bits(h0), abs_bits(h1)), max(abs_bits(t0v), abs_bits(t1v)));
#pragma unroll
  for (int k = 0; k < kSegTiles4PerWave; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) m = max(m, abs_bits4(v[k][j]));
  const ScaleInv si = make_scale(block_max_seg(m), qmax);
  if (threadIdx.x == 0) scales[c.tensor] = si.scale;
  uint8_t* pt = packed + (c.start >> 1);
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

__global__ __launch_bounds__(kBlock) void k_dequantize_batched(const int8_t* __restrict__ q,
                                                               const adfl_slq_chunk* __restrict__ chunks,
                                                               const float* __restrict__ scales,
                                                               float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kWaves][kTile / 4];
  const adfl_slq_chunk c = chunks[blockIdx.x];
  const float s = scales[c.tensor];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int8_t* qc = q + c.start;
  float* oc = out + c.start;
  const int head = chunk_head(c.start, c.len, 16);
  if (threadIdx.x < head) oc[threadIdx.x] = s * (float)qc[threadIdx.x];
  const int ntiles = (c.len - head) / kTile;
  for (int t = wave; t < ntiles; t += kWaves)
    dequantize_tile(reinterpret_cast<const uint4*>(qc + head) + t * (kTile / 16),
                    reinterpret_cast<float4*>(oc + head) + t * (kTile / 4), s, lds[wave], lane);
  for (int i = head + ntiles * kTile + threadIdx.x; i < c.len; i += kBlock) oc[i] = s * (float)qc[i];
}

// Peer mean of K bucketed payloads with per-tensor scales — the decentralized exchange of a whole state dict
// under SLQChannel's per-tensor codec (ray_ad.py:164-190 averaging every tensor; quant.py:74-94 giving each
// tensor its own scale), and SLQChannel.receive_mean (simple_aggregate over K decoded dicts, model.py:221-234):
// for tensor t and element i of the bucket, the torch-order sum (torch_sum_order.h, per tensor: the column
// index is i's offset in its tensor) of fp32(scale_r[t] * q_r[i]) over the row sequence (rows != self_row in
// r order, then self_x[i]), then / K correctly rounded — k_dequantize_mean's arithmetic per tensor. Row r's
// payload is q + r * row_stride (one bucket payload each, the same layout), its scales
// scales + r * scale_stride. One block per chunk: wave tiles over the chunk's SEQ columns (16-element aligned
// in the bucket), the < 16 head elements and everything past the tiles element-wise in each one's order.
struct TensorSpan {
  int64_t start, n;  // the chunk's tensor: bucket offset and element count
};
__device__ __forceinline__ TensorSpan tensor_span(const adfl_slq_chunk* __restrict__ chunks, const adfl_slq_chunk& c) {
  TensorSpan t;
  t.start = chunks[c.first_chunk].start;
  t.n = (int64_t)(c.nchunks - 1) * ADFL_SLQ_CHUNK_ELEMS + chunks[c.first_chunk + c.nchunks - 1].len;
  return t;
}

// wave tiles of `tile` elements the chunk can take: from `head` up to the tensor's last SEQ column
__device__ __forceinline__ int seq_tiles(const adfl_slq_chunk& c, const TensorSpan& ts, int head, int tile) {
  int64_t lim = ts.start + adfl_sum::seq_end(ts.n) - c.start;  // chunk-relative end of the SEQ columns
  lim = lim < c.len ? lim : c.len;
  return lim > head ? (int)((lim - head) / tile) : 0;
}

template <bool DEEP>
__global__ __launch_bounds__(kBlock) void k_dequantize_mean_batched(const int8_t* __restrict__ q, int64_t row_stride,
                                                                    int k, const adfl_slq_chunk* __restrict__ chunks,
                                                                    const float* __restrict__ scales,
                                                                    int64_t scale_stride, int self_row,
                                                                    const float* __restrict__ self_x,
                                                                    float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kWaves][kTile / 4];
  const adfl_slq_chunk c = chunks[blockIdx.x];
  const TensorSpan ts = tensor_span(chunks, c);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double dk = (double)k;
  const int head = chunk_head(c.start, c.len, 16);
  const int ntiles = seq_tiles(c, ts, head, kTile);
  auto dq = [&](int r, int64_t e) -> float {
    return scales[r * scale_stride + c.tensor] * (float)q[r * row_stride + e];
  };
  if ((int)threadIdx.x < head) {
    const int64_t e = c.start + threadIdx.x;
    out[e] = mean_elem_torch(dq, k, self_row, self_x, e, e - ts.start, ts.n, dk);
  }
  for (int t = wave; t < ntiles; t += kWaves) {
    const int64_t base = c.start + head + (int64_t)t * kTile;  // 16-element aligned
    adfl_sum::SeqTile<4, DEEP> acc;
    acc.init();
    for (int r = 0; r < k; ++r) {
      if (r == self_row) continue;
      const uint4* q16 = reinterpret_cast<const uint4*>(q + r * row_stride + base);
      const float s = scales[r * scale_stride + c.tensor];
      reinterpret_cast<uint4*>(lds[wave])[lane] = q16[lane];
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int j = 0; j < 4; ++j) acc.add(j, dequant4(lds[wave][j * 64 + lane], s));
      __builtin_amdgcn_wave_barrier();
      acc.step();
    }
    if (self_row >= 0) {
      const float4* xs = reinterpret_cast<const float4*>(self_x + base);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc.add(j, xs[j * 64 + lane]);
      acc.step();
    }
    float4* o4 = reinterpret_cast<float4*>(out + base);
#pragma unroll
    for (int j = 0; j < 4; ++j) store4_nt(o4 + j * 64 + lane, div4(acc.result(j), dk));
  }
  for (int i = head + ntiles * kTile + threadIdx.x; i < c.len; i += kBlock) {
    const int64_t e = c.start + i;
    out[e] = mean_elem_torch(dq, k, self_row, self_x, e, e - ts.start, ts.n, dk);
  }
}

// The same mean over K int4-packed bucket payloads (PackedSLQChannel per tensor; encode_batched_int4's
// layout: even tensor offsets, flat element e in byte e/2, high nibble for even e). Heads run to a 32-element
// (16-byte) boundary, wave tiles are kTile4 = 2048 elements = 1 KiB of packed bytes per row.
template <bool DEEP>
__global__ __launch_bounds__(kBlock) void k_dequantize_mean_batched_int4(
    const uint8_t* __restrict__ p, int64_t row_stride, int k, const adfl_slq_chunk* __restrict__ chunks,
    const float* __restrict__ scales, int64_t scale_stride, int self_row, const float* __restrict__ self_x,
    float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint16_t lds[kWaves][kTile4 / 4];
  const adfl_slq_chunk c = chunks[blockIdx.x];
  const TensorSpan ts = tensor_span(chunks, c);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double dk = (double)k;
  const int head = chunk_head(c.start, c.len, 32);
  const int ntiles = seq_tiles(c, ts, head, kTile4);
  auto dq = [&](int r, int64_t e) -> float {
    float e0, e1;
    dequant_byte_int4(p[r * row_stride + (e >> 1)], scales[r * scale_stride + c.tensor], e0, e1);
    return (e & 1) ? e1 : e0;
  };
  if ((int)threadIdx.x < head) {
    const int64_t e = c.start + threadIdx.x;
    out[e] = mean_elem_torch(dq, k, self_row, self_x, e, e - ts.start, ts.n, dk);
  }
  for (int t = wave; t < ntiles; t += kWaves) {
    const int64_t base = c.start + head + (int64_t)t * kTile4;  // 32-element aligned
    adfl_sum::SeqTile<8, DEEP> acc;
    acc.init();
    for (int r = 0; r < k; ++r) {
      if (r == self_row) continue;
      const uint4* p16 = reinterpret_cast<const uint4*>(p + r * row_stride + (base >> 1));
      const float s = scales[r * scale_stride + c.tensor];
      reinterpret_cast<uint4*>(lds[wave])[lane] = p16[lane];
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int j = 0; j < 8; ++j) acc.add(j, dequant2_int4(lds[wave][j * 64 + lane], s));
      __builtin_amdgcn_wave_barrier();
      acc.step();
    }
    if (self_row >= 0) {
      const float4* xs = reinterpret_cast<const float4*>(self_x + base);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc.add(j, xs[j * 64 + lane]);
      acc.step();
    }
    float4* o4 = reinterpret_cast<float4*>(out + base);
#pragma unroll
    for (int j = 0; j < 8; ++j) store4_nt(o4 + j * 64 + lane, div4(acc.result(j), dk));
  }
  for (int i = head + ntiles * kTile4 + threadIdx.x; i < c.len; i += kBlock) {
    const int64_t e = c.start + i;
    out[e] = mean_elem_torch(dq, k, self_row, self_x, e, e - ts.start, ts.n, dk);
  }
}

// Synchronous DELTA server step: Simple(CommType.DELTA, sync=True)._sync_update (Strategy/simple.py:87-89),
// add_parameters(g, simple_aggregate(K decodes), alpha, beta) in one launch. The mean kernels above with another
// tail (MeanAxpbyOut, apply_device.h): m is the value k_dequantize_mean_batched[_int4] writes (no self row), and
//   out = fp32(fp32(alpha * g) + fp32(beta * m))          apply_device.h's AXPBY, never an FMA
// with g and out addressed as server_flush.hip addresses its operands: one fp32 pointer per tensor (a.base /
// a.out, ntargets == 1), so separate tensors and bucket + offset[t] are one form. A tensor's slot in the payload
// bucket and its g / out tensor generally differ in phase: when the chunk's tile slices of g and out are both
// 16-byte aligned (every tile of a chunk starts a multiple of 1024 elements after the first, so the choice is
// block-uniform) they take 16-byte accesses, otherwise 4-byte accesses of the same elements. A tile's g is loaded
// before its row loop, so its latency hides under the K payload rows. Out of place the output takes the decode's
// non-temporal stores; in place (out == g: the thread that writes an element is the one that read it) plain ones.
template <bool DEEP>
__global__ __launch_bounds__(kBlock) void k_dequantize_mean_axpby_batched(const int8_t* __restrict__ q,
                                                                          int64_t row_stride, int k,
                                                                          const adfl_slq_chunk* __restrict__ chunks,
                                                                          const float* __restrict__ scales,
                                                                          int64_t scale_stride, ApplyTargets a) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kWaves][kTile / 4];
  const adfl_slq_chunk c = chunks[blockIdx.x];
  const TensorSpan ts = tensor_span(chunks, c);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double dk = (double)k;
  const int head = chunk_head(c.start, c.len, 16);
  const int ntiles = seq_tiles(c, ts, head, kTile);
  const MeanAxpbyOut w(a, c, c.start - ts.start, head);
  auto dq = [&](int r, int64_t e) -> float {
    return scales[r * scale_stride + c.tensor] * (float)q[r * row_stride + e];
  };
  auto one = [&](int i) {
    const int64_t e = c.start + i;
    w.store1(i, mean_elem_torch(dq, k, -1, nullptr, e, e - ts.start, ts.n, dk));
  };
  if ((int)threadIdx.x < head) one(threadIdx.x);
  for (int t = wave; t < ntiles; t += kWaves) {
    const int off = head + t * kTile;           // chunk-relative
    const int64_t base = c.start + off;         // 16-element aligned in the payload bucket
    float4 gv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) gv[j] = w.load4g(off + 4 * (j * 64 + lane));
    adfl_sum::SeqTile<4, DEEP> acc;
    acc.init();
    for (int r = 0; r < k; ++r) {
      const uint4* q16 = reinterpret_cast<const uint4*>(q + r * row_stride + base);
      const float s = scales[r * scale_stride + c.tensor];
      reinterpret_cast<uint4*>(lds[wave])[lane] = q16[lane];
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int j = 0; j < 4; ++j) acc.add(j, dequant4(lds[wave][j * 64 + lane], s));
      __builtin_amdgcn_wave_barrier();
      acc.step();
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) w.store4(off + 4 * (j * 64 + lane), gv[j], div4(acc.result(j), dk));
  }
  for (int i = head + ntiles * kTile + threadIdx.x; i < c.len; i += kBlock) one(i);
}

template <bool DEEP>
__global__ __launch_bounds__(kBlock) void k_dequantize_mean_axpby_batched_int4(
    const uint8_t* __restrict__ p, int64_t row_stride, int k, const adfl_slq_chunk* __restrict__ chunks,
    const float* __restrict__ scales, int64_t scale_stride, ApplyTargets a) {
  __shared__ __attribute__((aligned(16))) uint16_t lds[kWaves][kTile4 / 4];
  const adfl_slq_chunk c = chunks[blockIdx.x];
  const TensorSpan ts = tensor_span(chunks, c);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double dk = (double)k;
  const int head = chunk_head(c.start, c.len, 32);
  const int ntiles = seq_tiles(c, ts, head, kTile4);
  const MeanAxpbyOut w(a, c, c.start - ts.start, head);
  auto dq = [&](int r, int64_t e) -> float {
    float e0, e1;
    dequant_byte_int4(p[r * row_stride + (e >> 1)], scales[r * scale_stride + c.tensor], e0, e1);
    return (e & 1) ? e1 : e0;
  };
  auto one = [&](int i) {
    const int64_t e = c.start + i;
    w.store1(i, mean_elem_torch(dq, k, -1, nullptr, e, e - ts.start, ts.n, dk));
  };
  if ((int)threadIdx.x < head) one(threadIdx.x);
  for (int t = wave; t < ntiles; t += kWaves) {
    const int off = head + t * kTile4;          // chunk-relative
    const int64_t base = c.start + off;         // 32-element aligned in the payload bucket
    float4 gv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) gv[j] = w.load4g(off + 4 * (j * 64 + lane));
    adfl_sum::SeqTile<8, DEEP> acc;
    acc.init();
    for (int r = 0; r < k; ++r) {
      const uint4* p16 = reinterpret_cast<const uint4*>(p + r * row_stride + (base >> 1));
      const float s = scales[r * scale_stride + c.tensor];
      reinterpret_cast<uint4*>(lds[wave])[lane] = p16[lane];
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int j = 0; j < 8; ++j) acc.add(j, dequant2_int4(lds[wave][j * 64 + lane], s));
      __builtin_amdgcn_wave_barrier();
      acc.step();
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) w.store4(off + 4 * (j * 64 + lane), gv[j], div4(acc.result(j), dk));
  }
  for (int i = head + ntiles * kTile4 + threadIdx.x; i < c.len; i += kBlock) one(i);
}

// Decode + accumulate into K models (pool.py:62-75, qafel.py:176-179 via model.py:337-347): the chunk's
// payload is decoded once into registers (8 float4 per thread), then every model's slice is read, added
// (fp32(a + d), what mul_(1).add_(d, alpha=1) computes) and written back with 16-byte accesses when the
// tensor's offset in the bucket is a multiple of 4 (the payload dwords and the targets' float4s line up).
// Any other offset (a compact bucket) takes an element-wise path with the same sums: every chunk of a
// tensor shares its offset's residue mod 4, so the branch is block-uniform.
__global__ __launch_bounds__(kBlock) void k_dequantize_add_batched(const int8_t* __restrict__ q,
                                                                   const adfl_slq_chunk* __restrict__ chunks,
                                                                   const float* __restrict__ scales,
                                                                   float* const* __restrict__ targets,
                                                                   int ntensors, int ntargets) {
  constexpr int kPer = ADFL_SLQ_CHUNK_ELEMS / 4 / kBlock;
  const adfl_slq_chunk c = chunks[blockIdx.x];
  const float s = scales[c.tensor];
  const int64_t in_tensor = (int64_t)(blockIdx.x - c.first_chunk) * ADFL_SLQ_CHUNK_ELEMS;
  const int8_t* qc = q + c.start;
  if (c.start & 3) {
    for (int m = 0; m < ntargets; ++m) {
      float* tg = targets[(int64_t)m * ntensors + c.tensor] + in_tensor;
      for (int i = threadIdx.x; i < c.len; i += kBlock) tg[i] = tg[i] + s * (float)qc[i];
    }
    return;
  }
  const uint32_t* q4 = reinterpret_cast<const uint32_t*>(qc);
  const int n4 = c.len >> 2;
  float4 dv[kPer];
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int k = threadIdx.x + j * kBlock;
    dv[j] = k < n4 ? dequant4(q4[k], s) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const int tail = n4 << 2;
  const bool has_tail = (int)threadIdx.x < c.len - tail;
  const float dt = has_tail ? s * (float)qc[tail + threadIdx.x] : 0.0f;
  for (int m = 0; m < ntargets; ++m) {
    float* tg = targets[(int64_t)m * ntensors + c.tensor] + in_tensor;
    float4* t4 = reinterpret_cast<float4*>(tg);
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int k = threadIdx.x + j * kBlock;
      if (k < n4) t4[k] = add4(t4[k], dv[j]);
    }
    if (has_tail) tg[tail + threadIdx.x] = tg[tail + threadIdx.x] + dt;
  }
}

// Decode + axpby / scale — the asynchronous server's update step on every client update: FedAsync's
// add_parameters(g, decoded, 1 - a_t, a_t) (Strategy/fed_async.py:80-81), Simple DELTA's add_parameters(g,
// decoded, 1, 1) (Strategy/simple.py:100) and FedBuff's tensor.float().mul_(f) then add_parameters_inpace(buffer,
// decoded, 1, 1) (Strategy/fed_buff.py:72-80). k_dequantize_add_batched's shape: when the tensor's offset in the
// bucket is a multiple of 4 (block-uniform: every chunk of a tensor shares its offset's residue mod 4) the chunk's
// payload is loaded whole (a thread's group k is payload dword k; int4: halfword k), decoded once into 8 float4
// per thread, and apply_chunk (apply_device.h) reads each target's base slice, combines and writes that target's
// output with 16-byte accesses. Any other offset, and a target that is not 16-byte aligned, goes element by
// element with the same results. PACKED: an int4 bucket (pack_4bit layout, even tensor offsets).
template <bool PACKED>
__global__ __launch_bounds__(kBlock) void k_dequantize_axpby_batched(const uint8_t* __restrict__ q,
                                                                     const adfl_slq_chunk* __restrict__ chunks,
                                                                     const float* __restrict__ scales,
                                                                     ApplyTargets a) {
  static_assert(kApplyBlock == kBlock, "apply_chunk's thread layout");
  const adfl_slq_chunk c = chunks[blockIdx.x];
  const float s = scales[c.tensor];
  const int64_t in_tensor = (int64_t)(blockIdx.x - c.first_chunk) * ADFL_SLQ_CHUNK_ELEMS;
  const bool grouped = (c.start & 3) == 0;
  auto dec1 = [&](int i) -> float {
    const int64_t e = c.start + i;
    if (!PACKED) return s * (float)(int8_t)q[e];
    float e0, e1;
    dequant_byte_int4(q[e >> 1], s, e0, e1);
    return (e & 1) ? e1 : e0;
  };
  float4 dv[kApplyGroups];
  if (grouped) {
    const int n4 = c.len >> 2;
    const uint8_t* qc = PACKED ? q + (c.start >> 1) : q + c.start;  // 4-byte (int4: 2-byte) aligned
    uint32_t w[kApplyGroups];
#pragma unroll
    for (int j = 0; j < kApplyGroups; ++j) {  // every load of the chunk before the first use
      const int k = (int)threadIdx.x + j * kBlock;
      w[j] = k >= n4 ? 0u : PACKED ? (uint32_t) reinterpret_cast<const uint16_t*>(qc)[k]
                                   : reinterpret_cast<const uint32_t*>(qc)[k];
    }
#pragma unroll
    for (int j = 0; j < kApplyGroups; ++j) dv[j] = PACKED ? dequant2_int4(w[j], s) : dequant4(w[j], s);
  }
  apply_chunk(dv, grouped, c, in_tensor, a, dec1);
}

// Decode + accumulate + flush — the buffered servers' K-th client update, which fills the buffer: FedBuff's
// tensor.float().mul_(f), add_parameters_inpace(buffer, decoded, 1, 1), div_(K) and add_parameters(g, buffer, 1, lr)
// (Strategy/fed_buff.py:68-100) and FADAS's add, div_(K), _update_amsgrad and _compute_model_step
// (Strategy/fadas.py:56-80) in one pass: the buffer is read, never written (flush_device.h has the arithmetic).
// k_dequantize_axpby_batched's shape: when the tensor's offset in the bucket is a multiple of 4 and the chunk's slice
// of every operand is 16-byte aligned (both block-uniform), the chunk's payload words are loaded up front (8 VGPRs)
// and receive_flush_chunk walks the chunk in two halves, decoding a half's groups while its operand loads are in
// flight. Anything else goes element by element with the same results. PACKED: an int4 bucket (pack_4bit layout,
// even tensor offsets).
template <bool PACKED, bool FADAS>
__global__ __launch_bounds__(kBlock) void k_dequantize_flush_batched(const uint8_t* __restrict__ q,
                                                                     const adfl_slq_chunk* __restrict__ chunks,
                                                                     const float* __restrict__ scales,
                                                                     ReceiveFlush a) {
  static_assert(kFlushBlock == kBlock, "receive_flush_chunk's thread layout");
  const adfl_slq_chunk c = chunks[blockIdx.x];
  const float s = scales[c.tensor];
  const int64_t in_tensor = (int64_t)(blockIdx.x - c.first_chunk) * ADFL_SLQ_CHUNK_ELEMS;
  const FlushSlices<FADAS> sl(a, c, in_tensor);
  const bool vec = (c.start & 3) == 0 && sl.aligned16();
  auto dec1 = [&](int i) -> float {
    const int64_t e = c.start + i;
    if (!PACKED) return s * (float)(int8_t)q[e];
    float e0, e1;
    dequant_byte_int4(q[e >> 1], s, e0, e1);
    return (e & 1) ? e1 : e0;
  };
  uint32_t w[kFlushGroups];
  if (vec) {
    const int n4 = c.len >> 2;
    const uint8_t* qc = PACKED ? q + (c.start >> 1) : q + c.start;  // 4-byte (int4: 2-byte) aligned
#pragma unroll
    for (int j = 0; j < kFlushGroups; ++j) {  // the payload is dead after the read
      const int k = (int)threadIdx.x + j * kBlock;
      w[j] = k >= n4 ? 0u
             : PACKED ? (uint32_t)__builtin_nontemporal_load(reinterpret_cast<const uint16_t*>(qc) + k)
                      : __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(qc) + k);
    }
  }
  receive_flush_chunk<FADAS>(
      sl, vec, c, a, [&](int j, bool) -> float4 { return PACKED ? dequant2_int4(w[j], s) : dequant4(w[j], s); }, dec1);
}

// Quantization-error statistics of a bucket against its own payload (worker.py:186-189 computes
// parameter_relative_mse and parameter_cosine_similarity from a full decode; here they are four sums
// per chunk, fp64): S0 = sum (x - s*q)^2, S1 = sum x^2, S2 = sum x*(s*q), S3 = sum (s*q)^2.
// PACKED: q is an int4 bucket (pack_4bit layout, even tensor offsets): element e's code is the high
// (even e) or low (odd e) nibble of byte e/2, minus 8 — what unpack_4bit hands the dequantize.
template <bool PACKED>
__global__ __launch_bounds__(kBlock) void k_qerror_batched(const float* __restrict__ x, const int8_t* __restrict__ q,
                                                           const adfl_slq_chunk* __restrict__ chunks,
                                                           const float* __restrict__ scales,
                                                           double* __restrict__ partials) {
  __shared__ double red[4][kWaves];
  const adfl_slq_chunk c = chunks[blockIdx.x];
  const float s = scales[c.tensor];
  const float* xc = x + c.start;
  double a0 = 0, a1 = 0, a2 = 0, a3 = 0;
  for (int i = threadIdx.x; i < c.len; i += kBlock) {
    const double xv = xc[i];
    int code;
    if (PACKED) {
      const int64_t e = c.start + i;
      const uint32_t b = reinterpret_cast<const uint8_t*>(q)[e >> 1];
      code = (e & 1) ? (int)(b & 0xfu) - 8 : (int)((b >> 4) & 0xfu) - 8;
    } else {
      code = q[c.start + i];
    }
    const double dv = (double)(s * (float)code);  // the dequantized fp32 value the reference compares
    const double e = (double)(xc[i] - (float)dv);  // fp32 difference, as (a - b) in parameter_mse
    a0 += e * e;
    a1 += xv * xv;
    a2 += xv * dv;
    a3 += dv * dv;
  }
  double v[4] = {a0, a1, a2, a3};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
    if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = v[k];
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    double t = 0;
    for (int w = 0; w < kWaves; ++w) t += red[threadIdx.x][w];
    partials[4 * (int64_t)blockIdx.x + threadIdx.x] = t;
  }
}

// int4 buckets: every tensor offset is even, so flat element e's nibble lives in packed byte e/2 (high
// nibble = even element) and an odd-sized tensor's last byte pairs its last element with a zero pad
// (compression.py:42-43). Vector tiles need 32-element alignment (16-B packed, 64-B x).
__device__ __forceinline__ void quantize_pairs_int4(const float* __restrict__ xc, uint8_t* __restrict__ pc, int a,
                                                    int b, int len, float inv) {
  for (int i = a + 2 * (int)threadIdx.x; i < b; i += 2 * kBlock) {
    const int hi = quant1(xc[i], inv);
    const int lo = (i + 1 < len) ? quant1(xc[i + 1], inv) : 0;
    pc[i >> 1] = (uint8_t)pack_pair(hi, lo);
  }
}

__device__ __forceinline__ void dequantize_elems_int4(const uint8_t* __restrict__ pc, float* __restrict__ oc, int a,
                                                      int b, float s) {
  for (int i = a + (int)threadIdx.x; i < b; i += kBlock) {
    float e0, e1;
    dequant_byte_int4(pc[i >> 1], s, e0, e1);
    oc[i] = (i & 1) ? e1 : e0;
  }
}

__global__ __launch_bounds__(kBlock) void k_quantize_batched_int4(const float* __restrict__ x,
                                                                  const adfl_slq_chunk* __restrict__ chunks,
                                                                  int64_t nchunks, float qmax,
                                                                  const uint32_t* __restrict__ partials,
                                                                  uint8_t* __restrict__ packed,
                                                                  float* __restrict__ scales) {
  static_assert(ADFL_SLQ_CHUNK_ELEMS == kTile4 * kWaves, "one int4 tile per wave per chunk");
  __shared__ __attribute__((aligned(16))) uint16_t lds[kWaves][kTile4 / 4];
  const int64_t ci = nchunks - 1 - (int64_t)blockIdx.x;
  const adfl_slq_chunk c = chunks[ci];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* xc = x + c.start;
  uint8_t* pc = packed + (c.start >> 1);
  const int head = chunk_head(c.start, c.len, 32);
  const int ntiles = (c.len - head) / kTile4;
  // the wave's tile is loaded before the partial reduction, whose latency it hides
  float4 v[8];
  if (wave < ntiles) load_tile_int4(reinterpret_cast<const float4*>(xc + head) + wave * (kTile4 / 4), v, lane);
  const ScaleInv si = make_scale(reduce_partials(partials + c.first_chunk, c.nchunks), qmax);
  if (ci == c.first_chunk && threadIdx.x == 0) scales[c.tensor] = si.scale;
  quantize_pairs_int4(xc, pc, 0, head, c.len, si.inv);
  if (wave < ntiles)
    quantize_tile_int4_regs(v, reinterpret_cast<uint4*>(pc + (head >> 1)) + wave * 64, si.inv, lds[wave], lane);
  quantize_pairs_int4(xc, pc, head + ntiles * kTile4, c.len, c.len, si.inv);
}

__global__ __launch_bounds__(kBlock) void k_dequantize_batched_int4(const uint8_t* __restrict__ packed,
                                                                    const adfl_slq_chunk* __restrict__ chunks,
                                                                    const float* __restrict__ scales,
                                                                    float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint16_t lds[kWaves][kTile4 / 4];
  const adfl_slq_chunk c = chunks[blockIdx.x];
  const float s = scales[c.tensor];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint8_t* pc = packed + (c.start >> 1);
  float* oc = out + c.start;
  const int head = chunk_head(c.start, c.len, 32);
  dequantize_elems_int4(pc, oc, 0, head, s);
  const int ntiles = (c.len - head) / kTile4;
  for (int t = wave; t < ntiles; t += kWaves)
    dequantize_tile_int4(reinterpret_cast<const uint4*>(pc + (head >> 1)) + t * 64,
                         reinterpret_cast<float4*>(oc + head) + t * (kTile4 / 4), s, lds[wave], lane);
  dequantize_elems_int4(pc, oc, head + ntiles * kTile4, c.len, s);
}

// ------------------------------------------------------------------------------------------------
// host helpers
// ------------------------------------------------------------------------------------------------
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

inline int clamp_grid(int64_t g, int cap) { return (int)(g < 1 ? 1 : (g > cap ? cap : g)); }

// grid for a wave-tile kernel over `tiles` tiles (4 tiles per block per sweep)
inline int tile_grid(int64_t tiles) { return clamp_grid((tiles + kWaves - 1) / kWaves, kMaxFlatBlocks); }

inline int absmax_grid(int64_t n) { return clamp_grid((n >> 2) / (8 * kBlock), kAbsmaxBlocks); }

inline int check_bits(int bits) { return (bits >= 1 && bits <= 16) ? ADFL_OK : ADFL_E_BITS; }

// mean kernels: K rows from which the cascade needs its levels 2-3 (torch_sum_order.h), and the most rows
constexpr int kDeepRows = 256;
inline bool bad_rows(int k) { return k < 1 || k > adfl_sum::kMaxRows; }

}  // namespace

// ================================================================================================
// C ABI
// ================================================================================================
namespace {

template <bool PACKED>
int launch_fedbuff_flush(const uint8_t* d_q, const adfl_slq_chunk* d_chunks, int64_t nchunks, const float* d_scales,
                         const float* const* d_buf, const float* const* d_g, float* const* d_out, int32_t ntensors,
                         int32_t K, float factor, float lr, void* stream) {
  if (!d_q || !d_scales || !d_g || !d_out || receive_flush_bad_args(d_chunks, nchunks, ntensors, K)) return ADFL_E_ARG;
  if (!aligned16(d_q)) return ADFL_E_ALIGN;
  ReceiveFlush a{d_buf, d_g, nullptr, nullptr, nullptr, d_out, factor, lr, FadasScalars{}};
  a.s.k = (float)K;
  hipLaunchKernelGGL((k_dequantize_flush_batched<PACKED, false>), dim3((unsigned)nchunks), dim3(kBlock), 0,
                     (hipStream_t)stream, d_q, d_chunks, d_scales, a);
  return launch_status();
}

template <bool PACKED>
int launch_fadas_flush(const uint8_t* d_q, const adfl_slq_chunk* d_chunks, int64_t nchunks, const float* d_scales,
                       const float* const* d_buf, const float* const* d_g, float* const* d_m, float* const* d_v,
                       float* const* d_v_hat, float* const* d_out, int32_t ntensors, int32_t K,
                       const FadasScalars& s, void* stream) {
  if (!d_q || !d_scales || !d_g || !d_m || !d_v || !d_v_hat || !d_out ||
      receive_flush_bad_args(d_chunks, nchunks, ntensors, K))
    return ADFL_E_ARG;
  if (!aligned16(d_q)) return ADFL_E_ALIGN;
  const ReceiveFlush a{d_buf, d_g, d_m, d_v, d_v_hat, d_out, 1.0f, 0.0f, s};
  hipLaunchKernelGGL((k_dequantize_flush_batched<PACKED, true>), dim3((unsigned)nchunks), dim3(kBlock), 0,
                     (hipStream_t)stream, d_q, d_chunks, d_scales, a);
  return launch_status();
}

}  // namespace

extern "C" {

int adfl_slq_abi_version(void) { return ADFL_SLQ_ABI_VERSION; }

const char* adfl_slq_strerror(int status) {
  switch (status) {
    case ADFL_OK: return "ok";
    case ADFL_E_ARG: return "adfl_slq: invalid argument (null pointer, count or tensor table)";
    case ADFL_E_BITS: return "adfl_slq: bits must be in [1, 16]";
    case ADFL_E_ALIGN: return "adfl_slq: device data pointers must be 16-byte aligned";
    case ADFL_E_WORKSPACE: return "adfl_slq: workspace smaller than adfl_slq_workspace_bytes()";
    default: return status > 0 ? hipGetErrorString((hipError_t)status) : "adfl_slq: unknown error";
  }
}

int64_t adfl_slq_workspace_bytes(void) { return kWorkspaceBytes; }

int adfl_slq_absmax(const float* d_x, int64_t n, void* d_workspace, int64_t workspace_bytes, void* stream) {
  if (!d_x || !d_workspace || n < 1) return ADFL_E_ARG;
  if (!aligned16(d_x) || !aligned16(d_workspace)) return ADFL_E_ALIGN;
  if (workspace_bytes < kWorkspaceBytes) return ADFL_E_WORKSPACE;
  hipLaunchKernelGGL(k_absmax_flat<8>, dim3(absmax_grid(n)), dim3(kBlock), 0, (hipStream_t)stream, d_x, n,
                     (int64_t)(kCacheKeepBytes / 16), (uint32_t*)d_workspace);
  return launch_status();
}

int adfl_slq_absmax_value(const void* d_workspace, float* d_absmax, void* stream) {
  if (!d_workspace || !d_absmax) return ADFL_E_ARG;
  if (!aligned16(d_workspace)) return ADFL_E_ALIGN;
  hipLaunchKernelGGL(k_absmax_value, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, (const uint32_t*)d_workspace,
                     d_absmax);
  return launch_status();
}

int adfl_slq_quantize(const float* d_x, int64_t n, int bits, const void* d_workspace, int8_t* d_q, float* d_scale,
                      void* stream) {
  if (!d_x || !d_workspace || !d_q || !d_scale || n < 1) return ADFL_E_ARG;
  if (int s = check_bits(bits)) return s;
  if (!aligned16(d_x) || !aligned16(d_q)) return ADFL_E_ALIGN;
  hipLaunchKernelGGL((k_quantize_flat<true, false>), dim3(tile_grid(n / kTile)), dim3(kBlock), 0, (hipStream_t)stream, d_x, n,
                     qmax_f(bits), (const uint32_t*)d_workspace, d_q, d_scale);
  return launch_status();
}

int adfl_slq_encode(const float* d_x, int64_t n, int bits, int8_t* d_q, float* d_scale, void* d_workspace,
                    int64_t workspace_bytes, void* stream) {
  if (int s = check_bits(bits)) return s;
  if (int s = adfl_slq_absmax(d_x, n, d_workspace, workspace_bytes, stream)) return s;
  return adfl_slq_quantize(d_x, n, bits, d_workspace, d_q, d_scale, stream);
}

int adfl_slq_dequantize(const int8_t* d_q, int64_t n, const float* d_scale, float* d_out, void* stream) {
  if (!d_q || !d_scale || !d_out || n < 1) return ADFL_E_ARG;
  if (!aligned16(d_q) || !aligned16(d_out)) return ADFL_E_ALIGN;
  hipLaunchKernelGGL((k_dequantize_flat<false, false>), dim3(tile_grid(n / kTile)), dim3(kBlock), 0, (hipStream_t)stream, d_q, n,
                     d_scale, d_out);
  return launch_status();
}

int64_t adfl_slq_build_chunks(const int64_t* offsets, const int64_t* sizes, int32_t ntensors, adfl_slq_chunk* chunks,
                              int64_t capacity) {
  if (!offsets || !sizes || ntensors < 1) return ADFL_E_ARG;
  int64_t count = 0;
  for (int32_t t = 0; t < ntensors; ++t) {
    if (sizes[t] < 1 || offsets[t] < 0) return ADFL_E_ARG;
    const int64_t nc = (sizes[t] + ADFL_SLQ_CHUNK_ELEMS - 1) / ADFL_SLQ_CHUNK_ELEMS;
    if (nc > INT32_MAX || count + nc > INT32_MAX) return ADFL_E_ARG;
    if (chunks) {
      if (count + nc > capacity) return ADFL_E_ARG;
      for (int64_t k = 0; k < nc; ++k) {
        adfl_slq_chunk& c = chunks[count + k];
        c.start = offsets[t] + k * ADFL_SLQ_CHUNK_ELEMS;
        const int64_t rem = sizes[t] - k * ADFL_SLQ_CHUNK_ELEMS;
        c.len = (int32_t)(rem < ADFL_SLQ_CHUNK_ELEMS ? rem : ADFL_SLQ_CHUNK_ELEMS);
        c.tensor = t;
        c.first_chunk = (int32_t)count;
        c.nchunks = (int32_t)nc;
      }
    }
    count += nc;
  }
  return count;
}

int adfl_slq_encode_batched(const float* d_x, const adfl_slq_chunk* d_chunks, int64_t nchunks, int bits, int8_t* d_q,
                            float* d_scales, uint32_t* d_partials, void* stream) {
  if (!d_x || !d_chunks || !d_q || !d_scales || !d_partials || nchunks < 1 || nchunks > INT32_MAX) return ADFL_E_ARG;
  if (int s = check_bits(bits)) return s;
  if (!aligned16(d_x) || !aligned16(d_q)) return ADFL_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_absmax_batched, dim3((unsigned)nchunks), dim3(kBlock), 0, st, d_x, d_chunks, d_partials);
  if (int s = launch_status()) return s;
  hipLaunchKernelGGL(k_quantize_batched, dim3((unsigned)nchunks), dim3(kBlock), 0, st, d_x, d_chunks, qmax_f(bits),
                     (const uint32_t*)d_partials, d_q, d_scales, (int64_t)0);
  return launch_status();
}

int adfl_slq_quantize_batched_range(const float* d_x, const adfl_slq_chunk* d_chunks, int64_t chunk_begin,
                                    int64_t count, int bits, const uint32_t* d_partials, int8_t* d_q,
                                    float* d_scales, void* stream) {
  if (!d_x || !d_chunks || !d_q || !d_scales || !d_partials || chunk_begin < 0 || count < 1 || count > INT32_MAX)
    return ADFL_E_ARG;
  if (int s = check_bits(bits)) return s;
  if (!aligned16(d_x) || !aligned16(d_q)) return ADFL_E_ALIGN;
  hipLaunchKernelGGL(k_quantize_batched, dim3((unsigned)count), dim3(kBlock), 0, (hipStream_t)stream, d_x, d_chunks,
                     qmax_f(bits), d_partials, d_q, d_scales, chunk_begin);
  return launch_status();
}

int adfl_slq_absmax_batched_range(const float* d_x, const adfl_slq_chunk* d_chunks, int64_t chunk_begin, int64_t count,
                                  uint32_t* d_partials, void* stream) {
  if (!d_x || !d_chunks || !d_partials || chunk_begin < 0 || count < 1 || count > INT32_MAX) return ADFL_E_ARG;
  if (!aligned16(d_x)) return ADFL_E_ALIGN;
  hipLaunchKernelGGL(k_absmax_batched, dim3((unsigned)count), dim3(kBlock), 0, (hipStream_t)stream, d_x, d_chunks,
                     d_partials, chunk_begin);
  return launch_status();
}

int64_t adfl_slq_build_encode_work(const adfl_slq_chunk* chunks, int64_t nchunks, int32_t* work, int64_t capacity) {
  if (!chunks || nchunks < 1 || nchunks > INT32_MAX) return ADFL_E_ARG;
  int64_t n = 0;
  for (int64_t i = 0; i < nchunks; ++i) {
    const adfl_slq_chunk& c = chunks[i];
    if (c.first_chunk < 0 || c.nchunks < 1 || i < c.first_chunk || i >= (int64_t)c.first_chunk + c.nchunks)
      return ADFL_E_ARG;
    if (c.nchunks > kSegChunks) return 0;  // a tensor too large for one block: the two-pass encode
    if (i != c.first_chunk) continue;
    if (work) {
      if (n >= capacity) return ADFL_E_ARG;
      work[n] = (int32_t)i;
    }
    ++n;
  }
  return n;
}

int adfl_slq_encode_batched_work(const float* d_x, const adfl_slq_chunk* d_chunks, int64_t nchunks,
                                 const int32_t* d_work, int64_t nwork, int bits, int8_t* d_q, float* d_scales,
                                 uint32_t* d_partials, void* stream) {
  if (nwork == 0) return adfl_slq_encode_batched(d_x, d_chunks, nchunks, bits, d_q, d_scales, d_partials, stream);
  if (!d_x || !d_chunks || !d_work || !d_q || !d_scales || nchunks < 1 || nchunks > INT32_MAX || nwork < 0 ||
      nwork > nchunks)
    return ADFL_E_ARG;
  if (int s = check_bits(bits)) return s;
  if (!aligned16(d_x) || !aligned16(d_q)) return ADFL_E_ALIGN;
  hipLaunchKernelGGL(k_encode_resident<kResidentNtStores>, dim3((unsigned)nwork), dim3(kSegBlock), 0, (hipStream_t)stream, d_x,
                     d_chunks, d_work, qmax_f(bits), d_q, d_scales);
  return launch_status();
}

int adfl_slq_dequantize_batched(const int8_t* d_q, const adfl_slq_chunk* d_chunks, int64_t nchunks,
                                const float* d_scales, float* d_out, void* stream) {
  if (!d_q || !d_chunks || !d_scales || !d_out || nchunks < 1 || nchunks > INT32_MAX) return ADFL_E_ARG;
  if (!aligned16(d_q) || !aligned16(d_out)) return ADFL_E_ALIGN;
  hipLaunchKernelGGL(k_dequantize_batched, dim3((unsigned)nchunks), dim3(kBlock), 0, (hipStream_t)stream, d_q,
                     d_chunks, d_scales, d_out);
  return launch_status();
}

int adfl_slq_qerror_batched(const float* d_x, const int8_t* d_q, const adfl_slq_chunk* d_chunks, int64_t nchunks,
                            const float* d_scales, double* d_partials, void* stream) {
  if (!d_x || !d_q || !d_chunks || !d_scales || !d_partials || nchunks < 1 || nchunks > INT32_MAX) return ADFL_E_ARG;
  hipLaunchKernelGGL(k_qerror_batched<false>, dim3((unsigned)nchunks), dim3(kBlock), 0, (hipStream_t)stream, d_x,
                     d_q, d_chunks, d_scales, d_partials);
  return launch_status();
}

int adfl_slq_qerror_batched_int4(const float* d_x, const uint8_t* d_packed, const adfl_slq_chunk* d_chunks,
                                 int64_t nchunks, const float* d_scales, double* d_partials, void* stream) {
  if (!d_x || !d_packed || !d_chunks || !d_scales || !d_partials || nchunks < 1 || nchunks > INT32_MAX)
    return ADFL_E_ARG;
  hipLaunchKernelGGL(k_qerror_batched<true>, dim3((unsigned)nchunks), dim3(kBlock), 0, (hipStream_t)stream, d_x,
                     (const int8_t*)d_packed, d_chunks, d_scales, d_partials);
  return launch_status();
}

int adfl_slq_encode_batched_int4(const float* d_x, const adfl_slq_chunk* d_chunks, int64_t nchunks, int bits,
                                 uint8_t* d_packed, float* d_scales, uint32_t* d_partials, void* stream) {
  if (!d_x || !d_chunks || !d_packed || !d_scales || !d_partials || nchunks < 1 || nchunks > INT32_MAX)
    return ADFL_E_ARG;
  if (int s = check_bits(bits)) return s;
  if (!aligned16(d_x) || !aligned16(d_packed)) return ADFL_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_absmax_batched, dim3((unsigned)nchunks), dim3(kBlock), 0, st, d_x, d_chunks, d_partials);
  if (int s = launch_status()) return s;
  hipLaunchKernelGGL(k_quantize_batched_int4, dim3((unsigned)nchunks), dim3(kBlock), 0, st, d_x, d_chunks, nchunks,
                     qmax_f(bits), (const uint32_t*)d_partials, d_packed, d_scales);
  return launch_status();
}

int adfl_slq_encode_batched_int4_work(const float* d_x, const adfl_slq_chunk* d_chunks, int64_t nchunks,
                                      const int32_t* d_work, int64_t nwork, int bits, uint8_t* d_packed,
                                      float* d_scales, uint32_t* d_partials, void* stream) {
  if (nwork == 0)
    return adfl_slq_encode_batched_int4(d_x, d_chunks, nchunks, bits, d_packed, d_scales, d_partials, stream);
  if (!d_x || !d_chunks || !d_work || !d_packed || !d_scales || nchunks < 1 || nchunks > INT32_MAX || nwork < 0 ||
      nwork > nchunks)
    return ADFL_E_ARG;
  if (int s = check_bits(bits)) return s;
  if (!aligned16(d_x) || !aligned16(d_packed)) return ADFL_E_ALIGN;
  hipLaunchKernelGGL(k_encode_resident_int4, dim3((unsigned)nwork), dim3(kSegBlock), 0, (hipStream_t)stream, d_x,
                     d_chunks, d_work, qmax_f(bits), d_packed, d_scales);
  return launch_status();
}

int adfl_slq_dequantize_batched_int4(const uint8_t* d_packed, const adfl_slq_chunk* d_chunks, int64_t nchunks,
                                     const float* d_scales, float* d_out, void* stream) {
  if (!d_packed || !d_chunks || !d_scales || !d_out || nchunks < 1 || nchunks > INT32_MAX) return ADFL_E_ARG;
  if (!aligned16(d_packed) || !aligned16(d_out)) return ADFL_E_ALIGN;
  hipLaunchKernelGGL(k_dequantize_batched_int4, dim3((unsigned)nchunks), dim3(kBlock), 0, (hipStream_t)stream,
                     d_packed, d_chunks, d_scales, d_out);
  return launch_status();
}

int adfl_slq_quantize_int4(const float* d_x, int64_t n, int bits, const void* d_workspace, uint8_t* d_packed,
                           float* d_scale, void* stream) {
  if (!d_x || !d_workspace || !d_packed || !d_scale || n < 1) return ADFL_E_ARG;
  if (int s = check_bits(bits)) return s;
  if (!aligned16(d_x) || !aligned16(d_packed)) return ADFL_E_ALIGN;
  hipLaunchKernelGGL(k_quantize_int4_flat, dim3(tile_grid(n / kTile4)), dim3(kBlock), 0, (hipStream_t)stream, d_x, n,
                     qmax_f(bits), (const uint32_t*)d_workspace, d_packed, d_scale);
  return launch_status();
}

int adfl_slq_encode_int4(const float* d_x, int64_t n, int bits, uint8_t* d_packed, float* d_scale, void* d_workspace,
                         int64_t workspace_bytes, void* stream) {
  if (int s = check_bits(bits)) return s;
  if (int s = adfl_slq_absmax(d_x, n, d_workspace, workspace_bytes, stream)) return s;
  return adfl_slq_quantize_int4(d_x, n, bits, d_workspace, d_packed, d_scale, stream);
}

int adfl_slq_dequantize_int4(const uint8_t* d_packed, int64_t n, const float* d_scale, float* d_out, void* stream) {
  if (!d_packed || !d_scale || !d_out || n < 1) return ADFL_E_ARG;
  if (!aligned16(d_packed) || !aligned16(d_out)) return ADFL_E_ALIGN;
  hipLaunchKernelGGL(k_dequantize_int4_flat, dim3(tile_grid(n / kTile4)), dim3(kBlock), 0, (hipStream_t)stream,
                     d_packed, n, d_scale, d_out);
  return launch_status();
}

int adfl_pack_int4(const int8_t* d_q, int64_t n, uint8_t* d_packed, void* stream) {
  if (!d_q || !d_packed || n < 1) return ADFL_E_ARG;
  hipLaunchKernelGGL(k_pack_int4, dim3(clamp_grid((((n + 1) >> 1) + kBlock - 1) / kBlock, kMaxFlatBlocks)),
                     dim3(kBlock), 0, (hipStream_t)stream, d_q, n, d_packed);
  return launch_status();
}

int adfl_unpack_int4(const uint8_t* d_packed, int64_t n, int8_t* d_q, void* stream) {
  if (!d_packed || !d_q || n < 1) return ADFL_E_ARG;
  hipLaunchKernelGGL(k_unpack_int4, dim3(clamp_grid((n + kBlock - 1) / kBlock, kMaxFlatBlocks)), dim3(kBlock), 0,
                     (hipStream_t)stream, d_packed, n, d_q);
  return launch_status();
}

int adfl_slq_dequantize_mean(const int8_t* d_q, int64_t row_stride_bytes, int32_t k, int64_t n,
                             const float* d_scales, int64_t scale_stride, float* d_out, void* stream) {
  return adfl_slq_dequantize_mean_self(d_q, row_stride_bytes, k, n, d_scales, scale_stride, -1, nullptr, d_out,
                                       stream);
}

int adfl_slq_dequantize_mean_self(const int8_t* d_q, int64_t row_stride_bytes, int32_t k, int64_t n,
                                  const float* d_scales, int64_t scale_stride, int32_t self_row,
                                  const float* d_self_x, float* d_out, void* stream) {
  if (!d_q || !d_scales || !d_out || n < 1 || bad_rows(k) || row_stride_bytes < n || scale_stride < 1) return ADFL_E_ARG;
  if (self_row >= k || self_row < -1 || (self_row >= 0 && !d_self_x)) return ADFL_E_ARG;
  if (!aligned16(d_q) || !aligned16(d_out) || (row_stride_bytes & 15) != 0) return ADFL_E_ALIGN;
  if (self_row >= 0 && !aligned16(d_self_x)) return ADFL_E_ALIGN;
  auto kern = k >= kDeepRows ? k_dequantize_mean<true> : k_dequantize_mean<false>;
  hipLaunchKernelGGL(kern, dim3(tile_grid(n / kTile)), dim3(kBlock), 0, (hipStream_t)stream, d_q, row_stride_bytes,
                     (int)k, n, d_scales, scale_stride, (int)self_row, d_self_x, d_out);
  return launch_status();
}

int adfl_slq_dequantize_mean_batched(const int8_t* d_q, int64_t row_stride_bytes, int32_t k,
                                     const adfl_slq_chunk* d_chunks, int64_t nchunks, const float* d_scales,
                                     int64_t scale_stride, int32_t self_row, const float* d_self_x, float* d_out,
                                     void* stream) {
  if (!d_q || !d_chunks || !d_scales || !d_out || bad_rows(k) || nchunks < 1 || nchunks > INT32_MAX || scale_stride < 1 ||
      row_stride_bytes < 1)
    return ADFL_E_ARG;
  if (self_row >= k || self_row < -1 || (self_row >= 0 && !d_self_x)) return ADFL_E_ARG;
  if (!aligned16(d_q) || !aligned16(d_out) || (row_stride_bytes & 15) != 0) return ADFL_E_ALIGN;
  if (self_row >= 0 && !aligned16(d_self_x)) return ADFL_E_ALIGN;
  auto kern = k >= kDeepRows ? k_dequantize_mean_batched<true> : k_dequantize_mean_batched<false>;
  hipLaunchKernelGGL(kern, dim3((unsigned)nchunks), dim3(kBlock), 0, (hipStream_t)stream, d_q, row_stride_bytes,
                     (int)k, d_chunks, d_scales, scale_stride, (int)self_row, d_self_x, d_out);
  return launch_status();
}

int adfl_slq_dequantize_mean_batched_int4(const uint8_t* d_packed, int64_t row_stride_bytes, int32_t k,
                                          const adfl_slq_chunk* d_chunks, int64_t nchunks, const float* d_scales,
                                          int64_t scale_stride, int32_t self_row, const float* d_self_x,
                                          float* d_out, void* stream) {
  if (!d_packed || !d_chunks || !d_scales || !d_out || bad_rows(k) || nchunks < 1 || nchunks > INT32_MAX ||
      scale_stride < 1 || row_stride_bytes < 1)
    return ADFL_E_ARG;
  if (self_row >= k || self_row < -1 || (self_row >= 0 && !d_self_x)) return ADFL_E_ARG;
  if (!aligned16(d_packed) || !aligned16(d_out) || (row_stride_bytes & 15) != 0) return ADFL_E_ALIGN;
  if (self_row >= 0 && !aligned16(d_self_x)) return ADFL_E_ALIGN;
  auto kern = k >= kDeepRows ? k_dequantize_mean_batched_int4<true> : k_dequantize_mean_batched_int4<false>;
  hipLaunchKernelGGL(kern, dim3((unsigned)nchunks), dim3(kBlock), 0, (hipStream_t)stream, d_packed, row_stride_bytes,
                     (int)k, d_chunks, d_scales, scale_stride, (int)self_row, d_self_x, d_out);
  return launch_status();
}

int adfl_slq_dequantize_mean_axpby_batched(const int8_t* d_q, int64_t row_stride_bytes, int32_t k,
                                           const adfl_slq_chunk* d_chunks, int64_t nchunks, const float* d_scales,
                                           int64_t scale_stride, const float* const* d_base, float* const* d_out,
                                           int32_t ntensors, float alpha, float beta, void* stream) {
  if (!d_q || !d_scales || !d_base || apply_bad_args(d_chunks, nchunks, d_out, ntensors, 1) || bad_rows(k) ||
      scale_stride < 1 || row_stride_bytes < 1 || (row_stride_bytes & 15) != 0)
    return ADFL_E_ARG;
  if (!aligned16(d_q)) return ADFL_E_ALIGN;
  const ApplyTargets a{d_base, d_out, (int)ntensors, 1, alpha, beta};
  auto kern = k >= kDeepRows ? k_dequantize_mean_axpby_batched<true> : k_dequantize_mean_axpby_batched<false>;
  hipLaunchKernelGGL(kern, dim3((unsigned)nchunks), dim3(kBlock), 0, (hipStream_t)stream, d_q, row_stride_bytes,
                     (int)k, d_chunks, d_scales, scale_stride, a);
  return launch_status();
}

int adfl_slq_dequantize_mean_axpby_batched_int4(const uint8_t* d_packed, int64_t row_stride_bytes, int32_t k,
                                                const adfl_slq_chunk* d_chunks, int64_t nchunks,
                                                const float* d_scales, int64_t scale_stride,
                                                const float* const* d_base, float* const* d_out, int32_t ntensors,
                                                float alpha, float beta, void* stream) {
  if (!d_packed || !d_scales || !d_base || apply_bad_args(d_chunks, nchunks, d_out, ntensors, 1) || bad_rows(k) ||
      scale_stride < 1 || row_stride_bytes < 1 || (row_stride_bytes & 15) != 0)
    return ADFL_E_ARG;
  if (!aligned16(d_packed)) return ADFL_E_ALIGN;
  const ApplyTargets a{d_base, d_out, (int)ntensors, 1, alpha, beta};
  auto kern =
      k >= kDeepRows ? k_dequantize_mean_axpby_batched_int4<true> : k_dequantize_mean_axpby_batched_int4<false>;
  hipLaunchKernelGGL(kern, dim3((unsigned)nchunks), dim3(kBlock), 0, (hipStream_t)stream, d_packed, row_stride_bytes,
                     (int)k, d_chunks, d_scales, scale_stride, a);
  return launch_status();
}

int adfl_slq_dequantize_add_batched(const int8_t* d_q, const adfl_slq_chunk* d_chunks, int64_t nchunks,
                                    const float* d_scales, float* const* d_targets, int32_t ntensors,
                                    int32_t ntargets, void* stream) {
  if (!d_q || !d_chunks || !d_scales || !d_targets || nchunks < 1 || nchunks > INT32_MAX || ntensors < 1 ||
      ntargets < 1)
    return ADFL_E_ARG;
  if (!aligned16(d_q)) return ADFL_E_ALIGN;
  hipLaunchKernelGGL(k_dequantize_add_batched, dim3((unsigned)nchunks), dim3(kBlock), 0, (hipStream_t)stream, d_q,
                     d_chunks, d_scales, d_targets, (int)ntensors, (int)ntargets);
  return launch_status();
}

int adfl_slq_dequantize_axpby_batched(const int8_t* d_q, const adfl_slq_chunk* d_chunks, int64_t nchunks,
                                      const float* d_scales, const float* const* d_base, float* const* d_out,
                                      int32_t ntensors, int32_t ntargets, float alpha, float beta, void* stream) {
  if (!d_q || !d_scales || apply_bad_args(d_chunks, nchunks, d_out, ntensors, ntargets)) return ADFL_E_ARG;
  if (!aligned16(d_q)) return ADFL_E_ALIGN;
  const ApplyTargets a{d_base, d_out, (int)ntensors, (int)ntargets, alpha, beta};
  hipLaunchKernelGGL(k_dequantize_axpby_batched<false>, dim3((unsigned)nchunks), dim3(kBlock), 0, (hipStream_t)stream,
                     reinterpret_cast<const uint8_t*>(d_q), d_chunks, d_scales, a);
  return launch_status();
}

int adfl_slq_dequantize_axpby_batched_int4(const uint8_t* d_packed, const adfl_slq_chunk* d_chunks, int64_t nchunks,
                                           const float* d_scales, const float* const* d_base, float* const* d_out,
                                           int32_t ntensors, int32_t ntargets, float alpha, float beta,
                                           void* stream) {
  if (!d_packed || !d_scales || apply_bad_args(d_chunks, nchunks, d_out, ntensors, ntargets)) return ADFL_E_ARG;
  if (!aligned16(d_packed)) return ADFL_E_ALIGN;
  const ApplyTargets a{d_base, d_out, (int)ntensors, (int)ntargets, alpha, beta};
  hipLaunchKernelGGL(k_dequantize_axpby_batched<true>, dim3((unsigned)nchunks), dim3(kBlock), 0, (hipStream_t)stream,
                     d_packed, d_chunks, d_scales, a);
  return launch_status();
}

int adfl_slq_dequantize_fedbuff_flush_batched(const int8_t* d_q, const adfl_slq_chunk* d_chunks, int64_t nchunks,
                                              const float* d_scales, const float* const* d_buf,
                                              const float* const* d_g, float* const* d_out, int32_t ntensors,
                                              int32_t K, float factor, float lr, void* stream) {
  return launch_fedbuff_flush<false>(reinterpret_cast<const uint8_t*>(d_q), d_chunks, nchunks, d_scales, d_buf, d_g,
                                     d_out, ntensors, K, factor, lr, stream);
}

int adfl_slq_dequantize_fedbuff_flush_batched_int4(const uint8_t* d_packed, const adfl_slq_chunk* d_chunks,
                                                   int64_t nchunks, const float* d_scales, const float* const* d_buf,
                                                   const float* const* d_g, float* const* d_out, int32_t ntensors,
                                                   int32_t K, float factor, float lr, void* stream) {
  return launch_fedbuff_flush<true>(d_packed, d_chunks, nchunks, d_scales, d_buf, d_g, d_out, ntensors, K, factor, lr,
                                    stream);
}

int adfl_slq_dequantize_fadas_flush_batched(const int8_t* d_q, const adfl_slq_chunk* d_chunks, int64_t nchunks,
                                            const float* d_scales, const float* const* d_buf, const float* const* d_g,
                                            float* const* d_m, float* const* d_v, float* const* d_v_hat,
                                            float* const* d_out, int32_t ntensors, int32_t K, float beta1,
                                            float one_minus_beta1, float beta2, float one_minus_beta2, float sqrt_bc2,
                                            float eps, float step, void* stream) {
  const FadasScalars s{(float)K, beta1, one_minus_beta1, beta2, one_minus_beta2, sqrt_bc2, eps, step};
  return launch_fadas_flush<false>(reinterpret_cast<const uint8_t*>(d_q), d_chunks, nchunks, d_scales, d_buf, d_g, d_m,
                                   d_v, d_v_hat, d_out, ntensors, K, s, stream);
}

int adfl_slq_dequantize_fadas_flush_batched_int4(const uint8_t* d_packed, const adfl_slq_chunk* d_chunks,
                                                 int64_t nchunks, const float* d_scales, const float* const* d_buf,
                                                 const float* const* d_g, float* const* d_m, float* const* d_v,
                                                 float* const* d_v_hat, float* const* d_out, int32_t ntensors,
                                                 int32_t K, float beta1, float one_minus_beta1, float beta2,
                                                 float one_minus_beta2, float sqrt_bc2, float eps, float step,
                                                 void* stream) {
  const FadasScalars s{(float)K, beta1, one_minus_beta1, beta2, one_minus_beta2, sqrt_bc2, eps, step};
  return launch_fadas_flush<true>(d_packed, d_chunks, nchunks, d_scales, d_buf, d_g, d_m, d_v, d_v_hat, d_out,
                                  ntensors, K, s, stream);
}

int adfl_slq_dequantize_mean_int4(const uint8_t* d_packed, int64_t row_stride_bytes, int32_t k, int64_t n,
                                  const float* d_scales, int64_t scale_stride, float* d_out, void* stream) {
  return adfl_slq_dequantize_mean_self_int4(d_packed, row_stride_bytes, k, n, d_scales, scale_stride, -1, nullptr,
                                            d_out, stream);
}

int adfl_slq_dequantize_mean_self_int4(const uint8_t* d_packed, int64_t row_stride_bytes, int32_t k, int64_t n,
                                       const float* d_scales, int64_t scale_stride, int32_t self_row,
                                       const float* d_self_x, float* d_out, void* stream) {
  if (!d_packed || !d_scales || !d_out || n < 1 || bad_rows(k) || row_stride_bytes < (n + 1) / 2 || scale_stride < 1)
    return ADFL_E_ARG;
  if (self_row >= k || self_row < -1 || (self_row >= 0 && !d_self_x)) return ADFL_E_ARG;
  if (!aligned16(d_packed) || !aligned16(d_out) || (row_stride_bytes & 15) != 0) return ADFL_E_ALIGN;
  if (self_row >= 0 && !aligned16(d_self_x)) return ADFL_E_ALIGN;
  auto kern = k >= kDeepRows ? k_dequantize_mean_int4<true> : k_dequantize_mean_int4<false>;
  hipLaunchKernelGGL(kern, dim3(tile_grid(n / kTile4)), dim3(kBlock), 0, (hipStream_t)stream, d_packed,
                     row_stride_bytes, (int)k, n, d_scales, scale_stride, (int)self_row, d_self_x, d_out);
  return launch_status();
}

}  // extern "C"
