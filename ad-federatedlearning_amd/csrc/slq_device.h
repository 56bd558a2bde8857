// slq_device.h — the SLQ codec's device helpers shared by slq_codec.hip and slq_delta.hip: memory and element
// helpers, reductions, the wave-tile bodies and the chunk / resident-segment register layouts. Everything is
// in an anonymous namespace: each translation unit gets its own copy (internal linkage), as before the split.
#ifndef ADFL_SLQ_DEVICE_H
#define ADFL_SLQ_DEVICE_H

#include <hip/hip_runtime.h>

#include <cstdint>

#include "adfl_slq.h"

namespace {

constexpr int kBlock = 256;                        // 4 waves of 64
constexpr int kWaves = kBlock / 64;
constexpr int kTile = 1024;                        // int8 path: elements per wave tile
constexpr int kTile4 = 2048;                       // int4 path: elements per wave tile
typedef float f4v __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------
// memory helpers
// ------------------------------------------------------------------------------------------------
template <bool NT>
__device__ __forceinline__ float4 load4(const float4* p) {
  if (NT) {
    const f4v v = __builtin_nontemporal_load(reinterpret_cast<const f4v*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
  }
  return *p;
}

typedef uint32_t u4v __attribute__((ext_vector_type(4)));
template <bool NT>
__device__ __forceinline__ uint4 load16(const uint4* p) {
  if (NT) {
    const u4v v = __builtin_nontemporal_load(reinterpret_cast<const u4v*>(p));
    return make_uint4(v.x, v.y, v.z, v.w);
  }
  return *p;
}

template <bool NT>
__device__ __forceinline__ void store16(uint4* p, uint4 d) {
  if (NT) {
    const u4v v = {d.x, d.y, d.z, d.w};
    __builtin_nontemporal_store(v, reinterpret_cast<u4v*>(p));
  } else {
    *p = d;
  }
}

__device__ __forceinline__ void store4_nt(float4* p, float4 d) {
  const f4v v = {d.x, d.y, d.z, d.w};
  __builtin_nontemporal_store(v, reinterpret_cast<f4v*>(p));
}

// ------------------------------------------------------------------------------------------------
// element helpers
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t abs_bits(float v) { return __float_as_uint(v) & 0x7fffffffu; }

// max|x| as an unsigned compare of the magnitude bits: identical to the float order on non-NaN
// values, and every NaN (> 0x7f800000) wins, so NaN propagates exactly like torch.max.
__device__ __forceinline__ uint32_t abs_bits4(float4 v) {
  return max(max(abs_bits(v.x), abs_bits(v.y)), max(abs_bits(v.z), abs_bits(v.w)));
}

// torch.quantize_per_tensor(x, scale, 0, qint8) on one element, given inv = fp32(1/scale).
__device__ __forceinline__ int quant1(float x, float inv) {
  float y = x * inv;
  y = __builtin_isnan(y) ? 127.0f : __builtin_fminf(__builtin_fmaxf(y, -128.0f), 127.0f);
  return (int)__builtin_rintf(y);  // v_rndne_f32: round half to even
}

__device__ __forceinline__ uint32_t quant4(float4 v, float inv) {
  return (uint32_t(quant1(v.x, inv)) & 0xffu) | ((uint32_t(quant1(v.y, inv)) & 0xffu) << 8) |
         ((uint32_t(quant1(v.z, inv)) & 0xffu) << 16) | (uint32_t(quant1(v.w, inv)) << 24);
}

__device__ __forceinline__ float4 dequant4(uint32_t w, float s) {
  float4 r;
  r.x = s * (float)(int8_t)(w & 0xffu);
  r.y = s * (float)(int8_t)((w >> 8) & 0xffu);
  r.z = s * (float)(int8_t)((w >> 16) & 0xffu);
  r.w = s * (float)(int8_t)(w >> 24);
  return r;
}

// pack_4bit on one pair: ((hi+8) << 4 | (lo+8)) in int8 wraparound; lo is deliberately NOT masked
// to a nibble (compression.py:45-48 ORs the full shifted int8), so out-of-range values alias.
__device__ __forceinline__ uint32_t pack_pair(int hi, int lo) {
  return ((uint32_t(hi + 8) << 4) | uint32_t(lo + 8)) & 0xffu;
}

// 4 elements -> 2 packed bytes (high nibble = even element).
__device__ __forceinline__ uint32_t quant4_int4(float4 v, float inv) {
  return pack_pair(quant1(v.x, inv), quant1(v.y, inv)) | (pack_pair(quant1(v.z, inv), quant1(v.w, inv)) << 8);
}

// unpack_4bit (compression.py:60-61) on one packed byte: high nibble = even element.
__device__ __forceinline__ void dequant_byte_int4(uint32_t b, float s, float& e0, float& e1) {
  e0 = s * (float)((int)((b >> 4) & 0xfu) - 8);
  e1 = s * (float)((int)(b & 0xfu) - 8);
}

// 2 packed bytes -> 4 elements.
__device__ __forceinline__ float4 dequant2_int4(uint32_t h, float s) {
  float4 r;
  dequant_byte_int4(h & 0xffu, s, r.x, r.y);
  dequant_byte_int4((h >> 8) & 0xffu, s, r.z, r.w);
  return r;
}

__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// fp32 mean = correctly rounded acc / K (torch: sum then true division).
__device__ __forceinline__ float4 div4(float4 a, double k) {
  return make_float4((float)((double)a.x / k), (float)((double)a.y / k), (float)((double)a.z / k),
                     (float)((double)a.w / k));
}

// scale = fp32(absmax / q_max) (quant.py:99-100: fp32 tensor / Python int, i.e. / float(q_max));
// inv = fp32(1 / scale) as fbgemm's quantizer forms it.
struct ScaleInv {
  float scale, inv;
};
__device__ __forceinline__ ScaleInv make_scale(uint32_t absmax_bits, float qmax) {
  const float amax = __uint_as_float(absmax_bits);
  ScaleInv r;
  r.scale = (float)((double)amax / (double)qmax);
  r.inv = (float)(1.0 / (double)r.scale);
  return r;
}

// ------------------------------------------------------------------------------------------------
// reductions
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o, 64));
  return v;
}

// Block-wide max, result broadcast to every thread.
__device__ __forceinline__ uint32_t block_max(uint32_t v) {
  __shared__ uint32_t red[kWaves];
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  v = max(max(red[0], red[1]), max(red[2], red[3]));
  return v;
}

// Every block of a pass-2 kernel re-reduces the pass-1 partials (a kernel boundary separates them,
// so plain loads see pass 1's stores).
__device__ __forceinline__ uint32_t reduce_partials(const uint32_t* __restrict__ p, int count) {
  uint32_t m = 0;
  for (int k = threadIdx.x; k < count; k += kBlock) m = max(m, p[k]);
  return block_max(m);
}

// ------------------------------------------------------------------------------------------------
// wave-tile bodies (shared by the flat and the bucketed kernels)
//   lane l, instruction j in 0..3 of an int8 tile: elements 4*(j*64 + l) .. +3 (float4 j*64+l), whose
//   payload is dword j*64+l of the tile's 1 KiB; the LDS transpose hands lane l dwords 4l..4l+3.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void load_tile(const float4* __restrict__ x4, float4 (&v)[4], int lane) {
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = load4<true>(x4 + j * 64 + lane);
}

template <bool ST_NT = false>
__device__ __forceinline__ void quantize_tile_regs(const float4 (&v)[4], uint4* __restrict__ q16, float inv,
                                                   uint32_t* __restrict__ lds, int lane) {
#pragma unroll
  for (int j = 0; j < 4; ++j) lds[j * 64 + lane] = quant4(v[j], inv);
  __builtin_amdgcn_wave_barrier();
  const uint4 o = reinterpret_cast<const uint4*>(lds)[lane];
  __builtin_amdgcn_wave_barrier();
  store16<ST_NT>(q16 + lane, o);
}

// int4 wave tile: 2048 elements = 8 coalesced 16-byte loads per lane -> 16 packed bytes per lane,
// transposed through 1 KiB of LDS (lane l, load j packs float4 j*64+l into halfword j*64+l).
__device__ __forceinline__ void load_tile_int4(const float4* __restrict__ xs, float4 (&v)[8], int lane) {
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = load4<true>(xs + j * 64 + lane);
}

__device__ __forceinline__ void quantize_tile_int4_regs(const float4 (&v)[8], uint4* __restrict__ p16, float inv,
                                                        uint16_t* __restrict__ lds, int lane) {
#pragma unroll
  for (int j = 0; j < 8; ++j) lds[j * 64 + lane] = (uint16_t)quant4_int4(v[j], inv);
  __builtin_amdgcn_wave_barrier();
  const uint4 o = reinterpret_cast<const uint4*>(lds)[lane];
  __builtin_amdgcn_wave_barrier();
  p16[lane] = o;
}

// bucketed kernels (many tensors, one block per chunk of <= 8192 elements = 8 wave tiles)
// ------------------------------------------------------------------------------------------------
// Chunks may start anywhere (a compact bucket packs tensors back to back): the first `head` elements
// up to the next `align`-element boundary are done element-wise, the rest in vector units.
__device__ __forceinline__ int chunk_head(int64_t start, int len, int align) {
  const int h = (int)((align - (start % align)) % align);
  return h < len ? h : len;
}

// A chunk (<= 8192 elements) is at most 2 wave tiles per wave + < 1024 tail elements + < 16 head
// elements: small enough to hold in VGPRs, so each pass issues ALL of a chunk's loads before the first
// use (8 x 16 B per lane in flight; a one-tile-at-a-time loop leaves a 32 KiB chunk latency-bound).
constexpr int kChunkTilesPerWave = ADFL_SLQ_CHUNK_ELEMS / kTile / kWaves;  // 2
constexpr int kChunkTailPerThread = kTile / kBlock;                        // < 1024 tail elements -> 4
static_assert(ADFL_SLQ_CHUNK_ELEMS % (kTile * kWaves) == 0, "chunk = whole tiles per wave");

struct ChunkRegs {
  float4 v[kChunkTilesPerWave][4];
  float tail[kChunkTailPerThread];
  float head;
};

// Load chunk c (x non-temporal: dead after this pass) into registers in the quantize tile layout.
__device__ __forceinline__ void chunk_load(const float* __restrict__ x, const adfl_slq_chunk& c, ChunkRegs& r,
                                           int lane, int wave) {
  const float* xc = x + c.start;
  const int head = chunk_head(c.start, c.len, 16);  // 16 elements: 64-B x and 16-B payload alignment
  const int ntiles = (c.len - head) / kTile;
  const float4* x4 = reinterpret_cast<const float4*>(xc + head);
#pragma unroll
  for (int k = 0; k < kChunkTilesPerWave; ++k) {
    const int t = wave + k * kWaves;
    if (t < ntiles) load_tile(x4 + t * (kTile / 4), r.v[k], lane);
  }
  r.head = (int)threadIdx.x < head ? xc[threadIdx.x] : 0.0f;
  const int t0 = head + ntiles * kTile;
#pragma unroll
  for (int k = 0; k < kChunkTailPerThread; ++k) {
    const int i = t0 + k * kBlock + (int)threadIdx.x;
    r.tail[k] = i < c.len ? __builtin_nontemporal_load(xc + i) : 0.0f;
  }
}

// Quantize the registers of chunk c into the payload (tiles through the wave's LDS transpose).
__device__ __forceinline__ void chunk_store(const adfl_slq_chunk& c, const ChunkRegs& r, float inv,
                                            int8_t* __restrict__ q, uint32_t* __restrict__ lds, int lane, int wave) {
  int8_t* qc = q + c.start;
  const int head = chunk_head(c.start, c.len, 16);
  const int ntiles = (c.len - head) / kTile;
  uint4* q16 = reinterpret_cast<uint4*>(qc + head);
#pragma unroll
  for (int k = 0; k < kChunkTilesPerWave; ++k) {
    const int t = wave + k * kWaves;
    if (t < ntiles) quantize_tile_regs(r.v[k], q16 + t * (kTile / 16), inv, lds, lane);
  }
  if ((int)threadIdx.x < head) qc[threadIdx.x] = (int8_t)quant1(r.head, inv);
  const int t0 = head + ntiles * kTile;
#pragma unroll
  for (int k = 0; k < kChunkTailPerThread; ++k) {
    const int i = t0 + k * kBlock + (int)threadIdx.x;
    if (i < c.len) qc[i] = (int8_t)quant1(r.tail[k], inv);
  }
}

constexpr int kSegBlock = 1024;
constexpr int kSegWaves = kSegBlock / 64;
constexpr int kSegTilesPerWave = 4;
constexpr int64_t kSegMaxElems = (int64_t)kSegWaves * kSegTilesPerWave * kTile;  // 65536
constexpr int kSegChunks = (int)(kSegMaxElems / ADFL_SLQ_CHUNK_ELEMS);            // 8
static_assert(kSegChunks == ADFL_SLQ_RESIDENT_CHUNKS, "header constant");
static_assert(kSegMaxElems % ADFL_SLQ_CHUNK_ELEMS == 0, "segment = whole chunks");
static_assert(kSegBlock == kTile, "tail: one element per thread");

__device__ __forceinline__ uint32_t block_max_seg(uint32_t v) {
  __shared__ uint32_t red[kSegWaves];
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t m = red[0];
#pragma unroll
  for (int w = 1; w < kSegWaves; ++w) m = max(m, red[w]);
  return m;
}

// q_max as the fp32 value torch divides by (quant.py:99-100).
inline float qmax_f(int bits) { return (float)((1LL << (bits - 1)) - 1); }

inline int launch_status() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? ADFL_OK : (int)e;
}

}  // namespace

#endif  // ADFL_SLQ_DEVICE_H
