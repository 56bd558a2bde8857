// stoch_packed.hip — the QSGD / RQSGD wire format the bandwidth formula prices (bits + 1 bits per weight), for
// gfx950: quantize to it, decode from it, decode + axpby / scale from it. The C ABI is include/adfl_stoch.h's
// "packed planes" section; DESIGN.md §10 "Packed wire format" has the format and its measurements.
//
//   sign plane   bit (i & 7) of byte (i >> 3), LSB first: 1 exactly when the unpacked sign byte is -1 (x < 0)
//   level plane  bits > 4: the unpacked level byte; bits <= 4: byte j = (level[2j] << 4) | level[2j + 1]
//                (pack_4bit's nibble order), the low nibble 0 behind an odd tensor's last element
//
// Every tensor starts on a 64-element boundary of the bucket (ADFL_SLQ_ALIGN_ELEMS: 8 sign bytes, 32 nibble
// bytes), so every chunk does as well: a chunk never shares a byte of either plane with another tensor, its
// vector accesses are aligned, and there is no chunk head. A chunk that breaks the rule is skipped (nothing read
// or written); the Python layer, which knows the layout, raises instead.
//
// The arithmetic is stoch_device.h's, unchanged: quantize_regs with the unpacked kernels' fast / exact level
// forms and Philox counters, decode4 / decode_exact after a sign bit is widened to the +1 / -1 byte and a nibble
// to the level byte. The unpacked sign byte 0 (x == +-0, NaN) becomes +1 here, which changes no decoded value:
// such an element has level 0 (QSGD: fl(fl(norm * 0) / s) * (+1) = +0 as with 0; RQSGD: a zero element makes the
// minimum factor 0 and 0 * (+1) = +0; a NaN x makes the norm NaN and every value NaN either way).

#include <hip/hip_runtime.h>

#include <cstdint>

#include "adfl_stoch.h"
#include "apply_device.h"  // the axpby / scale tail shared with slq_codec.hip and stoch_codec.hip
#include "philox.h"
#include "stoch_device.h"

namespace {

constexpr int kPbQuantize = 4;  // Philox blocks per batch, as k_qsgd_quantize
constexpr uint32_t kAlignMask = ADFL_SLQ_ALIGN_ELEMS - 1;

__device__ __forceinline__ uint32_t sign_bit(float x) { return x < 0.0f ? 1u : 0u; }

__device__ __forceinline__ uint32_t sign_nibble(const float4& v) {
  return sign_bit(v.x) | (sign_bit(v.y) << 1) | (sign_bit(v.z) << 2) | (sign_bit(v.w) << 3);
}

// 4 sign bits -> the sign plane's dword of +1 (0x01) / -1 (0xff) bytes
__device__ __forceinline__ uint32_t sign_bytes(uint32_t nib) {
  const uint32_t m = (nib & 1u) | ((nib & 2u) << 7) | ((nib & 4u) << 14) | ((nib & 8u) << 21);
  return 0x01010101u + m * 0xfeu;
}

// the level dword l0 | l1 << 8 | l2 << 16 | l3 << 24 <-> its two nibble bytes (l0 << 4 | l1) | (l2 << 4 | l3) << 8
__device__ __forceinline__ uint32_t nibbles_of(uint32_t q) {
  return ((q & 0xfu) << 4) | ((q >> 8) & 0xfu) | (((q >> 16) & 0xfu) << 12) | (((q >> 24) & 0xfu) << 8);
}

__device__ __forceinline__ uint32_t levels_of(uint32_t h) {
  return ((h >> 4) & 0xfu) | ((h & 0xfu) << 8) | (((h >> 12) & 0xfu) << 16) | (((h >> 8) & 0xfu) << 24);
}

// one element's level and sign byte, read from a chunk's planes (lv / sb: the chunk's first byte of each)
template <bool NIB>
__device__ __forceinline__ uint32_t level_at(const uint8_t* __restrict__ lv, int i) {
  if (!NIB) return lv[i];
  return ((uint32_t)lv[i >> 1] >> ((i & 1) ? 0 : 4)) & 0xfu;
}

__device__ __forceinline__ uint32_t sign_at(const uint8_t* __restrict__ sb, int i) {
  return ((sb[i >> 3] >> (i & 7)) & 1u) ? 0xffu : 0x01u;
}

struct NoAcc {
  __device__ __forceinline__ void add4(const float4&) {}
};

// quantize_regs for a tensor whose uniform index u0 + 4k is not a multiple of 4 at its 4-element groups
// (u0 % 4 = p in 1..3): element e of group k draws word (p + e) % 4 of Philox block u0 / 4 + k + (p + e) / 4, words
// p..3 of the group's own block and words 0..p-1 of the next, both made by the lane (stoch_delta.hip's
// quantize_regs_straddle, the form without cross-lane moves). The same element rules, ballot and post hook; Philox
// uniforms only; LV false: the level dword is post's to store.
template <int PB, bool LV, class F, class E, class P>
__device__ __forceinline__ void quantize_regs_two_blocks(const float4 (&v)[kPer], int tg, int n4, int64_t u0,
                                                         const Uniforms& U, uint32_t* __restrict__ l4, F fast, E exact,
                                                         bool all_exact, P post) {
  static_assert(kPer % PB == 0, "batches tile a chunk's groups");
  const int p = (int)(u0 & 3);  // block-uniform
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
      const bool live = k < n4;
      const uint4 a = w[2 * i], b = w[2 * i + 1];
      const float4 uj = make_float4(u24(p == 1 ? a.y : p == 2 ? a.z : a.w), u24(p == 1 ? a.z : p == 2 ? a.w : b.x),
                                    u24(p == 1 ? a.w : p == 2 ? b.x : b.y), u24(p == 1 ? b.x : p == 2 ? b.y : b.z));
      bool bad = all_exact;
      uint32_t q = pack4(fast(v[j].x, uj.x, bad), fast(v[j].y, uj.y, bad), fast(v[j].z, uj.z, bad),
                         fast(v[j].w, uj.w, bad));
      if (wave_any(bad && live))
        q = pack4(exact(v[j].x, uj.x), exact(v[j].y, uj.y), exact(v[j].z, uj.z), exact(v[j].w, uj.w));
      if (LV && live) l4[k] = q;
      post(j, k, live, q);  // every lane
    }
  }
}

// ------------------------------------------------------------------------------------------------
// quantize given norms
// ------------------------------------------------------------------------------------------------
// k_qsgd_quantize's shape: one block per chunk, the chunk's float4 groups loaded up front, quantize_regs. A lane
// holds 4 consecutive elements: its 4 sign bits are combined with its 7 neighbours' by three xor-shuffles and the
// first lane of every 8 stores the dword; at bits <= 4 every lane stores its group's two nibble bytes (128 B per
// wave store). The vector part covers the chunk's whole 32-element sign dwords; the < 32 elements behind them go
// by octets, one thread per sign byte (8 elements: one sign byte, 8 level bytes or 4 nibble bytes, each written
// once, whole, zero-filled behind the tensor's last element).
//
// ushift (per tensor, or null = 0): element g of the bucket draws the uniform of index g + ushift — the compact
// bucket's index when the planes live in the aligned one (adfl_rqsgd_encode_delta_batched's rule). A tensor whose
// ushift is not a multiple of 4 draws a group's uniforms from two Philox blocks (quantize_regs_two_blocks); with
// injected uniforms, a test hook, it has no 16-byte load of the plane and its chunks go by octets whole (the exact
// forms, equal to the fast ones wherever those hold). Both decisions are per tensor, hence block-uniform.
// SHIFT false (the entry's d_ushift == NULL): the kernel without the shifted paths, 78 VGPRs and 6 waves per SIMD
// against 82 and 5 with them.
template <int PB, bool NIB, bool SHIFT>
__global__ __launch_bounds__(kBlock) void k_stoch_quantize_packed(const float* __restrict__ x,
                                                                  const adfl_slq_chunk* __restrict__ chunks, float s,
                                                                  const float* __restrict__ norms,
                                                                  const int64_t* __restrict__ ushift, Uniforms U,
                                                                  uint8_t* __restrict__ levels,
                                                                  uint8_t* __restrict__ signbits) {
  const adfl_slq_chunk c = chunks[gridDim.x - 1 - blockIdx.x];  // reverse, as k_qsgd_quantize
  if ((uint32_t)c.start & kAlignMask) return;
  const float norm = norms[c.tensor];
  uint8_t* lv = levels + (NIB ? c.start >> 1 : c.start);
  uint8_t* sb = signbits + (c.start >> 3);
  const int noct = (c.len + 7) >> 3;
  if (norm == 0.0f) {  // quant.py:227-228: level 0, sign +1 = bit 0
    const int nlv = NIB ? (c.len + 1) >> 1 : c.len;
    for (int i = threadIdx.x; i < nlv; i += kBlock) lv[i] = 0;
    for (int i = threadIdx.x; i < noct; i += kBlock) sb[i] = 0;
    return;
  }
  const int64_t us = SHIFT ? ushift[c.tensor] : 0;
  const Div d = make_div(norm);
  const float* xc = x + c.start;
  const auto fast = [&](float xv, float uv, bool& bad) { return qsgd_level_fast(xv, s, d, uv, bad); };
  const auto exact = [&](float xv, float uv) { return qsgd_level_exact(xv, s, norm, uv); };
  const bool straddle = SHIFT && (us & 3) != 0;
  const int n4 = (!straddle || !U.inj) ? (c.len >> 5) << 3 : 0;  // groups of the whole sign dwords
  if (n4 > 0) {                                            // block-uniform
    float4 v[kPer];
    const float4* x4 = reinterpret_cast<const float4*>(xc);
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int k = (int)threadIdx.x + j * kBlock;
      if (k < n4) v[j] = load4_nt(x4 + k);
    }
    uint32_t* s4 = reinterpret_cast<uint32_t*>(sb);
    uint16_t* l2 = reinterpret_cast<uint16_t*>(lv);
    const auto post = [&](int j, int k, bool live, uint32_t q) {  // every lane: the shuffles span the wave
      uint32_t w = live ? sign_nibble(v[j]) << (4 * (k & 7)) : 0u;
      w |= (uint32_t)__shfl_xor((int)w, 1, 64);
      w |= (uint32_t)__shfl_xor((int)w, 2, 64);
      w |= (uint32_t)__shfl_xor((int)w, 4, 64);
      if (live && (k & 7) == 0) s4[k >> 3] = w;  // n4 % 8 == 0: the 8 lanes of a dword are live together
      if (NIB && live) l2[k] = (uint16_t)nibbles_of(q);
    };
    if (straddle)
      quantize_regs_two_blocks<PB / 2, !NIB>(v, threadIdx.x, n4, c.start + us, U, reinterpret_cast<uint32_t*>(lv), fast,
                                             exact, !d.fast, post);
    else
      quantize_regs<PB, decltype(fast), decltype(exact), NoAcc, decltype(post), !NIB>(
          v, threadIdx.x, n4, c.start + us, U, reinterpret_cast<uint32_t*>(lv), nullptr, fast, exact, !d.fast,
          (NoAcc*)nullptr, nullptr, 0, post);
  }
  for (int o = (n4 >> 1) + (int)threadIdx.x; o < noct; o += kBlock) {
    const int e0 = o << 3;
    const int m = c.len - e0 < 8 ? c.len - e0 : 8;
    uint32_t bits = 0u, lo = 0u, hi = 0u;  // the octet's sign byte and its level bytes 0..3 / 4..7
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      if (e < m) {
        const float xv = xc[e0 + e];
        const uint32_t l = exact(xv, U.one(c.start + us + e0 + e));
        bits |= sign_bit(xv) << e;
        if (e < 4)
          lo |= l << (8 * e);
        else
          hi |= l << (8 * (e - 4));
      }
    }
    sb[o] = (uint8_t)bits;
    if (NIB) {
      const uint32_t h = nibbles_of(lo) | (nibbles_of(hi) << 16);
#pragma unroll
      for (int b = 0; b < 4; ++b)
        if (2 * b < m) lv[(e0 >> 1) + b] = (uint8_t)(h >> (8 * b));
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (e < m) lv[e0 + e] = (uint8_t)((e < 4 ? lo >> (8 * e) : hi >> (8 * (e - 4))));
    }
  }
}

// ------------------------------------------------------------------------------------------------
// decode
// ------------------------------------------------------------------------------------------------
// k_stoch_dequantize's shape, in wave tiles of 1024 elements: lane l loads 16 level bytes (8 nibble bytes at
// bits <= 4) and lanes 0..31 one dword of sign bits (1 KiB or 512 B, and 128 B, per tile), a per-wave LDS
// transpose hands lane l the level dwords (nibble halfwords) j * 64 + l, j = 0..3, a shuffle the sign dword its
// group's 4 bits sit in, and the four float4 results are non-temporal 16-byte stores contiguous across the wave. A
// wave issues all its tiles' loads before consuming the first. The < 1024 elements behind the last whole tile go
// per group, the tensor's last < 4 per element.
constexpr int kDecTile = 1024;
static_assert(ADFL_SLQ_CHUNK_ELEMS / kDecTile / kWaves == 2, "one chunk is two tiles per wave");

template <int KIND, bool NIB>
__global__ __launch_bounds__(kBlock) void k_stoch_dequantize_packed(const uint8_t* __restrict__ levels,
                                                                    const uint8_t* __restrict__ signbits,
                                                                    const adfl_slq_chunk* __restrict__ chunks,
                                                                    const float* __restrict__ norms,
                                                                    const float* __restrict__ mins, float s,
                                                                    float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kWaves][kDecTile / 4];
  const adfl_slq_chunk c = chunks[blockIdx.x];
  if ((uint32_t)c.start & kAlignMask) return;
  const float norm = norms[c.tensor];
  const float mn = KIND == 1 ? mins[c.tensor] : 0.0f;
  float* oc = out + c.start;
  if (norm == 0.0f) {  // quant.py:248-249 / :390-391
    for (int i = threadIdx.x; i < c.len; i += kBlock) oc[i] = 0.0f;
    return;
  }
  const Div d = make_div(s);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint8_t* lv = levels + (NIB ? c.start >> 1 : c.start);
  const uint8_t* sb = signbits + (c.start >> 3);
  constexpr int kTileLv = NIB ? kDecTile / 2 : kDecTile;  // level bytes per tile
  const int ntiles = c.len / kDecTile;
  const int t0 = wave, t1 = wave + kWaves;
  uint4 L0 = make_uint4(0u, 0u, 0u, 0u), L1 = L0;
  uint32_t S0 = 0u, S1 = 0u;
  const auto load = [&](int t, uint4& L, uint32_t& S) {
    if (NIB) {
      const uint2 p = reinterpret_cast<const uint2*>(lv + t * kTileLv)[lane];
      L.x = p.x;
      L.y = p.y;
    } else {
      L = reinterpret_cast<const uint4*>(lv + t * kTileLv)[lane];
    }
    if (lane < 32) S = reinterpret_cast<const uint32_t*>(sb + t * (kDecTile / 8))[lane];
  };
  if (t0 < ntiles) load(t0, L0, S0);  // wave-uniform
  if (t1 < ntiles) load(t1, L1, S1);
  const auto tile = [&](int t, const uint4& L, uint32_t S) {
    if (NIB)
      reinterpret_cast<uint2*>(lds[wave])[lane] = make_uint2(L.x, L.y);
    else
      reinterpret_cast<uint4*>(lds[wave])[lane] = L;
    __builtin_amdgcn_wave_barrier();
    uint32_t lw[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      lw[j] = NIB ? levels_of(reinterpret_cast<const uint16_t*>(lds[wave])[j * 64 + lane]) : lds[wave][j * 64 + lane];
    __builtin_amdgcn_wave_barrier();
    float4* o4 = reinterpret_cast<float4*>(oc + t * kDecTile);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      // group j * 64 + lane: bits 4 (lane & 7) .. + 3 of sign dword j * 8 + (lane >> 3), which lane (that) holds
      const uint32_t w = (uint32_t)__shfl((int)S, j * 8 + (lane >> 3), 64);
      const uint32_t g = sign_bytes((w >> (4 * (lane & 7))) & 0xfu);
      store4_nt(o4 + j * 64 + lane, decode4<KIND>(lw[j], g, norm, mn, d, s, true));
    }
  };
  if (t0 < ntiles) tile(t0, L0, S0);
  if (t1 < ntiles) tile(t1, L1, S1);
  const int rs = ntiles * kDecTile;
  const int n4 = (c.len - rs) >> 2;
  if (n4 > 0) {  // block-uniform: < 256 groups, one per thread
    const int k = threadIdx.x;
    const bool live = k < n4;
    uint32_t l = 0u, g = 0x01010101u;
    if (live) {
      l = NIB ? levels_of(reinterpret_cast<const uint16_t*>(lv + (rs >> 1))[k])
              : reinterpret_cast<const uint32_t*>(lv + rs)[k];
      g = sign_bytes(((uint32_t)sb[(rs >> 3) + (k >> 1)] >> (4 * (k & 1))) & 0xfu);
    }
    const float4 r = decode4<KIND>(l, g, norm, mn, d, s, live);
    if (live) store4_nt(reinterpret_cast<float4*>(oc + rs) + k, r);
  }
  const int i = rs + (n4 << 2) + (int)threadIdx.x;  // the tensor's last < 4 elements
  if (i < c.len) oc[i] = decode_exact<KIND>(level_at<NIB>(lv, i), sign_at(sb, i), norm, mn, s);
}

// ------------------------------------------------------------------------------------------------
// decode + axpby / scale
// ------------------------------------------------------------------------------------------------
// k_stoch_dequantize_axpby's shape: the chunk's level dwords (nibble halfwords) and the sign byte each group's 4
// bits sit in are loaded whole, decoded once (decode4, the decode kernel's values; +0 for a tensor whose norm is
// 0) into 8 float4 per thread, and apply_chunk walks the targets. A chunk always starts on a group boundary here,
// so only a target that is not 16-byte aligned, and the tensor's last < 4 elements, go element by element
// (decode_exact), with the same results.
template <int KIND, bool NIB>
__global__ __launch_bounds__(kBlock) void k_stoch_dequantize_axpby_packed(const uint8_t* __restrict__ levels,
                                                                          const uint8_t* __restrict__ signbits,
                                                                          const adfl_slq_chunk* __restrict__ chunks,
                                                                          const float* __restrict__ norms,
                                                                          const float* __restrict__ mins, float s,
                                                                          ApplyTargets a) {
  static_assert(kApplyBlock == kBlock && kApplyGroups == kPer, "apply_chunk's thread layout");
  const adfl_slq_chunk c = chunks[blockIdx.x];
  if ((uint32_t)c.start & kAlignMask) return;
  const float norm = norms[c.tensor];
  const float mn = KIND == 1 ? mins[c.tensor] : 0.0f;
  const int64_t in_tensor = (int64_t)(blockIdx.x - c.first_chunk) * ADFL_SLQ_CHUNK_ELEMS;
  const uint8_t* lv = levels + (NIB ? c.start >> 1 : c.start);
  const uint8_t* sb = signbits + (c.start >> 3);
  auto dec1 = [&](int i) -> float {  // quant.py:248-249 / :390-391: zeros when the norm is 0
    return norm == 0.0f ? 0.0f : decode_exact<KIND>(level_at<NIB>(lv, i), sign_at(sb, i), norm, mn, s);
  };
  float4 dv[kPer];
  const int n4 = c.len >> 2;
  uint32_t L[kPer], G[kPer];
#pragma unroll
  for (int j = 0; j < kPer; ++j) {  // every load of the chunk before the first use
    const int k = (int)threadIdx.x + j * kBlock;
    L[j] = k >= n4 ? 0u : NIB ? (uint32_t) reinterpret_cast<const uint16_t*>(lv)[k]
                              : reinterpret_cast<const uint32_t*>(lv)[k];
    G[j] = k >= n4 ? 0u : (uint32_t)sb[k >> 1];
  }
  if (norm == 0.0f) {  // block-uniform
#pragma unroll
    for (int j = 0; j < kPer; ++j) dv[j] = make_float4(0.f, 0.f, 0.f, 0.f);
  } else {
    const Div dd = make_div(s);
#pragma unroll
    for (int j = 0; j < kPer; ++j) {  // every lane calls (a wave ballot inside)
      const int k = (int)threadIdx.x + j * kBlock;
      dv[j] = decode4<KIND>(NIB ? levels_of(L[j]) : L[j], sign_bytes((G[j] >> (4 * (k & 1))) & 0xfu), norm, mn, dd, s,
                            k < n4);
    }
  }
  apply_chunk(dv, true, c, in_tensor, a, dec1);
}

// ------------------------------------------------------------------------------------------------
// host helpers
// ------------------------------------------------------------------------------------------------
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

inline int launch_status() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? ADFL_OK : (int)e;
}

inline bool bad_codec(int32_t codec) { return codec != ADFL_CODEC_QSGD && codec != ADFL_CODEC_RQSGD; }

inline bool bad_table(const adfl_slq_chunk* d_chunks, int64_t nchunks) {
  return !d_chunks || nchunks < 1 || nchunks > INT32_MAX;
}

inline int check_bits8(int bits) { return (bits >= 1 && bits <= 8) ? ADFL_OK : ADFL_E_BITS; }

inline float levels_f(int bits) { return (float)((1 << bits) - 1); }  // self.levels = 2**bits - 1

}  // namespace

extern "C" {

int adfl_stoch_quantize_packed_batched(int32_t codec, const float* d_x, const adfl_slq_chunk* d_chunks,
                                       int64_t nchunks, int bits, const float* d_norms, const float* d_uniforms,
                                       const int64_t* d_ushift, uint64_t seed, uint64_t counter, uint8_t* d_levels,
                                       uint8_t* d_signbits, void* stream) {
  if (bad_codec(codec) || !d_x || !d_norms || !d_levels || !d_signbits || bad_table(d_chunks, nchunks))
    return ADFL_E_ARG;
  if (int st = check_bits8(bits)) return st;
  if (!aligned16(d_x) || !aligned16(d_levels) || !aligned16(d_signbits) || (d_uniforms && !aligned16(d_uniforms)))
    return ADFL_E_ALIGN;
  const Uniforms U{d_uniforms, seed, counter};
  // one level rule for both codecs (quant.py:230-238, :371-379): the codec only names the norm the caller passes
  const bool nib = bits <= 4;
  auto kern = d_ushift ? (nib ? k_stoch_quantize_packed<kPbQuantize, true, true>
                              : k_stoch_quantize_packed<kPbQuantize, false, true>)
                       : (nib ? k_stoch_quantize_packed<kPbQuantize, true, false>
                              : k_stoch_quantize_packed<kPbQuantize, false, false>);
  hipLaunchKernelGGL(kern, dim3((unsigned)nchunks), dim3(kBlock), 0, (hipStream_t)stream, d_x, d_chunks,
                     levels_f(bits), d_norms, d_ushift, U, d_levels, d_signbits);
  return launch_status();
}

int adfl_stoch_dequantize_packed_batched(int32_t codec, const uint8_t* d_levels, const uint8_t* d_signbits,
                                         const adfl_slq_chunk* d_chunks, int64_t nchunks, int bits,
                                         const float* d_norms, const float* d_mins, float* d_out, void* stream) {
  if (bad_codec(codec) || !d_levels || !d_signbits || !d_norms || (codec == ADFL_CODEC_RQSGD && !d_mins) || !d_out ||
      bad_table(d_chunks, nchunks))
    return ADFL_E_ARG;
  if (int st = check_bits8(bits)) return st;
  if (!aligned16(d_levels) || !aligned16(d_signbits) || !aligned16(d_out)) return ADFL_E_ALIGN;
  const bool nib = bits <= 4;
  auto kern = codec == ADFL_CODEC_QSGD ? (nib ? k_stoch_dequantize_packed<0, true> : k_stoch_dequantize_packed<0, false>)
                                       : (nib ? k_stoch_dequantize_packed<1, true> : k_stoch_dequantize_packed<1, false>);
  hipLaunchKernelGGL(kern, dim3((unsigned)nchunks), dim3(kBlock), 0, (hipStream_t)stream, d_levels, d_signbits,
                     d_chunks, d_norms, d_mins, levels_f(bits), d_out);
  return launch_status();
}

int adfl_stoch_dequantize_axpby_packed_batched(int32_t codec, const uint8_t* d_levels, const uint8_t* d_signbits,
                                               const adfl_slq_chunk* d_chunks, int64_t nchunks, int bits,
                                               const float* d_norms, const float* d_mins, const float* const* d_base,
                                               float* const* d_out, int32_t ntensors, int32_t ntargets, float alpha,
                                               float beta, void* stream) {
  if (bad_codec(codec) || !d_levels || !d_signbits || !d_norms || (codec == ADFL_CODEC_RQSGD && !d_mins) ||
      apply_bad_args(d_chunks, nchunks, d_out, ntensors, ntargets))
    return ADFL_E_ARG;
  if (int st = check_bits8(bits)) return st;
  if (!aligned16(d_levels) || !aligned16(d_signbits)) return ADFL_E_ALIGN;
  const ApplyTargets a{d_base, d_out, (int)ntensors, (int)ntargets, alpha, beta};
  const bool nib = bits <= 4;
  auto kern = codec == ADFL_CODEC_QSGD
                  ? (nib ? k_stoch_dequantize_axpby_packed<0, true> : k_stoch_dequantize_axpby_packed<0, false>)
                  : (nib ? k_stoch_dequantize_axpby_packed<1, true> : k_stoch_dequantize_axpby_packed<1, false>);
  hipLaunchKernelGGL(kern, dim3((unsigned)nchunks), dim3(kBlock), 0, (hipStream_t)stream, d_levels, d_signbits,
                     d_chunks, d_norms, d_mins, levels_f(bits), a);
  return launch_status();
}

}  // extern "C"
