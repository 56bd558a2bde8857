// stoch_device.h — the stochastic codecs' device helpers shared by stoch_codec.hip, stoch_delta.hip and stoch_packed.hip: the
// Philox uniforms, the QSGD / RQSGD element rules, the max / min reduction, a chunk's head / edge indexing and
// the register quantize body. Everything is in an anonymous namespace: each translation unit gets its own copy
// (internal linkage), as before the split. The one host entry shared across the two units is
// adfl_stoch_detail::launch_finalize_linf (defined in stoch_codec.hip, beside the kernel it launches).
#ifndef ADFL_STOCH_DEVICE_H
#define ADFL_STOCH_DEVICE_H

#include <hip/hip_runtime.h>

#include <cstdint>

#include "adfl_stoch.h"
#include "philox.h"

namespace adfl_stoch_detail {
// k_norm_finalize<ADFL_NORM_LINF> over a workspace of one {max, min} |x| bit pair (8 bytes) per chunk:
// d_norms[t] = max, d_mins[t] = min, both NaN when any chunk's max is a NaN pattern.
int launch_finalize_linf(const adfl_slq_chunk* d_chunks, int64_t nchunks, const void* d_ws, float* d_norms,
                         float* d_mins, hipStream_t st);
}  // namespace adfl_stoch_detail

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int64_t kPartialBytes = 16;  // per chunk: fp64 sum of squares, or {max, min} |x| bits

// ------------------------------------------------------------------------------------------------
// uniforms
// ------------------------------------------------------------------------------------------------
using adfl::kPhiloxRounds;
using adfl::philox4x32;

__device__ __forceinline__ float u24(uint32_t w) { return (float)(w >> 8) * 0x1p-24f; }

// B independent Philox4x32 blocks with their rounds interleaved: a single block is a chain of dependent
// 64-bit multiply rounds, which with only 4-5 waves per SIMD leaves the VALU waiting on latency
// (tools/microbench_stoch_res.hip: 9.3 us of C3's resident QSGD encode); B chains in lockstep give the
// scheduler B independent instructions per step. Same words as philox4x32, bit for bit.
template <int B>
__device__ __forceinline__ void philox4x32_batch(const uint64_t (&ctr)[B], uint64_t seed, uint4 (&out)[B]) {
  uint32_t c0[B], c1[B], c2[B], c3[B];
#pragma unroll
  for (int i = 0; i < B; ++i) {
    c0[i] = (uint32_t)ctr[i];
    c1[i] = (uint32_t)(ctr[i] >> 32);
    c2[i] = 0;
    c3[i] = 0;
  }
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < kPhiloxRounds; ++r) {
#pragma unroll
    for (int i = 0; i < B; ++i) {
      const uint64_t p0 = (uint64_t)0xD2511F53u * c0[i], p1 = (uint64_t)0xCD9E8D57u * c2[i];
      c0[i] = (uint32_t)(p1 >> 32) ^ c1[i] ^ k0;  // no v_xor3_b32 on gfx950: two v_xor_b32
      c1[i] = (uint32_t)p1;
      c2[i] = (uint32_t)(p0 >> 32) ^ c3[i] ^ k1;
      c3[i] = (uint32_t)p0;
    }
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
#pragma unroll
  for (int i = 0; i < B; ++i) out[i] = make_uint4(c0[i], c1[i], c2[i], c3[i]);
}

struct Uniforms {
  const float* inj;  // injected plane (indexed like x) or null
  uint64_t seed, counter;

  // u for elements g .. g+3, g % 4 == 0
  __device__ __forceinline__ float4 group(int64_t g) const {
    if (inj) return *reinterpret_cast<const float4*>(inj + g);
    const uint4 w = philox4x32(counter + (uint64_t)(g >> 2), seed);
    return make_float4(u24(w.x), u24(w.y), u24(w.z), u24(w.w));
  }
  __device__ __forceinline__ float one(int64_t g) const {
    if (inj) return inj[g];
    const uint4 w = philox4x32(counter + (uint64_t)(g >> 2), seed);
    const int k = (int)(g & 3);
    return u24(k == 0 ? w.x : k == 1 ? w.y : k == 2 ? w.z : w.w);
  }
};

// ------------------------------------------------------------------------------------------------
// element rules
// ------------------------------------------------------------------------------------------------
// torch's fp32 -> uint8 / int8 conversion on x86: truncate to int32 (NaN and out-of-range give INT32_MIN,
// whose low byte is 0), keep the low byte.
__device__ __forceinline__ uint32_t low_byte(float v) {
  if (!(v > -2147483648.0f && v < 2147483648.0f)) return 0u;
  return (uint32_t)(int)v & 0xffu;
}

__device__ __forceinline__ uint32_t sign_byte(float x) { return (uint32_t)((x > 0.0f) - (x < 0.0f)) & 0xffu; }

__device__ __forceinline__ uint32_t pack4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  return a | (b << 8) | (c << 16) | (d << 24);
}

// Every element rule below comes in two forms:
//  * an EXACT form — the reference's fp32 arithmetic, including every special case (NaN, inf, overflow,
//    caller-supplied tiny norms), with correctly rounded __fdiv_rn divisions;
//  * a FAST form — branch-free, the same result wherever it sets no `bad` flag. The kernels evaluate the
//    fast form for a float4 group, and if any lane of the wave flagged its group (a wave-uniform ballot)
//    that wave recomputes the flagged lanes with the exact form. Per-element exec-mask branching on rare
//    cases made the kernels issue-bound (267 saveexec / 196 branches for 32 elements per lane).
//
// Division. The fast form uses a per-tensor reciprocal (Markstein): y = RN(1/b), q = RN(a*y),
// r = RN(a - b*q) (exact), q' = RN(q + r*y) = RN(a/b) while every intermediate stays normal; it is valid
// for b in [2^-60, 2^60] (block-uniform) and |a| in {0} U [2^-60, 2^60]. 4.4 vs 12.1 lane-cycles per
// quotient, and 0 of 1.7e10 random operand pairs differ from __fdiv_rn (tools/microbench_stoch.hip,
// profiles/r01/microbench_stoch.txt). That count is evidence; what guards the window, the flags and the ballot is
// tests/test_gpu_stoch_boundary.py on the inputs of tests/boundary_cases.py: scaled on every integer and one ulp
// to either side, u == prob, both window edges, waves with only some lanes flagged, and the reason for 2^60 —
// 2^-60 / 2^60 keeps the quotient normal; a denormal quotient can be an exact tie, which q' rounds by the sign of
// y's error instead of to even (the fixture's `tie` elements differ with the window at 2^+-70).
struct Div {
  float b, y;
  bool fast;
};

__device__ __forceinline__ Div make_div(float b) {
  Div d;
  d.b = b;
  d.y = __fdiv_rn(1.0f, b);
  d.fast = b >= 0x1p-60f && b <= 0x1p60f;
  return d;
}

__device__ __forceinline__ float div_fast(float a, const Div& d, bool& bad) {
  const float aa = __builtin_fabsf(a);
  bad |= !(aa <= 0x1p60f && (aa >= 0x1p-60f || aa == 0.0f));
  const float q = a * d.y;
  const float r = __builtin_fmaf(-d.b, q, a);
  return __builtin_fmaf(r, d.y, q);  // +0 for a = +0 (a is never -0 on these paths)
}

// QSGD / RQSGD level (quant.py:230-236): s * |x| / norm in fp32, floor, stochastic round up, u8.
__device__ __forceinline__ uint32_t qsgd_level_exact(float x, float s, float norm, float u) {
  const float scaled = __fdiv_rn(s * __builtin_fabsf(x), norm);
  const float l = __builtin_floorf(scaled);
  return low_byte(l + (u < scaled - l ? 1.0f : 0.0f));
}

// Fast form: for 0 <= scaled < 2^24 (every level of bits <= 16 against its own norm) the floor is an
// integer truncation and l + 1 is exact in fp32.
__device__ __forceinline__ uint32_t qsgd_level_fast(float x, float s, const Div& d, float u, bool& bad) {
  const float scaled = div_fast(s * __builtin_fabsf(x), d, bad);
  bad |= !(scaled < 16777216.0f);                          // also catches NaN
  const float sc = __builtin_fminf(scaled, 16777215.0f);   // keep the conversion defined when flagged
  const int l = (int)sc;
  return (uint32_t)(l + (u < sc - (float)l ? 1 : 0)) & 0xffu;
}

// ------------------------------------------------------------------------------------------------
// reductions
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint2 block_maxmin(uint32_t mx, uint32_t mn) {
  __shared__ uint32_t red[2][kWaves];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mx = max(mx, (uint32_t)__shfl_xor((int)mx, o, 64));
    mn = min(mn, (uint32_t)__shfl_xor((int)mn, o, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = mx;
    red[1][threadIdx.x >> 6] = mn;
  }
  __syncthreads();
  const uint2 r = make_uint2(max(max(red[0][0], red[0][1]), max(red[0][2], red[0][3])),
                             min(min(red[1][0], red[1][1]), min(red[1][2], red[1][3])));
  __syncthreads();
  return r;
}

__device__ __forceinline__ uint32_t abs_bits(float v) { return __float_as_uint(v) & 0x7fffffffu; }

// streaming (non-temporal) 16-byte load: x is read once per pass and must not evict the payload planes
__device__ __forceinline__ float4 load4_nt(const float4* p) {
  typedef float f4v __attribute__((ext_vector_type(4)));
  const f4v v = __builtin_nontemporal_load(reinterpret_cast<const f4v*>(p));
  return make_float4(v.x, v.y, v.z, v.w);
}

// elements [0, head) of a chunk are done one by one, up to the first 4-element boundary of the bucket
__device__ __forceinline__ int chunk_head4(int64_t start, int len) {
  const int h = (int)((4 - (start & 3)) & 3);
  return h < len ? h : len;
}

// Work layout: one block per chunk (<= 8192 elements; a 1 GiB tensor is 32768 blocks). Inside a chunk
// every thread first issues all its loads (at most kPer = 8192 / 4 / 256 = 8 float4 or plane dwords),
// then computes. Measured alternatives (profiles/r01/stoch_*): a loop that consumes each load before
// issuing the next is latency-bound; blocks that walk a range of chunks serialise them and were slower
// still (fresh blocks overlap one another's loads and compute).
constexpr int kPer = ADFL_SLQ_CHUNK_ELEMS / 4 / kBlock;

// Per-element head / tail of a chunk: the < 4 elements before the first 4-element boundary and after the
// last; thread t < head takes head element t, the next threads the tail elements. Returns -1 if none.
__device__ __forceinline__ int edge_elem_t(int t, int head, int tail, int len) {
  if (t < head) return t;
  return (t - head < len - tail) ? tail + t - head : -1;
}

__device__ __forceinline__ int edge_elem(int head, int tail, int len) { return edge_elem_t(threadIdx.x, head, tail, len); }

__device__ __forceinline__ void fill_zero_norm(uint8_t* __restrict__ lv, int8_t* __restrict__ sg, int len,
                                               int t = threadIdx.x) {
  for (int i = t; i < len; i += kBlock) {
    lv[i] = 0;
    sg[i] = 1;
  }
}

__device__ __forceinline__ bool wave_any(bool p) { return __ballot(p) != 0ull; }

// Quantize a chunk's float4 groups held in registers: v[j] is group tg + j * kBlock of the chunk (tg = the
// thread's index in its 256-thread group). Per group the level / exponent bytes (fast form; exact form for
// the wave if any lane flagged its group) and the sign bytes, stored as one dword each (contiguous across
// the wave). `all_exact` is uniform over the group.
// Philox uniforms are generated PB groups at a time (philox4x32_batch); injected uniforms (a test path)
// are loaded group by group.
// pre (LDS, or null): Philox words generated ahead of time, group j's at pre[j * pre_stride]. s4 null: the
// caller stores the sign bytes itself.
// post(j, k, live, q): called by every lane of the wave for each group the wave reaches, with the level dword q the
// group stores (live lanes) — the hook of the encodes that also apply the stored bytes (it may hold a ballot).
// LV false (stoch_packed.hip's nibble levels): the level dword is not stored either, post writes its own form of q.
struct NoPost {
  __device__ __forceinline__ void operator()(int, int, bool, uint32_t) const {}
};

template <int PB, class F, class E, class A, class P = NoPost, bool LV = true>
__device__ __forceinline__ void quantize_regs(const float4 (&v)[kPer], int tg, int n4, int64_t g0, const Uniforms& U,
                                              uint32_t* __restrict__ l4, uint32_t* __restrict__ s4, F fast, E exact,
                                              bool all_exact, A* acc, const uint4* pre = nullptr,
                                              int pre_stride = 0, P post = P{}) {
  static_assert(kPer % PB == 0, "batches tile a chunk's groups");
#pragma unroll
  for (int jb = 0; jb < kPer; jb += PB) {
    if (jb * kBlock >= n4) break;  // group-uniform: no thread has group jb or later
    uint4 w[PB];
    if (!U.inj && pre) {
#pragma unroll
      for (int i = 0; i < PB; ++i) w[i] = pre[(jb + i) * pre_stride];
    } else if (!U.inj) {
      uint64_t ctr[PB];
#pragma unroll
      for (int i = 0; i < PB; ++i) ctr[i] = U.counter + (uint64_t)((g0 >> 2) + tg + (jb + i) * kBlock);
      philox4x32_batch(ctr, U.seed, w);
    }
#pragma unroll
    for (int i = 0; i < PB; ++i) {
      const int j = jb + i;
      const int k = tg + j * kBlock;
      if (j * kBlock >= n4) break;  // group-uniform
      const bool live = k < n4;
      float4 uj;
      if (!U.inj)
        uj = make_float4(u24(w[i].x), u24(w[i].y), u24(w[i].z), u24(w[i].w));
      else
        uj = U.group(g0 + 4 * (int64_t)(live ? k : 0));
      bool bad = all_exact;
      uint32_t q = pack4(fast(v[j].x, uj.x, bad), fast(v[j].y, uj.y, bad), fast(v[j].z, uj.z, bad),
                         fast(v[j].w, uj.w, bad));
      // the whole wave takes the exact form when any live lane flagged (equal results where the fast form
      // holds): `bad` is then only a wave-wide OR of compare masks, never a per-lane value
      if (wave_any(bad && live))
        q = pack4(exact(v[j].x, uj.x), exact(v[j].y, uj.y), exact(v[j].z, uj.z), exact(v[j].w, uj.w));
      if (live) {
        if (LV) l4[k] = q;
        if (s4) s4[k] = pack4(sign_byte(v[j].x), sign_byte(v[j].y), sign_byte(v[j].z), sign_byte(v[j].w));
        if (acc) acc->add4(v[j]);
      }
      post(j, k, live, q);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// decoders (shared: stoch_codec.hip's decode kernels, and the encodes that also apply what they stored)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float pow2i(int k) {  // 2^k for k in [-126, 128] (128 -> inf), exact
  return __uint_as_float((uint32_t)(k + 127) << 23);
}


// decoders (d divides by levels)
__device__ __forceinline__ float qsgd_value_exact(uint32_t l, uint32_t sgn, float norm, float s) {
  return __fdiv_rn(norm * (float)l, s) * (float)(int8_t)sgn;
}

__device__ __forceinline__ float qsgd_value_fast(uint32_t l, uint32_t sgn, float norm, const Div& d, bool& bad) {
  return div_fast(norm * (float)l, d, bad) * (float)(int8_t)sgn;
}

__device__ __forceinline__ float rqsgd_value_exact(uint32_t l, uint32_t sgn, float norm, float mn, float s) {
  const float sf = (float)(int8_t)sgn;
  return l == 0u ? mn * sf : __fdiv_rn((norm * sf) * (float)l, s);
}

__device__ __forceinline__ float rqsgd_value_fast(uint32_t l, uint32_t sgn, float norm, float mn, const Div& d,
                                                  bool& bad) {
  const float sf = (float)(int8_t)sgn;
  bool b2 = false;
  const float v = div_fast((norm * sf) * (float)l, d, b2);
  bad |= b2 & (l != 0u);
  return l == 0u ? mn * sf : v;
}

__device__ __forceinline__ float cnat_value(uint32_t e, uint32_t sgn, float norm) {
  const int k = (int)(int8_t)e;  // in [-128, 127]
  // 2^k exactly: normal for k >= -126, the denormals 2^-127 / 2^-128 below
  const float p = k >= -126 ? pow2i(k) : __uint_as_float(0x00400000u >> (-127 - k));
  return (norm * (float)(int8_t)sgn) * p;
}

__device__ __forceinline__ void store4_nt(float4* p, float4 d) {
  typedef float f4v __attribute__((ext_vector_type(4)));
  const f4v v = {d.x, d.y, d.z, d.w};
  __builtin_nontemporal_store(v, reinterpret_cast<f4v*>(p));
}

// Decoders. KIND 0 = QSGD, 1 = RQSGD, 2 = CNAT.
template <int KIND>
__device__ __forceinline__ float decode_exact(uint32_t l, uint32_t sgn, float norm, float mn, float s) {
  if (KIND == 0) return qsgd_value_exact(l, sgn, norm, s);
  if (KIND == 1) return rqsgd_value_exact(l, sgn, norm, mn, s);
  return cnat_value(l, sgn, norm);
}

template <int KIND>
__device__ __forceinline__ float decode_fast(uint32_t l, uint32_t sgn, float norm, float mn, const Div& d, bool& bad) {
  if (KIND == 0) return qsgd_value_fast(l, sgn, norm, d, bad);
  if (KIND == 1) return rqsgd_value_fast(l, sgn, norm, mn, d, bad);
  return cnat_value(l, sgn, norm);
}

// Four decoded values from one dword of levels and one of signs. The fast division path falls back to the
// exact one for the whole wave if any live lane's quotient is in doubt (every lane must call this).
template <int KIND>
__device__ __forceinline__ float4 decode4(uint32_t l, uint32_t g, float norm, float mn, const Div& d, float s,
                                          bool live) {
  bool bad = KIND != 2 && !d.fast;
  float4 r;
  r.x = decode_fast<KIND>(l & 0xffu, g & 0xffu, norm, mn, d, bad);
  r.y = decode_fast<KIND>((l >> 8) & 0xffu, (g >> 8) & 0xffu, norm, mn, d, bad);
  r.z = decode_fast<KIND>((l >> 16) & 0xffu, (g >> 16) & 0xffu, norm, mn, d, bad);
  r.w = decode_fast<KIND>(l >> 24, g >> 24, norm, mn, d, bad);
  if (KIND != 2 && wave_any(bad && live)) {
    r.x = decode_exact<KIND>(l & 0xffu, g & 0xffu, norm, mn, s);
    r.y = decode_exact<KIND>((l >> 8) & 0xffu, (g >> 8) & 0xffu, norm, mn, s);
    r.z = decode_exact<KIND>((l >> 16) & 0xffu, (g >> 16) & 0xffu, norm, mn, s);
    r.w = decode_exact<KIND>(l >> 24, g >> 24, norm, mn, s);
  }
  return r;
}

// The 4 sign bytes of a float4 group as the sign plane's dword.
__device__ __forceinline__ uint32_t sign4(const float4& x) {
  return pack4(sign_byte(x.x), sign_byte(x.y), sign_byte(x.z), sign_byte(x.w));
}

// h' = fp32(h + d) for one 4-element group of a hidden tensor: a 16-byte store where the group's address allows it
// (vec, block-uniform), four 4-byte stores otherwise; the same bits either way. The 16-byte store is non-temporal
// when kStochHiddenNt (slq_delta.hip's switch: the next broadcast reads h only after a whole buffer of client
// updates; DESIGN.md §10 has the A/B for these kernels).
#ifndef ADFL_UPDATE_H_NT
#define ADFL_UPDATE_H_NT 1
#endif
constexpr bool kStochHiddenNt = ADFL_UPDATE_H_NT != 0;

__device__ __forceinline__ float4 load_h4(const float* p, bool vec) {
  if (vec) return *reinterpret_cast<const float4*>(p);
  return make_float4(p[0], p[1], p[2], p[3]);
}

__device__ __forceinline__ void store_sum_h4(float* p, bool vec, const float4& h, const float4& d) {
  const float4 r = make_float4(h.x + d.x, h.y + d.y, h.z + d.z, h.w + d.w);
  if (vec && kStochHiddenNt) {
    store4_nt(reinterpret_cast<float4*>(p), r);
  } else if (vec) {
    *reinterpret_cast<float4*>(p) = r;
  } else {
    p[0] = r.x;
    p[1] = r.y;
    p[2] = r.z;
    p[3] = r.w;
  }
}

}  // namespace

#endif  // ADFL_STOCH_DEVICE_H
