// flush_device.h — the buffered servers' per-element flush functions, shared by server_flush.hip (the flush of a
// full buffer) and by the fused decode + accumulate + flush kernels of slq_codec.hip and stoch_codec.hip (the
// K-th client update: Src/ADFL/Strategy/fed_buff.py:68-100, Strategy/fadas.py:56-80), and the tail those fused
// kernels share. Anonymous namespace: each translation unit gets its own copy.
//
// Arithmetic: every operation is spelled with its rounding (__fmul_rn, __fadd_rn, __fdiv_rn, __fmaf_rn), so
// -ffp-contract decides nothing here. The square root is sqrtf: this toolchain's __fsqrt_rn expands to the
// native, 1-ulp v_sqrt_f32 unless OCML_BASIC_ROUNDED_OPERATIONS is defined, while sqrtf (like `/`, which is
// what __fdiv_rn expands to) is correctly rounded and keeps denormals under hipcc's default
// -fhip-fp32-correctly-rounded-divide-sqrt.
#ifndef ADFL_FLUSH_DEVICE_H
#define ADFL_FLUSH_DEVICE_H

#include <hip/hip_runtime.h>

#include <cstdint>

#include "adfl_slq.h"

namespace {

typedef float f4v __attribute__((ext_vector_type(4)));

struct FadasScalars {
  float k, beta1, omb1, beta2, omb2, sqrt_bc2, eps, step;
};

__device__ __forceinline__ float sqrt_rn(float x) { return sqrtf(x); }

// torch.maximum: NaN when either operand is; b on a tie (the sign of a zero tie cannot arise: v' >= +0).
__device__ __forceinline__ float maximum_nan(float a, float b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }

__device__ __forceinline__ float fedbuff1(float buf, float g, float k, float lr) {
  const float b = __fdiv_rn(buf, k);
  return __fadd_rn(__fmul_rn(1.0f, g), __fmul_rn(lr, b));
}

__device__ __forceinline__ float fadas1(float buf, float g, float& m, float& v, float& vh, const FadasScalars& s) {
  const float b = __fdiv_rn(buf, s.k);
  m = __fmaf_rn(b, s.omb1, __fmul_rn(m, s.beta1));
  v = __fmaf_rn(__fmul_rn(s.omb2, b), b, __fmul_rn(v, s.beta2));
  vh = maximum_nan(vh, v);
  const float den = __fadd_rn(__fdiv_rn(sqrt_rn(vh), s.sqrt_bc2), s.eps);
  return __fadd_rn(g, __fdiv_rn(__fmul_rn(s.step, m), den));
}

__device__ __forceinline__ f4v fadas4(f4v buf, f4v g, f4v& m, f4v& v, f4v& vh, const FadasScalars& s) {
  f4v r;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float m1 = m[e], v1 = v[e], h1 = vh[e];
    r[e] = fadas1(buf[e], g[e], m1, v1, h1, s);
    m[e] = m1;
    v[e] = v1;
    vh[e] = h1;
  }
  return r;
}

// ------------------------------------------------------------------------------------------------
// The K-th update of a buffered server in one pass: decode + accumulate + flush. Per element, with d the codec's
// decode of the stored bytes,
//   u = fp32(factor * d)                     FedBuff's tensor.float().mul_(f) (fed_buff.py:72-75); FADAS: 1.0
//   B = buf ? fp32(buf + u) : u              add_parameters_inpace(buffer, ., 1, 1) (model.py:337-347)
//   out = fedbuff1(B, g, K, lr)  or  fadas1(B, g, m, v, v_hat, s)
// B lives in a register: the buffer is never written (the reference clears it right after, fed_buff.py:96,
// fadas.py:75). Cache policy as the flush kernels': buf and g are dead after the read and out is not re-read soon
// (non-temporal); the moments are updated in place with plain loads and stores.
// ------------------------------------------------------------------------------------------------
constexpr int kFlushBlock = 256;
constexpr int kFlushGroups = ADFL_SLQ_CHUNK_ELEMS / 4 / kFlushBlock;  // float4 groups per thread and chunk: 8
constexpr int kFlushHalf = kFlushGroups / 2;                          // ... in flight at a time
static_assert(4 * kFlushGroups * kFlushBlock == ADFL_SLQ_CHUNK_ELEMS && 2 * kFlushHalf == kFlushGroups,
              "a chunk is two halves");

struct ReceiveFlush {
  const float* const* buf;  // one pointer per tensor, or null: no buffer (K = 1, or the update that becomes it)
  const float* const* g;
  float* const* m;          // m, v, vh: FADAS only
  float* const* v;
  float* const* vh;
  float* const* out;
  float factor, lr;         // FedBuff only (FADAS: factor 1.0f)
  FadasScalars s;           // s.k = (float)K for both
};

// One chunk's slices of the operand tables.
template <bool FADAS>
struct FlushSlices {
  const float* buf;
  const float* g;
  float* m;
  float* v;
  float* vh;
  float* out;

  __device__ __forceinline__ FlushSlices(const ReceiveFlush& a, const adfl_slq_chunk& c, int64_t in_tensor)
      : buf(a.buf ? a.buf[c.tensor] + in_tensor : nullptr),
        g(a.g[c.tensor] + in_tensor),
        m(FADAS ? a.m[c.tensor] + in_tensor : nullptr),
        v(FADAS ? a.v[c.tensor] + in_tensor : nullptr),
        vh(FADAS ? a.vh[c.tensor] + in_tensor : nullptr),
        out(a.out[c.tensor] + in_tensor) {}

  // every slice 16-byte aligned (block-uniform; an absent operand is null)
  __device__ __forceinline__ bool aligned16() const {
    return (((uintptr_t)buf | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)vh | (uintptr_t)out) & 15u) == 0;
  }

  // element i of the chunk from its decode d, 4-byte accesses
  __device__ __forceinline__ void one(int i, float d, const ReceiveFlush& a) const {
    const float u = __fmul_rn(a.factor, d);
    const float b = buf ? __fadd_rn(__builtin_nontemporal_load(buf + i), u) : u;
    const float gi = __builtin_nontemporal_load(g + i);
    float r;
    if (FADAS) {
      float m1 = m[i], v1 = v[i], h1 = vh[i];
      r = fadas1(b, gi, m1, v1, h1, a.s);
      m[i] = m1;
      v[i] = v1;
      vh[i] = h1;
    } else {
      r = fedbuff1(b, gi, a.s.k, a.lr);
    }
    __builtin_nontemporal_store(r, out + i);
  }
};

// One chunk of a fused decode + accumulate + flush kernel. vec (block-uniform): the kernel holds the chunk's payload
// words in registers and `sl.aligned16()`: dec4(j, live) is the decode of the chunk's float4 group threadIdx.x +
// j * 256 (j a constant after unrolling; called by every lane of a half that has a live group, for the stochastic
// decode's wave ballot), and the chunk is walked in two halves as k_fadas_flush_batched walks it: a half's loads are
// issued, its groups decoded while they are in flight, then combined and stored; the chunk's last < 4 elements
// one by one. Otherwise everything goes element by element through dec1(i), with the same results.
template <bool FADAS, class Dec4, class Dec1>
__device__ __forceinline__ void receive_flush_chunk(const FlushSlices<FADAS>& sl, bool vec, const adfl_slq_chunk& c,
                                                    const ReceiveFlush& a, Dec4 dec4, Dec1 dec1) {
  const int tid = (int)threadIdx.x;
  if (!vec) {
    for (int i = tid; i < c.len; i += kFlushBlock) sl.one(i, dec1(i), a);
    return;
  }
  const int n4 = c.len >> 2;
  const f4v* b4 = reinterpret_cast<const f4v*>(sl.buf);
  const f4v* g4 = reinterpret_cast<const f4v*>(sl.g);
  f4v* m4 = reinterpret_cast<f4v*>(sl.m);
  f4v* v4 = reinterpret_cast<f4v*>(sl.v);
  f4v* h4 = reinterpret_cast<f4v*>(sl.vh);
  f4v* o4 = reinterpret_cast<f4v*>(sl.out);
  const f4v zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    if (h * kFlushHalf * kFlushBlock >= n4) break;  // block-uniform: the half has no group
    const int k0 = tid + h * kFlushHalf * kFlushBlock;
    f4v vb[kFlushHalf], vg[kFlushHalf], vm[kFlushHalf], vv[kFlushHalf], vx[kFlushHalf];
#pragma unroll
    for (int j = 0; j < kFlushHalf; ++j)
      vb[j] = (b4 && k0 + j * kFlushBlock < n4) ? __builtin_nontemporal_load(b4 + k0 + j * kFlushBlock) : zero;
    if (FADAS) {
#pragma unroll
      for (int j = 0; j < kFlushHalf; ++j) vm[j] = k0 + j * kFlushBlock < n4 ? m4[k0 + j * kFlushBlock] : zero;
#pragma unroll
      for (int j = 0; j < kFlushHalf; ++j) vv[j] = k0 + j * kFlushBlock < n4 ? v4[k0 + j * kFlushBlock] : zero;
#pragma unroll
      for (int j = 0; j < kFlushHalf; ++j) vx[j] = k0 + j * kFlushBlock < n4 ? h4[k0 + j * kFlushBlock] : zero;
    }
#pragma unroll
    for (int j = 0; j < kFlushHalf; ++j)
      vg[j] = k0 + j * kFlushBlock < n4 ? __builtin_nontemporal_load(g4 + k0 + j * kFlushBlock) : zero;
    float4 dv[kFlushHalf];
#pragma unroll
    for (int j = 0; j < kFlushHalf; ++j) dv[j] = dec4(h * kFlushHalf + j, k0 + j * kFlushBlock < n4);
#pragma unroll
    for (int j = 0; j < kFlushHalf; ++j) {
      const int k = k0 + j * kFlushBlock;
      if (k < n4) {
        f4v b = {__fmul_rn(a.factor, dv[j].x), __fmul_rn(a.factor, dv[j].y), __fmul_rn(a.factor, dv[j].z),
                 __fmul_rn(a.factor, dv[j].w)};
        if (b4) b = f4v{__fadd_rn(vb[j].x, b.x), __fadd_rn(vb[j].y, b.y), __fadd_rn(vb[j].z, b.z), __fadd_rn(vb[j].w, b.w)};
        f4v r;
        if (FADAS) {
          r = fadas4(b, vg[j], vm[j], vv[j], vx[j], a.s);
          m4[k] = vm[j];
          v4[k] = vv[j];
          h4[k] = vx[j];
        } else {
          r = f4v{fedbuff1(b.x, vg[j].x, a.s.k, a.lr), fedbuff1(b.y, vg[j].y, a.s.k, a.lr),
                  fedbuff1(b.z, vg[j].z, a.s.k, a.lr), fedbuff1(b.w, vg[j].w, a.s.k, a.lr)};
        }
        __builtin_nontemporal_store(r, o4 + k);
      }
    }
  }
  const int i = (n4 << 2) + tid;  // the chunk's last < 4 elements
  if (i < c.len) sl.one(i, dec1(i), a);
}

// Host-side argument check shared by the fused entries (nothing is launched when it fails): the flush entries' rule.
inline bool receive_flush_bad_args(const void* d_chunks, int64_t nchunks, int32_t ntensors, int32_t K) {
  return !d_chunks || nchunks < 1 || nchunks > INT32_MAX || ntensors < 1 || K < 1;
}

}  // namespace

#endif  // ADFL_FLUSH_DEVICE_H
