// apply_device.h — the axpby / scale tail shared by the fused decode + apply kernels of slq_codec.hip and
// stoch_codec.hip (the async server's update step: Src/ADFL/Strategy/fed_async.py:80-81, simple.py:100,
// fed_buff.py:72-80). A kernel decodes one chunk's payload into 8 float4 registers per thread, then apply_chunk
// walks the targets: each target's base slice is read, combined and written once. Anonymous namespace: each
// translation unit gets its own copy.
//
// Arithmetic (what torch's CPU kernels compute for fp32, three separately rounded operations):
//   AXPBY  out = fp32(fp32(af * y) + fp32(bf * d))        add_parameters (Src/ADFL/model.py:326-334)
//   SCALE  out = fp32(bf * d)                             tensor.float().mul_(f) (fed_buff.py:72-75); no base,
//                                                         so a -0.0 product keeps its sign
// __fmul_rn / __fadd_rn never contract into an FMA, whatever the translation unit is built with.
#ifndef ADFL_APPLY_DEVICE_H
#define ADFL_APPLY_DEVICE_H

#include <hip/hip_runtime.h>

#include <cstdint>

#include "adfl_slq.h"

namespace {

constexpr int kApplyBlock = 256;
constexpr int kApplyGroups = ADFL_SLQ_CHUNK_ELEMS / 4 / kApplyBlock;  // float4 groups per thread: 8
static_assert(4 * kApplyGroups * kApplyBlock == ADFL_SLQ_CHUNK_ELEMS, "a chunk fits one block's registers");

struct ApplyTargets {
  const float* const* base;  // ntargets * ntensors device pointers, or null (SCALE)
  float* const* out;         // likewise; out[i] == base[i] is the in-place update
  int ntensors, ntargets;
  float af, bf;
};

__device__ __forceinline__ float apply1(const float* y, int i, float d, float af, float bf) {
  const float b = __fmul_rn(bf, d);
  return y ? __fadd_rn(__fmul_rn(af, y[i]), b) : b;
}

__device__ __forceinline__ float4 apply4(float4 y, float4 d, float af, float bf, bool has_base) {
  float4 r = make_float4(__fmul_rn(bf, d.x), __fmul_rn(bf, d.y), __fmul_rn(bf, d.z), __fmul_rn(bf, d.w));
  if (has_base)
    r = make_float4(__fadd_rn(__fmul_rn(af, y.x), r.x), __fadd_rn(__fmul_rn(af, y.y), r.y),
                    __fadd_rn(__fmul_rn(af, y.z), r.z), __fadd_rn(__fmul_rn(af, y.w), r.w));
  return r;
}

// One chunk's targets. dv[j] (valid when `grouped`): the decode of the chunk's float4 group threadIdx.x + j * 256,
// for the groups wholly inside the chunk. dec1(i): the decode of chunk element i, for everything else.
// in_tensor: the chunk's first element's index in its tensor.
//  * grouped and the target's base and output 16-byte aligned (block-uniform per target): 16-byte accesses, all
//    of a target's base loads issued before their first use; the chunk's last < 4 elements one by one;
//  * otherwise element by element through dec1, with the same results.
// In place: plain loads and stores, as k_dequantize_add_batched. Out of place: the output is written with the
// decode's non-temporal stores (nothing re-reads it soon). Base and output are deliberately not __restrict__:
// they may be the same storage.
template <class Dec1>
__device__ __forceinline__ void apply_chunk(const float4 (&dv)[kApplyGroups], bool grouped, const adfl_slq_chunk& c,
                                            int64_t in_tensor, const ApplyTargets& a, Dec1 dec1) {
  typedef float f4v __attribute__((ext_vector_type(4)));
  const int n4 = c.len >> 2;
  for (int m = 0; m < a.ntargets; ++m) {
    const int64_t slot = (int64_t)m * a.ntensors + c.tensor;
    float* o = a.out[slot] + in_tensor;
    const float* y = a.base ? a.base[slot] + in_tensor : nullptr;
    const bool inplace = (y == o);
    const bool vec = grouped && (((reinterpret_cast<uintptr_t>(o) | reinterpret_cast<uintptr_t>(y)) & 15u) == 0);
    if (!vec) {
      for (int i = threadIdx.x; i < c.len; i += kApplyBlock) {
        const float v = apply1(y, i, dec1(i), a.af, a.bf);
        if (inplace) {
          o[i] = v;
        } else {
          __builtin_nontemporal_store(v, o + i);
        }
      }
      continue;
    }
    float4* o4 = reinterpret_cast<float4*>(o);
    const float4* y4 = reinterpret_cast<const float4*>(y);
    float4 yv[kApplyGroups];
#pragma unroll
    for (int j = 0; j < kApplyGroups; ++j) {
      const int k = (int)threadIdx.x + j * kApplyBlock;
      yv[j] = (y && k < n4) ? y4[k] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int j = 0; j < kApplyGroups; ++j) {
      const int k = (int)threadIdx.x + j * kApplyBlock;
      if (k < n4) {
        const float4 r = apply4(yv[j], dv[j], a.af, a.bf, y != nullptr);
        if (inplace) {
          o4[k] = r;
        } else {
          const f4v v = {r.x, r.y, r.z, r.w};
          __builtin_nontemporal_store(v, reinterpret_cast<f4v*>(o4 + k));
        }
      }
    }
    const int i = (n4 << 2) + (int)threadIdx.x;  // the chunk's last < 4 elements
    if (i < c.len) o[i] = apply1(y, i, dec1(i), a.af, a.bf);
  }
}

// The tail of the fused decode-mean + axpby kernels (the synchronous DELTA server step, Strategy/simple.py:87-89):
// one chunk's slice of its tensor's base g and output o (a.base / a.out: one pointer per tensor, ntargets == 1).
// m, the mean of element i of the chunk, becomes fp32(fp32(af * g[i]) + fp32(bf * m)). vec (block-uniform): the
// float4 groups from chunk element `head` on are 16-byte aligned in both g and o.
struct MeanAxpbyOut {
  const float* g;  // the chunk's slice of its tensor's base: element i of the chunk at g[i]
  float* o;        // likewise the output
  float af, bf;
  bool inplace;
  bool vec;        // tiles from chunk element `head` on: 16-byte accesses

  __device__ __forceinline__ MeanAxpbyOut(const ApplyTargets& a, const adfl_slq_chunk& c, int64_t in_tensor, int head)
      : g(a.base[c.tensor] + in_tensor), o(a.out[c.tensor] + in_tensor), af(a.af), bf(a.bf) {
    inplace = (g == o);
    vec = (((reinterpret_cast<uintptr_t>(g + head) | reinterpret_cast<uintptr_t>(o + head)) & 15u) == 0);
  }
  __device__ __forceinline__ void store1(int i, float m) const {
    const float v = apply1(g, i, m, af, bf);
    if (inplace) {
      o[i] = v;
    } else {
      __builtin_nontemporal_store(v, o + i);
    }
  }
  // the float4 of g at chunk element i (vec: 16-byte aligned)
  __device__ __forceinline__ float4 load4g(int i) const {
    if (vec) return *reinterpret_cast<const float4*>(g + i);
    return make_float4(g[i], g[i + 1], g[i + 2], g[i + 3]);
  }
  __device__ __forceinline__ void store4(int i, float4 gv, float4 m) const {
    const float4 r = apply4(gv, m, af, bf, true);
    if (vec) {
      if (inplace) {
        *reinterpret_cast<float4*>(o + i) = r;
      } else {
        typedef float f4v __attribute__((ext_vector_type(4)));
        const f4v v = {r.x, r.y, r.z, r.w};
        __builtin_nontemporal_store(v, reinterpret_cast<f4v*>(o + i));
      }
    } else if (inplace) {
      o[i] = r.x, o[i + 1] = r.y, o[i + 2] = r.z, o[i + 3] = r.w;
    } else {
      __builtin_nontemporal_store(r.x, o + i);
      __builtin_nontemporal_store(r.y, o + i + 1);
      __builtin_nontemporal_store(r.z, o + i + 2);
      __builtin_nontemporal_store(r.w, o + i + 3);
    }
  }
};

// Host-side argument check shared by the three entry points (nothing is launched when it fails).
inline bool apply_bad_args(const void* d_chunks, int64_t nchunks, const void* d_out, int32_t ntensors,
                           int32_t ntargets) {
  return !d_chunks || !d_out || nchunks < 1 || nchunks > INT32_MAX || ntensors < 1 || ntargets < 1;
}

}  // namespace

#endif  // ADFL_APPLY_DEVICE_H
