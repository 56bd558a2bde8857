// server_flush.hip — the buffered asynchronous servers' flush (include/adfl_slq.h): what FedBuff
// (Src/ADFL/Strategy/fed_buff.py:88-92) and FADAS (Strategy/fadas.py:69-73, 96-129) compute from a full buffer,
// one launch for the whole state dict in place of 3 (FedBuff) or 10 (FADAS) element-wise torch statements per
// tensor. FADAS moves 36 B per element (read buf, g, m, v, v_hat; write m, v, v_hat, out), FedBuff 12 B.
//
// k_dequantize_axpby_batched's shape (slq_codec.hip): one 256-thread block per chunk of the chunk table, every
// operand a table of one fp32 pointer per tensor. A chunk whose slice of every table is 16-byte aligned
// (block-uniform) takes 16-byte accesses, its last < 4 elements one by one; any other chunk goes element by
// element through the same per-element function. FADAS's five input streams of a whole chunk would be 160
// registers per lane, so a chunk is walked in two halves: the 20 16-byte loads of a half are issued, then
// combined and stored, before the next half's.
//
// Cache policy, as the apply kernels (apply_device.h): the moments are updated in place with plain loads and
// stores; buf and g are dead after the read and out is not re-read soon, so they are non-temporal.
//
// Arithmetic (the per-element functions, flush_device.h): every operation is spelled with its rounding (__fmul_rn, __fadd_rn, __fdiv_rn, __fmaf_rn), so
// -ffp-contract decides nothing here. The square root is sqrtf: this toolchain's __fsqrt_rn expands to the
// native, 1-ulp v_sqrt_f32 unless OCML_BASIC_ROUNDED_OPERATIONS is defined, while sqrtf (like `/`, which is
// what __fdiv_rn expands to) is correctly rounded and keeps denormals under hipcc's default
// -fhip-fp32-correctly-rounded-divide-sqrt. tests/test_gpu_flush_ops.py holds both to a correctly rounded
// restatement bit for bit.

#include <hip/hip_runtime.h>

#include <cstdint>

#include "adfl_slq.h"
#include "flush_device.h"  // the per-element functions, shared with the fused decode + accumulate + flush kernels

namespace {

constexpr int kBlock = 256;
constexpr int kGroups = ADFL_SLQ_CHUNK_ELEMS / 4 / kBlock;  // float4 groups per thread and chunk: 8
constexpr int kHalf = kGroups / 2;                          // ... in flight at a time in the FADAS kernel
static_assert(4 * kGroups * kBlock == ADFL_SLQ_CHUNK_ELEMS && 2 * kHalf == kGroups, "a chunk is two halves");

__device__ __forceinline__ bool aligned16(const void* a, const void* b, const void* c) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15u) == 0;
}

__global__ __launch_bounds__(kBlock) void k_fedbuff_flush_batched(const float* const* __restrict__ bufs,
                                                                  const float* const* __restrict__ gs,
                                                                  float* const* __restrict__ outs,
                                                                  const adfl_slq_chunk* __restrict__ chunks, float k,
                                                                  float lr) {
  const adfl_slq_chunk c = chunks[blockIdx.x];
  const int64_t in_tensor = (int64_t)((int)blockIdx.x - c.first_chunk) * ADFL_SLQ_CHUNK_ELEMS;
  const float* buf = bufs[c.tensor] + in_tensor;
  const float* g = gs[c.tensor] + in_tensor;
  float* out = outs[c.tensor] + in_tensor;
  const int tid = (int)threadIdx.x;
  if (!aligned16(buf, g, out)) {
    for (int i = tid; i < c.len; i += kBlock)
      __builtin_nontemporal_store(
          fedbuff1(__builtin_nontemporal_load(buf + i), __builtin_nontemporal_load(g + i), k, lr), out + i);
    return;
  }
  const int n4 = c.len >> 2;
  const f4v* b4 = reinterpret_cast<const f4v*>(buf);
  const f4v* g4 = reinterpret_cast<const f4v*>(g);
  f4v* o4 = reinterpret_cast<f4v*>(out);
  const f4v zero = {0.f, 0.f, 0.f, 0.f};
  f4v vb[kGroups], vg[kGroups];
#pragma unroll
  for (int j = 0; j < kGroups; ++j) vb[j] = tid + j * kBlock < n4 ? __builtin_nontemporal_load(b4 + tid + j * kBlock) : zero;
#pragma unroll
  for (int j = 0; j < kGroups; ++j) vg[j] = tid + j * kBlock < n4 ? __builtin_nontemporal_load(g4 + tid + j * kBlock) : zero;
#pragma unroll
  for (int j = 0; j < kGroups; ++j) {
    if (tid + j * kBlock < n4) {
      const f4v r = {fedbuff1(vb[j].x, vg[j].x, k, lr), fedbuff1(vb[j].y, vg[j].y, k, lr),
                     fedbuff1(vb[j].z, vg[j].z, k, lr), fedbuff1(vb[j].w, vg[j].w, k, lr)};
      __builtin_nontemporal_store(r, o4 + tid + j * kBlock);
    }
  }
  const int i = (n4 << 2) + tid;  // the chunk's last < 4 elements
  if (i < c.len) out[i] = fedbuff1(buf[i], g[i], k, lr);
}

__global__ __launch_bounds__(kBlock) void k_fadas_flush_batched(const float* const* __restrict__ bufs,
                                                                const float* const* __restrict__ gs,
                                                                float* const* __restrict__ ms,
                                                                float* const* __restrict__ vs,
                                                                float* const* __restrict__ vhs,
                                                                float* const* __restrict__ outs,
                                                                const adfl_slq_chunk* __restrict__ chunks,
                                                                FadasScalars s) {
  const adfl_slq_chunk c = chunks[blockIdx.x];
  const int64_t in_tensor = (int64_t)((int)blockIdx.x - c.first_chunk) * ADFL_SLQ_CHUNK_ELEMS;
  const float* buf = bufs[c.tensor] + in_tensor;
  const float* g = gs[c.tensor] + in_tensor;
  float* m = ms[c.tensor] + in_tensor;
  float* v = vs[c.tensor] + in_tensor;
  float* vh = vhs[c.tensor] + in_tensor;
  float* out = outs[c.tensor] + in_tensor;
  const int tid = (int)threadIdx.x;
  auto one = [&](int i) {  // element i of the chunk, 4-byte accesses
    float m1 = m[i], v1 = v[i], h1 = vh[i];
    const float r = fadas1(__builtin_nontemporal_load(buf + i), __builtin_nontemporal_load(g + i), m1, v1, h1, s);
    m[i] = m1;
    v[i] = v1;
    vh[i] = h1;
    __builtin_nontemporal_store(r, out + i);
  };
  if (!(aligned16(buf, g, out) && aligned16(m, v, vh))) {
    for (int i = tid; i < c.len; i += kBlock) one(i);
    return;
  }
  const int n4 = c.len >> 2;
  const f4v* b4 = reinterpret_cast<const f4v*>(buf);
  const f4v* g4 = reinterpret_cast<const f4v*>(g);
  f4v* m4 = reinterpret_cast<f4v*>(m);
  f4v* v4 = reinterpret_cast<f4v*>(v);
  f4v* h4 = reinterpret_cast<f4v*>(vh);
  f4v* o4 = reinterpret_cast<f4v*>(out);
#pragma unroll 1
  for (int h = 0; h < 2; ++h) {  // half a chunk of all five streams in flight at a time
    const int k0 = tid + h * kHalf * kBlock;
    if (k0 >= n4) break;  // a thread's groups ascend
    const f4v zero = {0.f, 0.f, 0.f, 0.f};
    f4v vb[kHalf], vg[kHalf], vm[kHalf], vv[kHalf], vx[kHalf];
#pragma unroll
    for (int j = 0; j < kHalf; ++j) vb[j] = k0 + j * kBlock < n4 ? __builtin_nontemporal_load(b4 + k0 + j * kBlock) : zero;
#pragma unroll
    for (int j = 0; j < kHalf; ++j) vm[j] = k0 + j * kBlock < n4 ? m4[k0 + j * kBlock] : zero;
#pragma unroll
    for (int j = 0; j < kHalf; ++j) vv[j] = k0 + j * kBlock < n4 ? v4[k0 + j * kBlock] : zero;
#pragma unroll
    for (int j = 0; j < kHalf; ++j) vx[j] = k0 + j * kBlock < n4 ? h4[k0 + j * kBlock] : zero;
#pragma unroll
    for (int j = 0; j < kHalf; ++j) vg[j] = k0 + j * kBlock < n4 ? __builtin_nontemporal_load(g4 + k0 + j * kBlock) : zero;
#pragma unroll
    for (int j = 0; j < kHalf; ++j) {
      const int k = k0 + j * kBlock;
      if (k < n4) {
        const f4v r = fadas4(vb[j], vg[j], vm[j], vv[j], vx[j], s);
        m4[k] = vm[j];
        v4[k] = vv[j];
        h4[k] = vx[j];
        __builtin_nontemporal_store(r, o4 + k);
      }
    }
  }
  const int i = (n4 << 2) + tid;  // the chunk's last < 4 elements
  if (i < c.len) one(i);
}

inline bool bad_args(const void* d_chunks, int64_t nchunks, int32_t ntensors, int32_t K) {
  return !d_chunks || nchunks < 1 || nchunks > INT32_MAX || ntensors < 1 || K < 1;
}

inline int launch_status() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? ADFL_OK : (int)e;
}

}  // namespace

extern "C" {

int adfl_fedbuff_flush_batched(const float* const* d_buf, const float* const* d_g, float* const* d_out,
                               const adfl_slq_chunk* d_chunks, int64_t nchunks, int32_t ntensors, int32_t K, float lr,
                               void* stream) {
  if (!d_buf || !d_g || !d_out || bad_args(d_chunks, nchunks, ntensors, K)) return ADFL_E_ARG;
  hipLaunchKernelGGL(k_fedbuff_flush_batched, dim3((unsigned)nchunks), dim3(kBlock), 0, (hipStream_t)stream, d_buf,
                     d_g, d_out, d_chunks, (float)K, lr);
  return launch_status();
}

int adfl_fadas_flush_batched(const float* const* d_buf, const float* const* d_g, float* const* d_m,
                             float* const* d_v, float* const* d_v_hat, float* const* d_out,
                             const adfl_slq_chunk* d_chunks, int64_t nchunks, int32_t ntensors, int32_t K, float beta1,
                             float one_minus_beta1, float beta2, float one_minus_beta2, float sqrt_bc2, float eps,
                             float step, void* stream) {
  if (!d_buf || !d_g || !d_m || !d_v || !d_v_hat || !d_out || bad_args(d_chunks, nchunks, ntensors, K))
    return ADFL_E_ARG;
  const FadasScalars s{(float)K, beta1, one_minus_beta1, beta2, one_minus_beta2, sqrt_bc2, eps, step};
  hipLaunchKernelGGL(k_fadas_flush_batched, dim3((unsigned)nchunks), dim3(kBlock), 0, (hipStream_t)stream, d_buf, d_g,
                     d_m, d_v, d_v_hat, d_out, d_chunks, s);
  return launch_status();
}

}  // extern "C"
