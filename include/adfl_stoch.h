/*
 * adfl_stoch.h — C ABI of the MI355X (gfx950) stochastic gradient codecs in libadfl_slq.so:
 * QSGD / RQSGD / CNAT (Src/ADFL/Channel/quant.py:140-570).
 *
 * Same conventions as adfl_slq.h (device pointers d_*, 16-byte aligned bases, int64 counts, void*
 * hipStream_t, asynchronous, no allocation, graph-capturable, 0 / hipError_t / ADFL_E_* returns) and the
 * same bucket description: an adfl_slq_chunk table from adfl_slq_build_chunks() over a flat buffer in
 * which tensor t owns elements [offset_t, offset_t + size_t). A single tensor is a one-entry table.
 *
 * Payload planes (what the reference's QuantParameter holds, quant.py:209-217,349-358,495-503):
 *   levels  uint8, one per element — QSGD/RQSGD quantization level l in [0, 2^bits - 1], or CNAT's
 *           int8 exponent in [-2^(bits-1), 2^(bits-1) - 1] (stored as its byte)
 *   signs   int8, one per element — torch.sign(x) in {-1, 0, 1} (NaN -> 0)
 *   norms   fp32, one per tensor — QSGD/CNAT: ||x||_2; RQSGD: max|x| (+ mins = min|x|)
 * Both planes are indexed like x (byte g of a plane belongs to element g of the bucket).
 *
 * Uniforms. Stochastic rounding compares u in [0, 1) with a per-element probability. d_uniforms == NULL
 * draws u from the counter-based Philox4x32-7 stream keyed by `seed`: element g of the bucket uses word
 * g % 4 of block (counter + g / 4), u = (word >> 8) * 2^-24. A caller that advances `counter` by
 * ceil(total / 4) per call never reuses a uniform. d_uniforms != NULL injects one fp32 uniform per
 * element (indexed like x) — with the reference's own uniforms the outputs are bit-identical to it.
 *
 * Norm: fp32 squares accumulated in fp64 per chunk and per tensor (fixed order: deterministic), rounded
 * once to fp32, correctly rounded sqrt. torch's fp32 vector_norm differs from it only by torch's own
 * accumulation error; every other output bit follows the reference exactly. For bit parity
 * with the reference's norm, compute it with ADFL_NORM_L2_TORCH and quantize with the given-norm entry.
 */
#ifndef ADFL_STOCH_H
#define ADFL_STOCH_H

#include <stdint.h>

#include "adfl_slq.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { ADFL_NORM_L2 = 0, ADFL_NORM_LINF = 1, ADFL_NORM_L2_TORCH = 2 };
enum { ADFL_CODEC_QSGD = 0, ADFL_CODEC_RQSGD = 1, ADFL_CODEC_CNAT = 2 };
enum { ADFL_DTYPE_F32 = 0, ADFL_DTYPE_F16 = 1, ADFL_DTYPE_BF16 = 2, ADFL_DTYPE_F64 = 3 };

/* Device workspace bytes the encode / norm calls need for a table of nchunks chunks (16 B per chunk). */
int64_t adfl_stoch_workspace_bytes(int64_t nchunks);

/* Per-tensor norms of a bucket (two launches: chunk partials, per-tensor finalize).
 *   ADFL_NORM_L2:   d_norms[t] = ||x_t||_2   (torch.linalg.vector_norm(x, ord=2), quant.py:226,512)
 *   ADFL_NORM_LINF: d_norms[t] = max|x_t|, d_mins[t] = min|x_t| (ord=inf / -inf, quant.py:367,380);
 *                   NaN anywhere in x_t makes both NaN. d_mins may be NULL for ADFL_NORM_L2.
 *   ADFL_NORM_L2_TORCH: ||x_t||_2 bit-identical to torch 2.10's CPU vector_norm (its fp32 reduction order:
 *                   8 FMA lane accumulators, lane sum, then the n % 8 tail: 4 rounded squares, then FMA),
 *                   i.e. the reference's own norm. One launch, no workspace (d_workspace may be NULL), but
 *                   sequential per tensor: about one element per cycle per tensor. */
int adfl_stoch_norms_batched(const float* d_x, const adfl_slq_chunk* d_chunks, int64_t nchunks, int mode,
                             void* d_workspace, int64_t workspace_bytes, float* d_norms, float* d_mins,
                             void* stream);

enum { ADFL_TORCH_NORM_SHORT = 1, ADFL_TORCH_NORM_LONG = 2 };

/* torch 2.10's CPU vector_norm(x, ord=2) — the reference's QSGD / CNAT norm (quant.py:226,512) — bit for bit
 * for fp32, bf16, fp16 and fp64 buckets (dtype ADFL_DTYPE_*: d_x holds elements of that type, indexed by the
 * chunk table), in phases with no cross-block waits (csrc/torch_norm.hip): per-tile fp64 sums, a per-chain
 * prefix that predicts each tile's binade, per-tile exact integer maps under the predicted binades, and one
 * block per tensor composing them, running the reference's fma only where an accumulator leaves its binade.
 * Orders restated: oracle/slq_oracle.c
 * oracle_torch_l2_norm{,_bf16,_f16,_f64}.
 *   threads: torch.get_num_threads() of the process whose norm is reproduced (fp16 tensors of >= 32768
 *            elements are summed in min(threads, ceil(n / 32768)) contiguous pieces: 1..512 for fp16 buckets;
 *            any value >= 1 for the other dtypes, which do not use it).
 *   kinds:   which tensors the bucket holds, so launches with nothing to do are skipped:
 *            ADFL_TORCH_NORM_SHORT (some of at most adfl_torch_norm_short_max_dt(dtype) elements: fp32, bf16
 *            and fp16 ones in one launch, one block per tensor) | ADFL_TORCH_NORM_LONG (some longer: the phased
 *            path); 0 = both. Any other bit set: ADFL_E_ARG, nothing launched. It is a hint that cannot drop a
 *            tensor: one it does not name (a longer one under ADFL_TORCH_NORM_SHORT alone, a short one under
 *            ADFL_TORCH_NORM_LONG alone, whatever the dtype) gets a quiet NaN in d_norms64 / d_norms32 — the
 *            launches that would compute it were not made — and every named tensor its norm. A correct hint
 *            costs no launch more than before (the kernel that skips a tensor for its size writes the NaN).
 *            Size it by adfl_torch_norm_short_max_dt(dtype), not by adfl_torch_norm_short_max().
 *   outputs: d_norms64[t] = the norm as a double (the dtype's value: exact for every dtype) and / or
 *            d_norms32[t] = (float) of it; either may be NULL, not both.
 * d_scratch: adfl_torch_norm_scratch_bytes(nchunks, ntensors) bytes, 256-byte aligned, no initialisation.
 * Up to nine launches, stream-ordered with no host waits (one for layouts of short fp32 / bf16 / fp16 tensors
 * only). */
int64_t adfl_torch_norm_scratch_bytes(int64_t nchunks, int64_t ntensors);
int64_t adfl_torch_norm_short_max(void);          /* the fp16 / fp64 bound only: 65,536. NOT the fp32 / bf16 one
                                                     (2^19): use adfl_torch_norm_short_max_dt for `kinds` */
int64_t adfl_torch_norm_short_max_dt(int32_t dtype); /* the short-tensor bound of a dtype (fp32, bf16: 2^19; fp16,
                                                        fp64: 2^16), or ADFL_E_ARG */
int adfl_torch_norms(int32_t dtype, const void* d_x, const adfl_slq_chunk* d_chunks, int64_t nchunks,
                     int64_t ntensors, int32_t kinds, int32_t threads, void* d_scratch, int64_t scratch_bytes,
                     double* d_norms64, float* d_norms32, void* stream);
/* The same with the caller's list of every tensor's first chunk (d_tfirst[t], ntensors int32 on the device; the
 * host has it from building the chunk table), which saves the launch that builds it; NULL: adfl_torch_norms. */
int adfl_torch_norms_work(int32_t dtype, const void* d_x, const adfl_slq_chunk* d_chunks, int64_t nchunks,
                          const int32_t* d_tfirst, int64_t ntensors, int32_t kinds, int32_t threads, void* d_scratch,
                          int64_t scratch_bytes, double* d_norms64, float* d_norms32, void* stream);

/* QSGD / RQSGD level quantization given per-tensor norms (quant.py:230-238 and :371-379), levels =
 * 2^bits - 1: scaled = fl(fl(levels*|x|) / norm); l = floor(scaled); q = u8(l + (u < scaled - l));
 * norm == 0 gives levels 0 and signs 1 (quant.py:227-228). One launch. */
int adfl_qsgd_quantize_batched(const float* d_x, const adfl_slq_chunk* d_chunks, int64_t nchunks, int bits,
                               const float* d_norms, const float* d_uniforms, uint64_t seed, uint64_t counter,
                               uint8_t* d_levels, int8_t* d_signs, void* stream);

/* QSGDChannel._quantize_tensor over a bucket (quant.py:223-240): L2 norms + quantize (three launches). */
int adfl_qsgd_encode_batched(const float* d_x, const adfl_slq_chunk* d_chunks, int64_t nchunks, int bits,
                             const float* d_uniforms, uint64_t seed, uint64_t counter, void* d_workspace,
                             int64_t workspace_bytes, uint8_t* d_levels, int8_t* d_signs, float* d_norms,
                             void* stream);

/* RQSGDChannel._quantize_tensor (quant.py:364-382): max|x| norms, min|x| factors + quantize. */
int adfl_rqsgd_encode_batched(const float* d_x, const adfl_slq_chunk* d_chunks, int64_t nchunks, int bits,
                              const float* d_uniforms, uint64_t seed, uint64_t counter, void* d_workspace,
                              int64_t workspace_bytes, uint8_t* d_levels, int8_t* d_signs, float* d_norms,
                              float* d_mins, void* stream);

/* QSGDChannel._dequantize_tensor (quant.py:243-252): out = fl(fl(norm*l) / levels) * sign; 0 if norm == 0. */
int adfl_qsgd_dequantize_batched(const uint8_t* d_levels, const int8_t* d_signs, const adfl_slq_chunk* d_chunks,
                                 int64_t nchunks, int bits, const float* d_norms, float* d_out, void* stream);

/* RQSGDChannel._dequantize_tensor (quant.py:385-398): out = fl(fl(norm*sign)*l) / levels, and
 * min*sign where l == 0; 0 if norm == 0. */
int adfl_rqsgd_dequantize_batched(const uint8_t* d_levels, const int8_t* d_signs, const adfl_slq_chunk* d_chunks,
                                  int64_t nchunks, int bits, const float* d_norms, const float* d_mins,
                                  float* d_out, void* stream);

/* CNATChannel._quantize_tensor (quant.py:509-534) in one pass over x (exponents, signs and the L2 norm
 * partials together), then a per-tensor finalize and the norm == 0 rewrite (levels 0, signs 1,
 * quant.py:513-514): three launches, x read once. d_exps holds each exponent's int8 byte. */
int adfl_cnat_encode_batched(const float* d_x, const adfl_slq_chunk* d_chunks, int64_t nchunks, int bits,
                             const float* d_uniforms, uint64_t seed, uint64_t counter, void* d_workspace,
                             int64_t workspace_bytes, int8_t* d_exps, int8_t* d_signs, float* d_norms,
                             void* stream);

/* CNATChannel._dequantize_tensor (quant.py:537-545): out = fl(fl(norm*sign) * 2^e); 0 if norm == 0. */
int adfl_cnat_dequantize_batched(const int8_t* d_exps, const int8_t* d_signs, const adfl_slq_chunk* d_chunks,
                                 int64_t nchunks, const float* d_norms, float* d_out, void* stream);

/* simple_aggregate (Src/ADFL/model.py:221-234) of K clients' decodes, one launch: out[i] =
 * fp32(((0 + d_0[i]) + ... + d_{K-1}[i]) / K), d_r the codec's decode (above) of row r's level / exponent
 * and sign bytes (d_levels / d_signs + r * row_stride_bytes, each a bucket payload over d_chunks) under row
 * r's norms d_norms + r * norm_stride (RQSGD: d_mins likewise; +0 where a norm is 0). codec: ADFL_CODEC_*
 * (bits unused for CNAT). Bases 16-byte aligned, row_stride_bytes a multiple of 16. The sum follows torch's
 * CPU order for sum(stack(rows), dim=0) (csrc/torch_sum_order.h: per tensor, by the element's index in it), so
 * the result is bit-identical to simple_aggregate on CPU tensors for every K up to 2^19. */
int adfl_stoch_dequantize_mean_batched(int32_t codec, const uint8_t* d_levels, const int8_t* d_signs,
                                       int64_t row_stride_bytes, int32_t k, const adfl_slq_chunk* d_chunks,
                                       int64_t nchunks, int bits, const float* d_norms, const float* d_mins,
                                       int64_t norm_stride, float* d_out, void* stream);

/* Fused decode-mean + axpby for the three stochastic codecs: adfl_slq_dequantize_mean_axpby_batched (adfl_slq.h)
 * with m the value adfl_stoch_dequantize_mean_batched writes for the same rows -- the synchronous DELTA server
 * step (Src/ADFL/Strategy/simple.py:87-89): out[t][i] = fp32(fp32(alpha * base[t][i]) + fp32(beta * m)). d_base /
 * d_out: device arrays of ntensors pointers, d_out[t] == d_base[t] in place. ADFL_E_ARG and nothing launched for
 * an unknown codec, a null pointer or table, nchunks outside [1, INT32_MAX], ntensors < 1, k < 1 or above 2^19, or
 * a row_stride_bytes that is not a multiple of 16; ADFL_E_BITS for bits outside [1, 16] (QSGD / RQSGD). */
int adfl_stoch_dequantize_mean_axpby_batched(int32_t codec, const uint8_t* d_levels, const int8_t* d_signs,
                                             int64_t row_stride_bytes, int32_t k, const adfl_slq_chunk* d_chunks,
                                             int64_t nchunks, int bits, const float* d_norms, const float* d_mins,
                                             int64_t norm_stride, const float* const* d_base, float* const* d_out,
                                             int32_t ntensors, float alpha, float beta, void* stream);

/* Fused decode + axpby for the three stochastic codecs: adfl_slq_dequantize_axpby_batched (adfl_slq.h) with d the
 * codec's decode (quant.py:243-252 / :385-398 / :537-545; +0 for a tensor whose norm is 0) — FedAsync's
 * add_parameters(g, decoded, 1 - a_t, a_t) (Src/ADFL/Strategy/fed_async.py:80-81), Simple DELTA's (1, 1)
 * (Strategy/simple.py:100) and FedBuff's mul_(f) then add_parameters_inpace(buffer, decoded, 1, 1)
 * (Strategy/fed_buff.py:72-80):
 *   d_base != NULL  out_k[t][i] = fp32(fp32(alpha * base_k[t][i]) + fp32(beta * d))
 *   d_base == NULL  out_k[t][i] = fp32(beta * d)
 * codec: ADFL_CODEC_* (bits unused for CNAT; d_mins for RQSGD only). d_levels / d_signs 16-byte aligned; d_base /
 * d_out device arrays of ntargets * ntensors pointers, d_out[i] == d_base[i] in place. ADFL_E_ARG and nothing
 * launched for an unknown codec, a null pointer, nchunks outside [1, INT32_MAX], bits outside [1, 16],
 * ntensors < 1 or ntargets < 1. */
int adfl_stoch_dequantize_axpby_batched(int32_t codec, const uint8_t* d_levels, const int8_t* d_signs,
                                        const adfl_slq_chunk* d_chunks, int64_t nchunks, int bits,
                                        const float* d_norms, const float* d_mins, const float* const* d_base,
                                        float* const* d_out, int32_t ntensors, int32_t ntargets, float alpha,
                                        float beta, void* stream);

/* Fused decode + accumulate + flush for the three stochastic codecs: adfl_slq_dequantize_fedbuff_flush_batched /
 * adfl_slq_dequantize_fadas_flush_batched (adfl_slq.h) with d the codec's decode (quant.py:243-252 / :385-398 /
 * :537-545; +0 for a tensor whose norm is 0) — the buffered servers' K-th client update, FedBuff's
 * (Src/ADFL/Strategy/fed_buff.py:68-100) and FADAS's (Src/ADFL/Strategy/fadas.py:56-80), in one launch,
 * bit-identical to adfl_stoch_dequantize_axpby_batched on the buffer followed by the flush entry. d_buf == NULL:
 * no buffer. codec: ADFL_CODEC_*; s = (float)(2^bits - 1), the level count the decode divides by (QSGD / RQSGD;
 * unused for CNAT); d_mins for RQSGD only; d_levels / d_signs 16-byte aligned (else ADFL_E_ALIGN). ADFL_E_ARG and
 * nothing launched for an unknown codec, a null pointer or table other than d_buf, nchunks outside
 * [1, INT32_MAX], ntensors < 1 or K < 1. */
int adfl_stoch_dequantize_fedbuff_flush_batched(int32_t codec, const uint8_t* d_levels, const int8_t* d_signs,
                                                const adfl_slq_chunk* d_chunks, int64_t nchunks, const float* d_norms,
                                                const float* d_mins, float s, const float* const* d_buf,
                                                const float* const* d_g, float* const* d_out, int32_t ntensors,
                                                int32_t K, float factor, float lr, void* stream);
int adfl_stoch_dequantize_fadas_flush_batched(int32_t codec, const uint8_t* d_levels, const int8_t* d_signs,
                                              const adfl_slq_chunk* d_chunks, int64_t nchunks, const float* d_norms,
                                              const float* d_mins, float s, const float* const* d_buf,
                                              const float* const* d_g, float* const* d_m, float* const* d_v,
                                              float* const* d_v_hat, float* const* d_out, int32_t ntensors, int32_t K,
                                              float beta1, float one_minus_beta1, float beta2, float one_minus_beta2,
                                              float sqrt_bc2, float eps, float step, void* stream);

/* One-launch encodes (same outputs, bit for bit) for a bucket whose tensors ALL have at most
 * ADFL_SLQ_RESIDENT_CHUNKS chunks: d_work / nwork is the work list of adfl_slq_build_encode_work (the first
 * chunk of every tensor; nwork == 0 when some tensor is larger). A 1024-thread block holds one whole tensor
 * in registers, reduces its norm and quantizes it: x read once, no workspace, no fix-up launch. With
 * nwork == 0 these run the multi-launch encodes above (which need the workspace). A work list entry naming a
 * tensor with more than ADFL_SLQ_RESIDENT_CHUNKS chunks gets a NaN norm and no payload. */
int adfl_qsgd_encode_batched_work(const float* d_x, const adfl_slq_chunk* d_chunks, int64_t nchunks,
                                  const int32_t* d_work, int64_t nwork, int bits, const float* d_uniforms,
                                  uint64_t seed, uint64_t counter, void* d_workspace, int64_t workspace_bytes,
                                  uint8_t* d_levels, int8_t* d_signs, float* d_norms, void* stream);
int adfl_rqsgd_encode_batched_work(const float* d_x, const adfl_slq_chunk* d_chunks, int64_t nchunks,
                                   const int32_t* d_work, int64_t nwork, int bits, const float* d_uniforms,
                                   uint64_t seed, uint64_t counter, void* d_workspace, int64_t workspace_bytes,
                                   uint8_t* d_levels, int8_t* d_signs, float* d_norms, float* d_mins, void* stream);
int adfl_cnat_encode_batched_work(const float* d_x, const adfl_slq_chunk* d_chunks, int64_t nchunks,
                                  const int32_t* d_work, int64_t nwork, int bits, const float* d_uniforms,
                                  uint64_t seed, uint64_t counter, void* d_workspace, int64_t workspace_bytes,
                                  int8_t* d_exps, int8_t* d_signs, float* d_norms, void* stream);

/* ---- DELTA rounds: the encode of new - prev (diff_parameters, Src/ADFL/model.py:350-358, then the codec) ----
 * Sources as adfl_slq_encode_delta_batched addresses them: d_new / d_prev are device arrays of one fp32 pointer
 * per tensor, read through the chunk table as ptrs[c.tensor] + (c.start - t0), t0 the tensor's offset in the
 * chunk table (where its planes start). No precondition on the source addresses (no ADFL_E_ALIGN for them):
 * a block whose two source addresses are 16-byte aligned where its planes reach a 4-byte boundary works in
 * 4-element groups, any other element by element with the same results. The plane bases are 16-byte aligned.
 *
 * RQSGD (max|x| and min|x| are order-free, so the difference is never written): two passes over both sources
 * and a per-tensor finalize, three launches, 18 bytes per element (any layout), or one launch (below).
 *   d_ushift: per tensor (int64, device), or NULL meaning 0. The element at chunk-table index g of tensor t uses
 *             uniform index g + d_ushift[t]: Philox word (g + ushift) % 4 of block counter + (g + ushift) / 4, or
 *             d_uniforms[g + ushift] when uniforms are injected. It decouples the draw from the plane address: a
 *             caller that keeps the planes in a 64-element-aligned layout passes compact_offset[t] -
 *             aligned_offset[t] and gets the compact layout's payload. g + ushift must be >= 0 for every
 *             tensor's first element; the library cannot see device memory, so the caller checks it
 *             (adfl_amd.stoch raises ValueError). Tensors with ushift % 4 == 0 draw one Philox block per four
 *             elements; the others draw from two (a lane takes the second from the next lane).
 *   Contract: d_levels, d_signs, d_norms and d_mins equal adfl_rqsgd_encode_batched_work's over a bucket that
 *             holds fl(new - prev) with tensor t at offset t0 + ushift[t], with the same bits / seed / counter /
 *             uniforms, bit for bit — the norm == 0 fill (levels 0, signs 1) and the NaN norm / min included.
 *   Errors, nothing launched: ADFL_E_ARG (a null table, plane, norms, mins or workspace; nchunks outside
 *             [1, INT32_MAX]; a null work list or nwork outside [0, nchunks]), ADFL_E_BITS, ADFL_E_WORKSPACE
 *             (fewer than adfl_stoch_workspace_bytes(nchunks) bytes), ADFL_E_ALIGN (workspace, plane or uniform base).
 * The _work entry is the one-launch form for a bucket whose tensors ALL have at most
 * ADFL_SLQ_DELTA_RESIDENT_CHUNKS chunks, over the work list of adfl_slq_build_encode_work (nwork == 0: the
 * two-pass entry): a 1024-thread block holds one whole tensor's difference in registers between its max / min
 * reduction and the quantize, so both sources are read once (10 bytes per element) and the workspace is not
 * used (it is still checked). Same outputs bit for bit. A work list entry naming a larger tensor gets a NaN norm
 * and min and no payload. */
int adfl_rqsgd_encode_delta_batched(const float* const* d_new, const float* const* d_prev,
                                    const adfl_slq_chunk* d_chunks, int64_t nchunks, int bits,
                                    const float* d_uniforms, const int64_t* d_ushift, uint64_t seed, uint64_t counter,
                                    void* d_workspace, int64_t workspace_bytes, uint8_t* d_levels, int8_t* d_signs,
                                    float* d_norms, float* d_mins, void* stream);
int adfl_rqsgd_encode_delta_batched_work(const float* const* d_new, const float* const* d_prev,
                                         const adfl_slq_chunk* d_chunks, int64_t nchunks, const int32_t* d_work,
                                         int64_t nwork, int bits, const float* d_uniforms, const int64_t* d_ushift,
                                         uint64_t seed, uint64_t counter, void* d_workspace, int64_t workspace_bytes,
                                         uint8_t* d_levels, int8_t* d_signs, float* d_norms, float* d_mins,
                                         void* stream);

/* QSGD / CNAT scale by the torch-order L2 norm, which reads one flat bucket: their DELTA route writes the
 * difference once and runs the entries above over it. d_out[c.start + i] = new_t[i] - prev_t[i] for every
 * chunk (one launch, 8 bytes read and 4 written per element; bytes outside every chunk untouched), equal to
 * torch's `new - prev` bit for bit (NaN by position, not payload). Any alignment: 16-byte words when the slot
 * and both sources share their phase mod 16, 4-byte words otherwise. ADFL_E_ARG for a null pointer or nchunks
 * outside [1, INT32_MAX]. */
int adfl_bucket_diff(float* d_out, const adfl_slq_chunk* d_chunks, int64_t nchunks, const float* const* d_new,
                     const float* const* d_prev, void* stream);

/* ---- QAFeL's broadcast (Src/ADFL/Server/qafel.py:156-180): the delta encode of g - h that also leaves
 * h' = fp32(h + d) in the hidden tensors, d being the codec's decode of the bytes the call stored (the level byte
 * after its uint8 wraparound, the sign byte, the tensor's fp32 norm, RQSGD's min factor; the decode kernels' own
 * arithmetic). A tensor whose norm is 0 decodes to +0, which is still added (a hidden -0 becomes +0); a NaN norm
 * makes the whole hidden tensor NaN. Bit-identical to the encode followed by the codec's decode and an fp32 add.
 * d_hidden: one fp32 pointer per tensor, addressed as the delta sources are; the tensors are written in place, must
 * not overlap d_new's, the planes or each other, and have no alignment precondition (16-byte accesses where the
 * address allows, 4-byte ones otherwise, the same bits). Additions: ADFL_SLQ_ABI_VERSION is unchanged.
 *
 * RQSGD: adfl_rqsgd_encode_delta_batched[_work] with d_hidden in d_prev's place — the same arguments, outputs
 * (bit for bit) and errors; 22 bytes per element for the two passes, 18 for the one launch. */
int adfl_rqsgd_encode_delta_update_batched(const float* const* d_new, float* const* d_hidden,
                                           const adfl_slq_chunk* d_chunks, int64_t nchunks, int bits,
                                           const float* d_uniforms, const int64_t* d_ushift, uint64_t seed,
                                           uint64_t counter, void* d_workspace, int64_t workspace_bytes,
                                           uint8_t* d_levels, int8_t* d_signs, float* d_norms, float* d_mins,
                                           void* stream);
int adfl_rqsgd_encode_delta_update_batched_work(const float* const* d_new, float* const* d_hidden,
                                                const adfl_slq_chunk* d_chunks, int64_t nchunks, const int32_t* d_work,
                                                int64_t nwork, int bits, const float* d_uniforms,
                                                const int64_t* d_ushift, uint64_t seed, uint64_t counter,
                                                void* d_workspace, int64_t workspace_bytes, uint8_t* d_levels,
                                                int8_t* d_signs, float* d_norms, float* d_mins, void* stream);

/* QSGD from given norms (the reference-order norm of the difference bucket d_x = g - h, adfl_bucket_diff's
 * output): adfl_qsgd_quantize_batched's planes, plus the update of d_hidden (ntensors pointers); 14 bytes per
 * element. Errors as adfl_qsgd_quantize_batched, and ADFL_E_ARG for a null d_hidden or ntensors < 1. */
int adfl_qsgd_quantize_update_batched(const float* d_x, const adfl_slq_chunk* d_chunks, int64_t nchunks, int bits,
                                      const float* d_norms, const float* d_uniforms, uint64_t seed, uint64_t counter,
                                      uint8_t* d_levels, int8_t* d_signs, float* const* d_hidden, int64_t ntensors,
                                      void* stream);

/* The Philox uniforms the codecs draw: d_out[i] = u(start + i) of stream (seed, counter), i < n.
 * (Exposed for tests and for callers that want the uniforms a call used.) */
int adfl_philox_uniforms(float* d_out, int64_t n, int64_t start, uint64_t seed, uint64_t counter, void* stream);

/* The Philox4x32 round count this library was built with: 7 (the product) or 10 (an ADFL_PHILOX_ROUNDS=10
 * build; csrc/philox.h records why 7). */
int adfl_philox_rounds(void);

/* ---- fp16 / bf16 / fp64 tensors -------------------------------------------------------------------
 * The reference computes QSGD / RQSGD / CNAT in the tensor's own dtype (quant.py:223-240, :364-382,
 * :509-534): each op on fp16 / bf16 computes in fp32 and rounds to the dtype; fp64 ops are fp64. These
 * entries do the same on a bucket of one dtype (d_x: uint16 bit patterns for fp16 / bf16, doubles for fp64;
 * 16-byte aligned bases, the level / sign planes too). Uniforms are on torch.rand's grid for the dtype:
 * d_uniforms (NULL or a plane of the dtype indexed like x) or the Philox4x32-7 stream — fp16 / bf16:
 * element g takes word g % 4 of block
 * (counter + g / 4), u = (word >> 21) * 2^-11 (fp16) or (word >> 24) * 2^-8 (bf16); fp64: element g takes
 * words 2 (g % 2), 2 (g % 2) + 1 of block (counter + g / 2) as the high / low halves of 64 bits,
 * u = (bits >> 11) * 2^-53 (advance counter by ceil(total / 4), fp64 ceil(total / 2), per call).
 * Norms are fp64 values of the dtype's norm: fp16 / bf16 L2 = R(sqrt(fp32(sum of fp32 squares in fp64)));
 * fp64 L2 = sqrt(fp64 sum); LINF = max|x| / min|x|. CNAT's floor / ceil(log2) is the exact band rule of
 * cnat_log2_dt_table.h. Decode with the fp32 dequantize entries and fp32(norm) (the reference decodes to
 * fp32 with the Python-float norm as an fp32 scalar). Workspace: adfl_stoch_workspace_bytes(nchunks). */
int adfl_stoch_norms_batched_dt(int32_t dtype, const void* d_x, const adfl_slq_chunk* d_chunks, int64_t nchunks,
                                int mode, void* d_workspace, int64_t workspace_bytes, double* d_norms, double* d_mins,
                                void* stream);
/* Levels (QSGD / RQSGD: codec's norm in d_norms) or CNAT exponents + signs; norm == 0 gives 0 / 1. */
int adfl_stoch_quantize_batched_dt(int32_t codec, int32_t dtype, const void* d_x, const adfl_slq_chunk* d_chunks,
                                   int64_t nchunks, int bits, const double* d_norms, const void* d_uniforms,
                                   uint64_t seed, uint64_t counter, uint8_t* d_levels, int8_t* d_signs, void* stream);
/* norms (L2; RQSGD: LINF with d_mins) + quantize. CNAT reads x once (its exponents do not depend on the norm:
 * exponents, signs and chunk partials in one pass, then the norms and the norm == 0 fill). */
int adfl_stoch_encode_batched_dt(int32_t codec, int32_t dtype, const void* d_x, const adfl_slq_chunk* d_chunks,
                                 int64_t nchunks, int bits, const void* d_uniforms, uint64_t seed, uint64_t counter,
                                 void* d_workspace, int64_t workspace_bytes, uint8_t* d_levels, int8_t* d_signs,
                                 double* d_norms, double* d_mins, void* stream);
/* The uniforms elements start .. start+n-1 draw from stream (seed, counter) in the dtype (tests). */
int adfl_philox_uniforms_dt(int32_t dtype, void* d_out, int64_t n, int64_t start, uint64_t seed, uint64_t counter,
                            void* stream);

/* ---- packed planes: bits + 1 bits per weight (csrc/stoch_packed.hip) -------------------------------------
 * The wire format QSGDChannel / RQSGDChannel.simulate_bandwidth prices (quant.py:173-184, :313-324), for fp32
 * buckets, ADFL_CODEC_QSGD / ADFL_CODEC_RQSGD and bits in [1, 8]. With n a tensor's element count and i an
 * element's index in it:
 *   sign plane   ceil(n / 8) bytes: bit i & 7 (least significant first) of byte i >> 3 is 1 exactly when the
 *                unpacked sign byte is -1 (x < 0); 0 for x > 0, +-0, NaN and every element of a zero-norm tensor;
 *                unused bits of the last byte are 0.
 *   level plane  bits > 4: n bytes, the unpacked level byte. bits <= 4: ceil(n / 2) bytes, byte j =
 *                (level[2j] << 4) | level[2j + 1] (pack_4bit's nibble order), the low nibble 0 when n is odd. A
 *                level is at most 2^bits - 1 against the tensor's own norm; only its low 4 bits are kept.
 * Bucket: the chunk table's tensor offsets MUST be multiples of ADFL_SLQ_ALIGN_ELEMS (64). A tensor at element
 * offset o has its sign bytes at o / 8 and its level bytes at o (bits > 4) or o / 2 (bits <= 4); no byte is shared
 * between tensors, and the bytes between tensors are unspecified. A chunk that breaks the rule is skipped: its
 * bytes are neither read nor written (the library cannot see the table; adfl_amd.stoch raises instead).
 * Decode widens a sign bit to the +1 / -1 byte and a nibble to the level byte and then computes what the unpacked
 * entries compute: every value equals theirs on the unpacked planes bit for bit (the unpacked sign byte 0 only
 * ever multiplies a +0 or a NaN). ADFL_SLQ_ABI_VERSION is unchanged: these are additions.
 *
 * Errors, nothing launched: ADFL_E_ARG for ADFL_CODEC_CNAT or an unknown codec (CNAT's zero elements decode to 0
 * only through the sign byte 0, a third sign state this format does not have), a null pointer other than
 * d_uniforms / d_ushift / QSGD's d_mins / d_base, nchunks outside [1, INT32_MAX], ntensors or ntargets < 1;
 * ADFL_E_BITS for bits outside [1, 8]; ADFL_E_ALIGN for a d_x, d_uniforms, plane or d_out base that is not 16-byte
 * aligned.
 *
 * Quantize given norms (QSGD: the L2 norm; RQSGD: max|x|): adfl_qsgd_quantize_batched's level values and sign
 * tests, one launch. d_uniforms / seed / counter as there; d_ushift as adfl_rqsgd_encode_delta_batched's (per
 * tensor, or NULL meaning 0: the element at chunk-table index g of tensor t uses uniform index g + d_ushift[t],
 * which must not be negative), so planes in the aligned bucket carry the compact bucket's draws. Tensors with
 * ushift % 4 != 0 draw from two Philox blocks per four elements (with injected uniforms they go element by
 * element), with the same results. norm == 0: all-zero level and sign bytes. */
int adfl_stoch_quantize_packed_batched(int32_t codec, const float* d_x, const adfl_slq_chunk* d_chunks,
                                       int64_t nchunks, int bits, const float* d_norms, const float* d_uniforms,
                                       const int64_t* d_ushift, uint64_t seed, uint64_t counter, uint8_t* d_levels,
                                       uint8_t* d_signbits, void* stream);
/* adfl_qsgd_dequantize_batched / adfl_rqsgd_dequantize_batched from packed planes (d_mins: RQSGD only). */
int adfl_stoch_dequantize_packed_batched(int32_t codec, const uint8_t* d_levels, const uint8_t* d_signbits,
                                         const adfl_slq_chunk* d_chunks, int64_t nchunks, int bits,
                                         const float* d_norms, const float* d_mins, float* d_out, void* stream);
/* adfl_stoch_dequantize_axpby_batched from packed planes: the same operands, arithmetic and in-place rule. */
int adfl_stoch_dequantize_axpby_packed_batched(int32_t codec, const uint8_t* d_levels, const uint8_t* d_signbits,
                                               const adfl_slq_chunk* d_chunks, int64_t nchunks, int bits,
                                               const float* d_norms, const float* d_mins, const float* const* d_base,
                                               float* const* d_out, int32_t ntensors, int32_t ntargets, float alpha,
                                               float beta, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* ADFL_STOCH_H */
