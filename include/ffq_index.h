/*
 * ffq_index.h — the gather / scatter entry points of the MI355X-native fake-quantization backend: the quantized index_add and
 * permute as one-pass kernels.
 *
 * A fourth header, for the reason ffq_3d.h is a second one: include/ffq.h is the ABI that BOTH libraries export (libffq_hip.so and
 * the C oracle), pinned at FFQ_ABI_VERSION 9. The entry points below exist in libffq_hip.so only (pointers are DEVICE pointers,
 * `stream` is a hipStream_t): a library without them is still a complete implementation of ffq.h, and a caller treats a missing
 * symbol as "not covered". Status codes, dtype tags and every convention of ffq.h (dense row-major tensors, caller-allocated
 * outputs, pure enqueues legal inside hipGraph capture, ffq_last_error()) hold here unchanged, and so do the conventions of the
 * one-pass families (ffq_cat_quantize, ffq_pad_quantize): `dt` is the value dtype T (FFQ_BF16 | FFQ_F16); an operand is plain
 * (`*_dt == dt`, scale NULL) or codes (`*_dt` FFQ_I8 or dt, fp32 scale, nullable fp32 offset) that are dequantized in registers
 * (A2: (q + rne(offset)) * scale in fp32, rounded to T); `out` (T, nullable) receives the value; `fan` (nullable) names up to
 * FFQ_MAX_FANOUT static per-tensor int8 quantizers whose codes are A1 of the value that `out` holds or would hold. Every vector-read
 * buffer is 16-byte aligned.
 */
#ifndef FFQ_INDEX_H
#define FFQ_INDEX_H

#include "ffq.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * index_add + A1 — ff.nn.functional.index_add through fallback.index_add (reference _gen/fallback.py:1483-1516: A2 of input and
 * source, torch.index_add(input, dim, index, source, alpha=alpha), the output quantizer). The tensors are viewed along `dim` as
 * x [outer, R, inner], src [outer, n, inner], index [n] (FFQ_I32 | FFQ_I64), out [outer, R, inner]; x and src have per-tensor
 * parameters. With a = rnd_T((float)alpha) (the number as ATen hands it to its kernel: double -> fp32 -> T):
 *   addend_j   = rnd_T( fp32(src[o,j,i]) * fp32(a) )
 *   out[o,r,i] = rnd_T( fp32(x[o,r,i]) + sum over j ascending with index[j] == r of fp32(addend_j) )
 * where the sum is taken in fp32 from left to right, starting from x, and rounded ONCE. With indices that are all different this is
 * bit for bit ATen's device index_add; with repeated indices ATen adds in the order its atomics land and rounds to T after every
 * addend, so its result changes from run to run, and this one does not. An index value outside [0, R) is SKIPPED (ATen asserts on
 * the device and leaves the result undefined); nothing outside the buffers is read or written for any index value.
 * n == 0 is a requantization of x. No workspace, no atomics, no memset, one launch; nothing is read on the host.
 * Errors, in this order: dt (FFQ_ERR_DTYPE); the form of x, then of src (FFQ_ERR_DTYPE); index_dt (FFQ_ERR_DTYPE); a negative
 * extent (FFQ_ERR_ARG); alpha not finite in T (FFQ_ERR_ARG); 2^31 or more elements in x or in src (FFQ_ERR_DTYPE); the fan-out
 * (ffq_fanout's own: FFQ_ERR_ARG, FFQ_ERR_PRECISION); then, unless x is empty (FFQ_OK, nothing launched), a NULL or misaligned x /
 * out, and with n > 0 a NULL index or a NULL or misaligned src (FFQ_ERR_ARG).
 */
int ffq_index_add_quantize(const void* x, int x_dt, const float* x_scale, const float* x_offset, const void* index, int index_dt,
                           int64_t n, const void* src, int src_dt, const float* src_scale, const float* src_offset, double alpha,
                           int dt, int64_t outer, int64_t R, int64_t inner, void* out, const ffq_fanout* fan, void* stream);

/*
 * permute + A1 — ff.nn.functional.permute through fallback.permute (reference _gen/fallback.py:1427-1449: A2, torch.permute, the
 * output quantizer, which reads the strided view). x is [shape[0], ..., shape[rank - 1]] contiguous, 1 <= rank <= 6; the result is
 * contiguous in the permuted shape, result axis i being axis dims[i] of x:
 *   out[c_0, ..., c_{rank-1}] = A2(x)[at axis dims[i]: c_i]
 * x has one parameter pair (param_axis < 0) or shape[param_axis] pairs indexed by the coordinate along axis `param_axis` of x
 * (PerChannel(param_axis)). There is no arithmetic but A2 and A1, so value and codes are bit for bit the chain's.
 * Two kernels: when the innermost axis of x stays innermost (after axes of extent 1 are dropped and axes that stay adjacent are
 * merged) rows are copied in groups of 8 elements (element by element when 8 does not divide the row); otherwise 64 x 64 tiles of
 * the two innermost axes involved are transposed through LDS. One launch, no workspace.
 * Errors, in this order: dt (FFQ_ERR_DTYPE); the form of x (FFQ_ERR_DTYPE); rank outside 1..6 or NULL shape / dims (FFQ_ERR_ARG);
 * a negative extent (FFQ_ERR_ARG); dims not a permutation of 0..rank-1 (FFQ_ERR_ARG); param_axis >= rank (FFQ_ERR_ARG); 2^31 or
 * more elements (FFQ_ERR_DTYPE); the fan-out; then, unless x is empty (FFQ_OK, nothing launched), a NULL or misaligned x / out
 * (FFQ_ERR_ARG).
 */
int ffq_permute_quantize(const void* x, int x_dt, const float* x_scale, const float* x_offset, int param_axis, int dt, int rank,
                         const int64_t* shape, const int64_t* dims, void* out, const ffq_fanout* fan, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FFQ_INDEX_H */
