/*
 * ffq_unfold.h — the im2col entry point of the MI355X-native fake-quantization backend: the quantized unfold as a one-pass kernel.
 *
 * A fifth header, for the reason ffq_index.h is a fourth one: include/ffq.h is the ABI that BOTH libraries export (libffq_hip.so and
 * the C oracle), pinned at FFQ_ABI_VERSION 9. The entry point below exists in libffq_hip.so only (pointers are DEVICE pointers,
 * `stream` is a hipStream_t): a library without it is still a complete implementation of ffq.h, and a caller treats a missing
 * symbol as "not covered". Status codes, dtype tags and every convention of ffq.h (dense row-major tensors, caller-allocated
 * outputs, pure enqueues legal inside hipGraph capture, ffq_last_error()) hold here unchanged, and so do the conventions of the
 * one-pass families (ffq_pad_quantize, ffq_permute_quantize): `dt` is the value dtype T (FFQ_BF16 | FFQ_F16); the operand is plain
 * (`x_dt == dt`, scale NULL) or codes (`x_dt` FFQ_I8 or dt, fp32 scale, nullable fp32 offset) that are dequantized in registers
 * (A2: (q + rne(offset)) * scale in fp32, rounded to T); `out` (T, nullable) receives the value; `fan` (nullable) names up to
 * FFQ_MAX_FANOUT static per-tensor int8 quantizers whose codes are A1 of the value that `out` holds or would hold. Every vector-read
 * buffer is 16-byte aligned.
 */
#ifndef FFQ_UNFOLD_H
#define FFQ_UNFOLD_H

#include "ffq.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * unfold + A1 — ff.nn.functional.unfold through fallback.unfold (reference _gen/fallback.py:1650-1677: A2, F.unfold — ATen's im2col
 * into a tensor KH * KW times the input — and the output quantizer over that tensor). x is [B, C, H, W] contiguous with one
 * parameter pair, or with `per_channel` C pairs indexed by the channel (PerChannel(1)). With ATen's output extents
 *   OH = (H + 2 * pad_h - dil_h * (KH - 1) - 1) / stride_h + 1,   OW likewise,   L = OH * OW,
 * the result is [B, C * KH * KW, L] contiguous:
 *   out[b, c * KH * KW + kh * KW + kw, oh * OW + ow] = A2(x)[b, c, oh * stride_h - pad_h + kh * dil_h, ow * stride_w - pad_w + kw * dil_w]
 * and +0.0 where that position lies outside the image. The +0.0 is the VALUE zero: its codes are A1(0.0) under each quantizer, not
 * code 0. An element inside the image keeps its own bits (a plain -0.0 stays -0.0, and so does the -0.0 that A2 gives for a
 * float-container code). There is no arithmetic but A2 and A1, so value and codes are bit for bit the chain's.
 * One kernel in two forms: when 8 divides L a lane writes 8 consecutive columns of one row of the result with one 16-byte store (and
 * one 8-byte store per quantizer), walking (oh, ow) element by element where such a group spans output rows or the window is strided
 * along W, and reading its 8 inputs with one load where it lies inside one output row of a stride-1 window; for any other L a lane
 * writes one element. The input is read through the caches. One launch, no workspace, no memset, no atomics; nothing is read on
 * the host.
 * Errors, in this order: dt (FFQ_ERR_DTYPE); the form of x (FFQ_ERR_DTYPE); a negative B, C, H, W, KH or KW (FFQ_ERR_ARG); an empty
 * window, KH == 0 or KW == 0 (FFQ_ERR_EMPTY); a stride or dilation < 1 or a padding < 0 (FFQ_ERR_ARG); H, W, KH, KW, a stride, a
 * dilation or a padding above 2^24 (FFQ_ERR_ARG); a dilated window dil * (K - 1) + 1 larger than the padded image along either axis
 * (FFQ_ERR_ARG); 2^31 or more elements in x or in the result (FFQ_ERR_DTYPE); the fan-out (ffq_fanout's own: FFQ_ERR_ARG,
 * FFQ_ERR_PRECISION); then, unless B == 0 or C == 0 (FFQ_OK, nothing launched), a NULL or misaligned x / out / codes buffer
 * (FFQ_ERR_ARG).
 */
int ffq_unfold_quantize(const void* x, int x_dt, const float* x_scale, const float* x_offset, int per_channel, int dt,
                        int64_t B, int64_t C, int64_t H, int64_t W, int64_t KH, int64_t KW,
                        int64_t dil_h, int64_t dil_w, int64_t pad_h, int64_t pad_w, int64_t stride_h, int64_t stride_w,
                        void* out, const ffq_fanout* fan, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FFQ_UNFOLD_H */
