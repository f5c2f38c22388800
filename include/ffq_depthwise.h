/*
 * ffq_depthwise.h — the depthwise entry point of the MI355X-native fake-quantization backend: the W8A8 conv2d / conv1d with
 * groups == C.
 *
 * A third header, for the reason ffq_3d.h is a second one: include/ffq.h is the ABI that BOTH libraries export (libffq_hip.so and
 * the C oracle), pinned at FFQ_ABI_VERSION 9. The entry point below exists in libffq_hip.so only (pointers are DEVICE pointers,
 * `stream` is a hipStream_t): a library without it is still a complete implementation of ffq.h, and a caller treats the missing
 * symbol as "not covered". Status codes, dtype tags and every convention of ffq.h (dense row-major tensors, caller-allocated
 * outputs, pure enqueues legal inside hipGraph capture, ffq_last_error()) hold here unchanged.
 */
#ifndef FFQ_DEPTHWISE_H
#define FFQ_DEPTHWISE_H

#include "ffq.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * W8A8 depthwise convolution — ff.nn.functional.conv2d / conv1d with groups == C through fallback.conv2d / fallback.conv1d
 * (reference _gen/fallback.py:116-214: A2 of input and weight, F.conv2d(groups=C), the output quantizer). ffq_conv2d_w8a8's contract
 * with a one-channel reduction: output channel n of C * M (M >= 1 the channel multiplier) reads input channel c = n / M. For output
 * (b, n, p), p = (oh, ow), V(p) = the taps t = (kh, kw) whose input pixel (ih, iw) = (oh * stride_h - pad_h + kh * dil_h,
 * ow * stride_w - pad_w + kw * dil_w) lies inside the H x W image:
 *   acc = sum_{t in V(p)} xq[b,c,ih,iw] * wq[n,t]                                           (int32, exact: |acc| <= 2^24)
 *   rsx = sum_{t in V(p)} xq[b,c,ih,iw]                                                     (only with w_offset)
 *   rsw = sum_{t in V(p)} wq[n,t]                                                           (only when rne(x_offset) != 0)
 *   v = float(acc); v = v + ox * rsw; v = v + ow * rsx; v = v + |V(p)| * ox * ow            (fp32, left to right, no FMA)
 *   y = (sx * sw[n']) * v  (+ bias[n])
 * with ox / ow = rne(offset) as in A2 and n' = n if w_per_channel else 0. Out-of-image taps read code 0 and leave V(p); a window
 * with no tap inside the image gives the bias (or 0). Channel n is bit for bit what ffq_conv2d_w8a8 writes for the one-channel
 * slice xq[:, c], wq[n] with the same parameters.
 * Layout: xq is [B, C, H, W] contiguous; wq is [C * M, 1, KH, KW] contiguous (torch.nn.Conv2d(groups=C)); out is
 * [B, C * M, OH, OW] contiguous, OH = (H + 2 pad_h - dil_h (KH - 1) - 1) / stride_h + 1 and likewise OW. conv1d is H = KH = 1.
 * Parameters: x per tensor; w per tensor or per output channel ([C * M]); fp32; bias nullable (f32 / bf16 / f16, [C * M]).
 * If out_scale != NULL the output quantizer (per tensor) runs in the epilogue under ffq_conv2d_w8a8's rule: y rounded once to
 * y_dt, then codes = clamp(rne(y / out_scale - rne(out_offset))) into out (out_dt must be int8) — bit-identical to
 * ffq_quantize_by_tile on the tensor the call without out_scale writes in y_dt. Else out holds y in out_dt (f32 / bf16 / f16).
 * Coverage: KH * KW <= 1024 (else FFQ_ERR_DTYPE: one channel's taps are held on chip), stride / dilation >= 1, padding >= 0,
 * extents <= 2^24, B * OH * OW < 2^31, fewer than 2^24 blocks (a block is up to 256 lanes of 4 consecutive outputs of one plane).
 * No workspace, no memset, one launch. Every argument check runs before the launch; B == 0 or C == 0 returns FFQ_OK without one.
 * Errors, in this order (ffq_conv3d_w8a8's): a negative extent (FFQ_ERR_ARG); M or a kernel extent 0 (FFQ_ERR_EMPTY); stride /
 * dilation < 1 or padding < 0 (FFQ_ERR_ARG); an extent, stride, padding or dilation above 2^24 (FFQ_ERR_ARG); KH * KW > 1024
 * (FFQ_ERR_DTYPE); a dilated filter larger than the padded input (FFQ_ERR_ARG); too many positions, elements or blocks for one
 * launch (FFQ_ERR_ARG); the bias dtype (FFQ_ERR_DTYPE); out_dt / out_num_bits / y_dt (FFQ_ERR_DTYPE, FFQ_ERR_PRECISION,
 * FFQ_ERR_DTYPE); then, unless B == 0 or C == 0, a NULL buffer (FFQ_ERR_ARG).
 */
int ffq_depthwise_conv2d_w8a8(const int8_t* xq, const int8_t* wq, const float* x_scale, const float* x_offset, const float* w_scale,
                              const float* w_offset, int w_per_channel, const void* bias, int bias_dt, void* out, int out_dt,
                              const float* out_scale, const float* out_offset, double out_num_bits, int y_dt, int64_t B, int64_t C,
                              int64_t M, int64_t H, int64_t W, int64_t KH, int64_t KW, int64_t stride_h, int64_t stride_w,
                              int64_t pad_h, int64_t pad_w, int64_t dil_h, int64_t dil_w, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FFQ_DEPTHWISE_H */
