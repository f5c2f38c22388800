/*
 * ffq_3d.h — the 3-D spatial entry points of the MI355X-native fake-quantization backend: the W8A8 conv3d and avg_pool3d.
 *
 * A second header on purpose. include/ffq.h is the ABI that BOTH libraries export (libffq_hip.so and the C oracle) and that the
 * guard-band harness wraps symbol by symbol; its set of declarations is pinned at FFQ_ABI_VERSION 9. The entry points below exist
 * in libffq_hip.so only (pointers are DEVICE pointers, `stream` is a hipStream_t): a library without one of them is still a
 * complete implementation of ffq.h, and a caller treats the missing symbol as "not covered". Status codes, dtype tags, ffq_fanout
 * and every convention of ffq.h (dense row-major tensors, caller-allocated outputs and workspace, pure enqueues legal inside
 * hipGraph capture, ffq_last_error()) hold here unchanged.
 */
#ifndef FFQ_3D_H
#define FFQ_3D_H

#include "ffq.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * W8A8 3-D convolution — ff.nn.functional.conv3d / QuantizedConv3d through fallback.conv3d (reference _gen/fallback.py:218-265: A2
 * of input and weight, F.conv3d, the output quantizer). ffq_conv2d_w8a8's contract with one more axis. For output (b, n, p),
 * p = (od, oh, ow), V(p) = the taps (kd, kh, kw) whose input voxel (od * stride_d - pad_d + kd * dil_d, oh * stride_h - pad_h +
 * kh * dil_h, ow * stride_w - pad_w + kw * dil_w) lies inside the D x H x W volume:
 *   acc = sum_{t in V(p), c < C} xq[b,c,id,ih,iw] * wq[n,c,t]                               (int32, exact)
 *   rsx = sum_{t in V(p), c < C} xq[b,c,id,ih,iw]                                           (only with w_offset)
 *   rsw = sum_{t in V(p)} sum_c wq[n,c,t]                                                    (only when rne(x_offset) != 0)
 *   v = float(acc); v = v + ox * rsw; v = v + ow * rsx; v = v + (C * |V(p)|) * ox * ow      (fp32, left to right, no FMA)
 *   y = (sx * sw[n']) * v  (+ bias[n])
 * with ox / ow = rne(offset) as in A2 and n' = n if w_per_channel else 0. Out-of-volume taps read code 0 and leave V(p) (the
 * reference pads the dequantized input with 0.0: the same real-valued sum). Channels are padded to a multiple of 16 with code 0
 * internally.
 * Layout: xq is [B, C, D, H, W] contiguous, or (x_ndhwc != 0, C % 16 == 0, 16-byte aligned) [B, D, H, W, C] — a
 * torch.channels_last_3d tensor; wq is [OC, C, KD, KH, KW] contiguous; out is [B, OC, OD, OH, OW] contiguous,
 * OD = (D + 2 pad_d - dil_d (KD - 1) - 1) / stride_d + 1 and likewise OH, OW. Parameters: x per tensor; w per tensor or per output
 * channel; fp32; bias nullable (f32 / bf16 / f16, [OC]).
 * If out_scale != NULL the output quantizer (per tensor) runs in the epilogue under ffq_conv2d_w8a8's rule: y rounded once to
 * y_dt, then codes = clamp(rne(y / out_scale - rne(out_offset))) into out (out_dt must be int8) — bit-identical to
 * ffq_quantize_by_tile on the tensor the call without out_scale writes in y_dt. Else out holds y in out_dt (f32 / bf16 / f16).
 * Coverage: groups == 1 (the caller's), C * KD * KH * KW <= 131071 (else FFQ_ERR_DTYPE: the int32 accumulator's bound of
 * docs/numerics.md), stride / dilation >= 1, padding >= 0, extents <= 2^24, B * OD * OH * OW < 2^31. Every argument check runs
 * before any launch; B == 0 or OC == 0 returns FFQ_OK without one.
 * Workspace: ffq_conv3d_w8a8_workspace_bytes(...) bytes, 16-byte aligned — the NDHWC input codes round256(B * D * H * W * Cp)
 * (none with x_ndhwc), the reordered weight round256(OC * KD * KH * KW * Cp) and the per-tap weight sums with their totals
 * round256(4 * (OC * KD * KH * KW + OC)), Cp = 16 * ceil(C / 16), round256 = up to a multiple of 256; less returns
 * FFQ_ERR_WORKSPACE. The query returns 0 for extents no launch takes. Two launches (layout, GEMM) and a memset.
 * Errors, in this order: a negative extent (FFQ_ERR_ARG); C or a kernel extent 0 (FFQ_ERR_EMPTY); stride / dilation < 1 or padding
 * < 0 (FFQ_ERR_ARG); an extent, stride, padding or dilation above 2^24 (FFQ_ERR_ARG); the reduction bound (FFQ_ERR_DTYPE);
 * x_ndhwc with C % 16 != 0 (FFQ_ERR_DTYPE); a dilated filter larger than the padded input (FFQ_ERR_ARG); too many positions or
 * elements for one launch (FFQ_ERR_ARG); the bias dtype (FFQ_ERR_DTYPE); out_dt / out_num_bits / y_dt (FFQ_ERR_DTYPE,
 * FFQ_ERR_PRECISION, FFQ_ERR_DTYPE); then, unless B == 0 or OC == 0, a NULL buffer or misaligned channels-last codes (FFQ_ERR_ARG)
 * and the workspace (FFQ_ERR_WORKSPACE).
 */
size_t ffq_conv3d_w8a8_workspace_bytes(int64_t B, int64_t C, int64_t D, int64_t H, int64_t W, int64_t OC, int64_t KD, int64_t KH,
                                       int64_t KW, int x_ndhwc);
int ffq_conv3d_w8a8(const int8_t* xq, int x_ndhwc, const int8_t* wq, const float* x_scale, const float* x_offset,
                    const float* w_scale, const float* w_offset, int w_per_channel, const void* bias, int bias_dt, void* out,
                    int out_dt, const float* out_scale, const float* out_offset, double out_num_bits, int y_dt, int64_t B,
                    int64_t C, int64_t D, int64_t H, int64_t W, int64_t OC, int64_t KD, int64_t KH, int64_t KW, int64_t stride_d,
                    int64_t stride_h, int64_t stride_w, int64_t pad_d, int64_t pad_h, int64_t pad_w, int64_t dil_d, int64_t dil_h,
                    int64_t dil_w, void* workspace, size_t workspace_bytes, void* stream);

/*
 * avg_pool3d + A1 — ff.nn.functional.avg_pool3d (reference _gen/fallback.py:579-612): x is [planes, D, H, W] (planes = B * C),
 * z [planes, OD, OH, OW] = dt(avg(v)), codes_j = A1(z; scale_j, offset_j), with ATen's device formula for avg_pool3d: one fp32
 * accumulator over the part of the window inside the input, depth outermost and width innermost, divided once by
 *   mode 0 (count_include_pad): the window's size clipped to the input plus its padding;   mode 1: its size inside the input.
 * v, param_channels, fan and out (nullable) as in ffq_pool2d_quantize. Bit for bit the chain's value (A2, F.avg_pool3d, A1).
 * [OD, OH, OW] must be ATen's pooling_output_shape(D / H / W, kernel, pad, stride, 1, ceil_mode) — the last window starts inside
 * the input or its left padding; kernel, stride >= 1, 0 <= pad <= kernel / 2, D, H, W >= 1: otherwise FFQ_ERR_ARG, as ATen refuses
 * them. Any plane size; fewer than 2^31 input and output elements. dt is bf16 or fp16. No workspace; one launch.
 * Errors, in ffq_pool2d_quantize's order: the mode (FFQ_ERR_ARG: 0 or 1, there is no max_pool3d here); dt or the input's form
 * (FFQ_ERR_DTYPE, before any buffer is looked at); kernel / stride < 1 or above 2^20, padding < 0 (FFQ_ERR_ARG); padding above half
 * the kernel (FFQ_ERR_ARG); [OD, OH, OW] (FFQ_ERR_ARG); a negative extent, planes no multiple of param_channels, an empty map, an
 * output extent < 1 (FFQ_ERR_ARG); 2^31 elements or more (FFQ_ERR_DTYPE); the fan-out; then, unless planes == 0 (FFQ_OK, no launch),
 * a NULL or misaligned buffer (FFQ_ERR_ARG).
 */
int ffq_pool3d_quantize(int mode, const void* x, int x_dt, const float* x_scale, const float* x_offset, int64_t param_channels, int dt,
                        int64_t planes, int64_t D, int64_t H, int64_t W, int64_t kd, int64_t kh, int64_t kw, int64_t sd, int64_t sh,
                        int64_t sw, int64_t pd, int64_t ph, int64_t pw, int ceil_mode, int64_t OD, int64_t OH, int64_t OW, void* out,
                        const ffq_fanout* fan, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FFQ_3D_H */
