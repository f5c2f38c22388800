/*
 * ffq_lpbq.h — LPBQ weights of the MI355X-native fake-quantization backend: a W4 block-quantized weight re-expressed as int8 codes with
 * one scale per output channel, so that the int8 GEMM (ffq_linear_w8a8, per-row weight scales in its epilogue) serves it unchanged.
 *
 * An eleventh header, for the reason ffq_unfold.h is a fifth one: include/ffq.h is the ABI that BOTH libraries export (libffq_hip.so
 * and the C oracle), pinned at FFQ_ABI_VERSION 9. The entry points below exist in libffq_hip.so only (pointers are DEVICE pointers,
 * `stream` is a hipStream_t): a library without them is still a complete implementation of ffq.h, and a caller treats a missing
 * symbol as "not covered". Status codes, dtype tags and every convention of ffq.h (caller-allocated outputs, pure enqueues legal
 * inside hipGraph capture, ffq_last_error()) hold here unchanged. (The header lives in include/lpbq/: include/ itself holds the ten
 * headers of the ABI and the KV caches.)
 *
 * The format (reference export/_lpbq.py, LPBQProcessor): a weight [N, K] with symmetric `bits`-bit codes c4 and one fp32 scale per
 * block of G input channels, s[n, j], j = k / G, J = K / G blocks per row. Per row
 *     m    = max_j s[n, j]
 *     d[n] = m / 2^bits                                    (the IEEE fp32 quotient)
 *     q[n, j] = clamp(rne(s[n, j] / d[n]), 1, 2^bits)      (IEEE quotient, round half to even, fmaxf / fminf)
 * — grouped_dynamic_quantize for PerBlock(block_dims=(1,), per_channel_dims=(0,)), bit for bit for finite positive scales. For a
 * zero, negative or non-finite scale the result is unspecified, except that every q stays in [1, 2^bits] and nothing outside the
 * outputs is written. The block scale is re-expressed as q[n, j] * d[n]; c4 * q is an integer in [-2^(2 bits - 1), 2^(2 bits - 1) -
 * 2^bits] ([-128, 112] at 4 bits): an int8 code of a per-channel symmetric tensor with scale d[n].
 *
 * Every entry point takes a stream, needs no workspace and is a single launch. Outputs are dense: codes8 [N, K] with rows K bytes
 * apart, int_scale [N, J] with rows J bytes apart, channel_scale [N]. Inputs that are matrices come with a row stride in elements, so
 * a column window of a wider matrix is read in place. bits is 2, 3 or 4; J <= 1024 (a row's q live in LDS).
 */
#ifndef FFQ_LPBQ_H
#define FFQ_LPBQ_H

#include "../ffq.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Scale compression alone: scales fp32 [N, J] (rows `scale_stride` elements apart) -> int_scale uint8 [N, J], channel_scale fp32 [N].
 * One wave per row, four rows per workgroup; the row maximum over wave shuffles.
 * Errors, in this order: bits outside {2, 3, 4} (FFQ_ERR_ARG); a negative N or J, or N >= 2^31 (FFQ_ERR_ARG); J > 1024 (FFQ_ERR_ARG);
 * scale_stride < J (FFQ_ERR_ARG); then, unless N == 0 or J == 0 (FFQ_OK, nothing launched), a NULL scales / int_scale / channel_scale
 * (FFQ_ERR_ARG); scales or channel_scale not 4-byte aligned (FFQ_ERR_ARG).
 */
int ffq_lpbq_compress_scales(const float* scales, int64_t scale_stride, int64_t N, int64_t J, int bits, uint8_t* int_scale,
                             float* channel_scale, void* stream);

/*
 * The per-step weight quantizer, fused: w [N, K] (w_dt FFQ_BF16 | FFQ_F16 | FFQ_F32, rows `w_stride` elements apart) and its block
 * scales fp32 [N, K / G] (rows `scale_stride` elements apart) -> codes8 int8 [N, K], channel_scale fp32 [N] and, unless it is NULL,
 * int_scale uint8 [N, K / G]. Per row the compression above (q kept in LDS), then
 *     codes8[n, k] = c4 * q[n, k / G],   c4 = A1 of w[n, k] at `bits` bits, symmetric, no offset (clamp(rne(w / s), -2^(bits-1), 2^(bits-1) - 1)),
 * with s = s[n, k / G] when requantize == 0 (the export's semantics: the codes of the calibrated scale, the encoding carries the
 * compressed one) and s = d[n] * (float)q[n, k / G], the fp32 product, when requantize == 1 (the codes round against the scale that
 * is applied). c4 is ffq_quantize_by_tile's code for the tile (1, G) into int8, bit for bit, whatever the element (ties, values beyond
 * the clamps, -0.0, NaN, Inf): the same arithmetic (csrc/ffq_affine.h).
 * One pass over w in one launch: one workgroup per row, or one wave per row and four rows per workgroup when K <= 8192; the row
 * maximum over wave shuffles, then LDS. Group form — 16-byte loads of w, 8-byte stores of codes8, 8 elements per lane and step — when
 * 8 divides G, w is 16-byte aligned with a row stride of whole 16 bytes and codes8 is 8-byte aligned; the element form otherwise.
 * Errors, in this order: w_dt (FFQ_ERR_DTYPE); bits outside {2, 3, 4} (FFQ_ERR_ARG); requantize not 0 or 1 (FFQ_ERR_ARG); a negative N
 * or K, N or K >= 2^31, or G < 1 (FFQ_ERR_ARG); K % G != 0 (FFQ_ERR_ARG); K / G > 1024 (FFQ_ERR_ARG); w_stride < K or scale_stride <
 * K / G (FFQ_ERR_ARG); then, unless N == 0 or K == 0 (FFQ_OK, nothing launched), a NULL w / scales / codes8 / channel_scale
 * (FFQ_ERR_ARG); w not aligned to its element, or scales / channel_scale not 4-byte aligned (FFQ_ERR_ARG).
 */
int ffq_lpbq_quantize(const void* w, int w_dt, int64_t w_stride, const float* scales, int64_t scale_stride, int64_t N, int64_t K,
                      int64_t G, int bits, int requantize, int8_t* codes8, float* channel_scale, uint8_t* int_scale, void* stream);

/*
 * The at-rest form back to a GEMM operand: codes8[n, k] = c4[n, k] * int_scale[n, k / G], with the `bits`-bit codes either as dense
 * int8 [N, K] (packed == 0; `block` is ignored) or as the N * K / 2 bytes of ffq_pack_int4 over the flat tensor (packed == 1, `block`
 * as in ffq_unpack_int4: the low nibbles of a block's bytes hold its first half, code + 8). Bit-equal to ffq_unpack_int4 followed by
 * the integer product, truncated to int8 (exact for codes in [-8, 7] and q in [1, 16]). int_scale is dense [N, K / G].
 * Group form — 8 codes per 8-byte store — when 8 divides G, N * K < 2^32, the pointers are 8-byte aligned and (packed) 16 divides
 * `block`; one code (packed: one byte) per lane otherwise.
 * Errors, in this order: packed not 0 or 1 (FFQ_ERR_ARG); a negative N or K, N or K >= 2^31, or G < 1 (FFQ_ERR_ARG); K % G != 0
 * (FFQ_ERR_ARG); K / G > 1024 (FFQ_ERR_ARG); packed and `block` < 2, odd, or not a divisor of N * K (FFQ_ERR_ARG); then, unless N == 0
 * or K == 0 (FFQ_OK, nothing launched), a NULL codes4 / int_scale / codes8 (FFQ_ERR_ARG).
 */
int ffq_lpbq_expand(const void* codes4, int packed, int64_t block, const uint8_t* int_scale, int64_t N, int64_t K, int64_t G,
                    int8_t* codes8, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FFQ_LPBQ_H */
