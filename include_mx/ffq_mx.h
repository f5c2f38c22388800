/*
 * ffq_mx.h — OCP microscaling (MX) formats of the MI355X-native fake-quantization backend: the MXFP8 / MXFP4 quantizer, its inverse,
 * and a linear on the block-scaled matrix-core instruction of CDNA4 (v_mfma_scale_f32_32x32x64_f8f6f4).
 *
 * A twelfth header, for the reason ffq_lpbq.h is an eleventh one (it lives in include_mx/: tests pin the set of headers under include/): the entry points below exist in libffq_hip.so only (pointers are
 * DEVICE pointers, `stream` is a hipStream_t); a library without them is still a complete implementation of ffq.h and a caller treats
 * a missing symbol as "not covered". Status codes, dtype tags and every convention of ffq.h (caller-allocated outputs, pure enqueues
 * legal inside hipGraph capture, ffq_last_error()) hold here unchanged. No entry point takes a workspace.
 *
 * The format (docs/numerics.md, "MX formats"). A block is 32 consecutive elements of the last dimension and has one E8M0 scale byte:
 * value 2^(code - 127), code 255 = NaN. Elements are
 *     FFQ_MX_E4M3  OCP e4m3fn, one byte, largest normal 448, emax = 8;
 *     FFQ_MX_E2M1  sign + the grid 0, 0.5, 1, 1.5, 2, 3, 4, 6 (codes 0 .. 7), emax = 2; at rest either one code per byte (low nibble)
 *                  or packed two per byte, element 2i in the low nibble and 2i + 1 in the high one (torch.float4_e2m1fn_x2).
 * Scale of a block: amax = max |x| in fp32, e = its biased exponent field (0 for zero and subnormals), code = max(e - emax, 0).
 * Elements: x * 2^(127 - code) (fp32), clamped to +- the largest normal, rounded to the nearest grid value, ties to the even code;
 * the sign bit is kept (-0.0 included). A block that holds a NaN or an Inf gets scale code 255 and all-zero element codes.
 * Dequantization: value(code) * 2^(scale - 127) as one fp32 product (2^-127 for scale 0, NaN for scale 255), rounded once to the
 * output dtype. An e4m3 code 0x7F / 0xFF (never produced by the quantizer) reads as NaN.
 */
#ifndef FFQ_MX_H
#define FFQ_MX_H

#include "../include/ffq.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FFQ_MX_E4M3 0
#define FFQ_MX_E2M1 1
#define FFQ_MX_BLOCK 32

/*
 * x [rows, K] (x_dt FFQ_BF16 | FFQ_F16 | FFQ_F32, rows `x_stride` elements apart) -> scales uint8 [rows, K / 32] and the element codes,
 * all dense: `codes` uint8 [rows, K], one code per byte, and / or (FFQ_MX_E2M1 only) `packed` uint8 [rows, K / 2]. Either code pointer
 * may be NULL, not both. One pass, one launch: a lane owns 16 consecutive elements (16-byte loads), the block maximum crosses the two
 * lanes of a block by a shuffle, stores are 16 bytes (codes) and 8 bytes (packed) per lane. That form needs x 16-byte aligned with a
 * row stride of whole 16 bytes, codes 16-byte and packed 8-byte aligned; any other pointer takes the element form (same bits).
 * Errors, in this order: x_dt (FFQ_ERR_DTYPE); format (FFQ_ERR_ARG); a negative rows or K, or rows * K >= 2^35 (FFQ_ERR_ARG); K % 32 != 0
 * (FFQ_ERR_ARG); x_stride < K (FFQ_ERR_ARG); `packed` given with FFQ_MX_E4M3 (FFQ_ERR_ARG); then, unless rows == 0 or K == 0 (FFQ_OK,
 * nothing launched), a NULL x or scales, or both code pointers NULL (FFQ_ERR_ARG); x not aligned to its element (FFQ_ERR_ARG).
 */
int ffq_mx_quantize(const void* x, int x_dt, int64_t x_stride, int64_t rows, int64_t K, int format, uint8_t* codes, uint8_t* packed,
                    uint8_t* scales, void* stream);

/*
 * The inverse: codes (is_packed == 0: uint8 [rows, K]; is_packed == 1, FFQ_MX_E2M1 only: uint8 [rows, K / 2]) and scales uint8
 * [rows, K / 32], all dense -> out [rows, K] dense in out_dt FFQ_BF16 | FFQ_F16 | FFQ_F32. One launch, 16 elements per lane.
 * Errors, in this order: out_dt (FFQ_ERR_DTYPE); format (FFQ_ERR_ARG); is_packed not 0 or 1, or 1 with FFQ_MX_E4M3 (FFQ_ERR_ARG); a
 * negative rows or K, or rows * K >= 2^35 (FFQ_ERR_ARG); K % 32 != 0 (FFQ_ERR_ARG); then, unless rows == 0 or K == 0 (FFQ_OK), a NULL
 * codes / scales / out (FFQ_ERR_ARG); out not aligned to its element (FFQ_ERR_ARG).
 */
int ffq_mx_dequantize(const uint8_t* codes, int is_packed, const uint8_t* scales, int64_t rows, int64_t K, int format, void* out, int out_dt,
                      void* stream);

/*
 * 1 when ffq_linear_mx takes (M, N, K, a_format, w_format): M, N >= 1, K >= 128 with K % 128 == 0 (one K step's four scale bytes of a
 * row are one aligned dword), M, N, K < 2^31, and the pair (a, w) one of (E4M3, E4M3), (E4M3, E2M1), (E2M1, E2M1). 0 otherwise.
 */
int ffq_linear_mx_supported(int64_t M, int64_t N, int64_t K, int a_format, int w_format);

/*
 * out[M, N] = A[M, K] . W[N, K]^T (+ bias[N]) on the block-scaled MFMA, fp32 accumulation, one rounding to out_dt (FFQ_F32 | FFQ_BF16 |
 * FFQ_F16); the bias (NULL: none; bias_dt FFQ_F32 or out_dt) is added in fp32 before that rounding. out is dense, rows N elements apart.
 * Operands: element codes as the quantizer leaves them for the GEMM — e4m3 one byte per element, e2m1 PACKED two per byte — and scale
 * bytes [rows, K / 32]; each of the four matrices comes with a row stride in BYTES, so a column window of a wider matrix is read in place.
 * One launch: 128 x 128 output tiles, 256 threads, K steps of 128; codes global -> LDS by global_load_lds; rows beyond M / N are never stored.
 * An output that reads a block whose scale byte is 255 is NaN; every other output keeps its bits (docs/numerics.md).
 * Errors, in this order: a_format / w_format not a format (FFQ_ERR_ARG); the pair (E2M1, E4M3) (FFQ_ERR_ARG); out_dt, or a bias with
 * bias_dt neither FFQ_F32 nor out_dt (FFQ_ERR_DTYPE); M, N or K negative or >= 2^31 (FFQ_ERR_ARG); then, when M == 0 or N == 0, FFQ_OK
 * with nothing launched; K == 0 or K % 128 != 0 (FFQ_ERR_ARG); a code row stride below the row's bytes or a scale row stride below K / 32
 * (FFQ_ERR_ARG); a NULL a_codes / a_scales / w_codes / w_scales / out (FFQ_ERR_ARG); a code pointer or code row stride not 16-byte
 * aligned (FFQ_ERR_ARG); a scale pointer or scale row stride not 4-byte aligned (FFQ_ERR_ARG); out or bias not aligned to its element
 * (FFQ_ERR_ARG). Every error returns before any launch.
 */
int ffq_linear_mx(const uint8_t* a_codes, int64_t a_stride, const uint8_t* a_scales, int64_t a_scale_stride, int a_format,
                  const uint8_t* w_codes, int64_t w_stride, const uint8_t* w_scales, int64_t w_scale_stride, int w_format, const void* bias,
                  int bias_dt, void* out, int out_dt, int64_t M, int64_t N, int64_t K, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FFQ_MX_H */
