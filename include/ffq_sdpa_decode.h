/*
 * ffq_sdpa_decode.h — scaled_dot_product_attention for a short query over int8 K / V codes (a quantized KV cache), split over the
 * keys.
 *
 * A sixth header, for the reason ffq_unfold.h is a fifth one: include/ffq.h is the ABI that BOTH libraries export (libffq_hip.so and
 * the C oracle), pinned at FFQ_ABI_VERSION 9. The entry points below exist in libffq_hip.so only (pointers are DEVICE pointers,
 * `stream` is a hipStream_t): a library without them is still a complete implementation of ffq.h, and a caller treats a missing
 * symbol as "not covered". Status codes, dtype tags and every convention of ffq.h (caller-allocated outputs and workspaces, pure
 * enqueues legal inside hipGraph capture, ffq_last_error()) hold here unchanged.
 */
#ifndef FFQ_SDPA_DECODE_H
#define FFQ_SDPA_DECODE_H

#include "ffq.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FFQ_SDPA_DECODE_MAX_ROWS 32   /* L * (q_heads / kv_heads): the query side of one MFMA tile */
#define FFQ_SDPA_DECODE_KEY_TILE 128  /* keys per workgroup step: every split but the last is a whole number of these */
#define FFQ_SDPA_DECODE_MAX_SPLITS 64 /* the cap on the number of key splits */

/*
 * The split plan: into how many contiguous runs of keys the S keys of one (batch, kv head) are cut when `splits` is 0 below. A pure
 * function of its arguments (no device state: the same inside and outside a hipGraph capture). With tiles = ceil(S / KEY_TILE)
 * every split takes per = ceil(tiles / splits) tiles (the last one what is left), no split is empty, and 1 <= splits <= MAX_SPLITS.
 * The rule asks for about one workgroup per compute unit (256 / (batch * kv_heads) splits) as long as a split keeps at least two
 * tiles. `rows` and `E` are part of the signature so that the rule may come to depend on them; today it does not.
 */
int64_t ffq_sdpa_decode_splits(int64_t batch, int64_t kv_heads, int64_t S, int64_t rows, int64_t E);

/*
 * Bytes of the workspace of one call with `splits` splits (the number the query above returned, or the forced one):
 * batch * kv_heads * splits * rows * (E + 2) floats — O[rows][E], m[rows] and l[rows] of every partial. 0 for a non-positive argument.
 */
size_t ffq_sdpa_decode_workspace_bytes(int64_t batch, int64_t kv_heads, int64_t rows, int64_t E, int64_t splits);

/*
 * out = softmax(q k^T * scale + bias) v for q [batch, q_heads, L, E], k / v [batch, kv_heads, S, E] and out [batch, q_heads, L, E]
 * (contiguous, dtype dt = FFQ_BF16 | FFQ_F16), with rows = L * (q_heads / kv_heads) <= MAX_ROWS and E in {64, 128}; query head h
 * reads kv head h / (q_heads / kv_heads).
 *   k, v   int8 codes with per-tensor fp32 parameters deq_scale[1] / deq_offset[1] and deq_scale[2] / deq_offset[2] (offsets
 *          nullable): the value is (code + rne(offset)) * scale in fp32, rounded once to dt.
 *   q      q_dt == dt: plain values (deq_scale[0] NULL) or codes held in dt; q_dt == FFQ_I8: int8 codes. Codes are dequantized as
 *          k and v are.
 *   strides  nine element strides, (batch, head, row) of q, k, v in their containers; the last dimension is contiguous and every
 *          row starts on a 16-byte boundary.
 *   mask   mask_kind 0 none, 1 causal (top-left: row l sees keys <= l), 2 bool (uint8, nonzero keeps), 3 float (added; mask_dt
 *          FFQ_F32 | FFQ_BF16 | FFQ_F16); mask_strides are the four element strides of the mask expanded to [batch, q_heads, L, S].
 *   sqrt_scale  sqrt of the softmax scale: the scores are the fp32 dot products times float(sqrt_scale)^2.
 *   out_scale / out_offset / out_num_bits  the optional per-tensor output quantizer (out_scale NULL: none): A1 then A2 on the fp32
 *          result, before the one rounding to dt. A row whose scores are all -inf gives exactly 0 (the safe softmax).
 *   splits 0: the rule above; 1 .. MAX_SPLITS: forced (for tests; a forced split may end up without a key).
 * Two launches: the partial kernel (one workgroup per (batch, kv head, split): online softmax over the split's keys, fp32 partials
 * into the workspace) and the combine kernel. No memset, no atomics, nothing read on the host. Nothing is read or written out of
 * bounds at any S >= 1.
 * Errors, in this order, before anything is enqueued: dt (FFQ_ERR_DTYPE); q_dt neither dt nor FFQ_I8 (FFQ_ERR_DTYPE); a NULL
 * strides / deq_scale / deq_offset table (FFQ_ERR_ARG); int8 q codes without a scale (FFQ_ERR_DTYPE); k or v without a scale
 * (FFQ_ERR_ARG); E (FFQ_ERR_ARG); a negative extent, a head count < 1 or q_heads not a multiple of kv_heads (FFQ_ERR_ARG);
 * rows > MAX_ROWS (FFQ_ERR_ARG); mask_kind (FFQ_ERR_ARG); a float mask's dtype (FFQ_ERR_DTYPE); an output offset without a scale, or
 * an output bit-width that is not an integer in 1..8 (FFQ_ERR_ARG); splits outside 0..MAX_SPLITS (FFQ_ERR_ARG); then batch == 0 or
 * L == 0 returns FFQ_OK with nothing launched; S == 0 (FFQ_ERR_ARG); S >= 2^30 or batch * kv_heads >= 2^24 (FFQ_ERR_ARG); a NULL q /
 * k / v / out (FFQ_ERR_ARG); a mask without data or strides (FFQ_ERR_ARG); a misaligned q / k / v / out (FFQ_ERR_ARG); a negative
 * stride or one that is not a multiple of 16 bytes (FFQ_ERR_ARG); a workspace that is NULL, misaligned or smaller than the size
 * query's figure (FFQ_ERR_WORKSPACE) — `out` is untouched by a call that fails.
 */
int ffq_sdpa_decode(const void* q, int q_dt, const void* k, const void* v, int dt, const float* const* deq_scale,
                    const float* const* deq_offset, int64_t batch, int64_t q_heads, int64_t kv_heads, int64_t L, int64_t S, int64_t E,
                    const int64_t* strides, const void* mask, int mask_kind, int mask_dt, const int64_t* mask_strides,
                    double sqrt_scale, const float* out_scale, const float* out_offset, double out_num_bits, int64_t splits,
                    void* out, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FFQ_SDPA_DECODE_H */
