/*
 * ffq_kv_cache.h — a preallocated int8 KV cache: the new tokens quantized and written in place, and attention for a short query
 * over the cache with every sequence's length on the device.
 *
 * A seventh header, for the reason ffq_sdpa_decode.h is a sixth one: include/ffq.h is the ABI that BOTH libraries export, pinned at
 * FFQ_ABI_VERSION 9. The entry points below exist in libffq_hip.so only (pointers are DEVICE pointers, `stream` is a hipStream_t), and
 * a caller treats a missing symbol as "not covered". Status codes, dtype tags and every convention of ffq.h (caller-allocated outputs
 * and workspaces, pure enqueues legal inside hipGraph capture, ffq_last_error()) hold here unchanged. Neither entry point reads `lens`
 * on the host and neither writes it: the caller advances it with an ordinary add on the stream, so a captured step can be replayed
 * while the sequences grow.
 */
#ifndef FFQ_KV_CACHE_H
#define FFQ_KV_CACHE_H

#include "ffq_sdpa_decode.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * One launch: A1 of the new K and V rows, their int8 codes written into the caches at every sequence's own position.
 *   k_new, v_new   [batch, kv_heads, L, E] plain values, dt = FFQ_BF16 | FFQ_F16, E in {64, 128}.
 *   k_cache, v_cache   int8 [batch, kv_heads, S_max, E].
 *   strides   twelve element strides, (batch, head, row) of k_new, v_new, k_cache, v_cache; the last dimension is contiguous and
 *          every row starts on a 16-byte boundary.
 *   lens   int32 [batch], contiguous: the length of sequence b INCLUDING the L rows of this call. Row l goes to position
 *          pos = lens[b] - L + l; a row with pos < 0 or pos >= S_max is skipped (neither an error nor a fault).
 *   k_scale / k_offset / k_num_bits, v_scale / v_offset / v_num_bits   the two per-tensor static quantizers: one fp32 element each
 *          (offsets nullable), an integral bit-width in 2..8. code = clamp(rne(x / scale - rne(offset)), -2^(bits-1), 2^(bits-1) - 1)
 *          with the correctly rounded quotient and a separately rounded subtraction: the codes of ffq_quantize_by_tile on the same
 *          tensor, NaN and +-Inf included.
 *   cos_table, sin_table   both NULL, or [table_rows, E] contiguous in dt with table_rows >= S_max: K (alone) is rotated with table
 *          row pos before it is quantized: rd(rd(x1 cos_lo) + rd(-x2 sin_lo)) and rd(rd(x2 cos_hi) + rd(x1 sin_hi)), rd rounding to dt
 *          (ffq_rope_inplace's arithmetic in bf16, ATen's x * cos + rotate_half(x) * sin in fp16).
 * Errors, in this order, before anything is enqueued: dt (FFQ_ERR_DTYPE); a NULL strides table (FFQ_ERR_ARG); E (FFQ_ERR_ARG); a
 * negative batch / L / S_max or kv_heads < 1 (FFQ_ERR_ARG); a bit-width that is not an integer in 2..8 (FFQ_ERR_ARG); a quantizer
 * without its scale, an offset without its scale included (FFQ_ERR_ARG); one rotary table without the other (FFQ_ERR_ARG);
 * table_rows < S_max with tables (FFQ_ERR_ARG); then batch == 0 or L == 0 returns FFQ_OK with nothing launched; S_max >= 2^30 or
 * batch * kv_heads * L * E >= 2^40 (FFQ_ERR_ARG); a misaligned k_new / v_new / k_cache / v_cache / table (16 bytes) or lens (4 bytes),
 * a negative stride or one that is not a multiple of 16 bytes (FFQ_ERR_ARG); a NULL k_new / v_new / k_cache / v_cache / lens
 * (FFQ_ERR_ARG).
 */
int ffq_kv_append(const void* k_new, const void* v_new, int dt, void* k_cache, void* v_cache, const void* lens, int64_t batch,
                  int64_t kv_heads, int64_t L, int64_t S_max, int64_t E, const int64_t* strides, const float* k_scale,
                  const float* k_offset, double k_num_bits, const float* v_scale, const float* v_offset, double v_num_bits,
                  const void* cos_table, const void* sin_table, int64_t table_rows, void* stream);

/*
 * ffq_sdpa_decode over a cache whose lengths live on the device: q [batch, q_heads, L, E], k / v int8 [batch, kv_heads, S_max, E],
 * out [batch, q_heads, L, E]; operands, strides, dequantization, sqrt_scale, the output quantizer and the workspace are those of
 * ffq_sdpa_decode (the same two kernels). What differs:
 *   lens   int32 [batch], contiguous. Sequence b attends to keys [0, S_b), S_b = clamp(lens[b], 0, S_max). Each batch cuts its own
 *          S_b keys over the launch's split count on the device: ceil(ceil(S_b / KEY_TILE) / splits) tiles per split; a split
 *          without keys contributes nothing. S_b == 0 gives exact zeros for that batch.
 *   splits / plan_len   splits 0: ffq_sdpa_decode_splits(batch, kv_heads, plan_len, rows, E), a pure function of host integers;
 *          plan_len is a hint in 1..S_max, 0 meaning S_max. splits 1 .. MAX_SPLITS: forced. The workspace is
 *          ffq_sdpa_decode_workspace_bytes(batch, kv_heads, rows, E, that count).
 *   causal 0: every one of the S_b keys. 1: bottom-right — row l sees key <= l + (S_b - L); a row without a visible key
 *          (l < L - S_b) gives exact zeros.
 * Errors, in this order, before anything is enqueued: dt (FFQ_ERR_DTYPE); q_dt neither dt nor FFQ_I8 (FFQ_ERR_DTYPE); a NULL
 * strides / deq_scale / deq_offset table (FFQ_ERR_ARG); int8 q codes without a scale (FFQ_ERR_DTYPE); k or v without a scale
 * (FFQ_ERR_ARG); E (FFQ_ERR_ARG); a negative extent, a head count < 1 or q_heads not a multiple of kv_heads (FFQ_ERR_ARG);
 * rows > MAX_ROWS (FFQ_ERR_ARG); causal neither 0 nor 1 (FFQ_ERR_ARG); an output offset without a scale, or an output bit-width that
 * is not an integer in 1..8 (FFQ_ERR_ARG); splits outside 0..MAX_SPLITS (FFQ_ERR_ARG); plan_len outside 0..S_max (FFQ_ERR_ARG); then
 * batch == 0 or L == 0 returns FFQ_OK with nothing launched; S_max == 0 (FFQ_ERR_ARG); S_max >= 2^30 or batch * kv_heads >= 2^24
 * (FFQ_ERR_ARG); a NULL q / k / v / out / lens (FFQ_ERR_ARG); a misaligned q / k / v / out (16 bytes) or lens (4 bytes)
 * (FFQ_ERR_ARG); a negative stride or one that is not a multiple of 16 bytes (FFQ_ERR_ARG); a workspace that is NULL, misaligned
 * or smaller than the size query's figure (FFQ_ERR_WORKSPACE).
 */
int ffq_kv_decode(const void* q, int q_dt, const void* k, const void* v, int dt, const float* const* deq_scale,
                  const float* const* deq_offset, const void* lens, int64_t batch, int64_t q_heads, int64_t kv_heads, int64_t L,
                  int64_t S_max, int64_t E, const int64_t* strides, int causal, double sqrt_scale, const float* out_scale,
                  const float* out_offset, double out_num_bits, int64_t splits, int64_t plan_len, void* out, void* workspace,
                  size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FFQ_KV_CACHE_H */
