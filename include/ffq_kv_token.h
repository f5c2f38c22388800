/*
 * ffq_kv_token.h — the int8 KV cache of ffq_kv_cache.h with one dynamic (scale, offset) per (sequence, kv head, position) for K and
 * for V: the parameters are computed on the device when a row is appended (A3 of that row, ffq_quantize_dynamic_by_tile with the
 * tile (1, 1, 1, E)) and read back by the decode kernel, so nothing is calibrated ahead of serving and a row of small magnitude keeps
 * all of its bits whatever the largest row of the cache holds.
 *
 * A ninth header, for the reason ffq_kv_paged.h is an eighth one: include/ffq.h is the ABI that BOTH libraries export, pinned at
 * FFQ_ABI_VERSION 9. The entry points below exist in libffq_hip.so only (pointers are DEVICE pointers, `stream` is a hipStream_t), and
 * a caller treats a missing symbol as "not covered". Status codes, dtype tags and every convention of ffq.h and ffq_kv_cache.h hold
 * here unchanged: caller-allocated outputs and workspaces, pure enqueues legal inside hipGraph capture, ffq_last_error(), `lens` read
 * on the device and never written.
 *
 * The parameter store both entry points share:
 *   params   fp32 [batch, kv_heads, S_max, 4]: position pos of (b, kv head) holds (k_scale, k_offset, v_scale, v_offset). The last
 *          dimension is contiguous and every position starts on a 16-byte boundary; three element strides (batch, head, row)
 *          describe the rest, so [batch, S_max, kv_heads, 4] is served as well. They ride at the END of the strides table, which
 *          therefore has 15 entries in both entry points. Offsets are stored already rounded, as A3 returns them, and are 0.0 for a
 *          symmetric quantizer.
 */
#ifndef FFQ_KV_TOKEN_H
#define FFQ_KV_TOKEN_H

#include "ffq_kv_cache.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * ffq_kv_append with a dynamic quantizer per row. One launch: every new row whose position pos = lens[b] - L + l lies in [0, S_max)
 * is rotated (K alone, when tables are given, with the arithmetic of ffq_kv_append: the min / max are taken after the rounding to
 * dt), reduced to its min and max over its E elements (NaN propagates, as in ffq_minmax_by_tile), turned into (scale, offset) by A5
 * with allow_one_sided = 0 and round_offset = 1, and quantized by A1; the codes go to the caches and the position's four parameters
 * to `params`. Codes and parameters are those of ffq_quantize_dynamic_by_tile on the same rows with the tile (1, 1, 1, E) and an
 * int8 container, bit for bit: rows that hold NaN or +-Inf, constant rows (the eps clamp of the scale) and all-zero rows included.
 * A row outside the cache is dropped before any load or store and its parameters stay untouched. k_new / v_new, dt, k_cache /
 * v_cache, lens and the rotary tables are those of ffq_kv_append.
 *   strides   fifteen element strides: (batch, head, row) of k_new, v_new, k_cache, v_cache and params.
 *   k_num_bits / k_symmetric, v_num_bits / v_symmetric   the two dynamic quantizers: an integral bit-width in 2..8; symmetric 0
 *          (scale = max((max - min) / (2^bits - 1), eps), offset = rne(min / scale + 2^(bits-1))) or 1 (scale = max(|min| /
 *          2^(bits-1), |max| / (2^(bits-1) - 1)), offset 0).
 * Errors, in this order, before anything is enqueued: dt (FFQ_ERR_DTYPE); a NULL strides table (FFQ_ERR_ARG); E (FFQ_ERR_ARG); a
 * negative batch / L / S_max or kv_heads < 1 (FFQ_ERR_ARG); a bit-width that is not an integer in 2..8 (FFQ_ERR_ARG); a symmetric
 * flag that is neither 0 nor 1 (FFQ_ERR_ARG); one rotary table without the other (FFQ_ERR_ARG); table_rows < S_max with tables
 * (FFQ_ERR_ARG); then batch == 0 or L == 0 returns FFQ_OK with nothing launched; S_max >= 2^30 or batch * kv_heads * L * E >= 2^40
 * (FFQ_ERR_ARG); a misaligned k_new / v_new / k_cache / v_cache / params / table (16 bytes) or lens (4 bytes) (FFQ_ERR_ARG); a
 * negative stride of the first twelve or one that is not a multiple of 16 bytes (FFQ_ERR_ARG); a NULL k_new / v_new / k_cache /
 * v_cache / params / lens (FFQ_ERR_ARG); a negative stride of params or one that is not a multiple of 16 bytes (FFQ_ERR_ARG). S_max == 0
 * then returns FFQ_OK with nothing launched: there is no position to write to.
 */
int ffq_kv_token_append(const void* k_new, const void* v_new, int dt, void* k_cache, void* v_cache, void* params, const void* lens,
                        int64_t batch, int64_t kv_heads, int64_t L, int64_t S_max, int64_t E, const int64_t* strides, double k_num_bits,
                        int k_symmetric, double v_num_bits, int v_symmetric, const void* cos_table, const void* sin_table,
                        int64_t table_rows, void* stream);

/*
 * ffq_kv_decode over such a cache: key row pos of (b, kv head) is dequantized with its own (k_scale, k_offset), value row pos with
 * its own (v_scale, v_offset), (c + o) * s in fp32 rounded once to dt. q_scale / q_offset (one fp32 element each, nullable) apply to
 * the query alone. Everything else is ffq_kv_decode's: q, q_dt, dt, lens, the split rule and plan_len, the workspace
 * (ffq_sdpa_decode_workspace_bytes(batch, kv_heads, rows, E, the split count)), bottom-right causality, exact zeros for S_b == 0 and
 * for a row without a visible key, the output quantizer and the combine kernel. With every position's parameters equal the result is
 * bit-equal to ffq_kv_decode with that per-tensor dequantization at the same split count. `params` is read, never written; the
 * parameters of positions at or beyond S_b are never read. A row whose scale is NaN makes the output of ITS sequence NaN and no
 * other's (docs/numerics.md has the one corner: a NaN key alone in its 32-key step).
 *   strides   fifteen element strides: (batch, head, row) of q, k, v, then three unused entries (0), then (batch, head, row) of
 *          params: params' strides sit where ffq_kv_token_append has them.
 * Errors, in this order, before anything is enqueued: dt (FFQ_ERR_DTYPE); q_dt neither dt nor FFQ_I8 (FFQ_ERR_DTYPE); a NULL
 * strides table (FFQ_ERR_ARG); int8 q codes without q_scale (FFQ_ERR_DTYPE); a NULL params store, which holds the scales of k and v
 * (FFQ_ERR_ARG); E (FFQ_ERR_ARG); a negative extent, a head count < 1 or q_heads not a multiple of kv_heads (FFQ_ERR_ARG);
 * rows > MAX_ROWS (FFQ_ERR_ARG); causal neither 0 nor 1 (FFQ_ERR_ARG); an output offset without a scale, or an output bit-width that
 * is not an integer in 1..8 (FFQ_ERR_ARG); splits outside 0..MAX_SPLITS (FFQ_ERR_ARG); plan_len outside 0..S_max (FFQ_ERR_ARG); then
 * batch == 0 or L == 0 returns FFQ_OK with nothing launched; S_max == 0 (FFQ_ERR_ARG); S_max >= 2^30 or batch * kv_heads >= 2^24
 * (FFQ_ERR_ARG); a NULL q / k / v / out / lens (FFQ_ERR_ARG); a negative stride of params or one that is not a multiple of 16 bytes
 * (FFQ_ERR_ARG); a misaligned q / k / v / out / params (16 bytes) or lens (4 bytes) (FFQ_ERR_ARG); a negative stride of q / k / v or
 * one that is not a multiple of 16 bytes (FFQ_ERR_ARG); a workspace that is NULL, misaligned or smaller than the size query's figure
 * (FFQ_ERR_WORKSPACE).
 */
int ffq_kv_token_decode(const void* q, int q_dt, const void* k, const void* v, int dt, const float* q_scale, const float* q_offset,
                        const void* params, const void* lens, int64_t batch, int64_t q_heads, int64_t kv_heads, int64_t L, int64_t S_max,
                        int64_t E, const int64_t* strides, int causal, double sqrt_scale, const float* out_scale, const float* out_offset,
                        double out_num_bits, int64_t splits, int64_t plan_len, void* out, void* workspace, size_t workspace_bytes,
                        void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FFQ_KV_TOKEN_H */
