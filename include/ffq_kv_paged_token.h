/*
 * ffq_kv_paged_token.h — the paged int8 KV cache of ffq_kv_paged.h with the per-position dynamic (scale, offset) of ffq_kv_token.h:
 * the codes live in fixed-size pages of two pools behind a per-sequence block table, and every (sequence, kv head, position) row
 * carries its own parameters in a third pool of the same pages. Nothing is calibrated ahead of serving, a sequence owns only the pages
 * it uses, and a page shared by two sequences shares its parameters with its codes.
 *
 * A tenth header, for the reason ffq_kv_token.h is a ninth one: include/ffq.h is the ABI that BOTH libraries export, pinned at
 * FFQ_ABI_VERSION 9. The entry points below exist in libffq_hip.so only (pointers are DEVICE pointers, `stream` is a hipStream_t), and
 * a caller treats a missing symbol as "not covered". Status codes, dtype tags and every convention of ffq.h, ffq_kv_cache.h,
 * ffq_kv_paged.h and ffq_kv_token.h hold here unchanged: caller-allocated outputs and workspaces, pure enqueues legal inside hipGraph
 * capture, ffq_last_error(), `lens` and the block table read on the device and never written, nothing read on the host.
 *
 * The storage both entry points share: k_pool, v_pool and block_table exactly as ffq_kv_paged.h defines them (P a power of two in
 * 16..256, C = max_pages * P the capacity of a sequence), and
 *   param_pool   fp32 [num_pages, kv_heads, P, 4]: row pos % P of page block_table[b][pos / P] holds (k_scale, k_offset, v_scale,
 *          v_offset) of position pos of sequence b. The last dimension is contiguous and every row starts on a 16-byte boundary;
 *          three element strides (page, head, row) describe the rest, so [num_pages, P, kv_heads, 4] is served as well. They ride at
 *          entries 12..14 of the strides table, where ffq_kv_token.h has the strides of `params`. Offsets are stored already
 *          rounded, as A3 returns them, and are 0.0 for a symmetric quantizer.
 */
#ifndef FFQ_KV_PAGED_TOKEN_H
#define FFQ_KV_PAGED_TOKEN_H

#include "ffq_kv_paged.h"
#include "ffq_kv_token.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * ffq_kv_token_append into pages. One launch: every new row whose position pos = lens[b] - L + l lies in [0, C) and whose table
 * entry block_table[b][pos / P] lies in [0, num_pages) gets the codes and the four parameters ffq_kv_token_append gives that row
 * (K rotated with table row pos before its min and max are taken; NaN, +-Inf, constant and all-zero rows included), written at row
 * pos % P of that page of the three pools. Any other row is dropped before any load or store, its parameters included. k_new / v_new,
 * dt, lens, the two dynamic quantizers and the rotary tables are those of ffq_kv_token_append; the pools, the table and the geometry
 * those of ffq_kv_paged_append.
 *   strides   fifteen element strides: (batch, head, row) of k_new and of v_new, then (page, head, row) of k_pool, v_pool and
 *          param_pool.
 * Errors, in this order, before anything is enqueued: dt (FFQ_ERR_DTYPE); a NULL strides table (FFQ_ERR_ARG); E (FFQ_ERR_ARG); a
 * negative batch / L or kv_heads < 1 (FFQ_ERR_ARG); the paging geometry — P not a power of two in 16..256, num_pages < 1 or >= 2^31,
 * max_pages < 1, max_pages * P >= 2^30, table_stride < max_pages, in that order (FFQ_ERR_ARG); a bit-width that is not an integer in
 * 2..8 (FFQ_ERR_ARG); a symmetric flag that is neither 0 nor 1 (FFQ_ERR_ARG); one rotary table without the other (FFQ_ERR_ARG);
 * table_rows < C with tables (FFQ_ERR_ARG); then batch == 0 or L == 0 returns FFQ_OK with nothing launched; batch * kv_heads * L * E
 * >= 2^40 (FFQ_ERR_ARG); a misaligned k_new / v_new / k_pool / v_pool / param_pool / rotary table (16 bytes) or lens / block_table
 * (4 bytes) (FFQ_ERR_ARG); a negative stride of the first twelve or one that is not a multiple of 16 bytes (FFQ_ERR_ARG); a NULL
 * k_new / v_new / k_pool / v_pool / param_pool / lens / block_table (FFQ_ERR_ARG); a negative stride of param_pool or one that is not
 * a multiple of 16 bytes (FFQ_ERR_ARG).
 */
int ffq_kv_paged_token_append(const void* k_new, const void* v_new, int dt, void* k_pool, void* v_pool, void* param_pool,
                              const void* lens, const void* block_table, int64_t batch, int64_t kv_heads, int64_t L,
                              int64_t num_pages, int64_t P, int64_t max_pages, int64_t table_stride, int64_t E,
                              const int64_t* strides, double k_num_bits, int k_symmetric, double v_num_bits, int v_symmetric,
                              const void* cos_table, const void* sin_table, int64_t table_rows, void* stream);

/*
 * ffq_kv_token_decode over pages: key row pos of (b, kv head) is row pos % P of page block_table[b][pos / P] of k_pool, dequantized
 * with the (k_scale, k_offset) of the same row of param_pool; value rows likewise. The key order, the arithmetic, the LDS and the
 * combine kernel are ffq_kv_token_decode's, with C in the place of S_max: S_b = clamp(lens[b], 0, C), plan_len is a hint in 1..C (0
 * meaning C), the workspace is ffq_sdpa_decode_workspace_bytes(batch, kv_heads, rows, E, the split count). The keys of a table entry
 * outside [0, num_pages) are neither loaded nor scored (-inf, as a bool mask would), and their parameters are not loaded either. The
 * result is bit-equal to ffq_kv_token_decode on the same codes and parameters laid out densely at the same split count, and, with
 * every position's parameters equal, to ffq_kv_paged_decode with that per-tensor dequantization.
 *   strides   fifteen element strides: (batch, head, row) of q, (page, head, row) of k_pool and of v_pool, then three unused entries
 *          (0), then (page, head, row) of param_pool.
 * Errors, in this order, before anything is enqueued: dt (FFQ_ERR_DTYPE); q_dt neither dt nor FFQ_I8 (FFQ_ERR_DTYPE); a NULL
 * strides table (FFQ_ERR_ARG); int8 q codes without q_scale (FFQ_ERR_DTYPE); a NULL param_pool, which holds the scales of k and v
 * (FFQ_ERR_ARG); E (FFQ_ERR_ARG); a negative batch / L, a head count < 1 or q_heads not a multiple of kv_heads (FFQ_ERR_ARG); the
 * paging geometry, as ffq_kv_paged_token_append lists it (FFQ_ERR_ARG); rows > MAX_ROWS (FFQ_ERR_ARG); causal neither 0 nor 1
 * (FFQ_ERR_ARG); an output offset without a scale, or an output bit-width that is not an integer in 1..8 (FFQ_ERR_ARG); splits
 * outside 0..MAX_SPLITS (FFQ_ERR_ARG); plan_len outside 0..C (FFQ_ERR_ARG); then batch == 0 or L == 0 returns FFQ_OK with nothing
 * launched; batch * kv_heads >= 2^24 (FFQ_ERR_ARG); a NULL q / k_pool / v_pool / out / lens / block_table (FFQ_ERR_ARG); a negative
 * stride of param_pool or one that is not a multiple of 16 bytes (FFQ_ERR_ARG); a misaligned q / k_pool / v_pool / out / param_pool
 * (16 bytes) or lens / block_table (4 bytes) (FFQ_ERR_ARG); a negative stride of q / k_pool / v_pool or one that is not a multiple of
 * 16 bytes (FFQ_ERR_ARG); a workspace that is NULL, misaligned or smaller than the size query's figure (FFQ_ERR_WORKSPACE).
 */
int ffq_kv_paged_token_decode(const void* q, int q_dt, const void* k_pool, const void* v_pool, int dt, const float* q_scale,
                              const float* q_offset, const void* param_pool, const void* lens, const void* block_table,
                              int64_t batch, int64_t q_heads, int64_t kv_heads, int64_t L, int64_t num_pages, int64_t P,
                              int64_t max_pages, int64_t table_stride, int64_t E, const int64_t* strides, int causal,
                              double sqrt_scale, const float* out_scale, const float* out_offset, double out_num_bits,
                              int64_t splits, int64_t plan_len, void* out, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FFQ_KV_PAGED_TOKEN_H */
