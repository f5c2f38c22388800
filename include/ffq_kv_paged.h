/*
 * ffq_kv_paged.h — the int8 KV cache of ffq_kv_cache.h held in fixed-size pages: two pools of pages shared by every sequence and a
 * per-sequence block table, so that a sequence owns only the pages it uses, a finished sequence's pages go to another without a
 * copy, and two sequences can point at the same prefix pages.
 *
 * An eighth header, for the reason ffq_kv_cache.h is a seventh one: include/ffq.h is the ABI that BOTH libraries export, pinned at
 * FFQ_ABI_VERSION 9. The entry points below exist in libffq_hip.so only (pointers are DEVICE pointers, `stream` is a hipStream_t), and
 * a caller treats a missing symbol as "not covered". Status codes, dtype tags and every convention of ffq.h and ffq_kv_cache.h hold
 * here unchanged: caller-allocated outputs and workspaces, pure enqueues legal inside hipGraph capture, ffq_last_error(), `lens` read
 * on the device and never written. Nothing reads the block table on the host either.
 *
 * The layout both entry points share:
 *   k_pool, v_pool   int8 pages, `num_pages` of them, each of P rows of E codes for every one of kv_heads heads. Three element
 *          strides (page, head, row) describe each pool and the last dimension E is contiguous, so [num_pages, kv_heads, P, E] and
 *          [num_pages, P, kv_heads, E] are both served. P, the page size, is a power of two in 16..256. Every stride is
 *          non-negative and a multiple of 16 bytes, every pool base 16-byte aligned.
 *   block_table   int32 [batch, max_pages], `table_stride` elements from one sequence's row to the next, 4-byte aligned. Sequence b
 *          has the capacity C = max_pages * P; its position pos lives in page block_table[b][pos / P] at row pos % P. Entries for
 *          pages at or beyond ceil(S_b / P) are never read. An entry in use that lies outside [0, num_pages) never makes a kernel
 *          touch memory: the append drops that row, the decode treats those keys as masked (score -inf), exactly as if a bool mask
 *          hid them. That is a property of the kernels, not an error return: nothing reads the table on the host.
 */
#ifndef FFQ_KV_PAGED_H
#define FFQ_KV_PAGED_H

#include "ffq_kv_cache.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * ffq_kv_append into pages. One launch: A1 of the new K and V rows, their int8 codes written into the pools at every sequence's
 * own position. k_new / v_new, dt, lens, the two quantizers and the rotary tables are those of ffq_kv_append, and so are the codes
 * (the rotation takes table row pos); C stands in the place of S_max:
 *   strides   twelve element strides: (batch, head, row) of k_new and of v_new, then (page, head, row) of k_pool and of v_pool.
 *   lens   int32 [batch]: the length of sequence b INCLUDING the L rows of this call. Row l goes to pos = lens[b] - L + l; a row with
 *          pos < 0 or pos >= C, or whose table entry lies outside [0, num_pages), is skipped (neither an error nor a fault).
 *   cos_table, sin_table   both NULL, or [table_rows, E] contiguous in dt with table_rows >= C.
 * Errors, in this order, before anything is enqueued: dt (FFQ_ERR_DTYPE); a NULL strides table (FFQ_ERR_ARG); E (FFQ_ERR_ARG); a
 * negative batch / L or kv_heads < 1 (FFQ_ERR_ARG); the paging geometry — P not a power of two in 16..256, num_pages < 1 or >= 2^31,
 * max_pages < 1, max_pages * P >= 2^30, table_stride < max_pages, in that order (FFQ_ERR_ARG); a bit-width that is not an integer in
 * 2..8 (FFQ_ERR_ARG); a quantizer without its scale, an offset without its scale included (FFQ_ERR_ARG); one rotary table without the
 * other (FFQ_ERR_ARG); table_rows < C with tables (FFQ_ERR_ARG); then batch == 0 or L == 0 returns FFQ_OK with nothing launched;
 * batch * kv_heads * L * E >= 2^40 (FFQ_ERR_ARG); a misaligned k_new / v_new / k_pool / v_pool / rotary table (16 bytes) or lens /
 * block_table (4 bytes) (FFQ_ERR_ARG); a negative stride or one that is not a multiple of 16 bytes (FFQ_ERR_ARG); a NULL k_new /
 * v_new / k_pool / v_pool / lens / block_table (FFQ_ERR_ARG).
 */
int ffq_kv_paged_append(const void* k_new, const void* v_new, int dt, void* k_pool, void* v_pool, const void* lens, const void* block_table,
                        int64_t batch, int64_t kv_heads, int64_t L, int64_t num_pages, int64_t P, int64_t max_pages, int64_t table_stride,
                        int64_t E, const int64_t* strides, const float* k_scale, const float* k_offset, double k_num_bits,
                        const float* v_scale, const float* v_offset, double v_num_bits, const void* cos_table, const void* sin_table,
                        int64_t table_rows, void* stream);

/*
 * ffq_kv_decode over pages: q [batch, q_heads, L, E], out [batch, q_heads, L, E]; q, dt, the dequantization tables, lens, causal,
 * sqrt_scale, the output quantizer, splits, plan_len and the workspace are those of ffq_kv_decode with C in the place of S_max:
 * S_b = clamp(lens[b], 0, C), plan_len is a hint in 1..C (0 meaning C), the workspace is
 * ffq_sdpa_decode_workspace_bytes(batch, kv_heads, rows, E, the split count).
 *   strides   nine element strides: (batch, head, row) of q, then (page, head, row) of k_pool and of v_pool.
 * The arithmetic and the key order are ffq_kv_decode's: the result is bit-equal to ffq_kv_decode on the same codes laid out densely,
 * at the same split count (and to ffq_sdpa_decode with a bool mask over the keys of table entries outside the pool).
 * Errors, in this order, before anything is enqueued: dt (FFQ_ERR_DTYPE); q_dt neither dt nor FFQ_I8 (FFQ_ERR_DTYPE); a NULL
 * strides / deq_scale / deq_offset table (FFQ_ERR_ARG); int8 q codes without a scale (FFQ_ERR_DTYPE); k or v without a scale
 * (FFQ_ERR_ARG); E (FFQ_ERR_ARG); a negative batch / L, a head count < 1 or q_heads not a multiple of kv_heads (FFQ_ERR_ARG); the
 * paging geometry, as ffq_kv_paged_append lists it (FFQ_ERR_ARG); rows > MAX_ROWS (FFQ_ERR_ARG); causal neither 0 nor 1
 * (FFQ_ERR_ARG); an output offset without a scale, or an output bit-width that is not an integer in 1..8 (FFQ_ERR_ARG); splits
 * outside 0..MAX_SPLITS (FFQ_ERR_ARG); plan_len outside 0..C (FFQ_ERR_ARG); then batch == 0 or L == 0 returns FFQ_OK with nothing
 * launched; batch * kv_heads >= 2^24 (FFQ_ERR_ARG); a NULL q / k_pool / v_pool / out / lens / block_table (FFQ_ERR_ARG); a misaligned
 * q / k_pool / v_pool / out (16 bytes) or lens / block_table (4 bytes) (FFQ_ERR_ARG); a negative stride or one that is not a multiple
 * of 16 bytes (FFQ_ERR_ARG); a workspace that is NULL, misaligned or smaller than the size query's figure (FFQ_ERR_WORKSPACE).
 */
int ffq_kv_paged_decode(const void* q, int q_dt, const void* k_pool, const void* v_pool, int dt, const float* const* deq_scale,
                        const float* const* deq_offset, const void* lens, const void* block_table, int64_t batch, int64_t q_heads,
                        int64_t kv_heads, int64_t L, int64_t num_pages, int64_t P, int64_t max_pages, int64_t table_stride, int64_t E,
                        const int64_t* strides, int causal, double sqrt_scale, const float* out_scale, const float* out_offset,
                        double out_num_bits, int64_t splits, int64_t plan_len, void* out, void* workspace, size_t workspace_bytes,
                        void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FFQ_KV_PAGED_H */
