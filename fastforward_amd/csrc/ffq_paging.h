// ffq_paging.h — what the paged kernels (kv_paged_store_kernel and kv_paged_token_store_kernel in ffq_kv_cache.hip,
// kv_paged_partial_kernel and kv_paged_token_partial_kernel in ffq_sdpa_decode.hip) share: how a sequence's position is found in a pool of fixed-size pages (include/ffq_kv_paged.h), and the
// alignment rule of the int32 tables (lens, block_table) that the host side of both files checks.
//
// Position `pos` of sequence b lives in pool page table[b][pos >> page_shift] at row pos & (P - 1). A kernel reads a table entry
// only for a position below the sequence's length, and dereferences it only when it lies in [0, num_pages): an entry outside that
// range (a -1 of a page never reserved, a stale index) makes the kernel skip the row, never touch memory.
#pragma once

#include <stdint.h>

namespace ffq {

struct Paging {
  const int32_t* table;  // [batch][table_stride]: the pool page of every logical page
  int64_t table_stride;  // elements between two sequences' rows, >= max_pages
  int32_t num_pages, page_shift;  // P = 1 << page_shift
};

// the pool page of `pos`, or -1 when the table does not place it inside the pool
__device__ __forceinline__ int32_t page_of(const Paging& pg, int64_t b, int64_t pos) {
  const int32_t page = pg.table[b * pg.table_stride + (pos >> pg.page_shift)];
  return (uint32_t)page < (uint32_t)pg.num_pages ? page : -1;
}

// The geometry both entry points refuse, in the documented order; nullptr when it is sound. C = max_pages * P < 2^30 then holds.
inline const char* paging_error(int64_t num_pages, int64_t P, int64_t max_pages, int64_t table_stride) {
  if (P < 16 || P > 256 || (P & (P - 1))) return "the page size P must be a power of two in 16..256";
  if (num_pages < 1 || num_pages >= ((int64_t)1 << 31)) return "num_pages must be in 1..2^31 - 1";
  if (max_pages < 1) return "max_pages must be >= 1";
  if (max_pages >= ((int64_t)1 << 30) / P) return "a sequence's capacity max_pages * P must stay below 2^30";
  if (table_stride < max_pages) return "the block table's row stride is below max_pages";
  return nullptr;
}

// the alignment of the int32 side tables the cache entry points read on the device (lens, block_table); true for nullptr
inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

inline int32_t page_shift_of(int64_t P) {
  int32_t shift = 0;
  while (((int64_t)1 << shift) < P) ++shift;
  return shift;
}

}  // namespace ffq
