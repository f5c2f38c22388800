// ffq_kv_cache.hip — the new K and V rows of a decode step (or of a prompt) quantized and written into a preallocated int8 cache, one
// launch for both tensors (include/ffq_kv_cache.h). ffq_kv_decode, the attention over such a cache, lives beside the kernels it runs
// (ffq_sdpa_decode.hip).
//
// kv_append_kernel: one lane = 16 elements of one new row (batch b, kv head, l) of K and the same 16 of V. The row's position is
// pos = lens[b] - L + l: `lens` is read, never written (the caller has advanced it with an ordinary add on the stream), so no
// workgroup races another on it; a row whose position falls outside [0, S_max) is dropped before any load.
//   * plain: the lane takes columns [16 j, +16) of both tensors: two 16-byte loads and one 16-byte store each;
//   * rotary: for K the lane takes [8 j, +8) of BOTH halves (rope_kernel's split, ffq_producers.hip), so it holds x1 and x2 of the
//     eight rotations it computes: rd(rd(x1 cos_lo) + rd(-x2 sin_lo)), rd(rd(x2 cos_hi) + rd(x1 sin_hi)) with the table row `pos`,
//     rd rounding to the data dtype; 16-byte loads, two 8-byte stores. V goes the plain way.
// A1 is quantize_chunk_to_bytes (ffq_affine.h): the codes of ffq_quantize_by_tile, NaN and +-Inf included. Every index is 64-bit.
// No LDS, no scratch.
//
// kv_paged_store_kernel (ffq_kv_paged_append, include/ffq_kv_paged.h) is the same body with the caches held in fixed-size pages of two
// pools: the lane reads the sequence's block table once (page table[b][pos / P]) and writes row pos % P of that page; a table entry
// outside [0, num_pages) drops the row. The codes, the rotation (table row `pos`) and the resources are the dense kernel's.
//
// Host side: both entry points run the shared rules (check_shape, check_quantizers_and_tables, check_sizes_and_buffers) in the order
// their error tables pin, with their own steps in between, fill() the kernel's arguments and launch through launch_rows.
#include "ffq_affine.h"
#include "ffq_common.h"
#include "ffq_paging.h"
#include "ffq_vec.h"

#include "../../include/ffq_kv_cache.h"
#include "../../include/ffq_kv_paged.h"

#include <math.h>

#include <initializer_list>

namespace ffq {
namespace {

struct AppendArgs {
  const void* kn;
  const void* vn;
  int8_t* kc;
  int8_t* vc;
  const int32_t* lens;
  const void* cos;
  const void* sin;
  const float* ks;
  const float* ko;  // nullable
  const float* vs;
  const float* vo;  // nullable
  int64_t kns[3], vns[3], kcs[3], vcs[3];  // element strides of (batch, head, row)
  int64_t items;                           // batch * kv_heads * L * (E / 16)
  int64_t L;                               // (not capped: a prompt goes through the same call)
  int32_t HKV, S_max, E, chunk_shift;      // E / 16 = 1 << chunk_shift
  float klo, khi, vlo, vhi;
};

template <typename T>
__device__ __forceinline__ float rd(float v) {
  return to_f32(from_f32<T>(v));
}

// 16 contiguous values -> 16 codes
template <typename T>
__device__ __forceinline__ void append16(const T* src, int8_t* dst, float s, float o, float lo, float hi) {
  Chunk<T, 16> x;
  x.load(src);
  float xf[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) xf[i] = x.get(i);
  Chunk<int8_t, 16> y;
  quantize_chunk_to_bytes<16>(xf, s, o, lo, hi, y);
  y.store(dst);
}

// Paged caches (include/ffq_kv_paged.h, ffq_paging.h): kc / vc are the pools, kcs / vcs their (page, head, row) strides, S_max the
// capacity max_pages * P of a sequence
struct PagedStoreArgs : AppendArgs {
  Paging pg;
};

// The body of both kernels. PAGED changes where a row's codes go: page table[b][pos / P], row pos % P of the pools; a row whose table
// entry lies outside the pool is dropped like one outside [0, S_max), before any load
template <typename T, bool ROPE, bool PAGED, typename Args>
__device__ __forceinline__ void append_rows(const Args& a) {
  const int64_t item = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (item >= a.items) return;
  const int64_t j = item & (((int64_t)1 << a.chunk_shift) - 1);
  const int64_t row = item >> a.chunk_shift;
  const int64_t l = row % a.L, bh = row / a.L;
  const int64_t kvh = bh % a.HKV, b = bh / a.HKV;
  const int64_t pos = (int64_t)a.lens[b] - a.L + l;
  if (pos < 0 || pos >= a.S_max) return;

  const T* kn = static_cast<const T*>(a.kn) + b * a.kns[0] + kvh * a.kns[1] + l * a.kns[2];
  const T* vn = static_cast<const T*>(a.vn) + b * a.vns[0] + kvh * a.vns[1] + l * a.vns[2];
  int64_t slot = b, at = pos;  // the cache's first and third index
  if constexpr (PAGED) {
    slot = page_of(a.pg, b, pos);
    if (slot < 0) return;
    at = pos & (((int64_t)1 << a.pg.page_shift) - 1);
  }
  int8_t* kc = a.kc + slot * a.kcs[0] + kvh * a.kcs[1] + at * a.kcs[2];
  int8_t* vc = a.vc + slot * a.vcs[0] + kvh * a.vcs[1] + at * a.vcs[2];
  const float ks = a.ks[0], ko = a.ko ? rne(a.ko[0]) : 0.0f;
  const float vs = a.vs[0], vo = a.vo ? rne(a.vo[0]) : 0.0f;

  append16<T>(vn + j * 16, vc + j * 16, vs, vo, a.vlo, a.vhi);
  if constexpr (!ROPE) {
    append16<T>(kn + j * 16, kc + j * 16, ks, ko, a.klo, a.khi);
  } else {
    const int64_t half = a.E / 2;
    const T* cr = static_cast<const T*>(a.cos) + pos * a.E;
    const T* sr = static_cast<const T*>(a.sin) + pos * a.E;
    Chunk<T, 8> x1c, x2c, cl, ch, sl, sh;
    x1c.load(kn + j * 8);
    x2c.load(kn + half + j * 8);
    cl.load(cr + j * 8);
    ch.load(cr + half + j * 8);
    sl.load(sr + j * 8);
    sh.load(sr + half + j * 8);
    float ol[8], oh[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float x1 = x1c.get(i), x2 = x2c.get(i);
      const float p = rd<T>(x1 * cl.get(i)), q = rd<T>((-x2) * sl.get(i));
      const float r = rd<T>(x2 * ch.get(i)), t = rd<T>(x1 * sh.get(i));
      ol[i] = rd<T>(p + q);
      oh[i] = rd<T>(r + t);
    }
    Chunk<int8_t, 8> yl, yh;
    quantize_chunk_to_bytes<8>(ol, ks, ko, a.klo, a.khi, yl);
    quantize_chunk_to_bytes<8>(oh, ks, ko, a.klo, a.khi, yh);
    yl.store(kc + j * 8);
    yh.store(kc + half + j * 8);
  }
}

template <typename T, bool ROPE>
__global__ __launch_bounds__(kBlock) void kv_append_kernel(AppendArgs a) {
  append_rows<T, ROPE, false>(a);
}

// (its name does not hold "kv_append": tests count the dense kernels by that)
template <typename T, bool ROPE>
__global__ __launch_bounds__(kBlock) void kv_paged_store_kernel(PagedStoreArgs a) {
  append_rows<T, ROPE, true>(a);
}

bool bits_ok(double bits) { return bits >= 2.0 && bits <= 8.0 && bits == (double)(int)bits; }

// Each rule of the two entry points once: it takes the entry point's name for its message and returns the first failing status. An
// entry point calls them in the order its error table pins (tests/test_kv_cache_cpu.py, tests/test_kv_paged_cpu.py) with its own
// steps in between. `capacity` is S_max, or max_pages * P.
// The value dtype, the strides table, E and the extents
int check_shape(const char* name, int dt, const int64_t* strides, int64_t E, int64_t batch, int64_t kv_heads, int64_t L, int64_t capacity) {
  if (dt != FFQ_BF16 && dt != FFQ_F16) return fail(FFQ_ERR_DTYPE, "%s: bf16 or fp16 values", name);
  if (!strides) return fail(FFQ_ERR_ARG, "%s: NULL strides table", name);
  if (E != 64 && E != 128) return fail(FFQ_ERR_ARG, "%s: E must be 64 or 128", name);
  if (batch < 0 || L < 0 || capacity < 0 || kv_heads <= 0) return fail(FFQ_ERR_ARG, "%s: bad extent", name);
  return FFQ_OK;
}

// The two quantizers and the rotary tables; `positions` is how the entry point words what the tables need a row for
int check_quantizers_and_tables(const char* name, const float* k_scale, double k_num_bits, const float* v_scale, double v_num_bits, const void* cos_table,
                                const void* sin_table, int64_t table_rows, int64_t capacity, const char* positions) {
  if (!bits_ok(k_num_bits) || !bits_ok(v_num_bits)) return fail(FFQ_ERR_ARG, "%s: the quantizers need an integral bit-width in 2..8", name);
  if (!k_scale || !v_scale) return fail(FFQ_ERR_ARG, "%s: a quantizer (and its offset) needs its scale", name);
  if (!cos_table != !sin_table) return fail(FFQ_ERR_ARG, "%s: the rotary tables come as a pair", name);
  if (cos_table && table_rows < capacity)
    return fail(FFQ_ERR_ARG, "%s: the rotary tables need a row for every %s (%lld < %lld)", name, positions, (long long)table_rows, (long long)capacity);
  return FFQ_OK;
}

// The sizes, the alignment, the twelve strides, then the NULL check. `rows`: the new rows and the caches (16-byte aligned, not NULL);
// `words`: the entry point's int32 tables (4-byte aligned, not NULL), `named` as its message names them; the rotary pair may be NULL
int check_sizes_and_buffers(const char* name, int64_t batch, int64_t kv_heads, int64_t L, int64_t capacity, int64_t E, const int64_t* strides,
                            std::initializer_list<const void*> rows, const void* cos_table, const void* sin_table,
                            std::initializer_list<const void*> words, const char* named) {
  if (capacity >= ((int64_t)1 << 30) || batch >= ((int64_t)1 << 31) || kv_heads >= ((int64_t)1 << 31) || L >= ((int64_t)1 << 40) ||
      (double)batch * (double)kv_heads * (double)L * (double)E >= 0x1p40)
    return fail(FFQ_ERR_ARG, "%s: too large", name);
  bool aligned = aligned16(cos_table) && aligned16(sin_table), present = true;
  for (const void* p : rows) { aligned &= aligned16(p); present &= p != nullptr; }
  for (const void* p : words) { aligned &= aligned4(p); present &= p != nullptr; }
  if (!aligned) return fail(FFQ_ERR_ARG, "%s: buffers must be 16-byte aligned (%s: 4-byte)", name, named);
  for (int i = 0; i < 12; ++i)
    if (strides[i] < 0 || strides[i] % (i < 6 ? 8 : 16)) return fail(FFQ_ERR_ARG, "%s: strides must be non-negative multiples of 16 bytes", name);
  if (!present) return fail(FFQ_ERR_ARG, "%s: NULL buffer", name);
  return FFQ_OK;
}

// one launch: `rotary` / `plain` are the dense or the paged kernel's two instantiations at the call's dtype
template <typename Args>
int launch_rows(void (*rotary)(Args), void (*plain)(Args), const Args& a, const char* what, hipStream_t s) {
  auto kernel = a.cos ? rotary : plain;
  kernel<<<(unsigned)((a.items + kBlock - 1) / kBlock), kBlock, 0, s>>>(a);
  return check_launch(what);
}

// what both entry points fill once their checks have passed (`capacity`: S_max, or max_pages * P)
void fill(AppendArgs& a, const void* k_new, const void* v_new, void* k_cache, void* v_cache, const void* lens, int64_t batch, int64_t kv_heads,
          int64_t L, int64_t capacity, int64_t E, const int64_t* strides, const float* k_scale, const float* k_offset, double k_num_bits,
          const float* v_scale, const float* v_offset, double v_num_bits, const void* cos_table, const void* sin_table) {
  a.kn = k_new; a.vn = v_new;
  a.kc = static_cast<int8_t*>(k_cache); a.vc = static_cast<int8_t*>(v_cache);
  a.lens = static_cast<const int32_t*>(lens);
  a.cos = cos_table; a.sin = sin_table;
  a.ks = k_scale; a.ko = k_offset; a.vs = v_scale; a.vo = v_offset;
  for (int i = 0; i < 3; ++i) {
    a.kns[i] = strides[i]; a.vns[i] = strides[3 + i]; a.kcs[i] = strides[6 + i]; a.vcs[i] = strides[9 + i];
  }
  a.L = L; a.HKV = (int32_t)kv_heads; a.S_max = (int32_t)capacity; a.E = (int32_t)E;
  a.chunk_shift = E == 64 ? 2 : 3;
  a.items = batch * kv_heads * L * (E / 16);
  const double khalf = ldexp(1.0, (int)k_num_bits - 1), vhalf = ldexp(1.0, (int)v_num_bits - 1);
  a.klo = (float)-khalf; a.khi = (float)(khalf - 1.0);
  a.vlo = (float)-vhalf; a.vhi = (float)(vhalf - 1.0);
}

}  // namespace
}  // namespace ffq

using namespace ffq;

extern "C" int ffq_kv_append(const void* k_new, const void* v_new, int dt, void* k_cache, void* v_cache, const void* lens, int64_t batch,
                             int64_t kv_heads, int64_t L, int64_t S_max, int64_t E, const int64_t* strides, const float* k_scale,
                             const float* k_offset, double k_num_bits, const float* v_scale, const float* v_offset, double v_num_bits,
                             const void* cos_table, const void* sin_table, int64_t table_rows, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = check_shape("kv_append", dt, strides, E, batch, kv_heads, L, S_max)) return rc;
  if (int rc = check_quantizers_and_tables("kv_append", k_scale, k_num_bits, v_scale, v_num_bits, cos_table, sin_table, table_rows, S_max, "cache position")) return rc;
  if (batch == 0 || L == 0) return FFQ_OK;
  if (int rc = check_sizes_and_buffers("kv_append", batch, kv_heads, L, S_max, E, strides, {k_new, v_new, k_cache, v_cache}, cos_table, sin_table, {lens}, "lens")) return rc;
  if (S_max == 0) return FFQ_OK;  // (no position to write to)

  AppendArgs a;
  fill(a, k_new, v_new, k_cache, v_cache, lens, batch, kv_heads, L, S_max, E, strides, k_scale, k_offset, k_num_bits, v_scale, v_offset, v_num_bits,
       cos_table, sin_table);
  if (dt == FFQ_F16) return launch_rows(kv_append_kernel<f16_t, true>, kv_append_kernel<f16_t, false>, a, "kv_append_kernel", s);
  return launch_rows(kv_append_kernel<bf16_t, true>, kv_append_kernel<bf16_t, false>, a, "kv_append_kernel", s);
}

extern "C" int ffq_kv_paged_append(const void* k_new, const void* v_new, int dt, void* k_pool, void* v_pool, const void* lens, const void* block_table,
                                   int64_t batch, int64_t kv_heads, int64_t L, int64_t num_pages, int64_t P, int64_t max_pages, int64_t table_stride,
                                   int64_t E, const int64_t* strides, const float* k_scale, const float* k_offset, double k_num_bits,
                                   const float* v_scale, const float* v_offset, double v_num_bits, const void* cos_table, const void* sin_table,
                                   int64_t table_rows, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = check_shape("kv_paged_append", dt, strides, E, batch, kv_heads, L, 0)) return rc;
  if (const char* why = paging_error(num_pages, P, max_pages, table_stride)) return fail(FFQ_ERR_ARG, "kv_paged_append: %s", why);
  const int64_t C = max_pages * P;  // a sequence's capacity, in the place of S_max (below 2^30)
  if (int rc = check_quantizers_and_tables("kv_paged_append", k_scale, k_num_bits, v_scale, v_num_bits, cos_table, sin_table, table_rows, C, "position of a sequence")) return rc;
  if (batch == 0 || L == 0) return FFQ_OK;
  if (int rc = check_sizes_and_buffers("kv_paged_append", batch, kv_heads, L, C, E, strides, {k_new, v_new, k_pool, v_pool}, cos_table, sin_table,
                                       {lens, block_table}, "lens, block_table"))
    return rc;

  PagedStoreArgs a;
  fill(a, k_new, v_new, k_pool, v_pool, lens, batch, kv_heads, L, C, E, strides, k_scale, k_offset, k_num_bits, v_scale, v_offset, v_num_bits,
       cos_table, sin_table);
  a.pg = {static_cast<const int32_t*>(block_table), table_stride, (int32_t)num_pages, page_shift_of(P)};
  if (dt == FFQ_F16) return launch_rows(kv_paged_store_kernel<f16_t, true>, kv_paged_store_kernel<f16_t, false>, a, "kv_paged_store_kernel", s);
  return launch_rows(kv_paged_store_kernel<bf16_t, true>, kv_paged_store_kernel<bf16_t, false>, a, "kv_paged_store_kernel", s);
}
