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
// kv_token_store_kernel (ffq_kv_token_append, include/ffq_kv_token.h) is the dense body with a dynamic quantizer per row: the E / 16
// neighbouring lanes of a row reduce its min / max (NaN apart, as ffq_minmax_by_tile propagates it) with three DPP steps at most,
// every one of them runs A5 (range_to_parameters: one copy of the arithmetic) on the same pair, quantizes its own 16 elements with A1,
// and the row's first lane writes (k_scale, k_offset, v_scale, v_offset) with one 16-byte store. In the rotary path the lane's 16
// elements are the two 8-element halves it rotated, after their rounding to the data dtype. No LDS, no scratch.
//
// kv_paged_token_store_kernel (ffq_kv_paged_token_append, include/ffq_kv_paged_token.h) is the body with both: the row's codes and its
// four parameters go to row pos % P of page table[b][pos / P] of three pools, and a row whose table entry lies outside the pool is
// dropped before any load, its parameters with it. The reduction, A5, A1 and the one 16-byte store are the dense token kernel's.
//
// Host side: the entry points run the shared rules (check_shape, check_quantizers_and_tables, check_sizes_and_buffers) in the order
// their error tables pin, with their own steps in between, fill() the kernel's arguments and launch through launch_rows.
#include "ffq_affine.h"
#include "ffq_common.h"
#include "ffq_extrema.h"
#include "ffq_paging.h"
#include "ffq_vec.h"

#include "../../include/ffq_kv_cache.h"
#include "../../include/ffq_kv_paged.h"
#include "../../include/ffq_kv_paged_token.h"
#include "../../include/ffq_kv_token.h"

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

// A cache with per-position parameters (include/ffq_kv_token.h): ks / ko / vs / vo are unused, `params` is the fp32 store with the
// (batch, head, row) strides ps, and krange / vrange hold A5's constants of the two dynamic quantizers
struct TokenStoreArgs : AppendArgs {
  float* params;
  int64_t ps[3];
  RangeArgs krange, vrange;
};

// Both (include/ffq_kv_paged_token.h): `params` is the parameter pool and ps its (page, head, row) strides
struct PagedTokenStoreArgs : TokenStoreArgs {
  Paging pg;
};

typedef __attribute__((ext_vector_type(4))) float kv_f32x4;

// min / max of a row's elements; torch.min / torch.max propagate NaN and v_min_f32 / v_max_f32 do not, so NaN travels apart
struct RowRange {
  float mn, mx;
  int nan;
};

template <int N>
__device__ __forceinline__ RowRange range_of(const float (&x)[N]) {
  RowRange m = {INFINITY, -INFINITY, 0};
#pragma unroll
  for (int i = 0; i < N; ++i) {
    m.mn = __builtin_fminf(m.mn, x[i]);
    m.mx = __builtin_fmaxf(m.mx, x[i]);
    m.nan |= x[i] != x[i];
  }
  return m;
}

template <int CTRL>
__device__ __forceinline__ void range_step(RowRange& m) {
  const int mn = __builtin_bit_cast(int, m.mn), mx = __builtin_bit_cast(int, m.mx);
  m.mn = __builtin_fminf(m.mn, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(mn, mn, CTRL, 0xf, 0xf, false)));
  m.mx = __builtin_fmaxf(m.mx, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(mx, mx, CTRL, 0xf, 0xf, false)));
  m.nan |= __builtin_amdgcn_update_dpp(m.nan, m.nan, CTRL, 0xf, 0xf, false);
}

// The butterfly over the 4 (E = 64) or 8 (E = 128) neighbouring lanes that hold one row: every one of them ends with the row's range.
// The lanes of a row are all active here (they leave together: `items` is a multiple of the group and `pos` is uniform over it)
__device__ __forceinline__ void range_over_row(RowRange& m, int chunk_shift) {
  range_step<0xB1>(m);                        // quad_perm [1,0,3,2]: lane ^ 1
  range_step<0x4E>(m);                        // quad_perm [2,3,0,1]: lane ^ 2
  if (chunk_shift == 3) range_step<0x141>(m); // row_half_mirror: lane -> 7 - lane within 8
  if (m.nan) m.mn = m.mx = NAN;
}

// A5 then A1 of this lane's N elements of a row whose range is `m`; returns the row's (scale, rounded offset)
template <int N>
__device__ __forceinline__ void quantize_row_part(const float (&x)[N], const RowRange& m, const RangeArgs& r, float lo, float hi, float& s, float& o,
                                                  Chunk<int8_t, N>& y) {
  range_to_parameters(m.mn, m.mx, 0, r, s, o);
  quantize_chunk_to_bytes<N>(x, s, o, lo, hi, y);
}

// K of one lane, rotated: columns [8 j, +8) of both halves with table row `pos` (the arithmetic both kernels' rotary paths share)
template <typename T, typename Args>
__device__ __forceinline__ void rotate_halves(const Args& a, const T* kn, int64_t pos, int64_t j, float (&ol)[8], float (&oh)[8]) {
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
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float x1 = x1c.get(i), x2 = x2c.get(i);
    const float p = rd<T>(x1 * cl.get(i)), q = rd<T>((-x2) * sl.get(i));
    const float r = rd<T>(x2 * ch.get(i)), t = rd<T>(x1 * sh.get(i));
    ol[i] = rd<T>(p + q);
    oh[i] = rd<T>(r + t);
  }
}

// The rows of ffq_kv_token_append, once a lane knows where its row goes: V, then K (rotated or plain), each reduced over the row,
// turned into parameters and quantized; the row's first lane stores the four parameters
template <typename T, bool ROPE>
__device__ __forceinline__ void token_row(const TokenStoreArgs& a, const T* kn, const T* vn, int8_t* kc, int8_t* vc, float* prm, int64_t pos, int64_t j) {
  float ks, ko, vs, vo;
  {
    Chunk<T, 16> x;
    x.load(vn + j * 16);
    float xf[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) xf[i] = x.get(i);
    RowRange m = range_of<16>(xf);
    range_over_row(m, a.chunk_shift);
    Chunk<int8_t, 16> y;
    quantize_row_part<16>(xf, m, a.vrange, a.vlo, a.vhi, vs, vo, y);
    y.store(vc + j * 16);
  }
  if constexpr (!ROPE) {
    Chunk<T, 16> x;
    x.load(kn + j * 16);
    float xf[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) xf[i] = x.get(i);
    RowRange m = range_of<16>(xf);
    range_over_row(m, a.chunk_shift);
    Chunk<int8_t, 16> y;
    quantize_row_part<16>(xf, m, a.krange, a.klo, a.khi, ks, ko, y);
    y.store(kc + j * 16);
  } else {
    float ol[8], oh[8];
    rotate_halves<T>(a, kn, pos, j, ol, oh);
    RowRange m = range_of<8>(ol);
    const RowRange mh = range_of<8>(oh);
    m.mn = __builtin_fminf(m.mn, mh.mn);
    m.mx = __builtin_fmaxf(m.mx, mh.mx);
    m.nan |= mh.nan;
    range_over_row(m, a.chunk_shift);
    Chunk<int8_t, 8> yl, yh;
    quantize_row_part<8>(ol, m, a.krange, a.klo, a.khi, ks, ko, yl);
    quantize_row_part<8>(oh, m, a.krange, a.klo, a.khi, ks, ko, yh);
    yl.store(kc + j * 8);
    yh.store(kc + a.E / 2 + j * 8);
  }
  if (j == 0) *reinterpret_cast<kv_f32x4*>(prm) = kv_f32x4{ks, ko, vs, vo};
}

// The body of both kernels. PAGED changes where a row's codes go: page table[b][pos / P], row pos % P of the pools; a row whose table
// entry lies outside the pool is dropped like one outside [0, S_max), before any load
// TOKEN (kv_token_store_kernel): the row's parameters are its own, computed here (token_row); with PAGED they go where the codes go,
// row `at` of page `slot` of the parameter pool
template <typename T, bool ROPE, bool PAGED, bool TOKEN = false, typename Args>
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
  if constexpr (TOKEN) {
    token_row<T, ROPE>(a, kn, vn, kc, vc, a.params + slot * a.ps[0] + kvh * a.ps[1] + at * a.ps[2], pos, j);
    return;
  }
  const float ks = a.ks[0], ko = a.ko ? rne(a.ko[0]) : 0.0f;
  const float vs = a.vs[0], vo = a.vo ? rne(a.vo[0]) : 0.0f;

  append16<T>(vn + j * 16, vc + j * 16, vs, vo, a.vlo, a.vhi);
  if constexpr (!ROPE) {
    append16<T>(kn + j * 16, kc + j * 16, ks, ko, a.klo, a.khi);
  } else {
    const int64_t half = a.E / 2;
    float ol[8], oh[8];
    rotate_halves<T>(a, kn, pos, j, ol, oh);
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

// (its name does not hold "kv_append" either)
template <typename T, bool ROPE>
__global__ __launch_bounds__(kBlock) void kv_token_store_kernel(TokenStoreArgs a) {
  append_rows<T, ROPE, false, true>(a);
}

// (its name holds none of the names the other three are counted by)
template <typename T, bool ROPE>
__global__ __launch_bounds__(kBlock) void kv_paged_token_store_kernel(PagedTokenStoreArgs a) {
  append_rows<T, ROPE, true, true>(a);
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

// The two bit-widths
int check_bits(const char* name, double k_num_bits, double v_num_bits) {
  if (!bits_ok(k_num_bits) || !bits_ok(v_num_bits)) return fail(FFQ_ERR_ARG, "%s: the quantizers need an integral bit-width in 2..8", name);
  return FFQ_OK;
}

// The two symmetric flags of dynamic quantizers
int check_symmetric(const char* name, int k_symmetric, int v_symmetric) {
  if ((k_symmetric != 0 && k_symmetric != 1) || (v_symmetric != 0 && v_symmetric != 1))
    return fail(FFQ_ERR_ARG, "%s: symmetric is 0 (scale and offset) or 1 (scale alone)", name);
  return FFQ_OK;
}

// The three strides of a parameter store (entries 12..14), `store` as the entry point names it
int check_param_strides(const char* name, const int64_t* strides, const char* store) {
  for (int i = 12; i < 15; ++i)
    if (strides[i] < 0 || strides[i] % 4) return fail(FFQ_ERR_ARG, "%s: the strides of %s must be non-negative multiples of 16 bytes", name, store);
  return FFQ_OK;
}

// The rotary tables; `positions` is how the entry point words what the tables need a row for
int check_tables(const char* name, const void* cos_table, const void* sin_table, int64_t table_rows, int64_t capacity, const char* positions) {
  if (!cos_table != !sin_table) return fail(FFQ_ERR_ARG, "%s: the rotary tables come as a pair", name);
  if (cos_table && table_rows < capacity)
    return fail(FFQ_ERR_ARG, "%s: the rotary tables need a row for every %s (%lld < %lld)", name, positions, (long long)table_rows, (long long)capacity);
  return FFQ_OK;
}

// The two static quantizers and the rotary tables
int check_quantizers_and_tables(const char* name, const float* k_scale, double k_num_bits, const float* v_scale, double v_num_bits, const void* cos_table,
                                const void* sin_table, int64_t table_rows, int64_t capacity, const char* positions) {
  if (int rc = check_bits(name, k_num_bits, v_num_bits)) return rc;
  if (!k_scale || !v_scale) return fail(FFQ_ERR_ARG, "%s: a quantizer (and its offset) needs its scale", name);
  return check_tables(name, cos_table, sin_table, table_rows, capacity, positions);
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

// what the two entry points with per-position parameters add to fill(): the store (or pool), its strides and A5's constants
void fill_token(TokenStoreArgs& a, void* params, const int64_t* strides, double k_num_bits, int k_symmetric, double v_num_bits, int v_symmetric) {
  a.params = static_cast<float*>(params);
  for (int i = 0; i < 3; ++i) a.ps[i] = strides[12 + i];
  a.krange = make_range_args(FFQ_F32, 1, k_num_bits, k_symmetric, 0, FFQ_F32, FFQ_F32, 1);
  a.vrange = make_range_args(FFQ_F32, 1, v_num_bits, v_symmetric, 0, FFQ_F32, FFQ_F32, 1);
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

extern "C" int ffq_kv_token_append(const void* k_new, const void* v_new, int dt, void* k_cache, void* v_cache, void* params, const void* lens,
                                   int64_t batch, int64_t kv_heads, int64_t L, int64_t S_max, int64_t E, const int64_t* strides, double k_num_bits,
                                   int k_symmetric, double v_num_bits, int v_symmetric, const void* cos_table, const void* sin_table,
                                   int64_t table_rows, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = check_shape("kv_token_append", dt, strides, E, batch, kv_heads, L, S_max)) return rc;
  if (int rc = check_bits("kv_token_append", k_num_bits, v_num_bits)) return rc;
  if (int rc = check_symmetric("kv_token_append", k_symmetric, v_symmetric)) return rc;
  if (int rc = check_tables("kv_token_append", cos_table, sin_table, table_rows, S_max, "cache position")) return rc;
  if (batch == 0 || L == 0) return FFQ_OK;
  if (int rc = check_sizes_and_buffers("kv_token_append", batch, kv_heads, L, S_max, E, strides, {k_new, v_new, k_cache, v_cache, params}, cos_table, sin_table, {lens}, "lens")) return rc;
  if (int rc = check_param_strides("kv_token_append", strides, "params")) return rc;
  if (S_max == 0) return FFQ_OK;  // (no position to write to)

  TokenStoreArgs a;
  fill(a, k_new, v_new, k_cache, v_cache, lens, batch, kv_heads, L, S_max, E, strides, nullptr, nullptr, k_num_bits, nullptr, nullptr, v_num_bits,
       cos_table, sin_table);
  fill_token(a, params, strides, k_num_bits, k_symmetric, v_num_bits, v_symmetric);
  if (dt == FFQ_F16) return launch_rows(kv_token_store_kernel<f16_t, true>, kv_token_store_kernel<f16_t, false>, a, "kv_token_store_kernel", s);
  return launch_rows(kv_token_store_kernel<bf16_t, true>, kv_token_store_kernel<bf16_t, false>, a, "kv_token_store_kernel", s);
}

extern "C" int ffq_kv_paged_token_append(const void* k_new, const void* v_new, int dt, void* k_pool, void* v_pool, void* param_pool, const void* lens,
                                         const void* block_table, int64_t batch, int64_t kv_heads, int64_t L, int64_t num_pages, int64_t P,
                                         int64_t max_pages, int64_t table_stride, int64_t E, const int64_t* strides, double k_num_bits,
                                         int k_symmetric, double v_num_bits, int v_symmetric, const void* cos_table, const void* sin_table,
                                         int64_t table_rows, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = check_shape("kv_paged_token_append", dt, strides, E, batch, kv_heads, L, 0)) return rc;
  if (const char* why = paging_error(num_pages, P, max_pages, table_stride)) return fail(FFQ_ERR_ARG, "kv_paged_token_append: %s", why);
  const int64_t C = max_pages * P;  // a sequence's capacity, in the place of S_max (below 2^30)
  if (int rc = check_bits("kv_paged_token_append", k_num_bits, v_num_bits)) return rc;
  if (int rc = check_symmetric("kv_paged_token_append", k_symmetric, v_symmetric)) return rc;
  if (int rc = check_tables("kv_paged_token_append", cos_table, sin_table, table_rows, C, "position of a sequence")) return rc;
  if (batch == 0 || L == 0) return FFQ_OK;
  if (int rc = check_sizes_and_buffers("kv_paged_token_append", batch, kv_heads, L, C, E, strides, {k_new, v_new, k_pool, v_pool, param_pool}, cos_table,
                                       sin_table, {lens, block_table}, "lens, block_table"))
    return rc;
  if (int rc = check_param_strides("kv_paged_token_append", strides, "param_pool")) return rc;

  PagedTokenStoreArgs a;
  fill(a, k_new, v_new, k_pool, v_pool, lens, batch, kv_heads, L, C, E, strides, nullptr, nullptr, k_num_bits, nullptr, nullptr, v_num_bits, cos_table,
       sin_table);
  fill_token(a, param_pool, strides, k_num_bits, k_symmetric, v_num_bits, v_symmetric);
  a.pg = {static_cast<const int32_t*>(block_table), table_stride, (int32_t)num_pages, page_shift_of(P)};
  if (dt == FFQ_F16)
    return launch_rows(kv_paged_token_store_kernel<f16_t, true>, kv_paged_token_store_kernel<f16_t, false>, a, "kv_paged_token_store_kernel", s);
  return launch_rows(kv_paged_token_store_kernel<bf16_t, true>, kv_paged_token_store_kernel<bf16_t, false>, a, "kv_paged_token_store_kernel", s);
}
