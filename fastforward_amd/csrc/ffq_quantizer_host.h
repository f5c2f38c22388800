// ffq_quantizer_host.h — the host side the quantizer core shares (ffq_quantize.hip, ffq_dequantize.hip, ffq_minmax.hip, ffq_pack.hip,
// ffq_backward.hip): the argument rules of their entry points, the route of the A1 / A2 streaming kernels, the fillers of their
// argument structs, the workspace layout of the dynamic quantizer, the dtype dispatch and the experiment knobs. Host code only —
// nothing here reaches a code object.
//
// Every helper states one rule once and knows nothing of its caller. The ORDER of an entry point's checks is part of its contract
// (include/ffq.h; tests/golden/quantizer_refusals.json pins it together with the statuses and the words), so each helper is one
// step of that order and the entry points call them in the order they always had.
#pragma once

#include "ffq_common.h"
#include "ffq_vec.h"

#include <initializer_list>
#include <math.h>
#include <stdlib.h>

namespace ffq {

// ---- argument rules ------------------------------------------------------------------------------------------------------------

inline int check_tags(std::initializer_list<int> tags) {
  for (int dt : tags)
    if (!dt_valid(dt)) return fail(FFQ_ERR_ARG, "bad dtype tag");
  return FFQ_OK;
}

inline int check_buffers(std::initializer_list<const void*> buffers) {
  for (const void* p : buffers)
    if (!p) return fail(FFQ_ERR_ARG, "NULL buffer");
  return FFQ_OK;
}

// scale[:, None] and offset[:, None] against the rows of the tiled view; an empty tensor has no rows to broadcast against
inline int check_param_counts(const TileInfo& info, int64_t scale_numel, bool has_offset, int64_t offset_numel) {
  if (info.numel == 0) return FFQ_OK;
  if (int rc = check_param_numel("scale", scale_numel, info.ntiles)) return rc;
  return has_offset ? check_param_numel("offset", offset_numel, info.ntiles) : FFQ_OK;
}

inline int check_container(int dt, double num_bits) {
  if (ffq_can_support_bitwidth(dt, num_bits)) return FFQ_OK;
  return fail(FFQ_ERR_PRECISION, "Provided dtype (%d) is not enough to store %g bits quantized values.", dt, num_bits);
}

// numel elements in whole blocks of an even number of codes (two nibbles per byte)
inline int check_pack_block(int64_t numel, int64_t block) {
  if (block <= 0 || (block & 1) || numel < 0 || numel % block) return fail(FFQ_ERR_ARG, "numel %% block != 0 or odd block");
  return FFQ_OK;
}

// min_threshold = -(2 ** (num_bits - 1)); max_threshold = -min_threshold - 1      (_quantizer_impl.py:158-159)
struct ClampBounds { double lo, hi; };
inline ClampBounds clamp_bounds(double num_bits) {
  const double lo = -pow(2.0, num_bits - 1.0);
  return {lo, -lo - 1.0};
}

// the kernels that clamp BEFORE they round (quantize_chunk_to_bytes) equal the reference's round-then-clamp only for integer bounds
inline bool integral_bits(double num_bits) { return num_bits == floor(num_bits) && num_bits >= 1; }
// what the fp32 streaming kernels take: bounds a float holds exactly, and nobody asked for the element-wise kernels
inline bool streaming_bits(double num_bits) { return integral_bits(num_bits) && num_bits <= 32 && !generic_kernels_forced(); }

inline uint32_t param_stride(int64_t numel) { return numel == 1 ? 0u : 1u; }  // 0: one value broadcast over the tiles

inline bool is_f32_bf16_f16(int dt) { return dt == FFQ_F32 || dt == FFQ_BF16 || dt == FFQ_F16; }

inline bool aligned16(const void* a, const void* b) { return aligned16(a) && aligned16(b); }

// the streaming kernels index 16-byte chunks with 32 bits (4096: room for the last block's overshoot)
inline bool fits_chunk_index(int64_t numel) { return numel < ((int64_t)1 << 32) - 4096; }

// one element per lane, at most 8192 blocks striding over the rest
inline unsigned generic_grid(int64_t items) {
  const int64_t blocks = (items + kBlock - 1) / kBlock;
  return (unsigned)(blocks > 8192 ? 8192 : blocks);
}

inline unsigned grid_for(int64_t work_items, int per_block) {
  const int64_t blocks = (work_items + per_block - 1) / per_block;
  return (unsigned)(blocks < 1 ? 1 : blocks);
}

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// ---- dtype tag -> template argument ---------------------------------------------------------------------------------------------
// for_dtype<float, bf16_t>(dt, [&](auto t) { using T = typename decltype(t)::type; ... }) calls the functor with the type whose tag
// is dt and returns true, or returns false when dt is none of them. The types are tried, and instantiated, in the order given
// (a LEFT fold: the compiler expands a right fold from its last element, which would emit the kernels in reverse).
template <typename T> struct TypeOf { using type = T; };
template <typename... Ts, typename F>
inline bool for_dtype(int dt, F&& f) {
  return (... || (dt == TypeTag<Ts>::value ? (f(TypeOf<Ts>{}), true) : false));
}
template <typename F> inline bool for_float_dtype(int dt, F&& f) { return for_dtype<float, bf16_t, f16_t>(dt, f); }

// ---- experiment knobs -------------------------------------------------------------------------------------------------------------
// The library reads NO environment variables; a -DFFQ_EXPERIMENTS build (tools/build_experiments.sh, docs/experiments.md) reads
// integer launch parameters here. `fallback` is what the product does.
#ifdef FFQ_EXPERIMENTS
constexpr bool kExperiments = true;
inline int experiment_knob(const char* name, int fallback) {
  const char* e = getenv(name);
  return e ? atoi(e) : fallback;
}
#else
constexpr bool kExperiments = false;
inline int experiment_knob(const char*, int fallback) { return fallback; }
#endif

// ---- A1 / A2: what quantize_impl / dequantize_impl hand to everything below them ------------------------------------------------------
struct AffineCall {
  const void* data;
  const void* scale;
  const void* offset;  // NULL: none
  void* out;
  int64_t scale_numel, offset_numel;
  TileInfo info;
  float lo, hi;  // A1's clamp bounds
  hipStream_t stream;
};

// ---- the route of the streaming kernels ---------------------------------------------------------------------------------------------------
// fp32 stages and fp32 parameters are the caller's business; here: 16 B alignment and a layout whose tiles never split a chunk.
// STREAM covers `covered` elements in chunks of `chunk`, COLUMNS (one channel per column, PerChannel(-1)) covers everything, and the
// generic kernel takes the rest: [covered, numel).
enum { ROUTE_NONE = 0, ROUTE_STREAM, ROUTE_COLUMNS };
struct StreamRoute {
  int kernel;
  int chunk;        // elements per lane and load: 16 or 8
  int64_t covered;
};
struct StreamQuery {
  int in_size, out_size;  // bytes per element
  bool in_aligned, out_aligned;
  bool forced_generic;
  bool wide_codes;        // FFQ_DQ_E16: one-byte inputs in 16-element chunks too
};

inline int64_t stream_covers(const TileInfo& info, int chunk) {
  const bool whole_chunks = info.layout == LAYOUT_SCALAR || (info.layout == LAYOUT_ROWS && info.run % chunk == 0) ||
                            (info.layout == LAYOUT_CHANNEL && info.inner % chunk == 0);
  if (!whole_chunks) return 0;
  // only the SCALAR layout can leave a tail (numel % chunk); ROWS / CHANNEL tiles are whole chunks
  return info.layout == LAYOUT_SCALAR ? info.numel / chunk * chunk : info.numel;
}

inline StreamRoute stream_route(const TileInfo& info, const StreamQuery& q) {
  if (q.forced_generic || !fits_chunk_index(info.numel) || !q.in_aligned || !q.out_aligned) return {ROUTE_NONE, 0, 0};
  // One-byte containers use 16-element chunks so that the store is 16 B per lane as well. One-byte CODES stay at 8 per chunk:
  // an 8 B load and ONE dense 16 B store per lane beats 16 codes per chunk (16 B load, two half-dense 16 B stores): 30.1 vs
  // 32.1 us on [14336, 4096] int8 -> bf16 (FFQ_DQ_E16=1 to compare)
  if (q.out_size == 1 || (q.in_size == 1 && q.wide_codes))
    if (const int64_t covered = stream_covers(info, 16)) return {ROUTE_STREAM, 16, covered};
  if (const int64_t covered = stream_covers(info, 8)) return {ROUTE_STREAM, 8, covered};
  if (info.layout == LAYOUT_CHANNEL && info.inner == 1 && info.channels % 8 == 0) return {ROUTE_COLUMNS, 8, info.numel};
  return {ROUTE_NONE, 0, 0};
}

// chunks per lane of the streaming kernels: measured on MI355X (interleaved A/B): short blocks win. Also measured and rejected for
// 2-byte -> 1-byte: two coalesced 16-B loads per lane (chunks l and l + 64) with a lane-pair exchange into 16-B stores (4.2-5.3 TB/s)
// or with two 8-B stores (4.1-5.4 TB/s) against 6.0 TB/s for the 16-element chunk —
// bf16 -> int8 [14336, 4096]: E=16/U=1 29.2 us vs E=16/U=2 32.4 us vs E=8/U=4 34.3 us; U=1 also wins for
// bf16 -> bf16 (38.5 vs 41.0 us at U=4) and per-tensor activations (33.2 vs 39.2 us); A2 finds the same.
// One in the product; FFQ_STREAM_U = 2 / 4 in tuning builds only (the product instantiates the one form it launches).
inline int stream_chunks_per_lane() {
  const int u = experiment_knob("FFQ_STREAM_U", 1);
  return u == 0 ? 1 : u;
}

// ---- argument structs ---------------------------------------------------------------------------------------------------------------------
template <typename Args>
inline auto set_bounds(Args& a, const AffineCall& c, int) -> decltype(a.lo, void()) { a.lo = c.lo; a.hi = c.hi; }
template <typename Args>
inline void set_bounds(Args&, const AffineCall&, long) {}

template <typename Args>
inline void set_params(Args& a, const AffineCall& c) {
  a.scale_stride = param_stride(c.scale_numel);
  a.offset_stride = param_stride(c.offset_numel);
  set_bounds(a, c, 0);
}

// StreamArgs / DqStreamArgs for chunks of E elements
template <typename Args>
inline Args stream_args(const AffineCall& c, int E) {
  Args a;
  set_params(a, c);
  a.nchunks = (uint32_t)(c.info.numel / E);
  const bool rows = c.info.layout == LAYOUT_ROWS, channel = c.info.layout == LAYOUT_CHANNEL;
  a.chunks_per_run = make_fastdiv(rows ? (uint32_t)(c.info.run / E) : channel ? (uint32_t)(c.info.inner / E) : 1u);
  a.channels = make_fastdiv(channel ? (uint32_t)c.info.channels : 1u);
  return a;
}

// rows of a [rows, channels] view are visited as row = group + k * groups: `rows_per_lane` rows amortise what a lane keeps per
// column, never more groups than `cap`, never none
inline uint32_t row_groups(uint32_t rows, uint32_t rows_per_lane, uint32_t cap) {
  const uint32_t groups = (rows + rows_per_lane - 1) / rows_per_lane;
  return groups > cap ? cap : groups < 1 ? 1 : groups;
}
inline uint32_t column_rows(const TileInfo& info) { return (uint32_t)(info.numel / info.channels); }

// the fields ColumnArgs / DqColumnArgs / ColsArgs share; the grid is one lane per (row group, column chunk)
template <typename Args>
inline Args column_args(const TileInfo& info, int E, uint32_t groups) {
  Args a;
  a.col_chunks = (uint32_t)(info.channels / E);
  a.rows = column_rows(info);
  a.row_groups = groups;
  a.col_chunks_div = make_fastdiv(a.col_chunks);
  return a;
}
template <typename Args>
inline unsigned column_grid(const Args& a) { return grid_for((int64_t)((uint64_t)a.row_groups * a.col_chunks), kBlock); }

// A1 / A2: ~8 rows per lane amortise the 2 * E parameter loads
template <typename Args>
inline Args affine_column_args(const AffineCall& c, int E) {
  Args a = column_args<Args>(c.info, E, row_groups(column_rows(c.info), 8, UINT32_MAX));
  set_params(a, c);
  return a;
}

// ---- dynamic quantize: [ minmax scratch | min (ntiles, data dtype) | max (ntiles, data dtype) ] -------------------------------------------
struct DynamicWorkspace {
  size_t scratch, min, max;  // offsets; the scratch (the reduction's, then A5's) is `min` bytes long
  size_t total;
};
inline DynamicWorkspace dynamic_workspace(size_t minmax_bytes, size_t a5_bytes, int64_t ntiles, int data_dt) {
  size_t mm = minmax_bytes;  // (a multiple of 256 already)
  if (mm < align256(a5_bytes)) mm = align256(a5_bytes);
  const size_t ranges = align256((size_t)ntiles * dt_size(data_dt));
  return {0, mm, mm + ranges, mm + 2 * ranges};
}

}  // namespace ffq
