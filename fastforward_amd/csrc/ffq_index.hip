// ffq_index.hip — the reference's quantized index_add and permute as one-pass kernels with A1 fused in.
//
// ff.nn.functional.{index_add, permute} run their generated fallbacks in the reference (_gen/fallback.py: permute :1427,
// index_add :1483): A2 of every quantized input into a data-dtype tensor, the ATen op (for permute a strided view), A1 of the output
// quantizer (which densifies the view first). Here each is one launch under the A2 / A1 contract of ffq_onepass.h.
//   index_add: viewed as x [outer, R, inner] += alpha * src [outer, n, inner] at rows index[n]. Output-stationary: a lane owns one
//        column (8 consecutive elements of one row of `inner`, or one element when 8 does not divide inner) of kRows consecutive rows
//        and keeps their fp32 sums in registers. Every wave walks index[0, n) in order, 64 values per step, and ballots on "this value
//        names one of my rows"; for each set bit, lowest first, the lanes read that source row's column and add it. Ascending j
//        therefore costs nothing: no atomics, no workspace, and the same bits on every run. Out-of-range values never match a row.
//        The walk is ceil(R / kRows) * ceil(n / 64) ballot steps per 256 columns: made for the rows x hidden shapes of a
//        mixture-of-experts combine, not for a long index into a narrow tensor.
//   permute: axes of extent 1 are dropped and axes that stay adjacent are merged (host). If x's innermost axis is still the result's,
//        lanes walk the flattened result and copy row pieces; otherwise 64 x 64 tiles over (the result's innermost axis, x's
//        innermost axis) go through a [64][65]-dword LDS tile: reads run along x's rows, writes along the result's, both coalesced,
//        and the odd leading dimension keeps the column reads of ds_read_b32 (32 banks per half wave) free of conflicts.
#include "ffq_onepass.h"

#include "../../include/ffq_index.h"

namespace ffq {
namespace index {

constexpr int kRows = 4;      // rows of the result a lane accumulates (kRows * 8 fp32 sums in registers)
constexpr int kTile = 64;     // the transposed tile: one wave wide both ways
constexpr int kMaxAxes = 5;   // axes of a permutation outside the innermost one (rank <= 6)

// W (8 or 1) consecutive elements of an operand as values of T held in fp32; the form (0 plain, 1 int8 codes, 2 value-dtype codes)
// is the launch's: a uniform branch.
template <typename T, int W>
__device__ __forceinline__ void load_values(const void* p, int form, size_t at, float s, float o, float (&v)[W]) {
  if constexpr (W == kE) {
    if (form == 0) operand_chunk<T, T, false>(static_cast<const T*>(p) + at, s, o, v);
    else if (form == 1) operand_chunk<T, int8_t, true>(static_cast<const int8_t*>(p) + at, s, o, v);
    else operand_chunk<T, T, true>(static_cast<const T*>(p) + at, s, o, v);
  } else {
    if (form == 0) v[0] = to_f32(element<T, T, false>(static_cast<const T*>(p), at, s, o));
    else if (form == 1) v[0] = to_f32(element<T, int8_t, true>(static_cast<const int8_t*>(p), at, s, o));
    else v[0] = to_f32(element<T, T, true>(static_cast<const T*>(p), at, s, o));
  }
}

// ---------------------------------------------------------------------------------------------------
// I1: index_add + A1. Block = 256 columns x kRows rows; blockIdx = row tile * col_blocks + column block.
//     Algorithmic bytes: x once + every source row once (2 B bf16 / 1 B int8 per element) + per output [2 (z)] + 1 per code tensor,
//     + the index once per wave.
// ---------------------------------------------------------------------------------------------------
struct IndexAdd {
  const void* x;
  const float* xs;
  const float* xo;
  const void* src;
  const float* ss;
  const float* so;
  const void* index;
  uint32_t n, R, inner;
  uint32_t columns;     // outer * per_row
  uint32_t col_blocks;  // ceil(columns / kBlock)
  FastDiv by_per_row;   // columns per row of `inner`
  FastDiv by_col_blocks;
  float alpha;          // rounded to T
  int32_t x_form, src_form, index64;
};

template <typename T, bool VEC>
__global__ __launch_bounds__(kBlock) void index_add_quantize_kernel(IndexAdd a, T* __restrict__ out, FanOut f) {
  constexpr int W = VEC ? kE : 1;
  const FanParams fp = load_fan(f);
  const uint32_t tile = fdiv(blockIdx.x, a.by_col_blocks);
  const uint32_t col = (blockIdx.x - tile * a.col_blocks) * kBlock + threadIdx.x;
  const uint32_t r0 = tile * kRows;
  const bool live = col < a.columns;  // (a lane without a column still takes part in the ballots)
  const uint32_t o = fdiv(col, a.by_per_row);
  const uint32_t within = (col - o * a.by_per_row.div) * W;
  float xs = 1.0f, xo = 0.0f, ss = 1.0f, so = 0.0f;
  if (a.x_form) {
    xs = a.xs[0];
    xo = a.xo ? rne(a.xo[0]) : 0.0f;
  }
  if (a.src_form) {
    ss = a.ss[0];
    so = a.so ? rne(a.so[0]) : 0.0f;
  }
  float acc[kRows][W];
#pragma unroll
  for (int t = 0; t < kRows; ++t) {
#pragma unroll
    for (int i = 0; i < W; ++i) acc[t][i] = 0.0f;
    if (live && r0 + t < a.R) load_values<T, W>(a.x, a.x_form, ((size_t)o * a.R + r0 + t) * a.inner + within, xs, xo, acc[t]);
  }
  const uint32_t lane = threadIdx.x & 63u;
  for (uint32_t j0 = 0; j0 < a.n; j0 += 64) {
    const uint32_t j = j0 + lane;
    int64_t value = -1;
    if (j < a.n) value = a.index64 ? static_cast<const int64_t*>(a.index)[j] : (int64_t)static_cast<const int32_t*>(a.index)[j];
    const int64_t rel = value - (int64_t)r0;
    const bool mine = rel >= 0 && rel < kRows && value < (int64_t)a.R;
    unsigned long long hits = __ballot(mine);
    while (hits) {  // (wave-uniform: lowest j first)
      const int k = __builtin_ctzll(hits);
      hits &= hits - 1;
      const int t = __builtin_amdgcn_readlane((int)rel, k);
      if (live) {
        float v[W], add[W];
        load_values<T, W>(a.src, a.src_form, ((size_t)o * a.n + j0 + k) * a.inner + within, ss, so, v);
#pragma unroll
        for (int i = 0; i < W; ++i) {
          v[i] = v[i] * a.alpha;
          asm volatile("" : "+v"(v[i]));  // (the product in a register of its own, as a2_value: no mul + convert fusion)
        }
        if constexpr (VEC) {
          Chunk<T, kE> h;
          h.pack(v);
          unpack(h, add);
        } else {
          add[0] = round_stage(v[0], TypeTag<T>::value);
        }
#pragma unroll
        for (int q = 0; q < kRows; ++q) {
          if (q == t) {
#pragma unroll
            for (int i = 0; i < W; ++i) acc[q][i] = acc[q][i] + add[i];
          }
        }
      }
    }
  }
  if (!live) return;
#pragma unroll
  for (int t = 0; t < kRows; ++t) {
    if (r0 + t >= a.R) break;
    const size_t at = ((size_t)o * a.R + r0 + t) * a.inner + within;
    if constexpr (VEC) store_chunk<T>(out, f, fp, acc[t], at);
    else store_one<T>(out, f, fp, acc[t][0], at);
  }
}

// ---------------------------------------------------------------------------------------------------
// P1 / P2: permute + A1.
//     Algorithmic bytes: the input once + per output [2 (z)] + 1 per code tensor.
// ---------------------------------------------------------------------------------------------------
// The axes of the result outside the kernel's own one or two, innermost first: a flat index over them gives the offsets.
struct PermAxes {
  int32_t count;
  int32_t chan;  // which of them indexes the parameters, or -1
  FastDiv by[kMaxAxes];
  uint32_t in_stride[kMaxAxes];
  uint32_t out_stride[kMaxAxes];
};

__device__ __forceinline__ void walk(const PermAxes& ax, uint32_t idx, uint32_t& in_at, uint32_t& out_at, uint32_t& chan) {
#pragma unroll
  for (int k = 0; k < kMaxAxes; ++k) {
    if (k >= ax.count) break;
    const uint32_t q = fdiv(idx, ax.by[k]);
    const uint32_t c = idx - q * ax.by[k].div;
    idx = q;
    in_at += c * ax.in_stride[k];
    out_at += c * ax.out_stride[k];
    if (k == ax.chan) chan = c;
  }
}

template <bool DEQ>
__device__ __forceinline__ void params_of(const float* xs, const float* xo, uint32_t p, float& s, float& o) {
  if constexpr (DEQ) {
    s = xs[p];
    o = xo ? rne(xo[p]) : 0.0f;
  }
}

// P1: x's innermost axis stays innermost. A unit is a group of 8 elements of one row (VEC) or one element.
template <typename T, typename TIn, bool DEQ, bool VEC>
__global__ __launch_bounds__(kBlock) void permute_rows_kernel(const TIn* __restrict__ x, const float* __restrict__ xs, const float* __restrict__ xo,
                                                              PermAxes ax, uint32_t units, FastDiv by_row, int32_t chan_inner,
                                                              T* __restrict__ out, FanOut f) {
  constexpr uint32_t kWidth = VEC ? kE : 1;
  const uint32_t u = blockIdx.x * kBlock + threadIdx.x;  // (one unit per lane: the axes and the fan-out fill the scalar registers)
  if (u >= units) return;
  const uint32_t row = fdiv(u, by_row);
  const uint32_t c = u - row * by_row.div;
  uint32_t in_at = 0, unused = 0, chan = 0;
  walk(ax, row, in_at, unused, chan);
  in_at += c * kWidth;
  if (chan_inner) chan = c;  // (element form only: the host keeps such a launch off the group form)
  float s = 1.0f, o = 0.0f;
  params_of<DEQ>(xs, xo, chan, s, o);
  const FanParams fp = load_fan(f);
  const size_t at = (size_t)u * kWidth;
  if constexpr (VEC) put_group<T>(out, f, fp, operand_packed<T, TIn, DEQ>(x + in_at, s, o), at);
  else put_one<T>(out, f, fp, element<T, TIn, DEQ>(x, in_at, s, o), at);
}

// P2: the result's innermost axis A (extent A, x stride a_stride) is not x's innermost axis B (extent B, result stride b_stride).
struct Transpose {
  uint32_t A, B, a_stride, b_stride;
  uint32_t tiles_a, tiles_b;
  FastDiv by_tiles_a, by_tiles_b;
  int32_t chan_kind;  // the parameters are indexed by: 0 nothing (one pair), 1 the A coordinate, 2 the B coordinate, 3 ax.chan
};

template <typename T, typename TIn, bool DEQ>
__global__ __launch_bounds__(kBlock) void permute_transpose_kernel(const TIn* __restrict__ x, const float* __restrict__ xs,
                                                                   const float* __restrict__ xo, PermAxes ax, Transpose g,
                                                                   T* __restrict__ out, FanOut f) {
  __shared__ uint32_t tile[kTile][kTile + 1];  // values of T, one per dword
  const FanParams fp = load_fan(f);
  uint32_t rest = fdiv(blockIdx.x, g.by_tiles_b);
  const uint32_t b0 = (blockIdx.x - rest * g.tiles_b) * kTile;
  const uint32_t batch = fdiv(rest, g.by_tiles_a);
  const uint32_t a0 = (rest - batch * g.tiles_a) * kTile;
  uint32_t in_at = 0, out_at = 0, chan = 0;
  walk(ax, batch, in_at, out_at, chan);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  // read along x's rows: lanes along B
  for (uint32_t i = wave; i < kTile; i += kBlock / 64) {
    const uint32_t a = a0 + i, b = b0 + lane;
    if (a < g.A && b < g.B) {
      float s = 1.0f, o = 0.0f;
      params_of<DEQ>(xs, xo, g.chan_kind == 1 ? a : (g.chan_kind == 2 ? b : chan), s, o);
      const T v = element<T, TIn, DEQ>(x, (size_t)in_at + (size_t)a * g.a_stride + b, s, o);
      tile[i][lane] = (uint32_t)__builtin_bit_cast(uint16_t, v);
    }
  }
  __syncthreads();
  // write along the result's rows: lanes along A
  for (uint32_t i = wave; i < kTile; i += kBlock / 64) {
    const uint32_t b = b0 + i, a = a0 + lane;
    if (a < g.A && b < g.B) put_one<T>(out, f, fp, __builtin_bit_cast(T, (uint16_t)tile[lane][i]), (size_t)out_at + (size_t)b * g.b_stride + a);
  }
}

static unsigned blocks_for(uint64_t units) { return (unsigned)((units + (uint64_t)kBlock - 1) / (uint64_t)kBlock); }

static int operand_form(const float* scale, int x_dt) { return scale ? (x_dt == FFQ_I8 ? 1 : 2) : 0; }

}  // namespace index
}  // namespace ffq

using namespace ffq;
using namespace ffq::index;

extern "C" int ffq_index_add_quantize(const void* x, int x_dt, const float* x_scale, const float* x_offset, const void* index, int index_dt,
                                      int64_t n, const void* src, int src_dt, const float* src_scale, const float* src_offset, double alpha,
                                      int dt, int64_t outer, int64_t R, int64_t inner, void* out, const ffq_fanout* fan, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (!value_dtype(dt)) return fail(FFQ_ERR_DTYPE, "fused index_add is built for bf16 / fp16 values");
  int rc = check_operand_form("fused index_add (input)", x_dt, x_scale, x_offset, false, dt);
  if (rc) return rc;
  rc = check_operand_form("fused index_add (source)", src_dt, src_scale, src_offset, false, dt);
  if (rc) return rc;
  if (index_dt != FFQ_I32 && index_dt != FFQ_I64) return fail(FFQ_ERR_DTYPE, "fused index_add: the index is int32 or int64");
  if (n < 0 || outer < 0 || R < 0 || inner < 0) return fail(FFQ_ERR_ARG, "fused index_add: negative extent");
  const float a = round_stage((float)alpha, dt);  // double -> fp32 -> T, as ATen converts the number
  if (!(a - a == 0.0f)) return fail(FFQ_ERR_ARG, "fused index_add: alpha %g is not finite in the value dtype", alpha);
  const int64_t limit = (int64_t)1 << 31;
  const auto too_many = [&](int64_t rows) {  // (every factor below 2^31 before it is multiplied: no int64 overflow)
    return outer >= limit || rows >= limit || inner >= limit || outer * rows >= limit || outer * rows * inner >= limit;
  };
  if (too_many(R) || too_many(n)) return fail(FFQ_ERR_DTYPE, "fused index_add needs fewer than 2^31 input and source elements");
  const int64_t total = outer * R * inner;
  FanOut f;
  rc = check_launch_args(fan, total, total == 0, x, {x, out}, &f);
  if (rc || total == 0) return rc;
  if (n) {
    if (!index) return fail(FFQ_ERR_ARG, "NULL buffer");
    rc = check_buffers(src, {src});
    if (rc) return rc;
  }
  const bool vec = inner % kE == 0;
  const uint32_t per_row = (uint32_t)(vec ? inner / kE : inner);
  IndexAdd g;
  g.x = x; g.xs = x_scale; g.xo = x_offset;
  g.src = src; g.ss = src_scale; g.so = src_offset;
  g.index = index;
  g.n = (uint32_t)n; g.R = (uint32_t)R; g.inner = (uint32_t)inner;
  g.columns = (uint32_t)outer * per_row;
  g.col_blocks = (g.columns + kBlock - 1) / kBlock;
  g.by_per_row = make_fastdiv(per_row);
  g.by_col_blocks = make_fastdiv(g.col_blocks);
  g.alpha = a;
  g.x_form = operand_form(x_scale, x_dt);
  g.src_form = operand_form(src_scale, src_dt);
  g.index64 = index_dt == FFQ_I64;
  const uint64_t blocks = (uint64_t)g.col_blocks * (uint64_t)((R + kRows - 1) / kRows);  // (< 2^31: no more than one per element)
  dispatch_dtype(dt, [&](auto t) {
    using T = typename decltype(t)::type;
    if (vec) index_add_quantize_kernel<T, true><<<(unsigned)blocks, kBlock, 0, s>>>(g, static_cast<T*>(out), f);
    else index_add_quantize_kernel<T, false><<<(unsigned)blocks, kBlock, 0, s>>>(g, static_cast<T*>(out), f);
  });
  return check_launch("index_add_quantize_kernel");
}

extern "C" int ffq_permute_quantize(const void* x, int x_dt, const float* x_scale, const float* x_offset, int param_axis, int dt, int rank,
                                    const int64_t* shape, const int64_t* dims, void* out, const ffq_fanout* fan, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  constexpr int kMaxRank = kMaxAxes + 1;
  if (!value_dtype(dt)) return fail(FFQ_ERR_DTYPE, "fused permute is built for bf16 / fp16 values");
  int rc = check_operand_form("fused permute", x_dt, x_scale, x_offset, param_axis >= 0, dt);
  if (rc) return rc;
  if (rank < 1 || rank > kMaxRank || !shape || !dims) return fail(FFQ_ERR_ARG, "fused permute takes 1..%d axes, got %d", kMaxRank, rank);
  for (int i = 0; i < rank; ++i)
    if (shape[i] < 0) return fail(FFQ_ERR_ARG, "fused permute: negative extent");
  unsigned seen = 0;
  for (int i = 0; i < rank; ++i) {
    if (dims[i] < 0 || dims[i] >= rank || (seen >> dims[i] & 1u)) return fail(FFQ_ERR_ARG, "fused permute: dims is not a permutation of 0..%d", rank - 1);
    seen |= 1u << dims[i];
  }
  if (param_axis >= rank) return fail(FFQ_ERR_ARG, "fused permute: parameter axis %d of %d axes", param_axis, rank);
  const int64_t limit = (int64_t)1 << 31;
  int64_t total = 1;
  for (int i = 0; i < rank; ++i) {
    if (shape[i] >= limit || total * shape[i] >= limit)
      return fail(FFQ_ERR_DTYPE, "fused permute needs fewer than 2^31 elements");
    total *= shape[i];
  }
  FanOut f;
  rc = check_launch_args(fan, total, total == 0, x, {x, out}, &f);
  if (rc || total == 0) return rc;
  // the result's axes, outermost first: extents of 1 dropped, neighbours that are neighbours in x merged (never the parameters' axis)
  int64_t in_strides[kMaxRank];
  for (int64_t i = rank - 1, run = 1; i >= 0; --i) {
    in_strides[i] = run;
    run *= shape[i];
  }
  struct Axis { uint32_t extent, in_stride; bool chan; } axes[kMaxRank];
  int m = 0;
  for (int i = 0; i < rank; ++i) {
    const int d = (int)dims[i];
    if (shape[d] == 1) continue;
    const Axis next = {(uint32_t)shape[d], (uint32_t)in_strides[d], d == param_axis};
    if (m && !next.chan && !axes[m - 1].chan && axes[m - 1].in_stride == next.in_stride * next.extent) {
      axes[m - 1].extent *= next.extent;
      axes[m - 1].in_stride = next.in_stride;
    } else {
      axes[m++] = next;
    }
  }
  if (m == 0) axes[m++] = {1u, 1u, false};
  uint32_t out_strides[kMaxRank];
  for (int64_t i = m - 1, run = 1; i >= 0; --i) {
    out_strides[i] = (uint32_t)run;
    run *= axes[i].extent;
  }
  const int last = m - 1;
  int inner_of_x = last;  // the axis that is innermost in x
  for (int i = 0; i < m; ++i)
    if (axes[i].in_stride == 1) inner_of_x = i;
  PermAxes ax;
  ax.count = 0;
  ax.chan = -1;
  for (int k = 0; k < kMaxAxes; ++k) {
    ax.by[k] = make_fastdiv(1u);
    ax.in_stride[k] = ax.out_stride[k] = 0u;
  }
  for (int i = last - 1; i >= 0; --i) {  // innermost first
    if (i == inner_of_x) continue;
    if (axes[i].chan) ax.chan = ax.count;
    ax.by[ax.count] = make_fastdiv(axes[i].extent);
    ax.in_stride[ax.count] = axes[i].in_stride;
    ax.out_stride[ax.count] = out_strides[i];
    ++ax.count;
  }
  if (inner_of_x == last) {
    const uint32_t inner = axes[last].extent;
    const bool vec = inner % kE == 0 && !axes[last].chan;
    const uint32_t units = (uint32_t)(vec ? total / kE : total);
    const FastDiv by_row = make_fastdiv(vec ? inner / kE : inner);
    const int32_t chan_inner = axes[last].chan;
    dispatch_input(dt, x_dt, x_scale != nullptr, [&](auto t, auto tin, auto deq) {
      using T = typename decltype(t)::type;
      using TIn = typename decltype(tin)::type;
      if (vec) permute_rows_kernel<T, TIn, decltype(deq)::value, true><<<blocks_for(units), kBlock, 0, s>>>(static_cast<const TIn*>(x), x_scale, x_offset, ax, units, by_row, chan_inner, static_cast<T*>(out), f);
      else permute_rows_kernel<T, TIn, decltype(deq)::value, false><<<blocks_for(units), kBlock, 0, s>>>(static_cast<const TIn*>(x), x_scale, x_offset, ax, units, by_row, chan_inner, static_cast<T*>(out), f);
    });
    return check_launch("permute_rows_kernel");
  }
  Transpose g;
  g.A = axes[last].extent;
  g.a_stride = axes[last].in_stride;
  g.B = axes[inner_of_x].extent;
  g.b_stride = out_strides[inner_of_x];
  g.tiles_a = (g.A + kTile - 1) / kTile;
  g.tiles_b = (g.B + kTile - 1) / kTile;
  g.by_tiles_a = make_fastdiv(g.tiles_a);
  g.by_tiles_b = make_fastdiv(g.tiles_b);
  g.chan_kind = axes[last].chan ? 1 : (axes[inner_of_x].chan ? 2 : (ax.chan >= 0 ? 3 : 0));
  const uint64_t blocks = (uint64_t)(total / ((int64_t)g.A * g.B)) * g.tiles_a * g.tiles_b;  // (< 2^31: no more than one per element)
  dispatch_input(dt, x_dt, x_scale != nullptr, [&](auto t, auto tin, auto deq) {
    using T = typename decltype(t)::type;
    using TIn = typename decltype(tin)::type;
    permute_transpose_kernel<T, TIn, decltype(deq)::value><<<(unsigned)blocks, kBlock, 0, s>>>(static_cast<const TIn*>(x), x_scale, x_offset, ax, g, static_cast<T*>(out), f);
  });
  return check_launch("permute_transpose_kernel");
}
