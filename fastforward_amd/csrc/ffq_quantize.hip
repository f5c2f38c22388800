// ffq_quantize.hip — A1: fastforward::quantize_by_tile on gfx950.
//
// Reference: quantize_by_tile_impl, src/fastforward/quantization/_quantizer_impl.py:144-169
//   q = cast(clamp(round(x / s_t - round(o_t)), -2^(b-1), 2^(b-1)-1))
// The reference runs this as five ATen passes over a tiles_to_rows view (a full copy for strided
// channels). Here it is ONE pass: 16 B per lane in, packed codes out, the tile -> parameter map
// folded into index arithmetic. HBM-bound: 3 B/elem for bf16 -> int8, 4 B/elem for bf16 -> bf16.
//
// Kernel families
//   quantize_stream_kernel   fp32 stages, fp32 parameters, layouts SCALAR / ROWS / CHANNEL(block)
//   quantize_columns_kernel  fp32 stages, fp32 parameters, one channel per COLUMN (PerChannel(-1)):
//                            each lane keeps the parameters of its 8 columns in registers and
//                            walks down the rows, so nothing is re-fetched and nothing is copied
//   quantize_generic_kernel  any dtype mix / any N-d tiling, one element per lane, every
//                            intermediate rounding of the eager chain reproduced
#include "ffq_affine.h"
#include "ffq_common.h"
#include "ffq_quantizer_host.h"
#include "ffq_vec.h"

#include <math.h>

namespace ffq {

struct StreamArgs {
  float lo, hi;
  uint32_t nchunks;
  uint32_t scale_stride;   // 0 when scale is a single broadcast value, else 1
  uint32_t offset_stride;  // same for offset
  FastDiv chunks_per_run;  // ROWS: run / E             CHANNEL: inner / E
  FastDiv channels;        // CHANNEL: number of channels
};

template <int LAYOUT>
__device__ __forceinline__ uint32_t tile_of_chunk(uint32_t chunk, const StreamArgs& a) {
  if constexpr (LAYOUT == LAYOUT_SCALAR) {
    return 0;
  } else if constexpr (LAYOUT == LAYOUT_ROWS) {
    return fdiv(chunk, a.chunks_per_run);
  } else {
    const uint32_t outer = fdiv(chunk, a.chunks_per_run);  // flat / inner
    return outer - fdiv(outer, a.channels) * a.channels.div;
  }
}

// One block = kBlock lanes x U chunks of E elements; chunk c of the block is read by lane
// (c % kBlock) so that every load instruction of a wave covers one contiguous 64 * 16 B span.
template <typename TIn, typename TOut, int LAYOUT, int E, int U, bool HAS_OFFSET, int DIVMODE, int NT = 0>
__global__ __launch_bounds__(kBlock) void quantize_stream_kernel(const TIn* __restrict__ in,
                                                                 TOut* __restrict__ out,
                                                                 const float* __restrict__ scale,
                                                                 const float* __restrict__ offset,
                                                                 StreamArgs a) {
  const uint32_t first = blockIdx.x * (uint32_t)(kBlock * U) + threadIdx.x;
  Chunk<TIn, E> x[U];
  float s[U], o[U];
  // all HBM loads first, then the (L2-resident) parameter loads: nothing below waits in series
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const uint32_t c = first + u * kBlock;
    if (c < a.nchunks) {
      if constexpr (NT & 1) x[u].load_nt(in + (size_t)c * E); else x[u].load(in + (size_t)c * E);
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const uint32_t c = first + u * kBlock;
    s[u] = 1.0f;
    o[u] = 0.0f;
    if (c < a.nchunks) {
      const uint32_t t = tile_of_chunk<LAYOUT>(c, a);
      s[u] = scale[t * a.scale_stride];
      if constexpr (HAS_OFFSET) o[u] = offset[t * a.offset_stride];
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const uint32_t c = first + u * kBlock;
    if (c >= a.nchunks) continue;
    float xf[E];
#pragma unroll
    for (int i = 0; i < E; ++i) xf[i] = x[u].get(i);
    Chunk<TOut, E> y;
    if constexpr (TypeTag<TOut>::value == FFQ_I8 && DIVMODE == 1 && E % 4 == 0) {
      quantize_chunk_to_bytes<E>(xf, s[u], HAS_OFFSET ? rne(o[u]) : 0.0f, a.lo, a.hi, y);  // packed arithmetic, self-checked
    } else {
      float r[E];
      quantize_chunk<DIVMODE, E>(xf, s[u], HAS_OFFSET ? rne(o[u]) : 0.0f, r);
      finalize_chunk<TOut, E>(r, a.lo, a.hi, y);
    }
    if constexpr (NT & 2) y.store_nt(out + (size_t)c * E); else y.store(out + (size_t)c * E);
  }
}


struct ColumnArgs {
  float lo, hi;
  uint32_t col_chunks;   // channels / E
  uint32_t rows;
  uint32_t row_groups;   // rows are visited as row = group + k * row_groups
  uint32_t scale_stride;
  uint32_t offset_stride;
  FastDiv col_chunks_div;
};

// data viewed as [rows, channels]; lane g owns column chunk g % col_chunks for every row of its
// row group. The 2 x E parameters stay in VGPRs across the whole walk.
template <typename TIn, typename TOut, int E, bool HAS_OFFSET>
__global__ __launch_bounds__(kBlock) void quantize_columns_kernel(const TIn* __restrict__ in,
                                                                  TOut* __restrict__ out,
                                                                  const float* __restrict__ scale,
                                                                  const float* __restrict__ offset,
                                                                  ColumnArgs a) {
  const uint32_t g = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  const uint32_t group = fdiv(g, a.col_chunks_div);
  if (group >= a.row_groups) return;
  const uint32_t cc = g - group * a.col_chunks;
  float s[E], o[E];
#pragma unroll
  for (int i = 0; i < E; ++i) {
    s[i] = scale[(cc * E + i) * a.scale_stride];
    o[i] = HAS_OFFSET ? rne(offset[(cc * E + i) * a.offset_stride]) : 0.0f;
  }
  const size_t row_elems = (size_t)a.col_chunks * E;
  for (uint32_t r = group; r < a.rows; r += a.row_groups) {
    const size_t at = (size_t)r * row_elems + (size_t)cc * E;
    Chunk<TIn, E> x;
    x.load(in + at);
    float q[E];
#pragma unroll
    for (int i = 0; i < E; ++i) q[i] = rne(x.get(i) / s[i] - o[i]);
    Chunk<TOut, E> y;
    finalize_chunk<TOut, E>(q, a.lo, a.hi, y);
    y.store(out + at);
  }
}

struct GenericArgs {
  int data_dt, scale_dt, offset_dt, out_dt;
  int div_dt, sub_dt;
  int has_offset;
  int64_t start, count;
  int64_t scale_numel, offset_numel;
  double lo, hi;
  GenericTiling g;
};

// Follows oracle-independent reading of the eager chain: each ATen op evaluates in float opmath
// (double for f64 tensors) and rounds its result into the promoted dtype.
__global__ __launch_bounds__(kBlock) void quantize_generic_kernel(const void* __restrict__ data,
                                                                  const void* __restrict__ scale,
                                                                  const void* __restrict__ offset,
                                                                  void* __restrict__ out, GenericArgs a) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < a.count; k += stride) {
    const int64_t i = a.start + k;
    const int64_t t = generic_tile_of(a.g, i);
    const double xs = load_any(data, a.data_dt, i);
    const double ss = load_any(scale, a.scale_dt, a.scale_numel == 1 ? 0 : t);
    double os = 0.0;
    if (a.has_offset) {
      os = load_any(offset, a.offset_dt, a.offset_numel == 1 ? 0 : t);
      if (dt_is_float(a.offset_dt)) os = rne(os);  // torch.round; identity on integer tensors
    }
    double q;
    if (a.sub_dt == FFQ_F64) {
      double d = (a.div_dt == FFQ_F64) ? xs / ss
                                       : (double)round_stage(round_stage((float)xs, a.div_dt) /
                                                                 round_stage((float)ss, a.div_dt),
                                                             a.div_dt);
      q = clamp_nan(rne(d - os), a.lo, a.hi);
    } else {
      const float x = round_stage((float)xs, a.div_dt);
      const float s = round_stage((float)ss, a.div_dt);
      float d = round_stage(x / s, a.div_dt);
      const float o = round_stage((float)os, a.sub_dt);
      d = round_stage(round_stage(d, a.sub_dt) - o, a.sub_dt);
      q = (double)clamp_nan(rne(d), round_stage((float)a.lo, a.sub_dt), round_stage((float)a.hi, a.sub_dt));
    }
    store_any(out, a.out_dt, i, q);
  }
}

// (-DFFQ_EXPERIMENTS builds) FFQ_DIV_MODE=0 forces the compiler's IEEE division sequence in the streaming kernels;
// the default is the Markstein iteration (bit-identical, see Divider).
static int div_mode() { return experiment_knob("FFQ_DIV_MODE", 1); }

template <typename TIn, typename TOut, int E, int U>
static int launch_stream_u(const AffineCall& c) {
  const StreamArgs a = stream_args<StreamArgs>(c, E);
  const unsigned grid = grid_for(a.nchunks, kBlock * U);
  const TIn* in = static_cast<const TIn*>(c.data);
  TOut* out = static_cast<TOut*>(c.out);
  const float* scale = static_cast<const float*>(c.scale);
  const float* offset = static_cast<const float*>(c.offset);
#define FFQ_LAUNCH_D(LAYOUT, D)                                                                      \
  do {                                                                                               \
    if (offset)                                                                                      \
      quantize_stream_kernel<TIn, TOut, LAYOUT, E, U, true, D><<<grid, kBlock, 0, c.stream>>>(in, out, scale, offset, a); \
    else                                                                                             \
      quantize_stream_kernel<TIn, TOut, LAYOUT, E, U, false, D><<<grid, kBlock, 0, c.stream>>>(in, out, scale, offset, a); \
  } while (0)
  // the IEEE-division form of the streaming kernels exists in tuning builds only (round 4: 1,637 -> ~500 device kernels)
#define FFQ_LAUNCH(LAYOUT)                                                                           \
  do {                                                                                               \
    if constexpr (kExperiments) {                                                                    \
      if (div_mode() == 1) FFQ_LAUNCH_D(LAYOUT, 1); else FFQ_LAUNCH_D(LAYOUT, 0);                    \
    } else {                                                                                         \
      FFQ_LAUNCH_D(LAYOUT, 1);                                                                       \
    }                                                                                                \
  } while (0)
  switch (c.info.layout) {
    case LAYOUT_SCALAR: FFQ_LAUNCH(LAYOUT_SCALAR); break;
    case LAYOUT_ROWS: FFQ_LAUNCH(LAYOUT_ROWS); break;
    default: FFQ_LAUNCH(LAYOUT_CHANNEL); break;
  }
#undef FFQ_LAUNCH
#undef FFQ_LAUNCH_D
  return check_launch("quantize_stream_kernel");
}

template <typename TIn, typename TOut, int E>
static int launch_stream(const AffineCall& c) {
  if constexpr (kExperiments) {
    switch (stream_chunks_per_lane()) {
      case 1: return launch_stream_u<TIn, TOut, E, 1>(c);
      case 4: return launch_stream_u<TIn, TOut, E, 4>(c);
      default: return launch_stream_u<TIn, TOut, E, 2>(c);
    }
  } else {
    return launch_stream_u<TIn, TOut, E, 1>(c);
  }
}

template <typename TIn, typename TOut, int E>
static int launch_columns(const AffineCall& c) {
  const ColumnArgs a = affine_column_args<ColumnArgs>(c, E);
  const TIn* in = static_cast<const TIn*>(c.data);
  TOut* out = static_cast<TOut*>(c.out);
  const float* scale = static_cast<const float*>(c.scale);
  const float* offset = static_cast<const float*>(c.offset);
  if (offset)
    quantize_columns_kernel<TIn, TOut, E, true><<<column_grid(a), kBlock, 0, c.stream>>>(in, out, scale, offset, a);
  else
    quantize_columns_kernel<TIn, TOut, E, false><<<column_grid(a), kBlock, 0, c.stream>>>(in, out, scale, offset, a);
  return check_launch("quantize_columns_kernel");
}

// the kernel stream_route() chose, on the types of this call; 16-element chunks exist for one-byte containers only
template <typename TIn, typename TOut>
static int launch_route(const AffineCall& c, const StreamRoute& route) {
  if (route.kernel == ROUTE_STREAM) {
    if constexpr (sizeof(TOut) == 1) {
      if (route.chunk == 16) return launch_stream<TIn, TOut, 16>(c);
    }
    return launch_stream<TIn, TOut, 8>(c);
  }
  return launch_columns<TIn, TOut, 8>(c);
}

int quantize_impl(const void* data, int data_dt, const void* scale, int scale_dt, int64_t scale_numel,
                  const void* offset, int offset_dt, int64_t offset_numel, const ffq_tiling* tiling,
                  double num_bits, void* out, int out_dt, hipStream_t stream) {
  AffineCall c;
  int rc = analyse(tiling, &c.info);
  if (rc) return rc;
  const int off_dt = offset ? offset_dt : scale_dt;
  if ((rc = check_tags({data_dt, scale_dt, out_dt, off_dt}))) return rc;
  if ((rc = check_param_counts(c.info, scale_numel, offset != nullptr, offset_numel))) return rc;
  const ClampBounds bounds = clamp_bounds(num_bits);
  int div_dt = ffq_promote_types(data_dt, scale_dt);
  if (!dt_is_float(div_dt)) div_dt = FFQ_F32;  // integer / integer is a true division in float
  const int sub_dt = ffq_promote_types(div_dt, off_dt);
  if ((rc = check_container(out_dt, num_bits))) return rc;
  if (c.info.numel == 0) return FFQ_OK;
  if ((rc = check_buffers({data, scale, out}))) return rc;
  c.data = data; c.scale = scale; c.offset = offset; c.out = out;
  c.scale_numel = scale_numel; c.offset_numel = offset_numel;
  c.lo = (float)bounds.lo; c.hi = (float)bounds.hi;
  c.stream = stream;

  // the streaming kernels: fp32 stages + fp32 parameters on a route stream_route() finds; everything else goes to the generic kernel
  int64_t done = 0;
  if (div_dt == FFQ_F32 && sub_dt == FFQ_F32 && scale_dt == FFQ_F32 && off_dt == FFQ_F32) {
    const StreamRoute route = stream_route(c.info, {dt_size(data_dt), dt_size(out_dt), aligned16(data), aligned16(out), !streaming_bits(num_bits), false});
    bool launched = false;
    if (route.kernel != ROUTE_NONE)
      for_float_dtype(data_dt, [&](auto tin) {
        using TIn = typename decltype(tin)::type;
        launched = for_dtype<float, bf16_t, f16_t, int8_t, int16_t, int32_t>(out_dt, [&](auto tout) {
          rc = launch_route<TIn, typename decltype(tout)::type>(c, route);
        });
      });
    if (rc) return rc;
    if (launched) done = route.covered;
  }
  if (done >= c.info.numel) return FFQ_OK;
  GenericArgs a;
  a.data_dt = data_dt; a.scale_dt = scale_dt; a.offset_dt = offset_dt; a.out_dt = out_dt;
  a.div_dt = div_dt; a.sub_dt = sub_dt;
  a.has_offset = offset != nullptr;
  a.start = done; a.count = c.info.numel - done;
  a.scale_numel = scale_numel; a.offset_numel = offset_numel;
  a.lo = bounds.lo; a.hi = bounds.hi;
  a.g = make_generic(tiling);
  quantize_generic_kernel<<<generic_grid(a.count), kBlock, 0, stream>>>(data, scale, offset, out, a);
  return check_launch("quantize_generic_kernel");
}

// A1 for a [rows, cols] weight with one parameter pair per row, int8 container, that also leaves the row sums of the codes
// (the zero-point term of A6) — one pass instead of A1 + a reduction over the codes. cols % 1024 == 0: the 64 chunks of a wave
// lie in one row, so a wave reduces its 1024 codes in registers (v_dot4 on the packed bytes, a shuffle butterfly) and adds one
// int32 to rowsum[row] (integer atomics: exact, order-independent; the caller zeroes the sums). Codes are those of
// quantize_stream_kernel.
template <bool HAS_OFFSET>
__global__ __launch_bounds__(kBlock) void quantize_rows_rowsum_kernel(const bf16_t* __restrict__ in, int8_t* __restrict__ out,
                                                                      const float* __restrict__ scale,
                                                                      const float* __restrict__ offset,
                                                                      int32_t* __restrict__ rowsum, StreamArgs a) {
  const uint32_t c = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  const bool live = c < a.nchunks;  // nchunks % 64 == 0: whole waves are live or not
  Chunk<bf16_t, 16> x;
  if (live) x.load(in + (size_t)c * 16);
  else {
#pragma unroll
    for (int i = 0; i < Chunk<bf16_t, 16>::kWords; ++i) x.w[i] = 0;
  }
  const uint32_t row = fdiv(live ? c : a.nchunks - 1, a.chunks_per_run);
  const float s = scale[row];
  const float o = HAS_OFFSET ? rne(offset[row]) : 0.0f;
  float xf[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) xf[i] = x.get(i);
  Chunk<int8_t, 16> y;
  quantize_chunk_to_bytes<16>(xf, s, o, a.lo, a.hi, y);
  if (live) y.store(out + (size_t)c * 16);
  int sum = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) sum = __builtin_amdgcn_sdot4((int)y.w[i], 0x01010101, sum, false);
  if (!live) sum = 0;
  // wave sum on the VALU (DPP inclusive scan: row_shr 1 / 2 / 4 / 8, then row_bcast15 / row_bcast31): no LDS round trips in
  // a wave that lives for one chunk; lane 63 ends up with the total
  sum += __builtin_amdgcn_update_dpp(0, sum, 0x111, 0xf, 0xf, false);
  sum += __builtin_amdgcn_update_dpp(0, sum, 0x112, 0xf, 0xf, false);
  sum += __builtin_amdgcn_update_dpp(0, sum, 0x114, 0xf, 0xf, false);
  sum += __builtin_amdgcn_update_dpp(0, sum, 0x118, 0xf, 0xf, false);
  sum += __builtin_amdgcn_update_dpp(0, sum, 0x142, 0xa, 0xf, false);
  sum += __builtin_amdgcn_update_dpp(0, sum, 0x143, 0xc, 0xf, false);
  // one atomic per block where its 4 waves share a row (cols % 4096 == 0, or the block does not straddle a row end): 64 waves
  // hammering the 16 sums of one cache line serialise in L2
  __shared__ int wave_sum[4];
  __shared__ uint32_t wave_row[4];
  const uint32_t wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 63 && live) {
    wave_sum[wave] = sum;
    wave_row[wave] = row;
  }
  __syncthreads();
  if (threadIdx.x == 63) {
    // only the LAST block can be short (nchunks % 64 == 0): count the waves this block really has
    const uint32_t waves = min(4u, (a.nchunks - blockIdx.x * (uint32_t)kBlock + 63u) / 64u);
    int acc = wave_sum[0];
    uint32_t cur = wave_row[0];
    for (uint32_t w = 1; w < waves; ++w) {
      if (wave_row[w] != cur) {
        atomicAdd(rowsum + cur, acc);
        acc = 0;
        cur = wave_row[w];
      }
      acc += wave_sum[w];
    }
    atomicAdd(rowsum + cur, acc);
  }
}


// ---- A1 of SEVERAL row-quantized weights in one launch (ffq_quantize_rows_batch) ---------------------------------------------------
// The reference re-quantizes all seven linears' weights of a decoder layer on every forward (nn/linear.py:34): seven launches,
// two of them (k_proj / v_proj, 4 M elements) far too short to reach the streaming rate (34 % of the HBM peak, profiles/r03_micro.md).
// One grid covers all members: every member's chunk count is a multiple of the block size, so a block lies inside ONE member and
// finds it with a handful of scalar compares; the arithmetic is quantize_stream_kernel's ROWS case (bf16 -> int8, one (scale,
// offset) per row, Markstein division).
struct BatchMember {
  const bf16_t* in;
  int8_t* out;
  const float* scale;
  const float* offset;
  int32_t* rowsum;          // ROWSUM: += sum of the member's codes per row (zero on entry; cols % 1024 == 0: a wave lies inside one row)
  uint32_t first_block;     // blocks [first_block, next member's first_block) belong to this member
  FastDiv chunks_per_row;   // cols / 16
};
struct BatchArgs {
  BatchMember m[FFQ_MAX_BATCH];
  int count;
  float lo, hi;
};

// ROWSUM (round 4): the int8 GEMM's zero-point term needs sum_k wq[n, k] of every weight (ffq_linear.hip); taken here from the
// codes while they are in registers (one v_dot4 per 4 codes, a DPP wave sum, at most two atomics per block) it replaces one
// rowsum_i8_kernel launch per linear and forward (224 launches, 2.1 ms of the Llama-3-8B step).
template <bool ROWSUM>
__global__ __launch_bounds__(kBlock) void quantize_rows_batch_kernel(BatchArgs a) {
  int k = 0;
#pragma unroll
  for (int i = 1; i < FFQ_MAX_BATCH; ++i)
    if (i < a.count && blockIdx.x >= a.m[i].first_block) k = i;
  // (k is wave-uniform: the selects below stay in scalar registers)
  const BatchMember& mem = a.m[k];
  const uint32_t c = (blockIdx.x - mem.first_block) * (uint32_t)kBlock + threadIdx.x;
  Chunk<bf16_t, 16> x;
  x.load(mem.in + (size_t)c * 16);
  const uint32_t row = fdiv(c, mem.chunks_per_row);
  const float s = mem.scale[row];
  const float o = mem.offset ? rne(mem.offset[row]) : 0.0f;
  float xf[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) xf[i] = x.get(i);
  Chunk<int8_t, 16> y;
  quantize_chunk_to_bytes<16>(xf, s, o, a.lo, a.hi, y);
  y.store(mem.out + (size_t)c * 16);
  if constexpr (ROWSUM) {
    int sum = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) sum = __builtin_amdgcn_sdot4((int)y.w[i], 0x01010101, sum, false);
    // wave sum on the VALU (DPP inclusive scan, as quantize_rows_rowsum_kernel): lane 63 ends up with the total
    sum += __builtin_amdgcn_update_dpp(0, sum, 0x111, 0xf, 0xf, false);
    sum += __builtin_amdgcn_update_dpp(0, sum, 0x112, 0xf, 0xf, false);
    sum += __builtin_amdgcn_update_dpp(0, sum, 0x114, 0xf, 0xf, false);
    sum += __builtin_amdgcn_update_dpp(0, sum, 0x118, 0xf, 0xf, false);
    sum += __builtin_amdgcn_update_dpp(0, sum, 0x142, 0xa, 0xf, false);
    sum += __builtin_amdgcn_update_dpp(0, sum, 0x143, 0xc, 0xf, false);
    __shared__ int wave_sum[4];
    __shared__ uint32_t wave_row[4];
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 63) {
      wave_sum[wave] = sum;
      wave_row[wave] = row;
    }
    __syncthreads();
    if (threadIdx.x == 63) {  // one atomic per row the block touches (its four waves usually share one)
      int acc = wave_sum[0];
      uint32_t cur = wave_row[0];
      for (uint32_t w = 1; w < 4; ++w) {
        if (wave_row[w] != cur) {
          atomicAdd(mem.rowsum + cur, acc);
          acc = 0;
          cur = wave_row[w];
        }
        acc += wave_sum[w];
      }
      atomicAdd(mem.rowsum + cur, acc);
    }
  }
}


// A1 of a per-tensor quantizer into int8 UNLESS an earlier quantizer's parameters are the same (ffq_affine.h: EarlierCodes) — then the
// launch returns before its first load and `out` keeps whatever it held. Otherwise quantize_stream_kernel's codes (its E = 16 body).
// At most kUnlessSameBlocks blocks striding over the chunks: the launch that does nothing is the common one (siblings that have
// seen the same data agree), and what it costs is its blocks' dispatch — 16384 one-chunk blocks for 16 k tokens x 4096: 6.1 us.
constexpr unsigned kUnlessSameBlocks = 2048;
template <typename TIn>
__global__ __launch_bounds__(kBlock) void quantize_unless_same_kernel(const TIn* __restrict__ in, int8_t* __restrict__ out,
                                                                      const float* __restrict__ scale, const float* __restrict__ offset,
                                                                      const float* __restrict__ scale2, const float* __restrict__ offset2,
                                                                      float lo, float hi, uint32_t nchunks) {
  if (same_parameters(scale, offset, scale2, offset2)) return;
  const float s = scale[0], o = offset ? rne(offset[0]) : 0.0f;
  const uint32_t stride = gridDim.x * (uint32_t)kBlock;
  for (uint32_t c = blockIdx.x * (uint32_t)kBlock + threadIdx.x; c < nchunks; c += 2 * stride) {
    const uint32_t c2 = c + stride;
    Chunk<TIn, 16> x, x2;
    x.load(in + (size_t)c * 16);
    if (c2 < nchunks) x2.load(in + (size_t)c2 * 16);
    float xf[16];
    Chunk<int8_t, 16> y;
#pragma unroll
    for (int i = 0; i < 16; ++i) xf[i] = x.get(i);
    quantize_chunk_to_bytes<16>(xf, s, o, lo, hi, y);
    y.store(out + (size_t)c * 16);
    if (c2 < nchunks) {
#pragma unroll
      for (int i = 0; i < 16; ++i) xf[i] = x2.get(i);
      quantize_chunk_to_bytes<16>(xf, s, o, lo, hi, y);
      y.store(out + (size_t)c2 * 16);
    }
  }
}

}  // namespace ffq

extern "C" int ffq_quantize_by_tile(const void* data, int data_dt, const void* scale, int scale_dt,
                                    int64_t scale_numel, const void* offset, int offset_dt,
                                    int64_t offset_numel, const ffq_tiling* tiling, double num_bits,
                                    void* out, int out_dt, void* stream) {
  return ffq::quantize_impl(data, data_dt, scale, scale_dt, scale_numel, offset, offset_dt, offset_numel,
                            tiling, num_bits, out, out_dt, static_cast<hipStream_t>(stream));
}

extern "C" int ffq_quantize_by_tile_unless_same(const void* data, int data_dt, const float* scale, const float* offset, int64_t numel,
                                                double num_bits, const float* earlier_scale, const float* earlier_offset, int8_t* out,
                                                void* stream) {
  using namespace ffq;
  if (numel < 0) return fail(FFQ_ERR_ARG, "negative extent");
  if (int rc = check_container(FFQ_I8, num_bits)) return rc;
  if (numel == 0) return FFQ_OK;
  if (int rc = check_buffers({data, scale, earlier_scale, out})) return rc;
  if (!integral_bits(num_bits) || numel % 16 != 0 || !fits_chunk_index(numel / 16) || !aligned16(data, out) || !is_f32_bf16_f16(data_dt))
    return fail(FFQ_ERR_DTYPE, "quantize unless same: whole 16-element chunks of f32 / bf16 / f16 data, 16-byte aligned (else ffq_quantize_by_tile)");
  const ClampBounds bounds = clamp_bounds(num_bits);
  const uint32_t nchunks = (uint32_t)(numel / 16);
  unsigned grid = grid_for(nchunks, kBlock);
  if (grid > kUnlessSameBlocks) grid = kUnlessSameBlocks;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const float lo = (float)bounds.lo, hi = (float)bounds.hi;
  switch (data_dt) {
    case FFQ_F32: quantize_unless_same_kernel<float><<<grid, kBlock, 0, s>>>(static_cast<const float*>(data), out, scale, offset, earlier_scale, earlier_offset, lo, hi, nchunks); break;
    case FFQ_BF16: quantize_unless_same_kernel<bf16_t><<<grid, kBlock, 0, s>>>(static_cast<const bf16_t*>(data), out, scale, offset, earlier_scale, earlier_offset, lo, hi, nchunks); break;
    default: quantize_unless_same_kernel<f16_t><<<grid, kBlock, 0, s>>>(static_cast<const f16_t*>(data), out, scale, offset, earlier_scale, earlier_offset, lo, hi, nchunks); break;
  }
  return check_launch("quantize_unless_same_kernel");
}

extern "C" int ffq_quantize_rows_rowsum(const void* data, int data_dt, const float* scale, const float* offset, int64_t rows,
                                        int64_t cols, double num_bits, int8_t* codes, int32_t* rowsum, void* stream) {
  using namespace ffq;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (rows < 0 || cols < 0) return fail(FFQ_ERR_ARG, "negative extent");
  if (data_dt != FFQ_BF16) return fail(FFQ_ERR_DTYPE, "fused weight quantize + row sums is built for bf16 weights");
  if (cols % 1024 != 0) return fail(FFQ_ERR_DTYPE, "fused weight quantize + row sums needs cols %% 1024 == 0");
  if (int rc = check_container(FFQ_I8, num_bits)) return rc;
  // the kernel clamps BEFORE it rounds (quantize_chunk_to_bytes), which equals the reference's round-then-clamp only for integer clamp
  // bounds: a fractional bit width goes back to ffq_quantize_by_tile
  if (!integral_bits(num_bits)) return fail(FFQ_ERR_DTYPE, "fused weight quantize + row sums needs an integral bit width (else ffq_quantize_by_tile)");
  if (rows == 0 || cols == 0) return FFQ_OK;
  if (int rc = check_buffers({data, scale, codes, rowsum})) return rc;
  if (!aligned16(data, codes)) return fail(FFQ_ERR_ARG, "buffers must be 16-byte aligned");
  const int64_t nchunks = rows * cols / 16;
  if (nchunks >= ((int64_t)1 << 32)) return fail(FFQ_ERR_ARG, "too many elements for one launch");
  StreamArgs a;
  const ClampBounds bounds = clamp_bounds(num_bits);
  a.lo = (float)bounds.lo; a.hi = (float)bounds.hi;
  a.nchunks = (uint32_t)nchunks;
  a.scale_stride = 1; a.offset_stride = 1;
  a.chunks_per_run = make_fastdiv((uint32_t)(cols / 16));
  a.channels = make_fastdiv(1);
  const unsigned grid = (unsigned)((nchunks + kBlock - 1) / kBlock);
  if (offset) quantize_rows_rowsum_kernel<true><<<grid, kBlock, 0, s>>>(static_cast<const bf16_t*>(data), codes, scale, offset, rowsum, a);
  else quantize_rows_rowsum_kernel<false><<<grid, kBlock, 0, s>>>(static_cast<const bf16_t*>(data), codes, scale, offset, rowsum, a);
  return check_launch("quantize_rows_rowsum_kernel");
}

extern "C" int ffq_quantize_rows_batch(const ffq_rows_batch* batch, int data_dt, void* stream) {
  using namespace ffq;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (!batch || batch->count < 0 || batch->count > FFQ_MAX_BATCH) return fail(FFQ_ERR_ARG, "batch count must be 0..%d", FFQ_MAX_BATCH);
  if (batch->count == 0) return FFQ_OK;
  if (data_dt != FFQ_BF16) return fail(FFQ_ERR_DTYPE, "batched weight quantization is built for bf16 weights");
  if (int rc = check_container(FFQ_I8, batch->num_bits)) return rc;
  if (!integral_bits(batch->num_bits))  // clamp-before-round needs integer bounds (see ffq_quantize_rows_rowsum)
    return fail(FFQ_ERR_DTYPE, "batched weight quantization needs an integral bit width (else ffq_quantize_by_tile per weight)");
  BatchArgs a;
  a.count = batch->count;
  const ClampBounds bounds = clamp_bounds(batch->num_bits);
  a.lo = (float)bounds.lo; a.hi = (float)bounds.hi;
  uint64_t blocks = 0;
  const bool rowsums = batch->rowsum[0] != nullptr;
  for (int i = 0; i < batch->count; ++i) {
    const int64_t rows = batch->rows[i], cols = batch->cols[i];
    if ((batch->rowsum[i] != nullptr) != rowsums) return fail(FFQ_ERR_ARG, "row sums for every member of the batch or for none");
    if (rowsums && cols % 1024 != 0) return fail(FFQ_ERR_DTYPE, "batched weight quantization with row sums needs cols %% 1024 == 0");
    if (rows <= 0 || cols <= 0 || cols % 16 != 0 || (rows * cols / 16) % kBlock != 0)
      return fail(FFQ_ERR_DTYPE, "batched weight quantization needs rows * cols %% %d == 0 and cols %% 16 == 0", 16 * kBlock);
    if (!batch->data[i] || !batch->scale[i] || !batch->codes[i]) return fail(FFQ_ERR_ARG, "NULL buffer in batch member %d", i);
    if (!aligned16(batch->data[i], batch->codes[i])) return fail(FFQ_ERR_ARG, "buffers must be 16-byte aligned");
    a.m[i].in = static_cast<const bf16_t*>(batch->data[i]);
    a.m[i].out = batch->codes[i];
    a.m[i].scale = batch->scale[i];
    a.m[i].offset = batch->offset[i];
    a.m[i].rowsum = batch->rowsum[i];
    a.m[i].first_block = (uint32_t)blocks;
    a.m[i].chunks_per_row = make_fastdiv((uint32_t)(cols / 16));
    blocks += (uint64_t)(rows * cols / 16) / kBlock;
    if (blocks >= ((uint64_t)1 << 31)) return fail(FFQ_ERR_ARG, "too many elements for one launch");
  }
  for (int i = batch->count; i < FFQ_MAX_BATCH; ++i) a.m[i] = a.m[0];
  if (rowsums) quantize_rows_batch_kernel<true><<<(unsigned)blocks, kBlock, 0, s>>>(a);
  else quantize_rows_batch_kernel<false><<<(unsigned)blocks, kBlock, 0, s>>>(a);
  return check_launch("quantize_rows_batch_kernel");
}
