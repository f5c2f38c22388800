// ffq_dequantize.hip — A2: fastforward::dequantize_by_tile on gfx950.
//
// Reference: dequantize_by_tile_impl, src/fastforward/quantization/_quantizer_impl.py:172-190
//   x^ = cast((q + round(o_t)) * s_t)
// Reference cost: add, mul, _to_copy passes with fp32 temporaries. Here: one pass, 16 B per lane.
// HBM-bound: 3 B/elem for int8 -> bf16, 4 B/elem for a bf16 container.
//
// The add and the multiply are two separately rounded fp32 operations (no FMA), and `q + 0.0f` is
// kept when there is no offset because it turns -0.0 into +0.0 exactly like the eager chain.
#include "ffq_common.h"
#include "ffq_quantizer_host.h"
#include "ffq_vec.h"

namespace ffq {

struct DqStreamArgs {
  uint32_t nchunks;
  uint32_t scale_stride;
  uint32_t offset_stride;
  FastDiv chunks_per_run;
  FastDiv channels;
};

template <int LAYOUT>
__device__ __forceinline__ uint32_t dq_tile_of_chunk(uint32_t chunk, const DqStreamArgs& a) {
  if constexpr (LAYOUT == LAYOUT_SCALAR) {
    return 0;
  } else if constexpr (LAYOUT == LAYOUT_ROWS) {
    return fdiv(chunk, a.chunks_per_run);
  } else {
    const uint32_t outer = fdiv(chunk, a.chunks_per_run);
    return outer - fdiv(outer, a.channels) * a.channels.div;
  }
}

template <typename TIn, typename TOut, int LAYOUT, int E, int U, bool HAS_OFFSET>
__global__ __launch_bounds__(kBlock) void dequantize_stream_kernel(const TIn* __restrict__ in,
                                                                   TOut* __restrict__ out,
                                                                   const float* __restrict__ scale,
                                                                   const float* __restrict__ offset,
                                                                   DqStreamArgs a) {
  const uint32_t first = blockIdx.x * (uint32_t)(kBlock * U) + threadIdx.x;
  Chunk<TIn, E> x[U];
  float s[U], o[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const uint32_t c = first + u * kBlock;
    if (c < a.nchunks) x[u].load(in + (size_t)c * E);
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const uint32_t c = first + u * kBlock;
    s[u] = 1.0f;
    o[u] = 0.0f;
    if (c < a.nchunks) {
      const uint32_t t = dq_tile_of_chunk<LAYOUT>(c, a);
      s[u] = scale[t * a.scale_stride];
      if constexpr (HAS_OFFSET) o[u] = offset[t * a.offset_stride];
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const uint32_t c = first + u * kBlock;
    if (c >= a.nchunks) continue;
    const float off = HAS_OFFSET ? rne(o[u]) : 0.0f;
    float v[E];
#pragma unroll
    for (int i = 0; i < E; ++i) {
      float q = x[u].get(i) + off;
      v[i] = q * s[u];
    }
    Chunk<TOut, E> y;
    y.pack(v);
    y.store(out + (size_t)c * E);
  }
}

struct DqColumnArgs {
  uint32_t col_chunks, rows, row_groups, scale_stride, offset_stride;
  FastDiv col_chunks_div;
};

template <typename TIn, typename TOut, int E, bool HAS_OFFSET>
__global__ __launch_bounds__(kBlock) void dequantize_columns_kernel(const TIn* __restrict__ in,
                                                                    TOut* __restrict__ out,
                                                                    const float* __restrict__ scale,
                                                                    const float* __restrict__ offset,
                                                                    DqColumnArgs a) {
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
  for (uint32_t row = group; row < a.rows; row += a.row_groups) {
    const size_t at = (size_t)row * row_elems + (size_t)cc * E;
    Chunk<TIn, E> x;
    x.load(in + at);
    float v[E];
#pragma unroll
    for (int i = 0; i < E; ++i) {
      float q = x.get(i) + o[i];
      v[i] = q * s[i];
    }
    Chunk<TOut, E> y;
    y.pack(v);
    y.store(out + at);
  }
}

struct DqGenericArgs {
  int data_dt, scale_dt, offset_dt, out_dt;
  int add_dt, mul_dt;
  int has_offset;
  int64_t start, count;
  int64_t scale_numel, offset_numel;
  GenericTiling g;
};

__global__ __launch_bounds__(kBlock) void dequantize_generic_kernel(const void* __restrict__ data,
                                                                    const void* __restrict__ scale,
                                                                    const void* __restrict__ offset,
                                                                    void* __restrict__ out,
                                                                    DqGenericArgs a) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < a.count; k += stride) {
    const int64_t i = a.start + k;
    const int64_t t = generic_tile_of(a.g, i);
    const double qs = load_any(data, a.data_dt, i);
    const double ss = load_any(scale, a.scale_dt, a.scale_numel == 1 ? 0 : t);
    double os = 0.0;
    if (a.has_offset) {
      os = load_any(offset, a.offset_dt, a.offset_numel == 1 ? 0 : t);
      if (dt_is_float(a.offset_dt)) os = rne(os);
    }
    double v;
    if (a.mul_dt == FFQ_F64) {
      double sum;
      if (a.add_dt == FFQ_F64) sum = qs + os;
      else if (dt_is_float(a.add_dt))
        sum = (double)round_stage(round_stage((float)qs, a.add_dt) + round_stage((float)os, a.add_dt), a.add_dt);
      else sum = qs + os;
      v = sum * ss;
    } else {
      float sum;
      if (dt_is_float(a.add_dt))
        sum = round_stage(round_stage((float)qs, a.add_dt) + round_stage((float)os, a.add_dt), a.add_dt);
      else
        sum = (float)(qs + os);  // integer add, exact; converted by the multiply's promotion
      v = (double)round_stage(round_stage(sum, a.mul_dt) * round_stage((float)ss, a.mul_dt), a.mul_dt);
    }
    store_any(out, a.out_dt, i, v);
  }
}

template <typename TIn, typename TOut, int E, int U>
static int dq_launch_stream_u(const AffineCall& c) {
  const DqStreamArgs a = stream_args<DqStreamArgs>(c, E);
  const unsigned grid = grid_for(a.nchunks, kBlock * U);
  const TIn* in = static_cast<const TIn*>(c.data);
  TOut* out = static_cast<TOut*>(c.out);
  const float* scale = static_cast<const float*>(c.scale);
  const float* offset = static_cast<const float*>(c.offset);
#define FFQ_LAUNCH(LAYOUT)                                                                             \
  do {                                                                                                 \
    if (offset)                                                                                        \
      dequantize_stream_kernel<TIn, TOut, LAYOUT, E, U, true><<<grid, kBlock, 0, c.stream>>>(in, out, scale, offset, a); \
    else                                                                                               \
      dequantize_stream_kernel<TIn, TOut, LAYOUT, E, U, false><<<grid, kBlock, 0, c.stream>>>(in, out, scale, offset, a); \
  } while (0)
  switch (c.info.layout) {
    case LAYOUT_SCALAR: FFQ_LAUNCH(LAYOUT_SCALAR); break;
    case LAYOUT_ROWS: FFQ_LAUNCH(LAYOUT_ROWS); break;
    default: FFQ_LAUNCH(LAYOUT_CHANNEL); break;
  }
#undef FFQ_LAUNCH
  return check_launch("dequantize_stream_kernel");
}

template <typename TIn, typename TOut, int E>
static int dq_launch_stream(const AffineCall& c) {
  if constexpr (kExperiments) {
    switch (stream_chunks_per_lane()) {
      case 1: return dq_launch_stream_u<TIn, TOut, E, 1>(c);
      case 4: return dq_launch_stream_u<TIn, TOut, E, 4>(c);
      default: return dq_launch_stream_u<TIn, TOut, E, 2>(c);
    }
  } else {
    return dq_launch_stream_u<TIn, TOut, E, 1>(c);
  }
}

template <typename TIn, typename TOut, int E>
static int dq_launch_columns(const AffineCall& c) {
  const DqColumnArgs a = affine_column_args<DqColumnArgs>(c, E);
  const TIn* in = static_cast<const TIn*>(c.data);
  TOut* out = static_cast<TOut*>(c.out);
  const float* scale = static_cast<const float*>(c.scale);
  const float* offset = static_cast<const float*>(c.offset);
  if (offset)
    dequantize_columns_kernel<TIn, TOut, E, true><<<column_grid(a), kBlock, 0, c.stream>>>(in, out, scale, offset, a);
  else
    dequantize_columns_kernel<TIn, TOut, E, false><<<column_grid(a), kBlock, 0, c.stream>>>(in, out, scale, offset, a);
  return check_launch("dequantize_columns_kernel");
}

// the kernel stream_route() chose, on the types of this call; 16-code chunks exist in tuning builds only (FFQ_DQ_E16)
template <typename TIn, typename TOut>
static int dq_launch_route(const AffineCall& c, const StreamRoute& route) {
  if (route.kernel == ROUTE_STREAM) {
    if constexpr (kExperiments && sizeof(TIn) == 1) {
      if (route.chunk == 16) return dq_launch_stream<TIn, TOut, 16>(c);
    }
    return dq_launch_stream<TIn, TOut, 8>(c);
  }
  return dq_launch_columns<TIn, TOut, 8>(c);
}

int dequantize_impl(const void* data, int data_dt, const void* scale, int scale_dt, int64_t scale_numel,
                    const void* offset, int offset_dt, int64_t offset_numel, const ffq_tiling* tiling,
                    void* out, int out_dt, hipStream_t stream) {
  AffineCall c;
  int rc = analyse(tiling, &c.info);
  if (rc) return rc;
  const int off_dt = offset ? offset_dt : scale_dt;
  if ((rc = check_tags({data_dt, scale_dt, out_dt, off_dt}))) return rc;
  if ((rc = check_param_counts(c.info, scale_numel, offset != nullptr, offset_numel))) return rc;
  // (row + offset[:, None]) * scale[:, None]                                           (:182)
  const int add_dt = ffq_promote_types(data_dt, off_dt);
  const int mul_dt = ffq_promote_types(add_dt, scale_dt);
  if (!dt_is_float(mul_dt)) return fail(FFQ_ERR_DTYPE, "integer-only dequantize is not built");
  if (c.info.numel == 0) return FFQ_OK;
  if ((rc = check_buffers({data, scale, out}))) return rc;
  c.data = data; c.scale = scale; c.offset = offset; c.out = out;
  c.scale_numel = scale_numel; c.offset_numel = offset_numel;
  c.lo = c.hi = 0.0f;
  c.stream = stream;

  // the streaming kernels: fp32 stages + fp32 parameters on a route stream_route() finds; everything else goes to the generic kernel
  int64_t done = 0;
  if (add_dt == FFQ_F32 && mul_dt == FFQ_F32 && scale_dt == FFQ_F32 && off_dt == FFQ_F32) {
    const StreamRoute route = stream_route(c.info, {dt_size(data_dt), dt_size(out_dt), aligned16(data), aligned16(out), generic_kernels_forced(),
                                                    experiment_knob("FFQ_DQ_E16", 0) == 1});
    bool launched = false;
    if (route.kernel != ROUTE_NONE)
      for_dtype<int8_t, int16_t, int32_t, float, bf16_t, f16_t>(data_dt, [&](auto tin) {
        using TIn = typename decltype(tin)::type;
        launched = for_float_dtype(out_dt, [&](auto tout) { rc = dq_launch_route<TIn, typename decltype(tout)::type>(c, route); });
      });
    if (rc) return rc;
    if (launched) done = route.covered;
  }
  if (done >= c.info.numel) return FFQ_OK;
  DqGenericArgs a;
  a.data_dt = data_dt; a.scale_dt = scale_dt; a.offset_dt = offset_dt; a.out_dt = out_dt;
  a.add_dt = add_dt; a.mul_dt = mul_dt;
  a.has_offset = offset != nullptr;
  a.start = done; a.count = c.info.numel - done;
  a.scale_numel = scale_numel; a.offset_numel = offset_numel;
  a.g = make_generic(tiling);
  dequantize_generic_kernel<<<generic_grid(a.count), kBlock, 0, stream>>>(data, scale, offset, out, a);
  return check_launch("dequantize_generic_kernel");
}

}  // namespace ffq

extern "C" int ffq_dequantize_by_tile(const void* data, int data_dt, const void* scale, int scale_dt,
                                      int64_t scale_numel, const void* offset, int offset_dt,
                                      int64_t offset_numel, const ffq_tiling* tiling, void* out,
                                      int out_dt, void* stream) {
  return ffq::dequantize_impl(data, data_dt, scale, scale_dt, scale_numel, offset, offset_dt, offset_numel,
                              tiling, out, out_dt, static_cast<hipStream_t>(stream));
}
