// ffq_pool.hip — the reference's quantized avg_pool1d / avg_pool2d / max_pool2d and nearest interpolate as one-pass kernels with A1
// fused in.
//
// ff.nn.functional.{avg_pool1d, avg_pool2d, max_pool2d, interpolate} run their generated fallbacks in the reference
// (_gen/fallback.py: avg_pool1d :505, avg_pool2d :542, max_pool2d :1574, interpolate :1611): A2 of the quantized input into a
// data-dtype tensor, the ATen op, A1 of the output quantizer — three launches with a full-size temporary between each. Here each is
// one pass under the A2 / op / A1 contract of ffq_onepass.h, with the parameters of the element's plane (one pair for the tensor, or
// one per channel of [B, C, H, W]).
// ATen's device formulas (torch 2.10; what the MI355X showed against them is in docs/kernels.md):
//   avg:      one fp32 accumulator per output, the window walked rows outer / columns inner over the part inside the input, divided
//             once by the window's size — (hend - hstart) * (wend - wstart) clipped to the input PLUS its padding when
//             count_include_pad, else clipped to the input — and rounded once
//   max:      a selection, `val > max || isnan(val)` from -inf over the dilated window inside the input (NaN wins, the last one)
//   nearest:  a gather from min(floor(dst * scale), in - 1), "nearest-exact" from min(floor((dst + 0.5) * scale), in - 1), with the
//             fp32 scale = 1 / scale_factor when one is given, else in / out
// A lane computes outputs of the FLATTENED [planes, OH, OW] result, consecutive lanes consecutive outputs (their windows are
// neighbours in memory: the overlap of a 3x3 stride-2 window is served by the caches), so maps of any width keep the lanes busy. The
// block's results meet in LDS and leave in 8-element groups — 16 B of values, 8 B of codes per lane through ffq_fanout.h; the last
// group of a result whose size is no multiple of 8 leaves element by element.
#include "ffq_pool_tile.h"

namespace ffq {
namespace pool {

enum { kAvg = 0, kAvgExcludePad = 1, kMax = 2 };  // the ABI's modes (include/ffq.h)

struct Geometry {
  uint32_t total;     // planes * OH * OW
  uint32_t channels;  // parameter pairs (1: per tensor): plane % channels indexes them
  int32_t H, W, OH, OW;
  int32_t kh, kw, sh, sw, ph, pw, dh, dw;
  float scale_h, scale_w;  // nearest: the fp32 source scales
  int32_t exact;           // nearest: "nearest-exact"
  FastDiv by_ow, by_oh, by_channels;
};

struct Place {
  uint32_t plane;
  int32_t oh, ow;
  float s, o;
};

template <bool DEQ>
__device__ __forceinline__ Place place_of(const Geometry& g, const float* xs, const float* xo, uint32_t idx) {
  Place p;
  const uint32_t t = fdiv(idx, g.by_ow);
  p.ow = (int32_t)(idx - t * (uint32_t)g.OW);
  p.plane = fdiv(t, g.by_oh);
  p.oh = (int32_t)(t - p.plane * (uint32_t)g.OH);
  p.s = 1.0f;
  p.o = 0.0f;
  if constexpr (DEQ) {
    const uint32_t c = g.channels > 1 ? p.plane - fdiv(p.plane, g.by_channels) * g.channels : 0u;
    p.s = xs[c];
    p.o = xo ? rne(xo[c]) : 0.0f;
  }
  return p;
}

// One output of the pools, in fp32 before the one rounding to T (max: a value of T already).
template <typename T, typename TIn, bool DEQ, int MODE>
__device__ __forceinline__ float pool_one(const TIn* __restrict__ x, const float* xs, const float* xo, const Geometry& g, uint32_t idx) {
  const Place p = place_of<DEQ>(g, xs, xo, idx);
  const TIn* plane = x + (size_t)p.plane * (size_t)(g.H * g.W);
  int32_t hstart = p.oh * g.sh - g.ph, wstart = p.ow * g.sw - g.pw;
  if constexpr (MODE == kMax) {
    const int32_t hend = min(hstart + (g.kh - 1) * g.dh + 1, g.H), wend = min(wstart + (g.kw - 1) * g.dw + 1, g.W);
    while (hstart < 0) hstart += g.dh;
    while (wstart < 0) wstart += g.dw;
    // A positive, finite scale of at least 2^-14 makes A2 monotone in the code and keeps every non-zero q + o away from a zero of
    // either sign in T, so equal values have equal bits: the selection runs on the codes and A2 once on the winner. Any other scale
    // (negative, zero, NaN, inf, tiny) compares the dequantized values, as the chain does.
    const bool on_codes = DEQ && p.s >= 0x1p-14f && p.s < INFINITY;
    float best = -INFINITY;
    if (on_codes) {
      for (int32_t h = hstart; h < hend; h += g.dh)
        for (int32_t w = wstart; w < wend; w += g.dw) {
          const float q = to_f32(plane[h * g.W + w]);
          if (q > best || q != q) best = q;
        }
      // (a window inside the input is never empty under ATen's padding rule; -inf stays -inf for one that is)
      return best == -INFINITY ? best : a2_value<T>(best, p.s, p.o);
    }
    for (int32_t h = hstart; h < hend; h += g.dh)
      for (int32_t w = wstart; w < wend; w += g.dw) {
        const float v = value_at<T, TIn, DEQ>(plane + h * g.W + w, p.s, p.o);
        if (v > best || v != v) best = v;
      }
    return best;
  } else {
    int32_t hend = min(hstart + g.kh, g.H + g.ph), wend = min(wstart + g.kw, g.W + g.pw);
    const int32_t padded = (hend - hstart) * (wend - wstart);
    hstart = max(hstart, 0);
    wstart = max(wstart, 0);
    hend = min(hend, g.H);
    wend = min(wend, g.W);
    if (hstart >= hend || wstart >= wend) return 0.0f;
    float acc = 0.0f;
    for (int32_t h = hstart; h < hend; ++h)
      for (int32_t w = wstart; w < wend; ++w) acc = acc + value_at<T, TIn, DEQ>(plane + h * g.W + w, p.s, p.o);
    const int32_t divisor = MODE == kAvg ? padded : (hend - hstart) * (wend - wstart);
    return acc / (float)divisor;
  }
}

__device__ __forceinline__ int32_t nearest_source(float scale, int32_t dst, int32_t size, bool exact) {
  const float at = exact ? ((float)dst + 0.5f) * scale : (float)dst * scale;
  return min((int32_t)floorf(at), size - 1);
}

template <typename T, typename TIn, bool DEQ>
__device__ __forceinline__ float nearest_one(const TIn* __restrict__ x, const float* xs, const float* xo, const Geometry& g, uint32_t idx) {
  const Place p = place_of<DEQ>(g, xs, xo, idx);
  const int32_t h = nearest_source(g.scale_h, p.oh, g.H, g.exact != 0), w = nearest_source(g.scale_w, p.ow, g.W, g.exact != 0);
  return value_at<T, TIn, DEQ>(x + (size_t)p.plane * (size_t)(g.H * g.W) + (h * g.W + w), p.s, p.o);
}

// ---------------------------------------------------------------------------------------------------
// P1: avg / max pool of [planes, H, W] + A1. A block computes kBlock * J consecutive outputs, lane t the outputs t, t + kBlock, ...
//     Algorithmic bytes: the input once (2 B bf16 / 1 B int8 per element) + per output [2 (z)] + 1 per code tensor.
// ---------------------------------------------------------------------------------------------------
template <typename T, typename TIn, bool DEQ, int MODE, int J>
__global__ __launch_bounds__(kBlock) void pool2d_quantize_kernel(const TIn* __restrict__ x, const float* __restrict__ xs,
                                                                 const float* __restrict__ xo, Geometry g, T* __restrict__ out, FanOut f) {
  __shared__ float z[kBlock * J];
  const uint32_t base = blockIdx.x * (uint32_t)(kBlock * J);
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const uint32_t idx = base + j * kBlock + threadIdx.x;
    z[j * kBlock + threadIdx.x] = idx < g.total ? pool_one<T, TIn, DEQ, MODE>(x, xs, xo, g, idx) : 0.0f;
  }
  __syncthreads();
  store_tile<T, J>(z, base, g.total, out, f);
}

// ---------------------------------------------------------------------------------------------------
// N1: nearest / nearest-exact upsampling of [planes, H, W] to [planes, OH, OW] + A1, the plan of P1.
//     Algorithmic bytes: the input once + per output [2 (z)] + 1 per code tensor (the output dominates when upsampling).
// ---------------------------------------------------------------------------------------------------
template <typename T, typename TIn, bool DEQ, int J>
__global__ __launch_bounds__(kBlock) void upsample_nearest_quantize_kernel(const TIn* __restrict__ x, const float* __restrict__ xs,
                                                                           const float* __restrict__ xo, Geometry g, T* __restrict__ out,
                                                                           FanOut f) {
  __shared__ float z[kBlock * J];
  const uint32_t base = blockIdx.x * (uint32_t)(kBlock * J);
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const uint32_t idx = base + j * kBlock + threadIdx.x;
    z[j * kBlock + threadIdx.x] = idx < g.total ? nearest_one<T, TIn, DEQ>(x, xs, xo, g, idx) : 0.0f;
  }
  __syncthreads();
  store_tile<T, J>(z, base, g.total, out, f);
}

static int check_extents(const char* what, int64_t channels, int64_t planes, int64_t H, int64_t W, int64_t OH, int64_t OW) {
  if (planes < 0 || H < 0 || W < 0 || channels < 0) return fail(FFQ_ERR_ARG, "%s: negative extent", what);
  if (channels && planes % channels != 0) return fail(FFQ_ERR_ARG, "%s: %lld planes are not whole images of %lld channels", what, (long long)planes, (long long)channels);
  if (H == 0 || W == 0) return fail(FFQ_ERR_ARG, "%s: an empty map ([%lld, %lld])", what, (long long)H, (long long)W);
  if (OH < 1 || OW < 1) return fail(FFQ_ERR_ARG, "%s: output size [%lld, %lld] is too small", what, (long long)OH, (long long)OW);
  const int64_t limit = (int64_t)1 << 31;
  if (H >= limit / W || planes * H * W >= limit || OH >= limit / OW || planes * OH * OW >= limit)
    return fail(FFQ_ERR_DTYPE, "%s needs fewer than 2^31 input and output elements", what);
  return FFQ_OK;
}

static void fill(Geometry* g, int64_t channels, int64_t planes, int64_t H, int64_t W, int64_t OH, int64_t OW) {
  g->total = (uint32_t)(planes * OH * OW);
  g->channels = channels ? (uint32_t)channels : 1u;
  g->H = (int32_t)H; g->W = (int32_t)W; g->OH = (int32_t)OH; g->OW = (int32_t)OW;
  g->kh = g->kw = g->sh = g->sw = g->dh = g->dw = 1;
  g->ph = g->pw = 0;
  g->scale_h = g->scale_w = 1.0f;
  g->exact = 0;
  g->by_ow = make_fastdiv((uint32_t)OW);
  g->by_oh = make_fastdiv((uint32_t)OH);
  g->by_channels = make_fastdiv(g->channels);
}

}  // namespace pool
}  // namespace ffq

using namespace ffq;
using namespace ffq::pool;

extern "C" int ffq_pool2d_quantize(int mode, const void* x, int x_dt, const float* x_scale, const float* x_offset, int64_t param_channels,
                                   int dt, int64_t planes, int64_t H, int64_t W, int64_t kh, int64_t kw, int64_t sh, int64_t sw,
                                   int64_t ph, int64_t pw, int64_t dh, int64_t dw, int ceil_mode, int64_t OH, int64_t OW, void* out,
                                   const ffq_fanout* fan, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (mode < kAvg || mode > kMax) return fail(FFQ_ERR_ARG, "unknown pool mode %d (0: avg, 1: avg without the padding, 2: max)", mode);
  int rc = check_dtypes("fused pooling", x_dt, x_scale, x_offset, param_channels, dt);
  if (rc) return rc;
  const int64_t most = (int64_t)1 << 20;
  if (kh < 1 || kw < 1 || sh < 1 || sw < 1 || dh < 1 || dw < 1 || ph < 0 || pw < 0 || kh > most || kw > most || sh > most || sw > most ||
      dh > most || dw > most)
    return fail(FFQ_ERR_ARG, "kernel size, stride and dilation must be positive (and below 2^20), padding non-negative");
  if (mode != kMax && (dh != 1 || dw != 1)) return fail(FFQ_ERR_ARG, "the average pools have no dilation");
  if (ph > kh / 2 || pw > kw / 2) return fail(FFQ_ERR_ARG, "pad should be at most half of the kernel size (pad [%lld, %lld], kernel [%lld, %lld])",
                                              (long long)ph, (long long)pw, (long long)kh, (long long)kw);
  if (planes >= 0 && H > 0 && W > 0 &&
      (OH != pooled(H, kh, ph, sh, dh, ceil_mode != 0) || OW != pooled(W, kw, pw, sw, dw, ceil_mode != 0)))
    return fail(FFQ_ERR_ARG, "the output of this pooling is [%lld, %lld], not [%lld, %lld]", (long long)pooled(H, kh, ph, sh, dh, ceil_mode != 0),
                (long long)pooled(W, kw, pw, sw, dw, ceil_mode != 0), (long long)OH, (long long)OW);
  rc = check_extents("fused pooling", param_channels, planes, H, W, OH, OW);
  if (rc) return rc;
  FanOut f;
  rc = check_launch_args(fan, planes * OH * OW, planes == 0, x, {x, out}, &f);
  if (rc || planes == 0) return rc;
  Geometry g;
  fill(&g, param_channels, planes, H, W, OH, OW);
  g.kh = (int32_t)kh; g.kw = (int32_t)kw; g.sh = (int32_t)sh; g.sw = (int32_t)sw;
  g.ph = (int32_t)ph; g.pw = (int32_t)pw; g.dh = (int32_t)dh; g.dw = (int32_t)dw;
  const int j = per_lane(g.total);
  const unsigned grid = (unsigned)(((uint64_t)g.total + (uint64_t)(kBlock * j) - 1) / (uint64_t)(kBlock * j));
  dispatch_input(dt, x_dt, x_scale != nullptr, [&](auto t, auto tin, auto deq) {
    using T = typename decltype(t)::type;
    using TIn = typename decltype(tin)::type;
    auto launch = [&](auto mode_, auto j_) {
      pool2d_quantize_kernel<T, TIn, decltype(deq)::value, decltype(mode_)::value, decltype(j_)::value><<<grid, kBlock, 0, s>>>(
          static_cast<const TIn*>(x), x_scale, x_offset, g, static_cast<T*>(out), f);
    };
    auto by_lane = [&](auto mode_) {
      if (j == 8) launch(mode_, Int<8>{}); else launch(mode_, Int<1>{});
    };
    switch (mode) {
      case kAvg: by_lane(Int<kAvg>{}); break;
      case kAvgExcludePad: by_lane(Int<kAvgExcludePad>{}); break;
      default: by_lane(Int<kMax>{}); break;
    }
  });
  return check_launch("pool2d_quantize_kernel");
}

extern "C" int ffq_upsample_nearest_quantize(const void* x, int x_dt, const float* x_scale, const float* x_offset, int64_t param_channels,
                                             int dt, int64_t planes, int64_t H, int64_t W, int64_t OH, int64_t OW, double scale_factor_h,
                                             double scale_factor_w, int exact, void* out, const ffq_fanout* fan, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  int rc = check_dtypes("fused nearest interpolation", x_dt, x_scale, x_offset, param_channels, dt);
  if (rc) return rc;
  if (!(scale_factor_h >= 0.0) || !(scale_factor_w >= 0.0) || isinf(scale_factor_h) || isinf(scale_factor_w))
    return fail(FFQ_ERR_ARG, "a scale factor is a positive finite number, or 0 for none");
  rc = check_extents("fused nearest interpolation", param_channels, planes, H, W, OH, OW);
  if (rc) return rc;
  FanOut f;
  rc = check_launch_args(fan, planes * OH * OW, planes == 0, x, {x, out}, &f);
  if (rc || planes == 0) return rc;
  Geometry g;
  fill(&g, param_channels, planes, H, W, OH, OW);
  // ATen's compute_scales_value<float>: 1 / scale_factor when one is given, else in / out
  g.scale_h = scale_factor_h > 0.0 ? (float)(1.0 / scale_factor_h) : (float)H / (float)OH;
  g.scale_w = scale_factor_w > 0.0 ? (float)(1.0 / scale_factor_w) : (float)W / (float)OW;
  g.exact = exact ? 1 : 0;
  const int j = per_lane(g.total);
  const unsigned grid = (unsigned)(((uint64_t)g.total + (uint64_t)(kBlock * j) - 1) / (uint64_t)(kBlock * j));
  dispatch_input(dt, x_dt, x_scale != nullptr, [&](auto t, auto tin, auto deq) {
    using T = typename decltype(t)::type;
    using TIn = typename decltype(tin)::type;
    auto launch = [&](auto j_) {
      upsample_nearest_quantize_kernel<T, TIn, decltype(deq)::value, decltype(j_)::value><<<grid, kBlock, 0, s>>>(
          static_cast<const TIn*>(x), x_scale, x_offset, g, static_cast<T*>(out), f);
    };
    if (j == 8) launch(Int<8>{}); else launch(Int<1>{});
  });
  return check_launch("upsample_nearest_quantize_kernel");
}
