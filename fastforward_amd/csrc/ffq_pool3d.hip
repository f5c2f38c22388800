// ffq_pool3d.hip — the reference's quantized avg_pool3d as a one-pass kernel with A1 fused in.
//
// ff.nn.functional.avg_pool3d runs its generated fallback in the reference (_gen/fallback.py:579-612): A2 of the quantized input
// into a data-dtype tensor, F.avg_pool3d, A1 of the output quantizer — three launches with a full-size temporary between each. Here
// it is one pass under the A2 / op / A1 contract of ffq_onepass.h, the plan of ffq_pool.hip's P1 with a depth axis: the parameters
// of the element's plane (one pair for the tensor, or one per channel of [B, C, D, H, W]) and ATen's device formula (torch 2.10,
// avg_pool3d_cuda_update_output): one fp32 accumulator per output, the window walked depth outer / rows / columns inner over the part
// inside the input, divided once by the window's size — (tend - tstart) * (hend - hstart) * (wend - wstart) clipped to the input PLUS
// its padding when count_include_pad, else clipped to the input — and rounded once.
// A lane computes outputs of the FLATTENED [planes, OD, OH, OW] result, consecutive lanes consecutive outputs; the block's results
// meet in LDS and leave in 8-element groups through ffq_pool_tile.h's store_tile.
#include "ffq_pool_tile.h"

#include "../../include/ffq_3d.h"

namespace ffq {
namespace pool {

enum { kAvg3 = 0, kAvg3ExcludePad = 1 };  // the ABI's modes (include/ffq_3d.h)

struct Geometry3 {
  uint32_t total;     // planes * OD * OH * OW
  uint32_t channels;  // parameter pairs (1: per tensor): plane % channels indexes them
  int32_t D, H, W, OD, OH, OW;
  int32_t kd, kh, kw, sd, sh, sw, pd, ph, pw;
  FastDiv by_ow, by_oh, by_od, by_channels;
};

// One output, in fp32 before the one rounding to T.
template <typename T, typename TIn, bool DEQ, int MODE>
__device__ __forceinline__ float pool3_one(const TIn* __restrict__ x, const float* xs, const float* xo, const Geometry3& g, uint32_t idx) {
  const uint32_t t1 = fdiv(idx, g.by_ow);
  const int32_t ow = (int32_t)(idx - t1 * (uint32_t)g.OW);
  const uint32_t t2 = fdiv(t1, g.by_oh);
  const int32_t oh = (int32_t)(t1 - t2 * (uint32_t)g.OH);
  const uint32_t plane = fdiv(t2, g.by_od);
  const int32_t od = (int32_t)(t2 - plane * (uint32_t)g.OD);
  float s = 1.0f, o = 0.0f;
  if constexpr (DEQ) {
    const uint32_t c = g.channels > 1 ? plane - fdiv(plane, g.by_channels) * g.channels : 0u;
    s = xs[c];
    o = xo ? rne(xo[c]) : 0.0f;
  }
  const TIn* vol = x + (size_t)plane * ((size_t)g.D * (size_t)(g.H * g.W));  // fewer than 2^31 input elements: H * W fits
  int32_t tstart = od * g.sd - g.pd, hstart = oh * g.sh - g.ph, wstart = ow * g.sw - g.pw;
  int32_t tend = min(tstart + g.kd, g.D + g.pd), hend = min(hstart + g.kh, g.H + g.ph), wend = min(wstart + g.kw, g.W + g.pw);
  const int32_t padded = (tend - tstart) * (hend - hstart) * (wend - wstart);
  tstart = max(tstart, 0);
  hstart = max(hstart, 0);
  wstart = max(wstart, 0);
  tend = min(tend, g.D);
  hend = min(hend, g.H);
  wend = min(wend, g.W);
  if (tstart >= tend || hstart >= hend || wstart >= wend) return 0.0f;
  float acc = 0.0f;
  for (int32_t t = tstart; t < tend; ++t)
    for (int32_t h = hstart; h < hend; ++h)
      for (int32_t w = wstart; w < wend; ++w) acc = acc + value_at<T, TIn, DEQ>(vol + ((t * g.H + h) * g.W + w), s, o);
  const int32_t divisor = MODE == kAvg3 ? padded : (tend - tstart) * (hend - hstart) * (wend - wstart);
  return acc / (float)divisor;
}

// ---------------------------------------------------------------------------------------------------
// P3: avg pool of [planes, D, H, W] + A1. A block computes kBlock * J consecutive outputs, lane t the outputs t, t + kBlock, ...
//     Algorithmic bytes: the input once (2 B bf16 / 1 B int8 per element) + per output [2 (z)] + 1 per code tensor.
// ---------------------------------------------------------------------------------------------------
template <typename T, typename TIn, bool DEQ, int MODE, int J>
__global__ __launch_bounds__(kBlock) void pool3d_quantize_kernel(const TIn* __restrict__ x, const float* __restrict__ xs,
                                                                 const float* __restrict__ xo, Geometry3 g, T* __restrict__ out, FanOut f) {
  __shared__ float z[kBlock * J];
  const uint32_t base = blockIdx.x * (uint32_t)(kBlock * J);
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const uint32_t idx = base + j * kBlock + threadIdx.x;
    z[j * kBlock + threadIdx.x] = idx < g.total ? pool3_one<T, TIn, DEQ, MODE>(x, xs, xo, g, idx) : 0.0f;
  }
  __syncthreads();
  store_tile<T, J>(z, base, g.total, out, f);
}

// a * b, or `limit` when the product reaches it (a, b >= 0)
static int64_t mul_capped(int64_t a, int64_t b, int64_t limit) {
  if (a == 0 || b == 0) return 0;
  return a >= (limit + b - 1) / b ? limit : a * b;
}

static int check_extents3(const char* what, int64_t channels, int64_t planes, const int64_t* in, const int64_t* out) {
  if (planes < 0 || in[0] < 0 || in[1] < 0 || in[2] < 0 || channels < 0) return fail(FFQ_ERR_ARG, "%s: negative extent", what);
  if (channels && planes % channels != 0)
    return fail(FFQ_ERR_ARG, "%s: %lld planes are not whole volumes of %lld channels", what, (long long)planes, (long long)channels);
  if (in[0] == 0 || in[1] == 0 || in[2] == 0)
    return fail(FFQ_ERR_ARG, "%s: an empty map ([%lld, %lld, %lld])", what, (long long)in[0], (long long)in[1], (long long)in[2]);
  if (out[0] < 1 || out[1] < 1 || out[2] < 1)
    return fail(FFQ_ERR_ARG, "%s: output size [%lld, %lld, %lld] is too small", what, (long long)out[0], (long long)out[1], (long long)out[2]);
  const int64_t limit = (int64_t)1 << 31;
  const int64_t n_in = mul_capped(mul_capped(mul_capped(in[0], in[1], limit), in[2], limit), planes ? planes : 1, limit);
  const int64_t n_out = mul_capped(mul_capped(mul_capped(out[0], out[1], limit), out[2], limit), planes ? planes : 1, limit);
  if (n_in >= limit || n_out >= limit) return fail(FFQ_ERR_DTYPE, "%s needs fewer than 2^31 input and output elements", what);
  return FFQ_OK;
}

}  // namespace pool
}  // namespace ffq

using namespace ffq;
using namespace ffq::pool;

extern "C" int ffq_pool3d_quantize(int mode, const void* x, int x_dt, const float* x_scale, const float* x_offset, int64_t param_channels,
                                   int dt, int64_t planes, int64_t D, int64_t H, int64_t W, int64_t kd, int64_t kh, int64_t kw, int64_t sd,
                                   int64_t sh, int64_t sw, int64_t pd, int64_t ph, int64_t pw, int ceil_mode, int64_t OD, int64_t OH,
                                   int64_t OW, void* out, const ffq_fanout* fan, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (mode < kAvg3 || mode > kAvg3ExcludePad) return fail(FFQ_ERR_ARG, "unknown 3-D pool mode %d (0: avg, 1: avg without the padding)", mode);
  int rc = check_dtypes("fused 3-D pooling", x_dt, x_scale, x_offset, param_channels, dt);
  if (rc) return rc;
  const int64_t most = (int64_t)1 << 20;
  const int64_t in[3] = {D, H, W}, k[3] = {kd, kh, kw}, st[3] = {sd, sh, sw}, pad[3] = {pd, ph, pw}, o[3] = {OD, OH, OW};
  for (int i = 0; i < 3; ++i)
    if (k[i] < 1 || st[i] < 1 || pad[i] < 0 || k[i] > most || st[i] > most)
      return fail(FFQ_ERR_ARG, "kernel size and stride must be positive (and below 2^20), padding non-negative");
  for (int i = 0; i < 3; ++i)
    if (pad[i] > k[i] / 2)
      return fail(FFQ_ERR_ARG, "pad should be at most half of the kernel size (pad [%lld, %lld, %lld], kernel [%lld, %lld, %lld])", (long long)pd,
                  (long long)ph, (long long)pw, (long long)kd, (long long)kh, (long long)kw);
  if (planes >= 0 && D > 0 && H > 0 && W > 0) {
    int64_t want[3];
    for (int i = 0; i < 3; ++i) want[i] = pooled(in[i], k[i], pad[i], st[i], 1, ceil_mode != 0);
    if (want[0] != OD || want[1] != OH || want[2] != OW)
      return fail(FFQ_ERR_ARG, "the output of this pooling is [%lld, %lld, %lld], not [%lld, %lld, %lld]", (long long)want[0], (long long)want[1],
                  (long long)want[2], (long long)OD, (long long)OH, (long long)OW);
  }
  rc = check_extents3("fused 3-D pooling", param_channels, planes, in, o);
  if (rc) return rc;
  FanOut f;
  rc = check_launch_args(fan, planes * OD * OH * OW, planes == 0, x, {x, out}, &f);
  if (rc || planes == 0) return rc;
  Geometry3 g;
  g.total = (uint32_t)(planes * OD * OH * OW);
  g.channels = param_channels ? (uint32_t)param_channels : 1u;
  g.D = (int32_t)D; g.H = (int32_t)H; g.W = (int32_t)W; g.OD = (int32_t)OD; g.OH = (int32_t)OH; g.OW = (int32_t)OW;
  g.kd = (int32_t)kd; g.kh = (int32_t)kh; g.kw = (int32_t)kw; g.sd = (int32_t)sd; g.sh = (int32_t)sh; g.sw = (int32_t)sw;
  g.pd = (int32_t)pd; g.ph = (int32_t)ph; g.pw = (int32_t)pw;
  g.by_ow = make_fastdiv((uint32_t)OW);
  g.by_oh = make_fastdiv((uint32_t)OH);
  g.by_od = make_fastdiv((uint32_t)OD);
  g.by_channels = make_fastdiv(g.channels);
  const int j = per_lane(g.total);
  const unsigned grid = (unsigned)(((uint64_t)g.total + (uint64_t)(kBlock * j) - 1) / (uint64_t)(kBlock * j));
  dispatch_input(dt, x_dt, x_scale != nullptr, [&](auto t, auto tin, auto deq) {
    using T = typename decltype(t)::type;
    using TIn = typename decltype(tin)::type;
    auto launch = [&](auto mode_, auto j_) {
      pool3d_quantize_kernel<T, TIn, decltype(deq)::value, decltype(mode_)::value, decltype(j_)::value><<<grid, kBlock, 0, s>>>(
          static_cast<const TIn*>(x), x_scale, x_offset, g, static_cast<T*>(out), f);
    };
    auto by_lane = [&](auto mode_) {
      if (j == 8) launch(mode_, Int<8>{}); else launch(mode_, Int<1>{});
    };
    if (mode == kAvg3) by_lane(Int<kAvg3>{}); else by_lane(Int<kAvg3ExcludePad>{});
  });
  return check_launch("pool3d_quantize_kernel");
}
