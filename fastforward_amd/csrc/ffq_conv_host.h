// ffq_conv_host.h — the host side the convolution entry points share (ffq_conv.hip, ffq_conv3d.hip, ffq_conv_transpose.hip,
// ffq_depthwise.hip): argument checks, the workspace of the implicit GEMMs, the operand fields of the kernels' argument structs
// and the output-type dispatch. Host code only — nothing here reaches a code object; what the kernels share is ffq_conv_tile.h.
//
// Every helper states one rule once and knows nothing of its caller: where the entry points differ they pass data (the axes, a
// noun for the messages, a count) or keep the lines themselves. The ORDER of an entry point's checks is part of its contract
// (include/ffq.h; the *_argument_checks_need_no_device tables of the tests pin it), so each helper is one contiguous run of that
// order and the entry points call them in it.
#pragma once

#include "ffq_common.h"
#include "ffq_vec.h"

#include <math.h>
#include <type_traits>

namespace ffq {

constexpr int64_t kConvMaxReduction = 131071;  // C * prod(kernel) bound: |acc| <= 2^14 * (2^17 - 1) < 2^31 (at 2^17 taps of -128 x -128 the sum is 2^31 and wraps; docs/numerics.md)
constexpr int64_t kConvBig = (int64_t)1 << 40;  // elements one launch addresses

static size_t round256(size_t v) { return (v + 255) & ~(size_t)255; }

// a * b, or `limit` when the product reaches it (a, b >= 0; limit <= 2^62): extents of 2^24 per axis overflow a plain product
static int64_t mul_capped(int64_t a, int64_t b, int64_t limit) {
  if (a == 0 || b == 0) return 0;
  return a >= (limit + b - 1) / b ? limit : a * b;
}

// first * v[0] * ... * v[n - 1], capped at kConvBig
static int64_t product_capped(int64_t first, int n, const int64_t* v) {
  for (int i = 0; i < n; ++i) first = mul_capped(first, v[i], kConvBig);
  return first;
}

// ---- argument checks ---------------------------------------------------------------------------------------------------------

// The checks an implicit GEMM's geometry starts with, over n spatial axes: no negative extent, a filter of at least one tap, stride
// and dilation >= 1 with padding >= 0, nothing above 2^24 (so sums and pairwise products of the per-axis values stay far inside int64).
static int check_conv_axes(const char* what, int n, int64_t B, int64_t C, int64_t OC, const int64_t* in, const int64_t* k, const int64_t* s,
                           const int64_t* p, const int64_t* d) {
  bool negative = B < 0 || C < 0 || OC < 0, empty = C == 0;
  for (int i = 0; i < n; ++i) {
    negative = negative || in[i] < 0 || k[i] < 0;
    empty = empty || k[i] == 0;
  }
  if (negative) return fail(FFQ_ERR_ARG, "negative extent");
  if (empty) return fail(FFQ_ERR_EMPTY, "a %s over an empty filter", what);
  for (int i = 0; i < n; ++i)
    if (s[i] < 1 || d[i] < 1 || p[i] < 0) return fail(FFQ_ERR_ARG, "stride and dilation >= 1, padding >= 0");
  const int64_t lim = (int64_t)1 << 24;
  for (int i = 0; i < n; ++i)
    if (in[i] > lim || k[i] > lim || s[i] > lim || d[i] > lim || p[i] > lim)
      return fail(FFQ_ERR_ARG, "extent, stride, padding or dilation above 2^24");
  return FFQ_OK;
}

// The int32 accumulator's bound on the reduction, without overflow on the way to it.
static int check_conv_reduction(int64_t C, int n, const int64_t* k) {
  const int64_t reduction = product_capped(C, n, k);
  if (reduction > kConvMaxReduction)
    return fail(FFQ_ERR_DTYPE, "C * prod(kernel) = %lld exceeds %lld (the int32 accumulator's bound)", (long long)reduction, (long long)kConvMaxReduction);
  return FFQ_OK;
}

// What a convolution may add and write: a bias of a real dtype; with an output quantizer int8 codes of enough bits, rounded from
// the real dtype `y_dt` first; without one a real dtype.
static int check_conv_output(const char* what, const void* bias, int bias_dt, bool requant, int out_dt, double out_num_bits, int y_dt) {
  if (bias && !(bias_dt == FFQ_F32 || bias_dt == FFQ_BF16 || bias_dt == FFQ_F16)) return fail(FFQ_ERR_DTYPE, "bias must be f32, bf16 or f16");
  if (requant) {
    if (out_dt != FFQ_I8) return fail(FFQ_ERR_DTYPE, "the re-quantized %s writes int8 codes", what);
    if (!ffq_can_support_bitwidth(out_dt, out_num_bits))
      return fail(FFQ_ERR_PRECISION, "Provided dtype (%d) is not enough to store %g bits quantized values.", out_dt, out_num_bits);
    if (!(y_dt == FFQ_F32 || y_dt == FFQ_BF16 || y_dt == FFQ_F16))
      return fail(FFQ_ERR_DTYPE, "the re-quantized %s's real-valued dtype must be f32, bf16 or f16", what);
  } else if (!(out_dt == FFQ_F32 || out_dt == FFQ_BF16 || out_dt == FFQ_F16)) {
    return fail(FFQ_ERR_DTYPE, "real-valued output must be f32, bf16 or f16");
  }
  return FFQ_OK;
}

// ---- the workspace of an implicit GEMM ----------------------------------------------------------------------------------------

// Three parts, each rounded up to 256 bytes: the input codes with channels innermost and padded to Cp (absent where the caller's
// channels-last codes serve as they are), the reordered weight codes, the int32 sums of the weight codes.
struct ConvWorkspace {
  size_t x_bytes, w_bytes, sum_bytes;
  size_t total() const { return x_bytes + w_bytes + sum_bytes; }
};

static ConvWorkspace conv_workspace(int64_t x_codes, int x_channels_last, int64_t w_codes, int64_t sums) {
  return {x_channels_last ? 0 : round256((size_t)x_codes), round256((size_t)w_codes), round256((size_t)sums * 4)};
}

// What the *_workspace_bytes queries answer: the workspace of a launch with `totals` sums per output channel beside its per-tap
// ones, or 0 where no launch takes the shapes (the entry point answers FFQ_ERR_ARG, FFQ_ERR_EMPTY or FFQ_ERR_DTYPE). No product wraps.
static size_t conv_workspace_query(int64_t B, int64_t C, int64_t OC, int n, const int64_t* in, const int64_t* k, int x_channels_last,
                                   int64_t totals) {
  if (B < 0 || C <= 0 || OC < 0) return 0;
  for (int i = 0; i < n; ++i)
    if (in[i] < 0 || k[i] <= 0) return 0;
  const int64_t Cp = mul_capped((C + 15) / 16, 16, kConvBig);
  const int64_t taps = product_capped(1, n, k);
  const int64_t x = mul_capped(product_capped(B, n, in), Cp, kConvBig);
  const int64_t w = mul_capped(mul_capped(OC, taps, kConvBig), Cp, kConvBig);
  if (x >= kConvBig || w >= kConvBig) return 0;
  return conv_workspace(x, x_channels_last, w, OC * taps + OC * totals).total();
}

// The buffers of an implicit GEMM's launch: the operands there, channels-last input codes aligned for the 16-byte gathers, the
// workspace large enough and aligned.
static int check_conv_buffers(const char* what, const int8_t* xq, int x_channels_last, const int8_t* wq, const float* x_scale,
                              const float* w_scale, const void* out, const void* workspace, size_t workspace_bytes, size_t need) {
  if (!xq || !wq || !x_scale || !w_scale || !out) return fail(FFQ_ERR_ARG, "NULL buffer");
  if (x_channels_last && !aligned16(xq)) return fail(FFQ_ERR_ARG, "channels-last input codes must be 16-byte aligned");
  if (!workspace || workspace_bytes < need || !aligned16(workspace))
    return fail(FFQ_ERR_WORKSPACE, "w8a8 %s needs %zu workspace bytes (16-byte aligned), got %zu", what, need, workspace_bytes);
  return FFQ_OK;
}

struct ConvBuffers {
  int8_t* xn;       // the channels-last input codes: in the workspace, or the caller's own
  int8_t* wn;       // the reordered weight codes
  int32_t* tapsum;  // the sums, the first `sums` of them zeroed on the stream
};

// Carve the workspace and zero the sums the layout pass adds into.
static int carve_conv_workspace(const int8_t* xq, int x_channels_last, void* workspace, const ConvWorkspace& w, int64_t sums, hipStream_t s,
                                ConvBuffers* b) {
  uint8_t* ws = static_cast<uint8_t*>(workspace);
  b->xn = x_channels_last ? const_cast<int8_t*>(xq) : reinterpret_cast<int8_t*>(ws);
  b->wn = reinterpret_cast<int8_t*>(ws + w.x_bytes);
  b->tapsum = reinterpret_cast<int32_t*>(ws + w.x_bytes + w.w_bytes);
  const hipError_t e = hipMemsetAsync(b->tapsum, 0, (size_t)sums * 4, s);
  if (e != hipSuccess) return fail(FFQ_ERR_LAUNCH, "hipMemsetAsync: %s", hipGetErrorString(e));
  return FFQ_OK;
}

// ---- the n-axis geometry of the forward convolutions ---------------------------------------------------------------------------

struct ConvGeometry {
  int64_t o[3];  // the output extent per axis
  int64_t Cp, taps, Kp, npos, voxels;  // npos = B * prod(o), voxels = B * prod(in)
  ConvWorkspace ws;
};

// 0 with the geometry filled in, else the status of the first check that fails (no HIP call is made here)
static int conv_geometry(int n, int64_t B, int64_t C, int64_t OC, const int64_t* in, const int64_t* k, const int64_t* s, const int64_t* p,
                         const int64_t* d, int x_channels_last, ConvGeometry* g) {
  int rc = check_conv_axes("convolution", n, B, C, OC, in, k, s, p, d);
  if (rc) return rc;
  rc = check_conv_reduction(C, n, k);
  if (rc) return rc;
  if (x_channels_last && C % 16 != 0) return fail(FFQ_ERR_DTYPE, "channels-last input codes need C %% 16 == 0");
  for (int i = 0; i < n; ++i) {
    const int64_t eff = d[i] * (k[i] - 1) + 1;
    if (in[i] + 2 * p[i] < eff) return fail(FFQ_ERR_ARG, "the dilated filter is larger than the padded input");
    g->o[i] = (in[i] + 2 * p[i] - eff) / s[i] + 1;
  }
  g->Cp = (C + 15) / 16 * 16;
  g->taps = product_capped(1, n, k);
  g->Kp = g->taps * g->Cp;
  g->npos = product_capped(B, n, g->o);
  g->voxels = product_capped(B, n, in);
  if (g->npos >= ((int64_t)1 << 31) || mul_capped(g->voxels, g->Cp, kConvBig) >= kConvBig || OC >= ((int64_t)1 << 31) ||
      mul_capped(g->npos, OC, kConvBig) >= kConvBig || mul_capped(OC, g->taps * (g->Cp / 16), kConvBig) >= kConvBig)
    return fail(FFQ_ERR_ARG, "extent too large for one launch");
  g->ws = conv_workspace(g->voxels * g->Cp, x_channels_last, OC * g->Kp, OC * g->taps + OC);
  return FFQ_OK;
}

// ---- the kernels' argument structs and their instantiations -------------------------------------------------------------------

// The operand fields every convolution's argument struct names alike: the quantization parameters, the bias, the output and its
// quantizer with the code range of `out_num_bits` bits.
template <typename Args>
static void fill_conv_operands(Args& a, const float* x_scale, const float* x_offset, const float* w_scale, const float* w_offset,
                               int w_per_channel, const void* bias, int bias_dt, void* out, const float* out_scale, const float* out_offset,
                               double out_num_bits, int y_dt) {
  a.x_scale = x_scale; a.x_offset = x_offset;
  a.w_scale = w_scale; a.w_offset = w_offset; a.w_per_row = w_per_channel ? 1 : 0;
  a.bias = bias; a.bias_dt = bias_dt;
  a.out = out;
  a.out_scale = out_scale; a.out_offset = out_offset;
  const double lo = -pow(2.0, out_num_bits - 1.0);
  a.out_lo = (float)lo; a.out_hi = (float)(-lo - 1.0);
  a.y_dt = y_dt;
}

template <typename T>
struct OutType {
  using type = T;
};

// launch(OutType<TOut>, bool_constant<REQUANT>): the four instantiations every convolution kernel has — int8 codes from the
// output quantizer, else the real dtype `out_dt` (checked by check_conv_output).
template <typename F>
static void dispatch_conv_output(bool requant, int out_dt, F&& launch) {
  if (requant) {
    launch(OutType<int8_t>{}, std::true_type{});
  } else {
    switch (out_dt) {
      case FFQ_BF16: launch(OutType<bf16_t>{}, std::false_type{}); break;
      case FFQ_F16: launch(OutType<f16_t>{}, std::false_type{}); break;
      default: launch(OutType<float>{}, std::false_type{}); break;
    }
  }
}

}  // namespace ffq
