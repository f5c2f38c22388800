// ffq_unfold.hip — the reference's quantized unfold (im2col) as a one-pass kernel with A1 fused in.
//
// ff.nn.functional.unfold runs its generated fallback in the reference (_gen/fallback.py: unfold :1650): A2 of the quantized input
// into a data-dtype tensor, ATen's im2col into a tensor KH * KW times larger, A1 of the output quantizer over that tensor. The
// operator only moves data, so here it is one pass under the A2 / A1 contract of ffq_onepass.h with nothing in between: an output
// element is A2 of the input element it comes from (a plain element keeps its bits), or +0.0 where the window lies in the padding,
// and the codes are A1 of that value.
//   Lanes walk the flattened result [B * C * KH * KW, L]: a unit is a group of 8 consecutive columns of one row (8 | L, so every
//   row base is 16-byte aligned: one 16 B value store and one 8 B store per quantizer) or one element (any other L). Stores run
//   along L and so do the reads: neighbouring lanes read neighbouring pieces of one input row. A group may span output rows (OW is
//   not a multiple of 8; several when OW < 8), so (oh, ow) advances per element. A group that lies inside one output row of a
//   stride-1 window reads its 8 inputs with one load, at whatever alignment the tap leaves it: at the left and right edge of the
//   image the load is moved to the nearest 8 elements inside the row and the chunk is shifted by whole elements, which brings in
//   the +0.0 of the padding; a group wholly in the padding is zeros.
//   The input is read from global memory through the caches (every element is read KH * KW / (stride_h * stride_w) times, by
//   blocks that run close together in time); the patch is not staged in LDS. No LDS, no cross-lane traffic.
#include "ffq_onepass.h"

#include "../../include/ffq_unfold.h"

namespace ffq {
namespace unfold {

// 8 consecutive elements from an address that is only element-aligned (the tap shifts the row by any amount).
template <typename TIn>
__device__ __forceinline__ Chunk<TIn, kE> load_unaligned(const TIn* p) {
  Chunk<TIn, kE> q;
  __builtin_memcpy(q.w, p, sizeof(q.w));
  return q;
}

// ---------------------------------------------------------------------------------------------------
// U1: unfold of [B, C, H, W] + A1. A unit is a group of 8 outputs of one row of the result (VEC: 8 | L) or one output.
//     Algorithmic bytes: the input once (2 B bf16 / 1 B int8 per element) + per output [2 (z)] + 1 per code tensor.
// ---------------------------------------------------------------------------------------------------
struct Geometry {
  uint32_t units;        // groups or elements of the result
  int32_t H, W, OW;
  int32_t sh, sw, ph, pw, dh, dw;
  int32_t per_channel;   // C parameter pairs, indexed by plane % C
  FastDiv by_row;        // units per row of the result (L / 8 or L)
  FastDiv by_taps;       // KH * KW: row of the result -> (plane = b * C + c, tap)
  FastDiv by_kw, by_ow, by_c;
};

template <typename T, typename TIn, bool DEQ, bool VEC>
__global__ __launch_bounds__(kBlock) void unfold_quantize_kernel(const TIn* __restrict__ x, const float* __restrict__ xs,
                                                                 const float* __restrict__ xo, Geometry g, T* __restrict__ out, FanOut f) {
  constexpr uint32_t kWidth = VEC ? kE : 1;
  const uint32_t u = blockIdx.x * kBlock + threadIdx.x;  // (one unit per lane: the geometry and the fan-out fill the scalar registers)
  if (u >= g.units) return;
  const uint32_t row = fdiv(u, g.by_row);
  const uint32_t col = (u - row * g.by_row.div) * kWidth;
  const uint32_t plane = fdiv(row, g.by_taps);
  const uint32_t tap = row - plane * g.by_taps.div;
  const uint32_t kh = fdiv(tap, g.by_kw);
  const uint32_t kw = tap - kh * g.by_kw.div;
  uint32_t oh = fdiv(col, g.by_ow);
  uint32_t ow = col - oh * g.by_ow.div;
  float s = 1.0f, o = 0.0f;
  if constexpr (DEQ) {
    const uint32_t p = g.per_channel ? plane - fdiv(plane, g.by_c) * g.by_c.div : 0u;
    s = xs[p];
    o = xo ? rne(xo[p]) : 0.0f;
  }
  const TIn* from = x + (size_t)plane * (size_t)g.H * (size_t)g.W;
  const int32_t h0 = (int32_t)kh * g.dh - g.ph, w0 = (int32_t)kw * g.dw - g.pw;  // the tap's position at (oh, ow) = (0, 0)
  int32_t ih = (int32_t)oh * g.sh + h0, iw = (int32_t)ow * g.sw + w0;
  const T zero = __builtin_bit_cast(T, (uint16_t)0);  // +0.0
  const FanParams fp = load_fan(f);
  const size_t at = (size_t)u * kWidth;
  if constexpr (VEC) {
    Chunk<T, kE> h;
    if (g.sw == 1 && g.W >= (int32_t)kE && ow + kE <= (uint32_t)g.OW) {  // 8 neighbours of one row of the image (or of the padding beside it)
      if (ih < 0 || ih >= g.H || iw <= -(int32_t)kE || iw >= g.W) {       // wholly in the padding
#pragma unroll
        for (int k = 0; k < Chunk<T, kE>::kWords; ++k) h.w[k] = 0u;
      } else {
        // one load of the 8 elements at the nearest column that keeps them inside the row, then a shift by whole elements:
        // out[k] = in[k + shift], and the elements the shift brings in from outside the row are the +0.0 of the padding
        const int32_t c0 = min(max(iw, 0), g.W - (int32_t)kE);
        const TIn* p = from + (size_t)ih * g.W + c0;
        if constexpr (DEQ) {
          float v[kE];
          a2_chunk(load_unaligned(p), s, o, v);
          h.pack(v);
        } else {
          h = load_unaligned(reinterpret_cast<const T*>(p));
        }
        const int32_t shift = iw - c0;  // in (-8, 8)
        if (shift != 0) {
          const uint64_t lo = (uint64_t)h.w[0] | ((uint64_t)h.w[1] << 32), hi = (uint64_t)h.w[2] | ((uint64_t)h.w[3] << 32);
          unsigned __int128 v = (unsigned __int128)lo | ((unsigned __int128)hi << 64);
          v = shift > 0 ? v >> (16 * shift) : v << (-16 * shift);
          h.w[0] = (uint32_t)v; h.w[1] = (uint32_t)(v >> 32); h.w[2] = (uint32_t)(v >> 64); h.w[3] = (uint32_t)(v >> 96);
        }
      }
    } else {  // a strided window, a row narrower than 8, or a group over several output rows: element by element
      uint16_t e[kE];
#pragma unroll
      for (int k = 0; k < kE; ++k) {
        const bool inside = ih >= 0 && ih < g.H && iw >= 0 && iw < g.W;
        const T v = inside ? element<T, TIn, DEQ>(from, (size_t)ih * g.W + iw, s, o) : zero;
        e[k] = __builtin_bit_cast(uint16_t, v);
        ++ow;
        iw += g.sw;
        if (ow == (uint32_t)g.OW) {  // the next output row (after a row's last group: never read)
          ow = 0;
          iw = w0;
          ih += g.sh;
        }
      }
#pragma unroll
      for (int k = 0; k < kE; k += 2) h.w[k >> 1] = (uint32_t)e[k] | ((uint32_t)e[k + 1] << 16);
    }
    put_group<T>(out, f, fp, h, at);
  } else {
    const bool inside = ih >= 0 && ih < g.H && iw >= 0 && iw < g.W;
    put_one<T>(out, f, fp, inside ? element<T, TIn, DEQ>(from, (size_t)ih * g.W + iw, s, o) : zero, at);
  }
}

// The product of `factors` when it is below 2^31 (0 when a factor is 0), else -1: no int64 overflow on the way.
static int64_t product_below_2_31(std::initializer_list<int64_t> factors) {
  const int64_t limit = (int64_t)1 << 31;
  for (int64_t v : factors)
    if (v == 0) return 0;
  int64_t total = 1;
  for (int64_t v : factors) {
    if (v >= limit || total * v >= limit) return -1;
    total *= v;
  }
  return total;
}

}  // namespace unfold
}  // namespace ffq

using namespace ffq;
using namespace ffq::unfold;

extern "C" int ffq_unfold_quantize(const void* x, int x_dt, const float* x_scale, const float* x_offset, int per_channel, int dt,
                                   int64_t B, int64_t C, int64_t H, int64_t W, int64_t KH, int64_t KW,
                                   int64_t dil_h, int64_t dil_w, int64_t pad_h, int64_t pad_w, int64_t stride_h, int64_t stride_w,
                                   void* out, const ffq_fanout* fan, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (!value_dtype(dt)) return fail(FFQ_ERR_DTYPE, "fused unfold is built for bf16 / fp16 values");
  int rc = check_operand_form("fused unfold", x_dt, x_scale, x_offset, per_channel != 0, dt);
  if (rc) return rc;
  if (B < 0 || C < 0 || H < 0 || W < 0 || KH < 0 || KW < 0) return fail(FFQ_ERR_ARG, "fused unfold: negative extent");
  if (KH == 0 || KW == 0) return fail(FFQ_ERR_EMPTY, "fused unfold: a window of %lld x %lld has no elements", (long long)KH, (long long)KW);
  if (stride_h < 1 || stride_w < 1 || dil_h < 1 || dil_w < 1 || pad_h < 0 || pad_w < 0)
    return fail(FFQ_ERR_ARG, "fused unfold: stride and dilation are at least 1 and padding at least 0");
  const int64_t axis_limit = (int64_t)1 << 24;  // (every 32-bit index of the kernel stays below 2^27: (OH - 1) * stride <= H + 2 * pad)
  for (int64_t v : {H, W, KH, KW, dil_h, dil_w, pad_h, pad_w, stride_h, stride_w})
    if (v > axis_limit) return fail(FFQ_ERR_ARG, "fused unfold: extents, window, stride, dilation and padding are at most 2^24 per axis");
  const int64_t span_h = dil_h * (KH - 1) + 1, span_w = dil_w * (KW - 1) + 1;
  if (span_h > H + 2 * pad_h || span_w > W + 2 * pad_w)
    return fail(FFQ_ERR_ARG, "fused unfold: the dilated window %lld x %lld is larger than the padded image %lld x %lld", (long long)span_h,
                (long long)span_w, (long long)(H + 2 * pad_h), (long long)(W + 2 * pad_w));
  const int64_t OH = (H + 2 * pad_h - span_h) / stride_h + 1, OW = (W + 2 * pad_w - span_w) / stride_w + 1;
  const int64_t total = product_below_2_31({B, C, KH, KW, OH, OW});
  if (product_below_2_31({B, C, H, W}) < 0 || total < 0) return fail(FFQ_ERR_DTYPE, "fused unfold needs fewer than 2^31 input and output elements");
  const bool empty = B == 0 || C == 0;
  FanOut f;
  rc = check_launch_args(fan, total, empty, x, {x, out}, &f);
  if (rc || empty) return rc;
  const int64_t L = OH * OW;
  const bool vec = L % kE == 0;
  Geometry g;
  g.units = (uint32_t)(vec ? total / kE : total);
  g.H = (int32_t)H; g.W = (int32_t)W; g.OW = (int32_t)OW;
  g.sh = (int32_t)stride_h; g.sw = (int32_t)stride_w;
  g.ph = (int32_t)pad_h; g.pw = (int32_t)pad_w;
  g.dh = (int32_t)dil_h; g.dw = (int32_t)dil_w;
  g.per_channel = per_channel != 0;
  g.by_row = make_fastdiv((uint32_t)(vec ? L / kE : L));
  g.by_taps = make_fastdiv((uint32_t)(KH * KW));
  g.by_kw = make_fastdiv((uint32_t)KW);
  g.by_ow = make_fastdiv((uint32_t)OW);
  g.by_c = make_fastdiv((uint32_t)C);
  const unsigned grid = (unsigned)(((uint64_t)g.units + kBlock - 1) / kBlock);
  dispatch_input(dt, x_dt, x_scale != nullptr, [&](auto t, auto tin, auto deq) {
    using T = typename decltype(t)::type;
    using TIn = typename decltype(tin)::type;
    if (vec) unfold_quantize_kernel<T, TIn, decltype(deq)::value, true><<<grid, kBlock, 0, s>>>(static_cast<const TIn*>(x), x_scale, x_offset, g, static_cast<T*>(out), f);
    else unfold_quantize_kernel<T, TIn, decltype(deq)::value, false><<<grid, kBlock, 0, s>>>(static_cast<const TIn*>(x), x_scale, x_offset, g, static_cast<T*>(out), f);
  });
  return check_launch("unfold_quantize_kernel");
}
