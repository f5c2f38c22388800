// ffq_depthwise.hip — the W8A8 depthwise convolution (groups == C, channel multiplier M >= 1) as a direct int8 stencil on gfx950.
//
// Replaces fallback.conv2d / fallback.conv1d (src/fastforward/_gen/fallback.py:116-214) for groups == C: the reference dequantizes
// input and weight codes, runs a float grouped convolution and optionally re-quantizes. Here the codes of ONE input channel are
// contracted exactly in int32 and the affine parameters are applied once per output element (include/ffq_depthwise.h), with the
// epilogue helpers of the implicit GEMMs (ffq_conv_tile.h: conv_affine, conv_store, tap_range), so that output channel n is bit for
// bit what ffq_conv2d_w8a8 gives on the one-channel slice x[:, n / M], w[n].
//
// The implicit GEMM cannot serve this shape (one channel of a 16-channel run: 15/16 of every MFMA wasted); a depthwise convolution
// is a stencil bound by memory. One launch, no workspace:
//   * a block owns a LY x (4 * LX) tile of one output plane (b, n); a lane owns 4 consecutive outputs of one row (lanes along OW).
//     LX and LY are powers of two the host fits to the plane (LX * LY <= 256 threads: 16 x 16 for a 56 x 56 plane, 1 x 256 for a
//     1-D convolution);
//   * the channel's taps sit in LDS for the whole block, one zero-padded row of 4 * ceil(KW / 4) bytes per kernel row;
//   * the input patch under the tile is staged in LDS once (zeros outside the image), from aligned 4-byte global loads where the
//     image's rows allow it (W % 4 == 0), so every input byte leaves HBM about once and the KH * KW-fold reuse is served on chip;
//   * kDense (stride_w == dil_w == 1): per kernel row and group of 4 taps a lane reads 2 dwords of the patch and one dword of taps,
//     forms its 4 windows with v_alignbyte and contracts them with v_dot4_i32_i8 (the code sum rsx with a mask of ones);
//     kStrided: one byte per tap and output from the staged patch; kDirect (a patch above the LDS budget: very large dilation or
//     stride): the same loop on bounds-checked global bytes, served by the caches;
//   * the 4 results leave as one 4 / 8 / 16-byte store (codes / 16-bit / fp32) when OW % 4 == 0, else element by element (the tail form).
#include "ffq_conv_host.h"
#include "ffq_conv_tile.h"

#include "../../include/ffq_depthwise.h"

namespace ffq {
namespace {

constexpr int kRun = 4;                   // consecutive outputs of one lane
constexpr int kDwMaxTaps = 1024;          // KH * KW: one channel's taps stay in LDS (at most 4 KiB with the row padding)
constexpr int64_t kDwLdsBudget = 49152;   // taps + patch; above it the patch is not staged (kDirect)
constexpr int64_t kDwMaxBlocks = 1 << 24;  // blocks of one launch (256 threads each: below 2^32 threads in the grid)
enum { kDense = 0, kStrided = 1, kDirect = 2 };

struct DepthwiseArgs {
  const int8_t* xq;  // [B, C, H, W]
  const int8_t* wq;  // [OC, KH * KW], OC = C * M
  const float* x_scale; const float* x_offset;
  const float* w_scale; const float* w_offset; int w_per_row;
  const void* bias; int bias_dt;
  void* out;  // [B, OC, OH, OW]
  const float* out_scale; const float* out_offset;
  float out_lo, out_hi;
  int y_dt;
  int C, M, OC, H, W, KH, KW, OH, OW;
  int sh, sw, ph, pw, dh, dw;
  int lx_log2, LY;         // the block's lanes: LX = 1 << lx_log2 along OW, LY rows
  int tiles_x, tiles_y;
  int G;                   // ceil(KW / 4): dwords of one padded tap row
  int tap_bytes;           // KH * 4 * G rounded up to 16: where the patch starts
  int pitch, PH;           // the staged patch: PH rows of `pitch` bytes (pitch % 4 == 0)
  int x_vec, out_vec;      // aligned dword loads of the input / one wide store per lane
};

template <typename TOut>
__device__ __forceinline__ void store_run(TOut* dst, const TOut (&v)[kRun]) {
  if constexpr (sizeof(TOut) == 1) {
    *reinterpret_cast<uint32_t*>(dst) = __builtin_bit_cast(uint32_t, v);
  } else if constexpr (sizeof(TOut) == 2) {
    *reinterpret_cast<u32x2*>(dst) = __builtin_bit_cast(u32x2, v);
  } else {
    *reinterpret_cast<u32x4*>(dst) = __builtin_bit_cast(u32x4, v);
  }
}

template <typename TOut, bool REQUANT, int MODE>
__global__ __launch_bounds__(256) void depthwise_w8a8_kernel(DepthwiseArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];  // [KH][4 G] taps, then [PH][pitch] patch
  __shared__ int wsum_s[4];

  const int tid = threadIdx.x, nthreads = blockDim.x;
  const int LX = 1 << a.lx_log2;
  const int lx = tid & (LX - 1), ly = tid >> a.lx_log2;
  uint32_t blk = blockIdx.x;
  const int tx = blk % a.tiles_x; blk /= a.tiles_x;
  const int ty = blk % a.tiles_y; blk /= a.tiles_y;
  const int n = blk % a.OC, b = blk / a.OC;
  const int c = n / a.M;
  const int taps = a.KH * a.KW, row4 = 4 * a.G;
  const int8_t* wrow = a.wq + (int64_t)n * taps;
  const int8_t* xplane = a.xq + ((int64_t)b * a.C + c) * a.H * a.W;

  // the channel's taps, each kernel row padded with zeros to 4 G bytes; the sum of all of them (rsw of an unclipped window)
  for (int i = tid; i < a.KH * row4; i += nthreads) {
    const int kh = i / row4, kw = i - kh * row4;
    lds[i] = kw < a.KW ? (uint8_t)wrow[kh * a.KW + kw] : (uint8_t)0;
  }
  {
    int s = 0;
    for (int i = tid; i < taps; i += nthreads) s += wrow[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((tid & 63) == 0) wsum_s[tid >> 6] = s;
  }
  uint8_t* patch = lds + a.tap_bytes;
  const int TW = LX * kRun;
  if constexpr (MODE != kDirect) {
    // patch column 0 is input column iw0; the loads walk 4-byte groups aligned in the image (whole dwords where x_vec allows)
    const int ih0 = ty * a.LY * a.sh - a.ph, iw0 = tx * TW * a.sw - a.pw;
    const int iwb = iw0 & ~3;
    const int ngrp = (iw0 + a.pitch - iwb + 3) >> 2;
    for (int i = tid; i < a.PH * ngrp; i += nthreads) {
      const int pr = i / ngrp, j = i - pr * ngrp;
      const int ih = ih0 + pr, iw4 = iwb + 4 * j;
      uint32_t v = 0;
      if ((unsigned)ih < (unsigned)a.H) {
        const int8_t* src = xplane + (int64_t)ih * a.W + iw4;
        if (a.x_vec && iw4 >= 0 && iw4 + 4 <= a.W) {
          v = *reinterpret_cast<const uint32_t*>(src);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if ((unsigned)(iw4 + e) < (unsigned)a.W) v |= (uint32_t)(uint8_t)src[e] << (8 * e);
        }
      }
      const int col = iw4 - iw0;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if ((unsigned)(col + e) < (unsigned)a.pitch) patch[pr * a.pitch + col + e] = (uint8_t)(v >> (8 * e));
    }
  }
  __syncthreads();

  const int oh = ty * a.LY + ly, ow0 = tx * TW + lx * kRun;
  if (ly >= a.LY || oh >= a.OH || ow0 >= a.OW) return;  // (no barrier below)
  const bool want_rsx = a.w_offset != nullptr;
  int acc[kRun] = {0, 0, 0, 0}, rs[kRun] = {0, 0, 0, 0};

  if constexpr (MODE == kDense) {
    const uint32_t* tap4 = reinterpret_cast<const uint32_t*>(lds);
    const uint32_t last_ones = 0x01010101u >> (8 * (row4 - a.KW));
    for (int kh = 0; kh < a.KH; ++kh) {
      const uint32_t* row = reinterpret_cast<const uint32_t*>(patch + (ly * a.sh + kh * a.dh) * a.pitch) + lx;
      for (int g = 0; g < a.G; ++g) {
        const uint32_t w = tap4[kh * a.G + g], d0 = row[g], d1 = row[g + 1];
        const uint32_t x[kRun] = {d0, __builtin_amdgcn_alignbyte(d1, d0, 1), __builtin_amdgcn_alignbyte(d1, d0, 2),
                                  __builtin_amdgcn_alignbyte(d1, d0, 3)};
#pragma unroll
        for (int r = 0; r < kRun; ++r) acc[r] = __builtin_amdgcn_sdot4((int)x[r], (int)w, acc[r], false);
        if (want_rsx) {
          const uint32_t ones = g == a.G - 1 ? last_ones : 0x01010101u;
#pragma unroll
          for (int r = 0; r < kRun; ++r) rs[r] = __builtin_amdgcn_sdot4((int)x[r], (int)ones, rs[r], false);
        }
      }
    }
  } else {
    const int8_t* tap = reinterpret_cast<const int8_t*>(lds);
    const int nrun = a.OW - ow0 < kRun ? a.OW - ow0 : kRun;
    for (int kh = 0; kh < a.KH; ++kh) {
      const int8_t* prow = reinterpret_cast<const int8_t*>(patch) + (ly * a.sh + kh * a.dh) * a.pitch;
      const int ih = oh * a.sh - a.ph + kh * a.dh;
      for (int kw = 0; kw < a.KW; ++kw) {
        const int w = tap[kh * row4 + kw];
#pragma unroll
        for (int r = 0; r < kRun; ++r) {
          int x = 0;
          if constexpr (MODE == kStrided) {
            x = prow[(lx * kRun + r) * a.sw + kw * a.dw];
          } else if (r < nrun) {
            const int iw = (ow0 + r) * a.sw - a.pw + kw * a.dw;
            if ((unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W) x = xplane[(int64_t)ih * a.W + iw];
          }
          acc[r] += x * w;
          rs[r] += x;
        }
      }
    }
  }

  // epilogue: ffq_conv2d_w8a8's, with C = 1
  const int8_t* tap = reinterpret_cast<const int8_t*>(lds);
  const int np = a.w_per_row ? n : 0;
  const float sx = a.x_scale[0], sw = a.w_scale[np];
  const float ox = a.x_offset ? rne(a.x_offset[0]) : 0.0f;
  const float ow = a.w_offset ? rne(a.w_offset[np]) : 0.0f;
  const float bias = a.bias ? (float)load_any(a.bias, a.bias_dt, n) : 0.0f;
  float oscale = 1.0f, ooff = 0.0f;
  if constexpr (REQUANT) {
    oscale = a.out_scale[0];
    ooff = a.out_offset ? rne(a.out_offset[0]) : 0.0f;
  }
  const int wsum = wsum_s[0] + (nthreads > 64 ? wsum_s[1] : 0) + (nthreads > 128 ? wsum_s[2] + wsum_s[3] : 0);
  int kh_lo, kh_hi;
  tap_range(oh * a.sh - a.ph, a.dh, a.KH, a.H, kh_lo, kh_hi);
  TOut res[kRun];
#pragma unroll
  for (int r = 0; r < kRun; ++r) {
    const int ow_ = ow0 + r < a.OW ? ow0 + r : a.OW - 1;  // (a lane past the row's end repeats the last column and stores nothing)
    int kw_lo, kw_hi;
    tap_range(ow_ * a.sw - a.pw, a.dw, a.KW, a.W, kw_lo, kw_hi);
    const float cnt = (float)((kh_hi - kh_lo) * (kw_hi - kw_lo));  // |V(p)| <= 1024: exact
    float rsw = 0.0f;
    if (ox != 0.0f) {  // sum of the weight codes over the taps inside the image (the whole row away from the border)
      if (kh_lo == 0 && kh_hi == a.KH && kw_lo == 0 && kw_hi == a.KW) {
        rsw = (float)wsum;
      } else {
        int s = 0;
        for (int y = kh_lo; y < kh_hi; ++y)
          for (int x = kw_lo; x < kw_hi; ++x) s += tap[y * row4 + x];
        rsw = (float)s;
      }
    }
    const float y = conv_affine(acc[r], ox, rsw, ow, want_rsx ? (float)rs[r] : 0.0f, cnt, sx, sw, a.bias != nullptr, bias);
    conv_store<TOut, REQUANT>(&res[r], y, a.y_dt, oscale, ooff, a.out_lo, a.out_hi);
  }
  TOut* dst = static_cast<TOut*>(a.out) + (((size_t)b * a.OC + n) * a.OH + oh) * a.OW + ow0;
  if (a.out_vec) {  // OW % 4 == 0: the run is whole and aligned
    store_run<TOut>(dst, res);
  } else {
#pragma unroll
    for (int r = 0; r < kRun; ++r)
      if (ow0 + r < a.OW) dst[r] = res[r];
  }
}

int pow2_at_least(int64_t v, int cap) {
  int p = 1;
  while (p < cap && p < v) p <<= 1;
  return p;
}

template <typename TOut, bool REQUANT>
void launch_depthwise(int mode, unsigned grid, unsigned block, size_t lds_bytes, hipStream_t s, const DepthwiseArgs& a) {
  switch (mode) {
    case kDense: depthwise_w8a8_kernel<TOut, REQUANT, kDense><<<grid, block, lds_bytes, s>>>(a); break;
    case kStrided: depthwise_w8a8_kernel<TOut, REQUANT, kStrided><<<grid, block, lds_bytes, s>>>(a); break;
    default: depthwise_w8a8_kernel<TOut, REQUANT, kDirect><<<grid, block, lds_bytes, s>>>(a); break;
  }
}

}  // namespace
}  // namespace ffq

using namespace ffq;

extern "C" int ffq_depthwise_conv2d_w8a8(const int8_t* xq, const int8_t* wq, const float* x_scale, const float* x_offset,
                                         const float* w_scale, const float* w_offset, int w_per_channel, const void* bias, int bias_dt,
                                         void* out, int out_dt, const float* out_scale, const float* out_offset, double out_num_bits,
                                         int y_dt, int64_t B, int64_t C, int64_t M, int64_t H, int64_t W, int64_t KH, int64_t KW,
                                         int64_t stride_h, int64_t stride_w, int64_t pad_h, int64_t pad_w, int64_t dil_h, int64_t dil_w,
                                         void* stream) {
  if (B < 0 || C < 0 || M < 0 || H < 0 || W < 0 || KH < 0 || KW < 0) return fail(FFQ_ERR_ARG, "negative extent");
  if (M == 0 || KH == 0 || KW == 0) return fail(FFQ_ERR_EMPTY, "a convolution over an empty filter");
  if (stride_h < 1 || stride_w < 1 || dil_h < 1 || dil_w < 1 || pad_h < 0 || pad_w < 0)
    return fail(FFQ_ERR_ARG, "stride and dilation >= 1, padding >= 0");
  const int64_t lim = (int64_t)1 << 24;
  if (H > lim || W > lim || KH > lim || KW > lim || stride_h > lim || stride_w > lim || dil_h > lim || dil_w > lim || pad_h > lim ||
      pad_w > lim)
    return fail(FFQ_ERR_ARG, "extent, stride, padding or dilation above 2^24");
  if (KH * KW > kDwMaxTaps)
    return fail(FFQ_ERR_DTYPE, "KH * KW = %lld exceeds %d (one channel's taps are held on chip)", (long long)(KH * KW), kDwMaxTaps);
  const int64_t eff_h = dil_h * (KH - 1) + 1, eff_w = dil_w * (KW - 1) + 1;
  if (H + 2 * pad_h < eff_h || W + 2 * pad_w < eff_w) return fail(FFQ_ERR_ARG, "the dilated filter is larger than the padded input");
  const int64_t OH = (H + 2 * pad_h - eff_h) / stride_h + 1, OW = (W + 2 * pad_w - eff_w) / stride_w + 1;
  const int64_t big = (int64_t)1 << 40, i31 = (int64_t)1 << 31;
  // (every factor is below 2^31 once the check before it has passed, so no product here overflows int64)
  if (B >= i31 || C >= i31 || M >= i31 || C * M >= i31 || OH * OW >= i31 || B * (OH * OW) >= i31 || B * C >= big / (H * W + 1) ||
      B * (C * M) >= big / (OH * OW))
    return fail(FFQ_ERR_ARG, "extent too large for one launch");
  const int64_t OC = C * M;
  // the block's lanes: 16 along OW (64 outputs) unless the plane is narrower; then as many rows as the plane has, and wider again
  const int lx_want = pow2_at_least((OW + kRun - 1) / kRun, 256), ly_want = pow2_at_least(OH, 256);
  int LX = lx_want < 16 ? lx_want : 16, LY = 256 / LX;
  if (LY > ly_want) {
    LY = ly_want;
    LX = lx_want < 256 / LY ? lx_want : 256 / LY;
  }
  const int64_t TW = (int64_t)LX * kRun;
  const int64_t tiles_x = (OW + TW - 1) / TW, tiles_y = (OH + LY - 1) / LY;
  if (B * OC >= kDwMaxBlocks / (tiles_x * tiles_y)) return fail(FFQ_ERR_ARG, "extent too large for one launch");
  const bool requant = out_scale != nullptr;
  int rc = check_conv_output("convolution", bias, bias_dt, requant, out_dt, out_num_bits, y_dt);
  if (rc) return rc;
  if (B == 0 || C == 0) return FFQ_OK;
  if (!xq || !wq || !x_scale || !w_scale || !out) return fail(FFQ_ERR_ARG, "NULL buffer");

  DepthwiseArgs a;
  a.xq = xq; a.wq = wq;
  fill_conv_operands(a, x_scale, x_offset, w_scale, w_offset, w_per_channel, bias, bias_dt, out, out_scale, out_offset, out_num_bits, y_dt);
  a.C = (int)C; a.M = (int)M; a.OC = (int)OC; a.H = (int)H; a.W = (int)W; a.KH = (int)KH; a.KW = (int)KW; a.OH = (int)OH; a.OW = (int)OW;
  a.sh = (int)stride_h; a.sw = (int)stride_w; a.ph = (int)pad_h; a.pw = (int)pad_w; a.dh = (int)dil_h; a.dw = (int)dil_w;
  a.lx_log2 = __builtin_ctz((unsigned)LX); a.LY = LY;
  a.tiles_x = (int)tiles_x; a.tiles_y = (int)tiles_y;
  a.G = (int)((KW + 3) / 4);
  a.tap_bytes = (int)((KH * 4 * a.G + 15) / 16 * 16);
  int mode = stride_w == 1 && dil_w == 1 ? kDense : kStrided;
  const int64_t pitch = mode == kDense ? TW + 4 * a.G : ((TW - 1) * stride_w + (KW - 1) * dil_w + 1 + 3) / 4 * 4;
  const int64_t PH = (LY - 1) * stride_h + (KH - 1) * dil_h + 1;
  if (a.tap_bytes + pitch * PH > kDwLdsBudget) mode = kDirect;
  a.pitch = mode == kDirect ? 0 : (int)pitch;
  a.PH = mode == kDirect ? 0 : (int)PH;
  const size_t lds_bytes = (size_t)a.tap_bytes + (size_t)a.pitch * a.PH;
  const size_t esize = requant ? 1 : (out_dt == FFQ_F32 ? 4 : 2);
  a.x_vec = W % 4 == 0 && (reinterpret_cast<uintptr_t>(xq) & 3u) == 0;
  a.out_vec = OW % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & (kRun * esize - 1)) == 0;
  const unsigned grid = (unsigned)(B * OC * tiles_x * tiles_y);
  const unsigned block = LX * LY < 64 ? 64u : (unsigned)(LX * LY);
  hipStream_t s = static_cast<hipStream_t>(stream);
  dispatch_conv_output(requant, out_dt, [&](auto t, auto q) {
    launch_depthwise<typename decltype(t)::type, decltype(q)::value>(mode, grid, block, lds_bytes, s, a);
  });
  return check_launch("depthwise_w8a8_kernel");
}
