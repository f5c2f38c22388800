// ffq_conv_tile.h — what the implicit-GEMM convolutions (ffq_conv.hip, ffq_conv3d.hip, ffq_conv_transpose.hip) share: the MFMA
// operand types, the swizzled LDS address of a 128 x 64 operand tile, the 16-channel packing of the layout passes with their common
// input half (and the weight half of the two forward convolutions), the valid-tap range of one axis, and the epilogue of one output
// element (include/ffq.h, ffq_conv2d_w8a8: fp32, left to right, no FMA).
#pragma once

#include "ffq_affine.h"
#include "ffq_common.h"
#include "ffq_epilogue.h"
#include "ffq_vec.h"

namespace ffq {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

constexpr int kConvBK = 64;  // k-bytes of one staged operand row

// byte address of 16-byte slot `slot` of row `row` in a [128][64] operand tile: the slot index is XORed with two row bits
__device__ __forceinline__ uint32_t conv_swizzled(uint32_t row, uint32_t slot) {
  return row * kConvBK + ((slot ^ ((row >> 2) & 3u)) << 4);
}

__device__ __forceinline__ u32x4 pack16(const uint8_t (&v)[16]) {
  u32x4 packed;
  packed.x = v[0] | (v[1] << 8) | (v[2] << 16) | ((uint32_t)v[3] << 24);
  packed.y = v[4] | (v[5] << 8) | (v[6] << 16) | ((uint32_t)v[7] << 24);
  packed.z = v[8] | (v[9] << 8) | (v[10] << 16) | ((uint32_t)v[11] << 24);
  packed.w = v[12] | (v[13] << 8) | (v[14] << 16) | ((uint32_t)v[15] << 24);
  return packed;
}

// The input half of a layout pass: thread idx moves one (b, 16-channel group, pixel), pixel fastest, so that each of the 16 byte
// loads of a wave reads 64 consecutive bytes of one channel plane; the 16 bytes leave as one store into [B, HW, groups * 16].
__device__ __forceinline__ void nchw_to_nhwc16(const int8_t* __restrict__ x, int8_t* __restrict__ xn, int64_t idx, int C, int64_t HW,
                                               int groups) {
  const int64_t hw = idx % HW, rest = idx / HW;
  const int g = (int)(rest % groups);
  const int64_t b = rest / groups;
  uint8_t v[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int c = g * 16 + k;
    v[k] = c < C ? (uint8_t)x[(b * C + c) * HW + hw] : (uint8_t)0;
  }
  *reinterpret_cast<u32x4*>(xn + (b * HW + hw) * (groups * 16) + g * 16) = pack16(v);
}

// The weight half of a layout pass: thread j moves one (n, tap, 16-channel group) of [OC, C, taps] into [OC, taps, Cp = groups * 16], and
// adds the group's code sum into tapsum[n, tap] and into the total of row n (both zeroed ahead of the launch).
__device__ __forceinline__ void weight_to_taps16(const int8_t* __restrict__ w, int8_t* __restrict__ wn, int64_t j, int C, int groups, int Cp,
                                                 int taps, int OC, int32_t* __restrict__ tapsum) {
  const int g = (int)(j % groups);
  const int64_t row_tap = j / groups;  // n * taps + t
  const int t = (int)(row_tap % taps);
  const int64_t n = row_tap / taps;
  uint8_t v[16];
  int sum = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int c = g * 16 + k;
    const int8_t q = c < C ? w[(n * C + c) * taps + t] : (int8_t)0;
    v[k] = (uint8_t)q;
    sum += q;
  }
  *reinterpret_cast<u32x4*>(wn + row_tap * Cp + g * 16) = pack16(v);
  if (sum != 0) {
    atomicAdd(tapsum + row_tap, sum);
    atomicAdd(tapsum + (int64_t)OC * taps + n, sum);
  }
}

// [lo, hi) of the taps k with 0 <= o0 + k * d < extent
__device__ __forceinline__ void tap_range(int o0, int d, int taps, int extent, int& lo, int& hi) {
  lo = o0 >= 0 ? 0 : (-o0 + d - 1) / d;
  hi = extent - o0 <= 0 ? 0 : (extent - o0 + d - 1) / d;
  hi = hi < taps ? hi : taps;
  if (hi < lo) hi = lo;
}

// y of one output element from its exact accumulator and the offset terms
__device__ __forceinline__ float conv_affine(int acc, float ox, float rsw, float ow, float rsx, float cnt, float sx, float sw, bool has_bias,
                                             float bias) {
  float v = (float)acc;
  v = v + ox * rsw;
  v = v + ow * rsx;
  v = v + cnt * ox * ow;
  float y = (sx * sw) * v;
  if (has_bias) y = y + bias;
  return y;
}

// y into `dst`, or with REQUANT its code: y rounded once to y_dt, then A1
template <typename TOut, bool REQUANT>
__device__ __forceinline__ void conv_store(TOut* dst, float y, int y_dt, float oscale, float ooff, float lo, float hi) {
  if constexpr (REQUANT) {
    y = round_to_dt(y, y_dt);
    float qv = rne(y / oscale - ooff);
    qv = clamp_nan(qv, lo, hi);
    store_out<TOut>(dst, qv);
  } else {
    store_out<TOut>(dst, y);
  }
}

}  // namespace ffq
