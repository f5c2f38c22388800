// ffq_conv_tile.h — what the two implicit-GEMM convolutions (ffq_conv.hip, ffq_conv_transpose.hip) share: the MFMA operand types,
// the swizzled LDS address of a 128 x 64 operand tile, the 16-channel packing of the layout passes with their common input half,
// and the epilogue of one output element (include/ffq.h, ffq_conv2d_w8a8: fp32, left to right, no FMA).
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
