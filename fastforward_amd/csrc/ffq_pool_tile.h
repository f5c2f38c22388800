// ffq_pool_tile.h — what the pooling units (ffq_pool.hip: 1-D / 2-D pools and nearest interpolate; ffq_pool3d.hip: avg_pool3d) share
// on top of ffq_onepass.h: one input element as a value of the data dtype, the block's results from LDS to the value and the code
// tensors in 8-element groups, ATen's pooling_output_shape, the dtype checks and the outputs-per-lane choice.
#pragma once

#include "ffq_onepass.h"

namespace ffq {
namespace pool {

template <typename T, typename TIn, bool DEQ>
__device__ __forceinline__ float value_at(const TIn* p, float s, float o) {
  const float q = to_f32(*p);
  if constexpr (DEQ) return a2_value<T>(q, s, o);
  return q;
}

// The block's kBlock * J results (fp32, in LDS) -> the data dtype and the codes, 8 per lane; the tail of the result one by one.
template <typename T, int J>
__device__ __forceinline__ void store_tile(const float* z, uint32_t base, uint32_t total, T* __restrict__ out, const FanOut& f) {
  const FanParams fp = load_fan(f);
  for (uint32_t c = threadIdx.x; c < (uint32_t)(kBlock * J / kE); c += kBlock) {
    const uint32_t at = base + c * kE;
    if (at >= total) return;
    float v[kE];
#pragma unroll
    for (int i = 0; i < kE; ++i) v[i] = z[c * kE + i];
    if (at + kE <= total) {  // (store_chunk's and, below, store_one's steps, spelled out: the helpers change this loop's registers)
      Chunk<T, kE> y;
      y.pack(v);  // the one rounding to the data dtype
      if (out) y.store(out + at);
#pragma unroll
      for (int i = 0; i < kE; ++i) v[i] = y.get(i);
      fan_store(f, fp, v, (size_t)at);
      continue;
    }
    const int ilo = (int)f.lo, ihi = (int)f.hi;
    for (uint32_t i = 0; at + i < total; ++i) {
      const float one[1] = {round_stage(z[c * kE + i], TypeTag<T>::value)};
      if (out) out[at + i] = from_f32<T>(one[0]);
#pragma unroll
      for (int j = 0; j < FFQ_MAX_FANOUT; ++j) {
        if (j >= f.n) break;
        const Divider<1> d(fp.s[j]);
        float r[1];
        quantize_chunk_with<1, 1>(d, one, fp.o[j], r);
        int code = (int)r[0];  // v_cvt_i32_f32 saturates and maps NaN to 0, as finalize_chunk
        code = code < ilo ? ilo : (code > ihi ? ihi : code);
        f.codes[j][at + i] = (int8_t)code;
      }
    }
  }
}

// ATen's pooling_output_shape: the last window starts inside the input or its left padding.
static int64_t pooled(int64_t in, int64_t k, int64_t pad, int64_t stride, int64_t dil, bool ceil_mode) {
  const int64_t num = in + 2 * pad - dil * (k - 1) - 1 + (ceil_mode ? stride - 1 : 0);
  int64_t out = (num >= 0 ? num / stride : -((-num + stride - 1) / stride)) + 1;
  if (ceil_mode && (out - 1) * stride >= in + pad) --out;
  return out;
}

// The checks both entry points share: dtypes first (before any buffer is looked at), then extents and buffers.
static int check_dtypes(const char* what, int x_dt, const float* scale, const float* offset, int64_t channels, int dt) {
  if (!value_dtype(dt)) return fail(FFQ_ERR_DTYPE, "%s is built for bf16 / fp16 values", what);
  return check_operand_form(what, x_dt, scale, offset, channels != 0, dt);
}

// Outputs per lane: 8 when that still leaves two blocks per CU of a 256-CU device, else 1 (small results want the lanes).
static int per_lane(uint32_t total) { return total >= 8u * kBlock * 512u ? 8 : 1; }

}  // namespace pool
}  // namespace ffq
