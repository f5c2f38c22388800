// ffq_epilogue.h — the int8 contractions' shared epilogue helpers: ffq_linear.hip (A6) and ffq_conv.hip (the W8A8 convolution).
// round_to_dt gives the value the op would have returned in its real-valued dtype (the one rounding before a fused A1);
// store_out writes one fp32 result into the output container.
#pragma once

#include "ffq_common.h"
#include "ffq_vec.h"

namespace ffq {

// The value the linear would have returned in dtype `y_dt` (one rounding), as fp32
__device__ __forceinline__ float round_to_dt(float y, int y_dt) {
  if (y_dt == FFQ_BF16) return bf16_bits_to_f32(f32_to_bf16_bits(y));
  if (y_dt == FFQ_F16) return (float)(_Float16)y;
  return y;
}

template <typename TOut>
__device__ __forceinline__ void store_out(TOut* p, float v);
template <> __device__ __forceinline__ void store_out<float>(float* p, float v) { *p = v; }
template <> __device__ __forceinline__ void store_out<bf16_t>(bf16_t* p, float v) { *p = from_f32<bf16_t>(v); }
template <> __device__ __forceinline__ void store_out<f16_t>(f16_t* p, float v) { *p = from_f32<f16_t>(v); }
template <> __device__ __forceinline__ void store_out<int8_t>(int8_t* p, float v) { *p = from_f32<int8_t>(v); }

}  // namespace ffq
