// ffq_fanout.h — the static per-tensor A1 outputs ("fan-out", include/ffq.h ffq_fanout) of the one-pass producer kernels:
// ffq_producers.hip (RMSNorm / SiLU*up behind the Llama recipe) and ffq_modules.hip (LayerNorm / Embedding / ReLU / SiLU).
// The host half validates an ffq_fanout before any launch; the device half quantizes a chunk of values for every quantizer.
#pragma once

#include "ffq_affine.h"
#include "ffq_common.h"
#include "ffq_vec.h"

#include <math.h>

namespace ffq {

struct FanOut {
  const float* scale[FFQ_MAX_FANOUT];
  const float* offset[FFQ_MAX_FANOUT];
  int8_t* codes[FFQ_MAX_FANOUT];
  int n;
  float lo, hi;
};

// Round two fp32 values to bf16 and back with ONE v_cvt_pk_bf16_f32 (RNE) + two bit moves, instead of the
// ~6-instruction integer sequence per value: the producers round after every ATen op of the eager chain.
__device__ __forceinline__ void bf16_round2(float& a, float& b) {
  const uint32_t w = pack2<bf16_t>(a, b);
  a = __builtin_bit_cast(float, w << 16);
  b = __builtin_bit_cast(float, w & 0xFFFF0000u);
}

// E (16 or 8) floats that hold values of the data dtype -> int8 codes for every quantizer of the fan-out. Quantizers that hold the same
// (scale, offset) — q/k/v_proj see the same tensor, so RunningMinMax gives them the same range — reuse
// the codes of the first one (wave-uniform test).
struct FanParams {
  float s[FFQ_MAX_FANOUT], o[FFQ_MAX_FANOUT];
};
__device__ __forceinline__ FanParams load_fan(const FanOut& f) {
  FanParams p;
#pragma unroll
  for (int j = 0; j < FFQ_MAX_FANOUT; ++j) {
    p.s[j] = 1.0f;
    p.o[j] = 0.0f;
    if (j < f.n) {
      p.s[j] = f.scale[j][0];
      p.o[j] = f.offset[j] ? rne(f.offset[j][0]) : 0.0f;
    }
  }
  return p;
}
template <int E>
__device__ __forceinline__ void fan_store(const FanOut& f, const FanParams& p, const float (&z)[E], size_t at) {
  Chunk<int8_t, E> y[FFQ_MAX_FANOUT];
#pragma unroll
  for (int j = 0; j < FFQ_MAX_FANOUT; ++j) {
    if (j >= f.n) break;
    bool reuse = false;
#pragma unroll
    for (int i = 0; i < j; ++i) {
      if (!reuse && p.s[i] == p.s[j] && p.o[i] == p.o[j]) {
        y[j] = y[i];
        reuse = true;
      }
    }
    if (!reuse) quantize_chunk_to_bytes<E>(z, p.s[j], p.o[j], f.lo, f.hi, y[j]);
    y[j].FFQ_SSTORE(f.codes[j] + at);
  }
}

static inline int fan_from_abi(const ffq_fanout* fan, int64_t numel, FanOut* out) {
  out->n = 0;
  out->lo = out->hi = 0.0f;
  for (int j = 0; j < FFQ_MAX_FANOUT; ++j) { out->scale[j] = nullptr; out->offset[j] = nullptr; out->codes[j] = nullptr; }
  if (!fan) return FFQ_OK;
  if (fan->count < 0 || fan->count > FFQ_MAX_FANOUT) return fail(FFQ_ERR_ARG, "fan-out count must be 0..%d", FFQ_MAX_FANOUT);
  if (fan->count == 0) return FFQ_OK;
  if (!(fan->num_bits >= 1 && fan->num_bits <= 8 && fan->num_bits == floor(fan->num_bits)))
    return fail(FFQ_ERR_PRECISION, "Provided dtype (%d) is not enough to store %g bits quantized values.", FFQ_I8, fan->num_bits);
  out->n = fan->count;
  const double lo = -pow(2.0, fan->num_bits - 1.0);
  out->lo = (float)lo;
  out->hi = (float)(-lo - 1.0);
  for (int j = 0; j < fan->count; ++j) {
    if (!fan->scale[j] || !fan->codes[j]) return fail(FFQ_ERR_ARG, "NULL scale / codes in fan-out %d", j);
    if (numel && !aligned16(fan->codes[j])) return fail(FFQ_ERR_ARG, "codes buffer %d must be 16-byte aligned", j);
    out->scale[j] = fan->scale[j];
    out->offset[j] = fan->offset[j];
    out->codes[j] = fan->codes[j];
  }
  return FFQ_OK;
}

}  // namespace ffq
