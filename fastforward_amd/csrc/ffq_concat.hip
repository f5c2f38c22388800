// ffq_concat.hip — the reference's quantized cat and pad as one-pass kernels with A1 fused in.
//
// ff.nn.functional.{cat, pad} run their generated fallbacks in the reference (_gen/fallback.py: cat :1453, pad :1546): A2 of every
// quantized input into a data-dtype tensor (one launch per input of a cat), torch.cat / F.pad, A1 of the output quantizer — N + 2
// launches for a cat of N inputs, with full-size temporaries between them. Both operators only move data, so here each is one pass
// under the A2 / A1 contract of ffq_onepass.h with nothing in between: an output element is A2 of the input element it comes from (a
// plain element keeps its bits), or the fill of a constant pad, and the codes are A1 of that value.
//   cat: along any dim the concatenation is 2-D, input i [outer, run_i] into the columns [col_i, col_i + run_i) of [outer, out_run].
//        The grid is partitioned by input, so the input's form (plain / int8 codes / value-dtype codes, its own scale and offset) is
//        uniform in a block. Lanes walk an input in memory order; only the output index needs a division.
//   pad: lanes walk the flattened output [outer, O2, O1, O0]; an index map per mode gives the input element (or none: the fill).
// Both have a group form — 8 consecutive elements per lane, 16 B of values and 8 B of codes per store — taken when every row length
// and column offset involved is a multiple of 8 (decided per launch on the host), and an element form for everything else. A pad
// group that lies inside one input row reads its 8 inputs with one load, at whatever alignment the shift leaves it.
// No LDS, no cross-lane traffic.
#include "ffq_onepass.h"

namespace ffq {
namespace concat {

constexpr int kPerLane = 4;  // units (groups or elements) per lane, kBlock apart: independent loads in flight

// 8 consecutive elements from an address that is only element-aligned (a pad shifts rows by any amount).
template <typename TIn>
__device__ __forceinline__ Chunk<TIn, kE> load_unaligned(const TIn* p) {
  Chunk<TIn, kE> q;
  __builtin_memcpy(q.w, p, sizeof(q.w));
  return q;
}

// ---------------------------------------------------------------------------------------------------
// C1: cat of up to 8 inputs + A1. Block b serves the input whose block range holds it; a unit is a group (VEC) or an element.
//     Algorithmic bytes: every input once (2 B bf16 / 1 B int8 per element) + per output [2 (z)] + 1 per code tensor.
// ---------------------------------------------------------------------------------------------------
struct CatInputs {
  const void* data[FFQ_CAT_MAX_INPUTS];
  const float* scale[FFQ_CAT_MAX_INPUTS];
  const float* offset[FFQ_CAT_MAX_INPUTS];
  uint32_t units[FFQ_CAT_MAX_INPUTS];   // groups or elements of the input
  uint32_t col[FFQ_CAT_MAX_INPUTS];     // the first column of the input in the result, in elements
  uint32_t first[FFQ_CAT_MAX_INPUTS];   // the first block of the input (a prefix sum of ceil(units / (kBlock * kPerLane)))
  FastDiv by_row[FFQ_CAT_MAX_INPUTS];   // units per row of the input
  uint8_t form[FFQ_CAT_MAX_INPUTS];     // 0 plain, 1 int8 codes, 2 value-dtype codes
  int32_t count;
  uint32_t out_run;
};

template <typename T, typename TIn, bool DEQ, bool VEC>
__device__ __forceinline__ void cat_units(const TIn* __restrict__ x, float s, float o, uint32_t units, const FastDiv& by_row, uint32_t col,
                                          uint32_t out_run, uint32_t block, T* __restrict__ out, const FanOut& f, const FanParams& fp) {
  constexpr uint32_t kWidth = VEC ? kE : 1;
#pragma unroll
  for (int j = 0; j < kPerLane; ++j) {
    const uint32_t u = (block * kPerLane + j) * kBlock + threadIdx.x;
    if (u >= units) return;
    const uint32_t row = fdiv(u, by_row);
    const size_t at = (size_t)row * out_run + col + (u - row * by_row.div) * kWidth;
    if constexpr (VEC) put_group<T>(out, f, fp, operand_packed<T, TIn, DEQ, false>(x + (size_t)u * kE, s, o), at);
    else put_one<T>(out, f, fp, element<T, TIn, DEQ>(x, u, s, o), at);
  }
}

template <typename T, bool VEC>
__global__ __launch_bounds__(kBlock) void cat_quantize_kernel(CatInputs in, T* __restrict__ out, FanOut f) {
  int i = 0;
#pragma unroll
  for (int k = 1; k < FFQ_CAT_MAX_INPUTS; ++k)
    if (k < in.count && blockIdx.x >= in.first[k]) i = k;
  const FanParams fp = load_fan(f);
  const uint32_t block = blockIdx.x - in.first[i];
  const int form = in.form[i];
  float s = 1.0f, o = 0.0f;
  if (form) {
    s = in.scale[i][0];
    o = in.offset[i] ? rne(in.offset[i][0]) : 0.0f;
  }
  // (the form is the block's: a uniform branch)
  if (form == 0) cat_units<T, T, false, VEC>(static_cast<const T*>(in.data[i]), s, o, in.units[i], in.by_row[i], in.col[i], in.out_run, block, out, f, fp);
  else if (form == 1) cat_units<T, int8_t, true, VEC>(static_cast<const int8_t*>(in.data[i]), s, o, in.units[i], in.by_row[i], in.col[i], in.out_run, block, out, f, fp);
  else cat_units<T, T, true, VEC>(static_cast<const T*>(in.data[i]), s, o, in.units[i], in.by_row[i], in.col[i], in.out_run, block, out, f, fp);
}

// ---------------------------------------------------------------------------------------------------
// D1: pad of [outer, D2, D1, D0] + A1. A unit is a group of 8 outputs of one row (VEC: 8 | O0) or one output.
//     Algorithmic bytes: the input once + per output [2 (z)] + 1 per code tensor.
// ---------------------------------------------------------------------------------------------------
enum { kConstant = 0, kReflect = 1, kReplicate = 2 };  // the ABI's modes (include/ffq.h)

struct PadGeometry {
  uint32_t units;     // groups or elements of the result
  uint32_t channels;  // parameter pairs (1: per tensor): (row of outer / channel_inner) % channels indexes them
  int32_t D0, D1, D2, O0, O1, O2;
  int32_t l0, l1, l2;
  int32_t mode;
  int32_t aligned;  // 8 | D0 and 8 | l0: a group inside an input row starts at a multiple of 8 elements
  uint32_t fill;    // the fill's bits in T
  FastDiv by_o0, by_o1, by_o2, by_inner, by_channels;  // by_o0: units per row of the result
};

// The input index of output index `o` along one dimension, or -1 for the fill.
__device__ __forceinline__ int32_t source(int32_t o, int32_t left, int32_t extent, int32_t mode) {
  int32_t i = o - left;
  if (mode == kConstant) return (i < 0 || i >= extent) ? -1 : i;
  if (mode == kReflect) {
    i = i < 0 ? -i : i;
    return i >= extent ? 2 * (extent - 1) - i : i;
  }
  return min(max(i, 0), extent - 1);
}

template <typename T, typename TIn, bool DEQ, bool VEC>
__global__ __launch_bounds__(kBlock) void pad_quantize_kernel(const TIn* __restrict__ x, const float* __restrict__ xs,
                                                              const float* __restrict__ xo, PadGeometry g, T* __restrict__ out, FanOut f) {
  constexpr int32_t kWidth = VEC ? kE : 1;
  const FanParams fp = load_fan(f);
  const T fill = __builtin_bit_cast(T, (uint16_t)g.fill);
#pragma unroll
  for (int j = 0; j < kPerLane; ++j) {
    const uint32_t u = (blockIdx.x * kPerLane + j) * kBlock + threadIdx.x;
    if (u >= g.units) return;
    uint32_t t = fdiv(u, g.by_o0);
    const int32_t o0 = (int32_t)(u - t * g.by_o0.div) * kWidth;
    uint32_t n = fdiv(t, g.by_o1);
    const int32_t o1 = (int32_t)(t - n * (uint32_t)g.O1);
    t = n;
    n = fdiv(t, g.by_o2);
    const int32_t o2 = (int32_t)(t - n * (uint32_t)g.O2);
    const size_t at = (size_t)u * kWidth;
    const int32_t i1 = source(o1, g.l1, g.D1, g.mode), i2 = source(o2, g.l2, g.D2, g.mode);
    const bool row = i1 >= 0 && i2 >= 0;
    const TIn* from = x + ((size_t)n * g.D2 + (row ? i2 : 0)) * g.D1 * g.D0 + (size_t)(row ? i1 : 0) * g.D0;
    float s = 1.0f, o = 0.0f;
    if constexpr (DEQ) {
      uint32_t c = 0;
      if (g.channels > 1) {
        c = fdiv(n, g.by_inner);
        c = c - fdiv(c, g.by_channels) * g.channels;
      }
      s = xs[c];
      o = xo ? rne(xo[c]) : 0.0f;
    }
    if constexpr (VEC) {
      const int32_t i0 = o0 - g.l0;
      Chunk<T, kE> h;
      if (row && i0 >= 0 && i0 + kE <= g.D0) {  // the group lies inside the input row: one load
        if constexpr (DEQ) {
          Chunk<TIn, kE> q;
          if (g.aligned) q.load(from + i0); else q = load_unaligned(from + i0);
          float v[kE];
          a2_chunk(q, s, o, v);
          h.pack(v);
        } else {
          if (g.aligned) h.load(reinterpret_cast<const T*>(from) + i0); else h = load_unaligned(reinterpret_cast<const T*>(from) + i0);
        }
      } else {  // an edge of the row, or a row of the fill: element by element
        uint16_t e[kE];
#pragma unroll
        for (int k = 0; k < kE; ++k) {
          const int32_t ik = row ? source(o0 + k, g.l0, g.D0, g.mode) : -1;
          const T v = ik >= 0 ? element<T, TIn, DEQ>(from, (size_t)ik, s, o) : fill;
          e[k] = __builtin_bit_cast(uint16_t, v);
        }
#pragma unroll
        for (int k = 0; k < kE; k += 2) h.w[k >> 1] = (uint32_t)e[k] | ((uint32_t)e[k + 1] << 16);
      }
      put_group<T>(out, f, fp, h, at);
    } else {
      const int32_t i0 = row ? source(o0, g.l0, g.D0, g.mode) : -1;
      put_one<T>(out, f, fp, i0 >= 0 ? element<T, TIn, DEQ>(from, (size_t)i0, s, o) : fill, at);
    }
  }
}

static unsigned blocks_for(uint64_t units) { return (unsigned)((units + (uint64_t)(kBlock * kPerLane) - 1) / (uint64_t)(kBlock * kPerLane)); }

}  // namespace concat
}  // namespace ffq

using namespace ffq;
using namespace ffq::concat;

extern "C" int ffq_cat_quantize(const ffq_cat_inputs* inputs, int dt, int64_t outer, int64_t out_run, int64_t col0, void* out,
                                const ffq_fanout* fan, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (!value_dtype(dt)) return fail(FFQ_ERR_DTYPE, "fused cat is built for bf16 / fp16 values");
  if (!inputs) return fail(FFQ_ERR_ARG, "NULL inputs");
  if (inputs->count < 1 || inputs->count > FFQ_CAT_MAX_INPUTS)
    return fail(FFQ_ERR_ARG, "a cat launch takes 1..%d inputs, got %d", FFQ_CAT_MAX_INPUTS, (int)inputs->count);
  for (int i = 0; i < inputs->count; ++i) {
    const int rc = check_operand_form("fused cat", inputs->dt[i], inputs->scale[i], inputs->offset[i], false, dt);
    if (rc) return rc;
  }
  if (outer < 0 || out_run < 0 || col0 < 0) return fail(FFQ_ERR_ARG, "fused cat: negative extent");
  int64_t width = 0;
  bool vec = out_run % kE == 0 && col0 % kE == 0;
  for (int i = 0; i < inputs->count; ++i) {
    if (inputs->run[i] < 1) return fail(FFQ_ERR_ARG, "fused cat: input %d has a row of %lld elements", i, (long long)inputs->run[i]);
    if (inputs->run[i] > out_run) return fail(FFQ_ERR_ARG, "fused cat: input %d is wider than the result", i);
    width += inputs->run[i];
    vec = vec && inputs->run[i] % kE == 0;
  }
  if (col0 + width > out_run)
    return fail(FFQ_ERR_ARG, "fused cat: columns [%lld, %lld) are outside a row of %lld", (long long)col0, (long long)(col0 + width), (long long)out_run);
  const int64_t limit = (int64_t)1 << 31;
  if (out_run >= limit || (outer && out_run >= limit / outer) || outer * out_run >= limit)
    return fail(FFQ_ERR_DTYPE, "fused cat needs fewer than 2^31 output elements");
  FanOut f;
  int rc = check_launch_args(fan, outer * out_run, outer == 0, inputs->data[0], {out}, &f);
  if (rc || outer == 0) return rc;
  for (int i = 0; i < inputs->count; ++i) {
    rc = check_buffers(inputs->data[i], {inputs->data[i]});
    if (rc) return rc;
  }
  CatInputs in;
  in.count = inputs->count;
  in.out_run = (uint32_t)out_run;
  uint32_t blocks = 0, col = (uint32_t)col0;
  const uint32_t width_of = vec ? (uint32_t)kE : 1u;
  for (int i = 0; i < FFQ_CAT_MAX_INPUTS; ++i) {
    const bool live = i < inputs->count;
    const uint32_t per_row = live ? (uint32_t)inputs->run[i] / width_of : 1u;
    in.data[i] = live ? inputs->data[i] : nullptr;
    in.scale[i] = live ? inputs->scale[i] : nullptr;
    in.offset[i] = live ? inputs->offset[i] : nullptr;
    in.form[i] = live && inputs->scale[i] ? (inputs->dt[i] == FFQ_I8 ? 1 : 2) : 0;
    in.units[i] = live ? (uint32_t)outer * per_row : 0u;
    in.by_row[i] = make_fastdiv(per_row);
    in.col[i] = col;
    in.first[i] = blocks;
    if (live) {
      col += (uint32_t)inputs->run[i];
      blocks += blocks_for(in.units[i]);
    }
  }
  dispatch_dtype(dt, [&](auto t) {
    using T = typename decltype(t)::type;
    if (vec) cat_quantize_kernel<T, true><<<blocks, kBlock, 0, s>>>(in, static_cast<T*>(out), f);
    else cat_quantize_kernel<T, false><<<blocks, kBlock, 0, s>>>(in, static_cast<T*>(out), f);
  });
  return check_launch("cat_quantize_kernel");
}

extern "C" int ffq_pad_quantize(int mode, const void* x, int x_dt, const float* x_scale, const float* x_offset, int64_t param_channels,
                                int64_t channel_inner, int dt, int64_t outer, int64_t D2, int64_t D1, int64_t D0, const int64_t* pads,
                                int fill_bits, void* out, const ffq_fanout* fan, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (mode < kConstant || mode > kReplicate) return fail(FFQ_ERR_ARG, "unknown pad mode %d (0: constant, 1: reflect, 2: replicate)", mode);
  if (!value_dtype(dt)) return fail(FFQ_ERR_DTYPE, "fused pad is built for bf16 / fp16 values");
  int rc = check_operand_form("fused pad", x_dt, x_scale, x_offset, param_channels != 0, dt);
  if (rc) return rc;
  if (!pads) return fail(FFQ_ERR_ARG, "NULL pads");
  if (outer < 0 || D0 < 1 || D1 < 1 || D2 < 1 || param_channels < 0 || channel_inner < 0) return fail(FFQ_ERR_ARG, "fused pad: every extent is at least 1");
  if (param_channels && (channel_inner < 1 || outer % (param_channels * channel_inner) != 0))
    return fail(FFQ_ERR_ARG, "fused pad: %lld rows are not whole images of %lld channels of %lld rows", (long long)outer, (long long)param_channels,
                (long long)channel_inner);
  const int64_t limit = (int64_t)1 << 31;
  const int64_t D[3] = {D0, D1, D2};
  int64_t O[3];
  for (int d = 0; d < 3; ++d) {
    const int64_t l = pads[2 * d], r = pads[2 * d + 1];
    if (l <= -limit || l >= limit || r <= -limit || r >= limit || D[d] >= limit) return fail(FFQ_ERR_DTYPE, "fused pad needs fewer than 2^31 elements");
    if (mode != kConstant && (l < 0 || r < 0)) return fail(FFQ_ERR_ARG, "fused pad: negative pads crop in constant mode only");
    if (mode == kReflect && (l >= D[d] || r >= D[d]))
      return fail(FFQ_ERR_ARG, "fused pad: reflect pads (%lld, %lld) must be smaller than the extent %lld", (long long)l, (long long)r, (long long)D[d]);
    O[d] = D[d] + l + r;
    if (O[d] < 1) return fail(FFQ_ERR_ARG, "fused pad: the pads (%lld, %lld) leave nothing of an extent of %lld", (long long)l, (long long)r, (long long)D[d]);
    if (O[d] >= limit) return fail(FFQ_ERR_DTYPE, "fused pad needs fewer than 2^31 elements");
  }
  if (D0 * D1 >= limit || D0 * D1 * D2 >= limit || (outer && D0 * D1 * D2 >= limit / outer) || O[0] * O[1] >= limit ||
      O[0] * O[1] * O[2] >= limit || (outer && O[0] * O[1] * O[2] >= limit / outer))
    return fail(FFQ_ERR_DTYPE, "fused pad needs fewer than 2^31 input and output elements");
  if (fill_bits < 0 || fill_bits > 0xFFFF) return fail(FFQ_ERR_ARG, "fused pad: the fill is 16 bits of the value dtype");
  const int64_t total = outer * O[0] * O[1] * O[2];
  FanOut f;
  rc = check_launch_args(fan, total, outer == 0, x, {x, out}, &f);
  if (rc || outer == 0) return rc;
  const bool vec = O[0] % kE == 0;
  PadGeometry g;
  g.units = (uint32_t)(vec ? total / kE : total);
  g.channels = param_channels ? (uint32_t)param_channels : 1u;
  g.D0 = (int32_t)D0; g.D1 = (int32_t)D1; g.D2 = (int32_t)D2;
  g.O0 = (int32_t)O[0]; g.O1 = (int32_t)O[1]; g.O2 = (int32_t)O[2];
  g.l0 = (int32_t)pads[0]; g.l1 = (int32_t)pads[2]; g.l2 = (int32_t)pads[4];
  g.mode = mode;
  g.aligned = D0 % kE == 0 && pads[0] % kE == 0;
  g.fill = (uint32_t)fill_bits;
  g.by_o0 = make_fastdiv((uint32_t)(vec ? O[0] / kE : O[0]));
  g.by_o1 = make_fastdiv((uint32_t)O[1]);
  g.by_o2 = make_fastdiv((uint32_t)O[2]);
  g.by_inner = make_fastdiv(param_channels ? (uint32_t)channel_inner : 1u);
  g.by_channels = make_fastdiv(g.channels);
  const unsigned grid = blocks_for(g.units);
  dispatch_input(dt, x_dt, x_scale != nullptr, [&](auto t, auto tin, auto deq) {
    using T = typename decltype(t)::type;
    using TIn = typename decltype(tin)::type;
    if (vec) pad_quantize_kernel<T, TIn, decltype(deq)::value, true><<<grid, kBlock, 0, s>>>(static_cast<const TIn*>(x), x_scale, x_offset, g, static_cast<T*>(out), f);
    else pad_quantize_kernel<T, TIn, decltype(deq)::value, false><<<grid, kBlock, 0, s>>>(static_cast<const TIn*>(x), x_scale, x_offset, g, static_cast<T*>(out), f);
  });
  return check_launch("pad_quantize_kernel");
}
