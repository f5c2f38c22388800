// ffq_modules.hip — the reference's generic quantized modules as one-pass kernels with A1 fused in.
//
// QuantizedLayerNorm / QuantizedEmbedding / QuantizedRelu / QuantizedSilu (reference nn/normalization.py, nn/embedding.py,
// nn/activations.py) run their generated fallbacks (_gen/fallback.py: relu :296, embedding :616, layer_norm :655, silu :1348):
// A2 of the quantized operand into a data-dtype tensor, the ATen op, A1 of the output quantizer — three launches, each a full
// pass over HBM with a temporary in between. Here each is one pass under the A2 / op / A1 contract of ffq_onepass.h.
// Algorithmic bytes per element are stated at each kernel; all three are HBM-bound streams.
#ifndef FFQ_NT_STREAMS
#define FFQ_NT_STREAMS 3  // nt loads and stores of the streamed tensors, as ffq_producers.hip
#endif
#ifndef FFQ_MODULES_GRID
#define FFQ_MODULES_GRID 1024  // blocks of the table-driven SiLU kernel: two 512-thread blocks per CU, twice over
#endif
#include "ffq_onepass.h"
#include "ffq_silu.h"

namespace ffq {

// ---------------------------------------------------------------------------------------------------
// M1: LayerNorm (F.layer_norm over the last `cols` elements) + A1.
//     v = x, or A2(x; s, o) rounded to T (per-tensor or per-row parameters);
//     mean = sum(v) / cols, var = sum((v - mean)^2) / cols (fp32, two passes over the row held in registers);
//     z = T(w * (rstd * (v - mean)) + b) (one fma, as ATen's kernel; without w: a multiply or an add), rstd = rsqrt(var + eps);
//     codes_j = A1(z; s_j, o_j).
//     WPR wavefronts per row (1: four rows per block for rows of at most 512 elements; 4: the whole block), CPL chunks of 8 per
//     lane: cols <= 8 * 64 * WPR * CPL. The row is read once.
//     Algorithmic bytes / element: 2 (bf16 input) or 1 (int8 codes) [+ 2 (z)] + 1 per code tensor.
// ---------------------------------------------------------------------------------------------------
template <typename T, typename TIn, bool DEQ, int CPL, int WPR>
__global__ __launch_bounds__(kBlock) void layer_norm_quantize_kernel(const TIn* __restrict__ x, const float* __restrict__ xs,
                                                                     const float* __restrict__ xo, uint32_t per_row,
                                                                     const T* __restrict__ weight, const T* __restrict__ bias,
                                                                     T* __restrict__ out, FanOut f, uint32_t rows,
                                                                     uint32_t chunks_per_row, float cols_f, float eps) {
  constexpr uint32_t LPR = 64u * WPR;
  const uint32_t lane = threadIdx.x % LPR;
  const uint32_t row = blockIdx.x * (kBlock / LPR) + threadIdx.x / LPR;
  if (row >= rows) return;  // block-uniform when WPR == 4
  const size_t base = (size_t)row * chunks_per_row * kE;
  float s = 1.0f, o = 0.0f;
  row_params<DEQ>(xs, xo, per_row, row, s, o);
  Chunk<T, kE> h[CPL];
#pragma unroll
  for (int u = 0; u < CPL; ++u) {
    const uint32_t c = lane + LPR * u;
    if (c >= chunks_per_row) continue;
    if constexpr (DEQ) {  // (operand_packed's steps, spelled out: through the helper some of this loop's loads lose their nt hint)
      Chunk<TIn, kE> q;
      q.FFQ_SLOAD(x + base + (size_t)c * kE);
      float v[kE];
      a2_chunk(q, s, o, v);
      h[u].pack(v);
    } else {
      h[u].FFQ_SLOAD(reinterpret_cast<const T*>(x) + base + (size_t)c * kE);
    }
  }
  __shared__ float wave_part[2][kBlock / 64];
  // mean
  float acc = 0.0f;
#pragma unroll
  for (int u = 0; u < CPL; ++u) {
    const uint32_t c = lane + LPR * u;
    if (c >= chunks_per_row) continue;
    float part = 0.0f;
#pragma unroll
    for (int i = 0; i < kE; ++i) part = part + h[u].get(i);
    acc = acc + part;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) acc = acc + __shfl_xor(acc, d, 64);
  if constexpr (WPR > 1) {
    if ((threadIdx.x & 63u) == 0) wave_part[0][threadIdx.x >> 6] = acc;
    __syncthreads();
    acc = ((wave_part[0][0] + wave_part[0][1]) + wave_part[0][2]) + wave_part[0][3];
  }
  const float mean = acc / cols_f;
  // biased variance around that mean
  acc = 0.0f;
#pragma unroll
  for (int u = 0; u < CPL; ++u) {
    const uint32_t c = lane + LPR * u;
    if (c >= chunks_per_row) continue;
    float part = 0.0f;
#pragma unroll
    for (int i = 0; i < kE; ++i) {
      const float d = h[u].get(i) - mean;
      part = part + d * d;
    }
    acc = acc + part;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) acc = acc + __shfl_xor(acc, d, 64);
  if constexpr (WPR > 1) {
    if ((threadIdx.x & 63u) == 0) wave_part[1][threadIdx.x >> 6] = acc;
    __syncthreads();
    acc = ((wave_part[1][0] + wave_part[1][1]) + wave_part[1][2]) + wave_part[1][3];
  }
  const float rstd = rsqrtf(acc / cols_f + eps);
  const FanParams p = load_fan(f);
#pragma unroll
  for (int u = 0; u < CPL; ++u) {
    const uint32_t c = lane + LPR * u;
    if (c >= chunks_per_row) continue;
    // ATen's form: gamma * (rstd * (x - mean)) + beta, the multiply-add contracted
    float z[kE];
#pragma unroll
    for (int i = 0; i < kE; ++i) z[i] = rstd * (h[u].get(i) - mean);
    Chunk<T, kE> w, b;
    if (weight) w.load(weight + (size_t)c * kE);
    if (bias) b.load(bias + (size_t)c * kE);
    if (weight && bias) {
#pragma unroll
      for (int i = 0; i < kE; ++i) z[i] = __builtin_fmaf(w.get(i), z[i], b.get(i));
    } else if (weight) {
#pragma unroll
      for (int i = 0; i < kE; ++i) z[i] = w.get(i) * z[i];
    } else if (bias) {
#pragma unroll
      for (int i = 0; i < kE; ++i) z[i] = z[i] + b.get(i);
    }
    Chunk<T, kE> zc;
    zc.pack(z);  // the one rounding to the data dtype
    if (out) zc.FFQ_SSTORE(out + base + (size_t)c * kE);
    unpack(zc, z);
    fan_store(f, p, z, base + (size_t)c * kE);
  }
}

// ---------------------------------------------------------------------------------------------------
// M2: Embedding gather + A2 of the table's codes + A1:   z = T((table[id, d] + round(o)) * s);   codes_j = A1(z; s_j, o_j).
//     One lane per 8-element chunk of an output row. Parameters: one pair per chunk (per tensor, per table row, or groups of
//     G % 8 == 0 along D: pair (id * D / G + d / G)), or one pair per column (PER_COLUMN: PerChannel(1)). An id outside [0, V)
//     reads nothing: its row is zeros (codes: A1(0)) and its position is folded into *bad with atomicMin.
//     Algorithmic bytes / element: 1 (int8 table row) or 2 [+ 2 (z)] + 1 per code tensor (+ the ids, 8 B per D elements).
// ---------------------------------------------------------------------------------------------------
struct EmbArgs {
  uint32_t nchunks, dchunks, V, D;
  uint32_t per_row, groups_per_row;  // parameter grid [per_row ? V : 1, groups_per_row]
  FastDiv by_dchunks, by_group_chunks;
};

template <typename T, typename TIn, typename TId, bool PER_COLUMN>
__global__ __launch_bounds__(kBlock) void embedding_quantize_kernel(const TId* __restrict__ ids, const TIn* __restrict__ table,
                                                                    const float* __restrict__ scale, const float* __restrict__ offset,
                                                                    EmbArgs a, T* __restrict__ out, FanOut f, int32_t* bad) {
  const uint32_t c = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  if (c >= a.nchunks) return;
  const uint32_t t = fdiv(c, a.by_dchunks);
  const uint32_t j = c - t * a.dchunks;
  const int64_t id = (int64_t)ids[t];
  const FanParams fp = load_fan(f);
  float z[kE];
  if (id < 0 || id >= (int64_t)a.V) {
#pragma unroll
    for (int i = 0; i < kE; ++i) z[i] = 0.0f;
    if (j == 0) atomicMin(bad, (int32_t)t);
  } else {
    Chunk<TIn, kE> q;
    q.load(table + (size_t)id * a.D + (size_t)j * kE);  // a table row is reused by every token that names it: no nt hint
    if constexpr (PER_COLUMN) {
#pragma unroll
      for (int i = 0; i < kE; ++i) {
        const uint32_t col = j * kE + i;
        const float o = offset ? rne(offset[col]) : 0.0f;
        const float v = q.get(i) + o;
        z[i] = v * scale[col];
      }
      Chunk<T, kE> h;
      h.pack(z);
      unpack(h, z);
    } else {
      const size_t pidx = (a.per_row ? (size_t)id * a.groups_per_row : 0) + (a.groups_per_row > 1 ? fdiv(j, a.by_group_chunks) : 0u);
      const float s = scale[pidx];
      const float o = offset ? rne(offset[pidx]) : 0.0f;
      a2_chunk(q, s, o, z);
      Chunk<T, kE> h;
      h.pack(z);
      unpack(h, z);
    }
  }
  const size_t at = (size_t)c * kE;
  if (out) {
    Chunk<T, kE> h;
    h.pack(z);
    h.FFQ_SSTORE(out + at);
  }
  fan_store(f, fp, z, at);
}

// ---------------------------------------------------------------------------------------------------
// M3: ReLU / SiLU + A1:   v = x or T(A2(x)) (per-tensor or per-row parameters),   z = T(op(v)),   codes_j = A1(z; s_j, o_j).
//     relu(v) = NaN ? v : max(v, 0) (ATen's clamp_min); silu(v) = v / (1 + exp(-v)) in fp32 (ffq_silu.h silu_exact). For bf16
//     values of large tensors (TABLE) silu is the LDS table of ffq_silu.h, equal to silu_exact on all 65536 patterns.
//     Grid-stride over 8-element chunks. Algorithmic bytes / element: 2 (bf16 input) or 1 (int8 codes) [+ 2 (z)] + 1 per code tensor.
// ---------------------------------------------------------------------------------------------------
constexpr int kPwBlock = 512;
enum { kOpRelu = 0, kOpSilu = 1 };

template <typename T, typename TIn, bool DEQ, int OP, bool TABLE>
__global__ __launch_bounds__(kPwBlock) void pointwise_quantize_kernel(const TIn* __restrict__ x, const float* __restrict__ xs,
                                                                      const float* __restrict__ xo, uint32_t per_row, FastDiv by_run,
                                                                      T* __restrict__ out, FanOut f, uint32_t nchunks) {
  static_assert(!TABLE || (OP == kOpSilu && TypeTag<T>::value == FFQ_BF16), "the table holds bf16 silu");
  __shared__ uint16_t table[TABLE ? kSiluEntries : 1];
  if constexpr (TABLE) {
    silu_table_fill(table, threadIdx.x, kPwBlock);
    __syncthreads();
  }
  const FanParams fp = load_fan(f);
  float s = 1.0f, o = 0.0f;
  if constexpr (DEQ) {
    if (!per_row) {
      s = xs[0];
      o = xo ? rne(xo[0]) : 0.0f;
    }
  }
  const uint32_t stride = gridDim.x * (uint32_t)kPwBlock;
  for (uint32_t c = blockIdx.x * (uint32_t)kPwBlock + threadIdx.x; c < nchunks; c += stride) {
    if constexpr (DEQ) {
      if (per_row) {
        const uint32_t r = fdiv(c, by_run);
        s = xs[r];
        o = xo ? rne(xo[r]) : 0.0f;
      }
    }
    const Chunk<T, kE> h = operand_packed<T, TIn, DEQ>(x + (size_t)c * kE, s, o);
    Chunk<T, kE> y;
    if constexpr (TABLE) {
      uint32_t bad = 0;
#pragma unroll
      for (int k = 0; k < kE / 2; ++k) y.w[k] = silu_pair_lookup(h.w[k], table, bad);
      if (__builtin_expect(silu_any_outside(bad), 0)) {
#pragma unroll
        for (int k = 0; k < kE / 2; ++k) y.w[k] = silu_pair_patch(h.w[k], y.w[k]);
      }
    } else {
      float v[kE];
#pragma unroll
      for (int i = 0; i < kE; ++i) {
        const float a = h.get(i);
        if constexpr (OP == kOpRelu) {
          v[i] = a != a ? a : __builtin_fmaxf(a, 0.0f);
        } else {
          v[i] = silu_exact(a);
        }
      }
      y.pack(v);
    }
    if (out) y.FFQ_SSTORE(out + (size_t)c * kE);
    float z[kE];
    unpack(y, z);
    fan_store(f, fp, z, (size_t)c * kE);
  }
}

}  // namespace ffq

using namespace ffq;

extern "C" int ffq_layer_norm_quantize(const void* x, int x_dt, const float* x_scale, const float* x_offset, int x_per_row,
                                       const void* weight, const void* bias, int dt, int64_t rows, int64_t cols, double eps,
                                       void* out, const ffq_fanout* fan, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (rows < 0 || cols < 0) return fail(FFQ_ERR_ARG, "negative extent");
  if (!value_dtype(dt)) return fail(FFQ_ERR_DTYPE, "fused LayerNorm is built for bf16 / fp16 values");
  int rc = check_operand_form("fused LayerNorm", x_dt, x_scale, x_offset, x_per_row != 0, dt);
  if (rc) return rc;
  if (cols == 0) return fail(FFQ_ERR_EMPTY, "LayerNorm over an empty row");
  if (cols % kE != 0 || cols > 16384)
    return fail(FFQ_ERR_DTYPE, "fused LayerNorm needs cols %% 8 == 0 and cols <= 16384 (got %lld)", (long long)cols);
  if (rows >= ((int64_t)1 << 31)) return fail(FFQ_ERR_ARG, "too many rows");
  FanOut f;
  rc = check_launch_args(fan, rows * cols, rows == 0, x, {x, weight, bias, out}, &f);
  if (rc || rows == 0) return rc;
  const uint32_t cpr = (uint32_t)(cols / kE);
  const uint32_t per_row = x_per_row ? 1u : 0u;
  dispatch_input(dt, x_dt, x_scale != nullptr, [&](auto t, auto tin, auto deq) {
    using T = typename decltype(t)::type;
    using TIn = typename decltype(tin)::type;
    dispatch_row_shape(cpr, [&](auto cpl, auto wpr) {
      layer_norm_quantize_kernel<T, TIn, decltype(deq)::value, decltype(cpl)::value, decltype(wpr)::value>
          <<<row_grid<decltype(wpr)::value>(rows), kBlock, 0, s>>>(static_cast<const TIn*>(x), x_scale, x_offset, per_row, static_cast<const T*>(weight),
                                                                   static_cast<const T*>(bias), static_cast<T*>(out), f, (uint32_t)rows, cpr,
                                                                   (float)cols, (float)eps);
    });
  });
  return check_launch("layer_norm_quantize_kernel");
}

extern "C" int ffq_embedding_quantize(const void* ids, int ids_dt, int64_t n_ids, const void* table, int table_dt, int64_t V,
                                      int64_t D, const float* scale, const float* offset, int per_row, int64_t group, int dt,
                                      void* out, const ffq_fanout* fan, int32_t* bad_id, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n_ids < 0 || V < 0 || D < 0) return fail(FFQ_ERR_ARG, "negative extent");
  if (!value_dtype(dt)) return fail(FFQ_ERR_DTYPE, "fused Embedding is built for bf16 / fp16 values");
  if (ids_dt != FFQ_I64 && ids_dt != FFQ_I32) return fail(FFQ_ERR_DTYPE, "ids must be int64 or int32");
  if (table_dt != FFQ_I8 && table_dt != dt) return fail(FFQ_ERR_DTYPE, "the table holds int8 or value-dtype codes");
  if (D == 0 || D % kE != 0) return fail(FFQ_ERR_DTYPE, "fused Embedding needs D %% 8 == 0 and D > 0 (got %lld)", (long long)D);
  if (V >= ((int64_t)1 << 31) || V * D >= ((int64_t)1 << 40)) return fail(FFQ_ERR_ARG, "table too large");
  if (group <= 0 || D % group != 0) return fail(FFQ_ERR_TILE_DIVIDE, "the parameter group (%lld) must divide D (%lld)", (long long)group, (long long)D);
  if (group != 1 && group % kE != 0) return fail(FFQ_ERR_DTYPE, "parameter groups along D are 1 or a multiple of 8 elements");
  if (group == 1 && per_row) return fail(FFQ_ERR_DTYPE, "element-wise parameters are not built");
  const int64_t nchunks = n_ids * (D / kE);
  if (nchunks >= ((int64_t)1 << 32) - kBlock) return fail(FFQ_ERR_ARG, "too many elements for one launch");
  FanOut f;
  int rc = fan_from_abi(fan, n_ids * D, &f);
  if (rc) return rc;
  if (n_ids == 0) return FFQ_OK;
  if (!ids || !table || !scale || !bad_id) return fail(FFQ_ERR_ARG, "NULL buffer");
  if (V == 0) return fail(FFQ_ERR_EMPTY, "an empty table has no rows to gather");
  if (!aligned16(table) || (out && !aligned16(out))) return fail(FFQ_ERR_ARG, "buffers must be 16-byte aligned");
  EmbArgs a;
  a.nchunks = (uint32_t)nchunks;
  a.dchunks = (uint32_t)(D / kE);
  a.V = (uint32_t)V;
  a.D = (uint32_t)D;
  a.per_row = per_row ? 1u : 0u;
  a.groups_per_row = (uint32_t)(D / group);
  a.by_dchunks = make_fastdiv(a.dchunks);
  a.by_group_chunks = make_fastdiv(group == 1 ? 1u : (uint32_t)(group / kE));
  const unsigned grid = (unsigned)((nchunks + kBlock - 1) / kBlock);
  dispatch_dtype(dt, [&](auto t) {
    using T = typename decltype(t)::type;
    dispatch_form<T>(table_dt, true, [&](auto tin, auto) {  // (the table is always codes)
      using TIn = typename decltype(tin)::type;
      auto launch = [&](auto tid, auto per_column) {
        using TId = typename decltype(tid)::type;
        embedding_quantize_kernel<T, TIn, TId, decltype(per_column)::value><<<grid, kBlock, 0, s>>>(
            static_cast<const TId*>(ids), static_cast<const TIn*>(table), scale, offset, a, static_cast<T*>(out), f, bad_id);
      };
      auto by_ids = [&](auto per_column) {
        if (ids_dt == FFQ_I64) launch(Tag<int64_t>{}, per_column); else launch(Tag<int32_t>{}, per_column);
      };
      if (group == 1) by_ids(std::true_type{}); else by_ids(std::false_type{});
    });
  });
  return check_launch("embedding_quantize_kernel");
}

extern "C" int ffq_pointwise_quantize(int op, const void* x, int x_dt, const float* x_scale, const float* x_offset, int64_t param_run,
                                      int dt, int64_t numel, void* out, const ffq_fanout* fan, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (numel < 0 || param_run < 0) return fail(FFQ_ERR_ARG, "negative extent");
  if (op != kOpRelu && op != kOpSilu) return fail(FFQ_ERR_ARG, "unknown pointwise op %d (0: relu, 1: silu)", op);
  if (!value_dtype(dt)) return fail(FFQ_ERR_DTYPE, "fused ReLU / SiLU is built for bf16 / fp16 values");
  if (numel % kE != 0 || numel >= ((int64_t)1 << 35)) return fail(FFQ_ERR_DTYPE, "fused ReLU / SiLU needs numel %% 8 == 0 and numel < 2^35");
  int rc = check_operand("fused ReLU / SiLU", x_dt, x_scale, x_offset, param_run, dt, numel, kRowLimit);
  if (rc) return rc;
  FanOut f;
  rc = check_launch_args(fan, numel, numel == 0, x, {x, out}, &f);
  if (rc || numel == 0) return rc;
  const uint32_t nchunks = (uint32_t)(numel / kE);
  const uint32_t per_row = param_run ? 1u : 0u;
  const FastDiv by_run = make_fastdiv(param_run ? (uint32_t)(param_run / kE) : 1u);
  // the table pays from ~4 chunks per thread of a two-blocks-per-CU grid on (as in ffq_producers.hip)
  const bool table = op == kOpSilu && dt == FFQ_BF16 && nchunks >= 4u * kPwBlock * 512u;
  const unsigned grid = table ? FFQ_MODULES_GRID : (unsigned)((nchunks + kPwBlock - 1) / kPwBlock);
  dispatch_input(dt, x_dt, x_scale != nullptr, [&](auto t, auto tin, auto deq) {
    using T = typename decltype(t)::type;
    using TIn = typename decltype(tin)::type;
    auto launch = [&](auto op_, auto tab) {
      pointwise_quantize_kernel<T, TIn, decltype(deq)::value, decltype(op_)::value, decltype(tab)::value><<<grid, kPwBlock, 0, s>>>(
          static_cast<const TIn*>(x), x_scale, x_offset, per_row, by_run, static_cast<T*>(out), f, nchunks);
    };
    if (op == kOpRelu) return launch(Int<kOpRelu>{}, std::false_type{});
    if constexpr (std::is_same_v<T, bf16_t>) {  // (the table holds bf16 silu)
      if (table) return launch(Int<kOpSilu>{}, std::true_type{});
    }
    launch(Int<kOpSilu>{}, std::false_type{});
  });
  return check_launch("pointwise_quantize_kernel");
}
