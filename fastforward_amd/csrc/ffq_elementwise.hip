// ffq_elementwise.hip — the reference's quantized add / sub / mul / div, softmax, sigmoid and GELU as one-pass kernels with A1
// fused in.
//
// ff.nn.functional.{add, sub, mul, div, softmax, sigmoid, gelu} run their generated fallbacks in the reference
// (_gen/fallback.py: softmax :269, sigmoid :321, add :801, sub :840, mul :879, div :917, gelu :1373): A2 of each quantized
// operand into a data-dtype tensor, the ATen op, A1 of the output quantizer — up to four launches with a full-size temporary
// between each. Here each is one pass under the A2 / op / A1 contract of ffq_onepass.h.
// ATen's device formulas, as its kernels evaluate them (the library's contraction of a * b + c into one fma included):
//   add / sub:  a + b * alpha  ->  fma(b, +-alpha, a)           (sub is add with -alpha); a scalar b: a + float(b) * (+-alpha)
//   mul / div:  a * b,  a / b (the IEEE quotient);  div by a scalar s: a * float(1 / s), the reciprocal taken of the double s
//   scalar operands enter as float(s), not rounded to the data dtype
//   sigmoid:    1 / (1 + exp(-v))
//   gelu:       (v * 0.5) * (1 + erf(v * M_SQRT1_2));  tanh form: (0.5 * v) * (1 + tanh(kBeta * fma(0.044715, v^3, v)))
//   softmax:    exp(v - max) / sum(exp(v - max))                 (max, sum, quotient in fp32)
// Algorithmic bytes per element are stated at each kernel; all three are HBM-bound streams.
#ifndef FFQ_NT_STREAMS
#define FFQ_NT_STREAMS 3  // nt loads and stores of the streamed tensors, as ffq_producers.hip
#endif
#include "ffq_onepass.h"

namespace ffq {

constexpr int kEwBlock = 512;  // the streaming kernels' block (as ffq_modules.hip's pointwise kernel)

// ---------------------------------------------------------------------------------------------------
// E1: add / sub / mul / div + A1:   z = T(op(A, B)),   codes_j = A1(z; s_j, o_j).
//     A = a or T(A2(a)); B = b or T(A2(b)) of b_chunks chunks (b_chunks == nchunks: same shape; otherwise b's shape is a suffix
//     of a's and element i reads b[i % b_numel]), or the fp32 scalar. Grid-stride over 8-element chunks.
//     Algorithmic bytes / element: 2 or 1 (a) + 2 or 1 (b; ~0 for a broadcast b or a scalar) [+ 2 (z)] + 1 per code tensor.
// ---------------------------------------------------------------------------------------------------
enum { kAdd = 0, kSub = 1, kMul = 2, kDiv = 3 };           // the ABI's ops (include/ffq.h)
enum { kBinAdd = 0, kBinMul = 1, kBinDiv = 2 };           // the device's: sub is add with -alpha, div by a scalar a product

struct BinArgs {
  OperandParams pa, pb;
  uint32_t nchunks, b_chunks;
  uint32_t broadcast;  // b_chunks != nchunks
  FastDiv by_b;
  int op;
  float alpha, scalar;
};

template <typename T, typename TA, bool DEQA, typename TB, bool DEQB, bool SCALAR>
__global__ __launch_bounds__(kEwBlock) void binary_quantize_kernel(const TA* __restrict__ a, const TB* __restrict__ b, BinArgs g,
                                                                   T* __restrict__ out, FanOut f) {
  const FanParams fp = load_fan(f);
  const uint32_t stride = gridDim.x * (uint32_t)kEwBlock;
  for (uint32_t c = blockIdx.x * (uint32_t)kEwBlock + threadIdx.x; c < g.nchunks; c += stride) {
    float sa = 1.0f, oa = 0.0f;
    params_at<DEQA>(g.pa, c, sa, oa);
    float va[kE], vb[kE];
    operand_chunk<T, TA, DEQA>(a + (size_t)c * kE, sa, oa, va);
    if constexpr (SCALAR) {
#pragma unroll
      for (int i = 0; i < kE; ++i) vb[i] = g.scalar;
    } else {
      const uint32_t cb = g.broadcast ? c - fdiv(c, g.by_b) * g.b_chunks : c;
      float sb = 1.0f, ob = 0.0f;
      params_at<DEQB>(g.pb, cb, sb, ob);
      if (g.broadcast) operand_chunk<T, TB, DEQB, false>(b + (size_t)cb * kE, sb, ob, vb);
      else operand_chunk<T, TB, DEQB>(b + (size_t)cb * kE, sb, ob, vb);
    }
    float z[kE];
    if (g.op == kBinAdd) {
#pragma unroll
      for (int i = 0; i < kE; ++i) z[i] = __builtin_fmaf(vb[i], g.alpha, va[i]);
    } else if (g.op == kBinMul) {
#pragma unroll
      for (int i = 0; i < kE; ++i) z[i] = va[i] * vb[i];
    } else {
#pragma unroll
      for (int i = 0; i < kE; ++i) z[i] = va[i] / vb[i];
    }
    store_chunk<T>(out, f, fp, z, (size_t)c * kE);
  }
}

// ---------------------------------------------------------------------------------------------------
// E2: softmax over the last `cols` elements + A1:   v = x or T(A2(x)) (per-tensor or per-row parameters);
//     m = max(v) (NaN-ignoring: a NaN still reaches the sum), e = exp(v - m), z = T(e / sum(e)),   codes_j = A1(z; s_j, o_j).
//     A row of -inf (or holding +inf or NaN) gives NaN, as ATen. The geometry and reduction plan of layer_norm_quantize_kernel
//     (ffq_modules.hip): WPR wavefronts per row, CPL chunks of 8 per lane, cols <= 8 * 64 * WPR * CPL; the row is read once and
//     its exponentials stay in registers.
//     Algorithmic bytes / element: 2 (bf16 input) or 1 (int8 codes) [+ 2 (z)] + 1 per code tensor.
// ---------------------------------------------------------------------------------------------------
template <typename T, typename TIn, bool DEQ, int CPL, int WPR>
__global__ __launch_bounds__(kBlock) void softmax_quantize_kernel(const TIn* __restrict__ x, const float* __restrict__ xs,
                                                                  const float* __restrict__ xo, uint32_t per_row, T* __restrict__ out,
                                                                  FanOut f, uint32_t rows, uint32_t chunks_per_row) {
  constexpr uint32_t LPR = 64u * WPR;
  const uint32_t lane = threadIdx.x % LPR;
  const uint32_t row = blockIdx.x * (kBlock / LPR) + threadIdx.x / LPR;
  if (row >= rows) return;  // block-uniform when WPR == 4
  const size_t base = (size_t)row * chunks_per_row * kE;
  float s = 1.0f, o = 0.0f;
  row_params<DEQ>(xs, xo, per_row, row, s, o);
  float v[CPL][kE];
  float m = -INFINITY;
#pragma unroll
  for (int u = 0; u < CPL; ++u) {
    const uint32_t c = lane + LPR * u;
    if (c >= chunks_per_row) continue;
    operand_chunk<T, TIn, DEQ>(x + base + (size_t)c * kE, s, o, v[u]);
#pragma unroll
    for (int i = 0; i < kE; ++i) m = __builtin_fmaxf(m, v[u][i]);
  }
  __shared__ float wave_part[2][kBlock / 64];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) m = __builtin_fmaxf(m, __shfl_xor(m, d, 64));
  if constexpr (WPR > 1) {
    if ((threadIdx.x & 63u) == 0) wave_part[0][threadIdx.x >> 6] = m;
    __syncthreads();
    m = __builtin_fmaxf(__builtin_fmaxf(wave_part[0][0], wave_part[0][1]), __builtin_fmaxf(wave_part[0][2], wave_part[0][3]));
  }
  float acc = 0.0f;
#pragma unroll
  for (int u = 0; u < CPL; ++u) {
    const uint32_t c = lane + LPR * u;
    if (c >= chunks_per_row) continue;
    float part = 0.0f;
#pragma unroll
    for (int i = 0; i < kE; ++i) {
      v[u][i] = expf(v[u][i] - m);
      part = part + v[u][i];
    }
    acc = acc + part;
  }
  // (wave_sum's and store_chunk's steps stay spelled out in this kernel: through the helpers the compiler allocates its registers differently)
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) acc = acc + __shfl_xor(acc, d, 64);
  if constexpr (WPR > 1) {
    if ((threadIdx.x & 63u) == 0) wave_part[1][threadIdx.x >> 6] = acc;
    __syncthreads();
    acc = ((wave_part[1][0] + wave_part[1][1]) + wave_part[1][2]) + wave_part[1][3];
  }
  const FanParams p = load_fan(f);
#pragma unroll
  for (int u = 0; u < CPL; ++u) {
    const uint32_t c = lane + LPR * u;
    if (c >= chunks_per_row) continue;
    float z[kE];
#pragma unroll
    for (int i = 0; i < kE; ++i) z[i] = v[u][i] / acc;
    Chunk<T, kE> zc;
    zc.pack(z);
    if (out) zc.FFQ_SSTORE(out + base + (size_t)c * kE);
    unpack(zc, z);
    fan_store(f, p, z, base + (size_t)c * kE);
  }
}

// ---------------------------------------------------------------------------------------------------
// E3: sigmoid / GELU + A1:   v = x or T(A2(x)) (per-tensor or per-row parameters),   z = T(op(v)),   codes_j = A1(z; s_j, o_j).
//     Grid-stride over 8-element chunks. Algorithmic bytes / element: 2 (bf16 input) or 1 (int8 codes) [+ 2 (z)] + 1 per code
//     tensor.
// ---------------------------------------------------------------------------------------------------
enum { kActSigmoid = 0, kActGeluErf = 1, kActGeluTanh = 2 };

template <int OP>
__device__ __forceinline__ float activation(float v) {
  if constexpr (OP == kActSigmoid) {
    return 1.0f / (1.0f + expf(-v));
  } else if constexpr (OP == kActGeluErf) {
    constexpr float kAlpha = (float)M_SQRT1_2;
    const float h = v * 0.5f;
    return h * (1.0f + erff(v * kAlpha));
  } else {
    constexpr float kBeta = (float)(M_SQRT2 * M_2_SQRTPI * 0.5);
    constexpr float kKappa = 0.044715f;
    const float cube = (v * v) * v;
    const float inner = kBeta * __builtin_fmaf(kKappa, cube, v);
    const float h = 0.5f * v;
    return h * (1.0f + tanhf(inner));
  }
}

template <typename T, typename TIn, bool DEQ, int OP>
__global__ __launch_bounds__(kEwBlock) void activation_quantize_kernel(const TIn* __restrict__ x, OperandParams px, T* __restrict__ out,
                                                                       FanOut f, uint32_t nchunks) {
  const FanParams fp = load_fan(f);
  const uint32_t stride = gridDim.x * (uint32_t)kEwBlock;
  for (uint32_t c = blockIdx.x * (uint32_t)kEwBlock + threadIdx.x; c < nchunks; c += stride) {
    float s = 1.0f, o = 0.0f;
    params_at<DEQ>(px, c, s, o);
    float v[kE];
    operand_chunk<T, TIn, DEQ>(x + (size_t)c * kE, s, o, v);
#pragma unroll
    for (int i = 0; i < kE; ++i) v[i] = activation<OP>(v[i]);
    Chunk<T, kE> y;  // (store_chunk's steps, spelled out: the helper flips a branch of the GELU forms)
    y.pack(v);
    if (out) y.FFQ_SSTORE(out + (size_t)c * kE);
    unpack(y, v);
    fan_store(f, fp, v, (size_t)c * kE);
  }
}

static unsigned stream_grid(uint32_t nchunks) { return (unsigned)((nchunks + kEwBlock - 1) / kEwBlock); }

}  // namespace ffq

using namespace ffq;

extern "C" int ffq_binary_quantize(int op, const void* a, int a_dt, const float* a_scale, const float* a_offset, int64_t a_param_run,
                                   const void* b, int b_dt, const float* b_scale, const float* b_offset, int64_t b_param_run,
                                   int64_t b_numel, double scalar, double alpha, int dt, int64_t numel, void* out,
                                   const ffq_fanout* fan, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (numel < 0 || b_numel < 0) return fail(FFQ_ERR_ARG, "negative extent");
  if (op < kAdd || op > kDiv) return fail(FFQ_ERR_ARG, "unknown binary op %d (0: add, 1: sub, 2: mul, 3: div)", op);
  if ((op == kMul || op == kDiv) && alpha != 1.0) return fail(FFQ_ERR_ARG, "alpha belongs to add / sub");
  if (!value_dtype(dt)) return fail(FFQ_ERR_DTYPE, "fused add / sub / mul / div is built for bf16 / fp16 values");
  if (numel % kE != 0 || numel >= ((int64_t)1 << 35)) return fail(FFQ_ERR_DTYPE, "fused add / sub / mul / div needs numel %% 8 == 0 and numel < 2^35");
  int rc = check_operand("input", a_dt, a_scale, a_offset, a_param_run, dt, numel, kRowLimit);
  if (rc) return rc;
  if (b) {
    if (numel && (b_numel == 0 || numel % b_numel != 0))
      return fail(FFQ_ERR_TILE_DIVIDE, "other's numel (%lld) must divide input's (%lld)", (long long)b_numel, (long long)numel);
    if (b_numel % kE != 0) return fail(FFQ_ERR_DTYPE, "fused add / sub / mul / div needs other's numel %% 8 == 0");
    rc = check_operand("other", b_dt, b_scale, b_offset, b_param_run, dt, b_numel, kRowLimit);
    if (rc) return rc;
  } else if (b_scale || b_offset || b_param_run || b_numel) {
    return fail(FFQ_ERR_ARG, "a scalar other has no parameters and no extent");
  }
  FanOut f;
  rc = check_launch_args(fan, numel, numel == 0, a, {a, b, out}, &f);
  if (rc || numel == 0) return rc;
  BinArgs g;
  g.pa = operand_params(a_scale, a_offset, a_param_run);
  g.pb = operand_params(b_scale, b_offset, b_param_run);
  g.nchunks = (uint32_t)(numel / kE);
  g.b_chunks = b ? (uint32_t)(b_numel / kE) : 0u;
  g.broadcast = b && b_numel != numel ? 1u : 0u;
  g.by_b = make_fastdiv(g.b_chunks ? g.b_chunks : 1u);
  g.alpha = 1.0f;
  g.scalar = 0.0f;
  if (op == kAdd || op == kSub) {
    g.op = kBinAdd;
    g.alpha = op == kSub ? -(float)alpha : (float)alpha;
    if (!b) {  // ATen scales a scalar other once, in fp32, and adds: a + float(s) * alpha
      g.scalar = (float)scalar * g.alpha;
      g.alpha = 1.0f;
    }
  } else if (op == kMul || b) {
    g.op = op == kMul ? kBinMul : kBinDiv;
    g.scalar = (float)scalar;
  } else {  // torch.div by a scalar: the product with the fp32 reciprocal
    g.op = kBinMul;
    g.scalar = (float)(1.0 / scalar);
  }
  const unsigned grid = stream_grid(g.nchunks);
  dispatch_input(dt, a_dt, a_scale != nullptr, [&](auto t, auto ta, auto da) {
    using T = typename decltype(t)::type;
    using TA = typename decltype(ta)::type;
    auto launch = [&](auto tb, auto db, auto scalar_b) {
      using TB = typename decltype(tb)::type;
      binary_quantize_kernel<T, TA, decltype(da)::value, TB, decltype(db)::value, decltype(scalar_b)::value><<<grid, kEwBlock, 0, s>>>(
          static_cast<const TA*>(a), static_cast<const TB*>(b), g, static_cast<T*>(out), f);
    };
    if (!b) launch(t, std::false_type{}, std::true_type{});
    else dispatch_form<T>(b_dt, b_scale != nullptr, [&](auto tb, auto db) { launch(tb, db, std::false_type{}); });
  });
  return check_launch("binary_quantize_kernel");
}

extern "C" int ffq_softmax_quantize(const void* x, int x_dt, const float* x_scale, const float* x_offset, int x_per_row, int dt,
                                    int64_t rows, int64_t cols, void* out, const ffq_fanout* fan, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (rows < 0 || cols < 0) return fail(FFQ_ERR_ARG, "negative extent");
  if (!value_dtype(dt)) return fail(FFQ_ERR_DTYPE, "fused softmax is built for bf16 / fp16 values");
  int rc = check_operand_form("fused softmax", x_dt, x_scale, x_offset, x_per_row != 0, dt);
  if (rc) return rc;
  if (cols % kE != 0 || cols > 16384)
    return fail(FFQ_ERR_DTYPE, "fused softmax needs cols %% 8 == 0 and cols <= 16384 (got %lld)", (long long)cols);
  if (rows >= ((int64_t)1 << 31)) return fail(FFQ_ERR_ARG, "too many rows");
  FanOut f;
  rc = check_launch_args(fan, rows * cols, rows == 0 || cols == 0, x, {x, out}, &f);
  if (rc || rows == 0 || cols == 0) return rc;
  const uint32_t cpr = (uint32_t)(cols / kE);
  const uint32_t per_row = x_per_row ? 1u : 0u;
  dispatch_input(dt, x_dt, x_scale != nullptr, [&](auto t, auto tin, auto deq) {
    using T = typename decltype(t)::type;
    using TIn = typename decltype(tin)::type;
    dispatch_row_shape(cpr, [&](auto cpl, auto wpr) {
      softmax_quantize_kernel<T, TIn, decltype(deq)::value, decltype(cpl)::value, decltype(wpr)::value>
          <<<row_grid<decltype(wpr)::value>(rows), kBlock, 0, s>>>(static_cast<const TIn*>(x), x_scale, x_offset, per_row, static_cast<T*>(out), f,
                                                                   (uint32_t)rows, cpr);
    });
  });
  return check_launch("softmax_quantize_kernel");
}

extern "C" int ffq_activation_quantize(int op, const void* x, int x_dt, const float* x_scale, const float* x_offset, int64_t param_run,
                                       int dt, int64_t numel, void* out, const ffq_fanout* fan, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (numel < 0) return fail(FFQ_ERR_ARG, "negative extent");
  if (op < kActSigmoid || op > kActGeluTanh) return fail(FFQ_ERR_ARG, "unknown activation %d (0: sigmoid, 1: gelu, 2: gelu tanh)", op);
  if (!value_dtype(dt)) return fail(FFQ_ERR_DTYPE, "fused sigmoid / GELU is built for bf16 / fp16 values");
  if (numel % kE != 0 || numel >= ((int64_t)1 << 35)) return fail(FFQ_ERR_DTYPE, "fused sigmoid / GELU needs numel %% 8 == 0 and numel < 2^35");
  int rc = check_operand("input", x_dt, x_scale, x_offset, param_run, dt, numel, kRowLimit);
  if (rc) return rc;
  FanOut f;
  rc = check_launch_args(fan, numel, numel == 0, x, {x, out}, &f);
  if (rc || numel == 0) return rc;
  const uint32_t nchunks = (uint32_t)(numel / kE);
  const OperandParams px = operand_params(x_scale, x_offset, param_run);
  const unsigned grid = stream_grid(nchunks);
  dispatch_input(dt, x_dt, x_scale != nullptr, [&](auto t, auto tin, auto deq) {
    using T = typename decltype(t)::type;
    using TIn = typename decltype(tin)::type;
    auto launch = [&](auto form) {
      activation_quantize_kernel<T, TIn, decltype(deq)::value, decltype(form)::value><<<grid, kEwBlock, 0, s>>>(
          static_cast<const TIn*>(x), px, static_cast<T*>(out), f, nchunks);
    };
    if (op == kActSigmoid) launch(Int<kActSigmoid>{});
    else if (op == kActGeluErf) launch(Int<kActGeluErf>{});
    else launch(Int<kActGeluTanh>{});
  });
  return check_launch("activation_quantize_kernel");
}
