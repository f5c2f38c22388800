// ffq_elementwise.hip — the reference's quantized add / sub / mul / div, softmax, sigmoid and GELU as one-pass kernels with A1
// fused in.
//
// ff.nn.functional.{add, sub, mul, div, softmax, sigmoid, gelu} run their generated fallbacks in the reference
// (_gen/fallback.py: softmax :269, sigmoid :321, add :801, sub :840, mul :879, div :917, gelu :1373): A2 of each quantized
// operand into a data-dtype tensor, the ATen op, A1 of the output quantizer — up to four launches with a full-size temporary
// between each. Here each is one pass, with the arithmetic of ffq_modules.hip: an operand's codes are dequantized in registers as
// ffq_dequantize.hip does ((q + round(o)) * s in fp32, rounded to the data dtype, exactly the chain's intermediate tensor), the op
// runs in fp32 with ATen's formula and rounds once to the data dtype, and the value goes through the A1 arithmetic of ffq_affine.h
// for up to FFQ_MAX_FANOUT static per-tensor quantizers (ffq_fanout.h). The value itself is stored only when the caller asks.
// ATen's device formulas, as its kernels evaluate them (the library's contraction of a * b + c into one fma included):
//   add / sub:  a + b * alpha  ->  fma(b, +-alpha, a)           (sub is add with -alpha); a scalar b: a + float(b) * (+-alpha)
//   mul / div:  a * b,  a / b (the IEEE quotient);  div by a scalar s: a * float(1 / s), the reciprocal taken of the double s
//   scalar operands enter as float(s), not rounded to the data dtype
//   sigmoid:    1 / (1 + exp(-v))
//   gelu:       (v * 0.5) * (1 + erf(v * M_SQRT1_2));  tanh form: (0.5 * v) * (1 + tanh(kBeta * fma(0.044715, v^3, v)))
//   softmax:    exp(v - max) / sum(exp(v - max))                 (max, sum, quotient in fp32)
// Chunks are 8 elements: 16 B per lane for bf16 / fp16 values, 8 B for int8 codes. Algorithmic bytes per element are stated at
// each kernel; all three are HBM-bound streams.
#ifndef FFQ_NT_STREAMS
#define FFQ_NT_STREAMS 3  // nt loads and stores of the streamed tensors, as ffq_producers.hip
#endif
#include "ffq_affine.h"
#include "ffq_common.h"
#include "ffq_fanout.h"
#include "ffq_vec.h"

#include <math.h>

namespace ffq {

constexpr int kE = 8;          // elements per chunk
constexpr int kEwBlock = 512;  // the streaming kernels' block (as ffq_modules.hip's pointwise kernel)

template <typename T>
__device__ __forceinline__ void unpack8(const Chunk<T, kE>& h, float (&v)[kE]) {
#pragma unroll
  for (int i = 0; i < kE; ++i) v[i] = h.get(i);
}

// One chunk of an operand as values of the data dtype T (held in fp32): plain T, or A2 of codes TIn — (q + round(o)) * s in fp32
// (two roundings, no FMA), rounded once to T. `o` is already rounded. NT: a streamed operand (nt hint); a broadcast one is re-read
// by every row and stays in the caches.
template <typename T, typename TIn, bool DEQ, bool NT = true>
__device__ __forceinline__ void operand_chunk(const TIn* p, float s, float o, float (&v)[kE]) {
  if constexpr (DEQ) {
    Chunk<TIn, kE> q;
    if constexpr (NT) q.FFQ_SLOAD(p); else q.load(p);
#pragma unroll
    for (int i = 0; i < kE; ++i) {
      const float a = q.get(i) + o;
      v[i] = a * s;
    }
    Chunk<T, kE> h;
    h.pack(v);
    unpack8(h, v);
  } else {
    Chunk<T, kE> h;
    if constexpr (NT) h.FFQ_SLOAD(reinterpret_cast<const T*>(p)); else h.load(reinterpret_cast<const T*>(p));
    unpack8(h, v);
  }
}

// Parameters of an operand: one pair, or one per run of `by_run.div` chunks (a row of the last dimension).
struct OperandParams {
  const float* scale;
  const float* offset;
  uint32_t per_row;
  FastDiv by_run;
};

template <bool DEQ>
__device__ __forceinline__ void params_at(const OperandParams& p, uint32_t chunk, float& s, float& o) {
  if constexpr (DEQ) {
    const uint32_t r = p.per_row ? fdiv(chunk, p.by_run) : 0u;
    s = p.scale[r];
    o = p.offset ? rne(p.offset[r]) : 0.0f;
  }
}

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
    Chunk<T, kE> y;
    y.pack(z);  // the one rounding to the data dtype
    if (out) y.FFQ_SSTORE(out + (size_t)c * kE);
    unpack8(y, z);
    fan_store(f, fp, z, (size_t)c * kE);
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
  if constexpr (DEQ) {
    const uint32_t p = per_row ? row : 0u;
    s = xs[p];
    o = xo ? rne(xo[p]) : 0.0f;
  }
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
    zc.pack(z);  // the one rounding to the data dtype
    if (out) zc.FFQ_SSTORE(out + base + (size_t)c * kE);
    unpack8(zc, z);
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
    Chunk<T, kE> y;
    y.pack(v);
    if (out) y.FFQ_SSTORE(out + (size_t)c * kE);
    unpack8(y, v);
    fan_store(f, fp, v, (size_t)c * kE);
  }
}

static bool value_dtype(int dt) { return dt == FFQ_BF16 || dt == FFQ_F16; }

// The host checks of one streamed operand: plain `dt`, or codes of int8 / `dt` with a scale and one parameter pair or one per run
// of `run` elements (run % 8 == 0, run divides numel).
static int check_operand(const char* what, int x_dt, const float* scale, const float* offset, int64_t run, int dt, int64_t numel) {
  if (run < 0) return fail(FFQ_ERR_ARG, "%s: negative parameter run", what);
  const bool deq = scale != nullptr;
  if (deq ? (x_dt != FFQ_I8 && x_dt != dt) : (x_dt != dt || offset || run))
    return fail(FFQ_ERR_DTYPE, "%s: a plain operand of the value dtype, or int8 / value-dtype codes with a scale", what);
  if (run && (run % kE != 0 || numel % run != 0 || numel / run >= ((int64_t)1 << 31)))
    return fail(FFQ_ERR_DTYPE, "%s: per-row parameters need a row length that divides numel and is a multiple of 8", what);
  return FFQ_OK;
}

static OperandParams operand_params(const float* scale, const float* offset, int64_t run) {
  OperandParams p;
  p.scale = scale;
  p.offset = offset;
  p.per_row = run ? 1u : 0u;
  p.by_run = make_fastdiv(run ? (uint32_t)(run / kE) : 1u);
  return p;
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
  int rc = check_operand("input", a_dt, a_scale, a_offset, a_param_run, dt, numel);
  if (rc) return rc;
  if (b) {
    if (numel && (b_numel == 0 || numel % b_numel != 0))
      return fail(FFQ_ERR_TILE_DIVIDE, "other's numel (%lld) must divide input's (%lld)", (long long)b_numel, (long long)numel);
    if (b_numel % kE != 0) return fail(FFQ_ERR_DTYPE, "fused add / sub / mul / div needs other's numel %% 8 == 0");
    rc = check_operand("other", b_dt, b_scale, b_offset, b_param_run, dt, b_numel);
    if (rc) return rc;
  } else if (b_scale || b_offset || b_param_run || b_numel) {
    return fail(FFQ_ERR_ARG, "a scalar other has no parameters and no extent");
  }
  FanOut f;
  rc = fan_from_abi(fan, numel, &f);
  if (rc) return rc;
  if (numel == 0) return FFQ_OK;
  if (!a) return fail(FFQ_ERR_ARG, "NULL buffer");
  if (!aligned16(a) || (b && !aligned16(b)) || (out && !aligned16(out))) return fail(FFQ_ERR_ARG, "buffers must be 16-byte aligned");
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
#define FFQ_E1(T, TA, DA, TB, DB, SC) \
  binary_quantize_kernel<T, TA, DA, TB, DB, SC><<<grid, kEwBlock, 0, s>>>(static_cast<const TA*>(a), static_cast<const TB*>(b), g, static_cast<T*>(out), f)
#define FFQ_E1_B(T, TA, DA)                                           \
  if (!b) { FFQ_E1(T, TA, DA, T, false, true); }                      \
  else if (!b_scale) { FFQ_E1(T, TA, DA, T, false, false); }           \
  else if (b_dt == FFQ_I8) { FFQ_E1(T, TA, DA, int8_t, true, false); } \
  else { FFQ_E1(T, TA, DA, T, true, false); }
#define FFQ_E1_A(T)                                       \
  if (!a_scale) { FFQ_E1_B(T, T, false) }                  \
  else if (a_dt == FFQ_I8) { FFQ_E1_B(T, int8_t, true) }   \
  else { FFQ_E1_B(T, T, true) }
  if (dt == FFQ_BF16) { FFQ_E1_A(bf16_t) } else { FFQ_E1_A(f16_t) }
#undef FFQ_E1_A
#undef FFQ_E1_B
#undef FFQ_E1
  return check_launch("binary_quantize_kernel");
}

extern "C" int ffq_softmax_quantize(const void* x, int x_dt, const float* x_scale, const float* x_offset, int x_per_row, int dt,
                                    int64_t rows, int64_t cols, void* out, const ffq_fanout* fan, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (rows < 0 || cols < 0) return fail(FFQ_ERR_ARG, "negative extent");
  if (!value_dtype(dt)) return fail(FFQ_ERR_DTYPE, "fused softmax is built for bf16 / fp16 values");
  const bool deq = x_scale != nullptr;
  if (deq ? (x_dt != FFQ_I8 && x_dt != dt) : (x_dt != dt || x_offset || x_per_row))
    return fail(FFQ_ERR_DTYPE, "fused softmax takes a plain input of the value dtype, or int8 / value-dtype codes with a scale");
  if (cols % kE != 0 || cols > 16384)
    return fail(FFQ_ERR_DTYPE, "fused softmax needs cols %% 8 == 0 and cols <= 16384 (got %lld)", (long long)cols);
  if (rows >= ((int64_t)1 << 31)) return fail(FFQ_ERR_ARG, "too many rows");
  FanOut f;
  int rc = fan_from_abi(fan, rows * cols, &f);
  if (rc) return rc;
  if (rows == 0 || cols == 0) return FFQ_OK;
  if (!x) return fail(FFQ_ERR_ARG, "NULL buffer");
  if (!aligned16(x) || (out && !aligned16(out))) return fail(FFQ_ERR_ARG, "buffers must be 16-byte aligned");
  const uint32_t cpr = (uint32_t)(cols / kE);
  const uint32_t per_row = x_per_row ? 1u : 0u;
#define FFQ_E2(T, TIN, DEQ, CPL, WPR)                                                                                     \
  softmax_quantize_kernel<T, TIN, DEQ, CPL, WPR><<<(unsigned)((rows + 4 / WPR - 1) / (4 / WPR)), kBlock, 0, s>>>(        \
      static_cast<const TIN*>(x), x_scale, x_offset, per_row, static_cast<T*>(out), f, (uint32_t)rows, cpr)
#define FFQ_E2_SHAPE(T, TIN, DEQ)                 \
  if (cpr <= 64) FFQ_E2(T, TIN, DEQ, 1, 1);       \
  else if (cpr <= 256) FFQ_E2(T, TIN, DEQ, 1, 4); \
  else if (cpr <= 512) FFQ_E2(T, TIN, DEQ, 2, 4); \
  else if (cpr <= 1024) FFQ_E2(T, TIN, DEQ, 4, 4); \
  else FFQ_E2(T, TIN, DEQ, 8, 4)
#define FFQ_E2_INPUT(T)                                       \
  if (!deq) { FFQ_E2_SHAPE(T, T, false); }                    \
  else if (x_dt == FFQ_I8) { FFQ_E2_SHAPE(T, int8_t, true); }  \
  else { FFQ_E2_SHAPE(T, T, true); }
  if (dt == FFQ_BF16) { FFQ_E2_INPUT(bf16_t) } else { FFQ_E2_INPUT(f16_t) }
#undef FFQ_E2_INPUT
#undef FFQ_E2_SHAPE
#undef FFQ_E2
  return check_launch("softmax_quantize_kernel");
}

extern "C" int ffq_activation_quantize(int op, const void* x, int x_dt, const float* x_scale, const float* x_offset, int64_t param_run,
                                       int dt, int64_t numel, void* out, const ffq_fanout* fan, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (numel < 0) return fail(FFQ_ERR_ARG, "negative extent");
  if (op < kActSigmoid || op > kActGeluTanh) return fail(FFQ_ERR_ARG, "unknown activation %d (0: sigmoid, 1: gelu, 2: gelu tanh)", op);
  if (!value_dtype(dt)) return fail(FFQ_ERR_DTYPE, "fused sigmoid / GELU is built for bf16 / fp16 values");
  if (numel % kE != 0 || numel >= ((int64_t)1 << 35)) return fail(FFQ_ERR_DTYPE, "fused sigmoid / GELU needs numel %% 8 == 0 and numel < 2^35");
  int rc = check_operand("input", x_dt, x_scale, x_offset, param_run, dt, numel);
  if (rc) return rc;
  FanOut f;
  rc = fan_from_abi(fan, numel, &f);
  if (rc) return rc;
  if (numel == 0) return FFQ_OK;
  if (!x) return fail(FFQ_ERR_ARG, "NULL buffer");
  if (!aligned16(x) || (out && !aligned16(out))) return fail(FFQ_ERR_ARG, "buffers must be 16-byte aligned");
  const uint32_t nchunks = (uint32_t)(numel / kE);
  const OperandParams px = operand_params(x_scale, x_offset, param_run);
  const unsigned grid = stream_grid(nchunks);
#define FFQ_E3(T, TIN, DEQ, OP) \
  activation_quantize_kernel<T, TIN, DEQ, OP><<<grid, kEwBlock, 0, s>>>(static_cast<const TIN*>(x), px, static_cast<T*>(out), f, nchunks)
#define FFQ_E3_INPUT(T, OP)                              \
  if (!x_scale) { FFQ_E3(T, T, false, OP); }              \
  else if (x_dt == FFQ_I8) { FFQ_E3(T, int8_t, true, OP); } \
  else { FFQ_E3(T, T, true, OP); }
#define FFQ_E3_OP(T)                                                  \
  if (op == kActSigmoid) { FFQ_E3_INPUT(T, kActSigmoid) }              \
  else if (op == kActGeluErf) { FFQ_E3_INPUT(T, kActGeluErf) }         \
  else { FFQ_E3_INPUT(T, kActGeluTanh) }
  if (dt == FFQ_BF16) { FFQ_E3_OP(bf16_t) } else { FFQ_E3_OP(f16_t) }
#undef FFQ_E3_OP
#undef FFQ_E3_INPUT
#undef FFQ_E3
  return check_launch("activation_quantize_kernel");
}
