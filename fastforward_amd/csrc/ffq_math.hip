// ffq_math.hip — the reference's quantized rms_norm, pow by a number, exp, sin, cos, sum and cumsum as one-pass kernels with A1
// fused in.
//
// ff.nn.functional.{rms_norm, pow, exp, sin, cos, sum, cumsum} run their generated fallbacks in the reference (_gen/fallback.py:
// pow :955, sum :993, cumsum :1520, exp :1831, sin :1856, cos :1881, rms_norm :1906): A2 of the quantized input into a data-dtype
// tensor, the ATen op, A1 of the output quantizer — three launches with a full-size temporary between each. Here each is one pass
// under the A2 / op / A1 contract of ffq_onepass.h.
// ATen's device formulas (torch 2.10, MI355X; each confirmed bit for bit against its kernels on every bf16 / fp16 value):
//   exp / sin / cos:  expf / sinf / cosf of the fp32 value
//   pow(v, e):  e == 0: 1;  e == 1: v;  e == 0.5: sqrtf(v);  e == -0.5: rsqrtf(v);  e == -1: 1 / v;  else with e' = dt(e) (ATen
//               converts the exponent to the data dtype):  e' == 2: v * v;  e' == 3: dt(v * v) * v;  e' == -2: 1 / dt(v * v);
//               otherwise powf(v, e')        (dt(.): a product ATen rounds to the data dtype before the next step)
//   rms_norm:   r = rsqrt(sum(v^2) / cols + eps);  dt((v * r) * w), one rounding (ATen's fused kernel; fp32 products commute)
//   sum:        an fp32 sum rounded once (ATen accumulates in fp32; the order is the kernel's own here)
//   cumsum:     ATen's device kernel keeps its running sum in the DATA dtype (up to ~2 of an N(0, 1) row of 4096 bf16 values
//               away from the exact scan); these kernels keep an fp32 running sum and round each prefix once, as ATen's CPU kernel
// All kernels are HBM-bound streams.
#ifndef FFQ_NT_STREAMS
#define FFQ_NT_STREAMS 3  // nt loads and stores of the streamed tensors, as ffq_elementwise.hip
#endif
#include "ffq_onepass.h"

namespace ffq {

constexpr int kStreamBlock = 512;  // the grid-stride kernels' block (as ffq_elementwise.hip)
constexpr uint32_t kSegmentRows = 64;        // rows a lane of the column reduction walks at least
constexpr uint32_t kTargetLanes = 256u * 1024u;  // lanes the column reduction aims for (1024 blocks of 256)
constexpr uint32_t kAllBlocks = 1024;        // first-stage blocks of the full reduction (its workspace: one fp32 each)
constexpr int kRowsInFlight = 8;             // rows a lane of the column kernels loads before it adds them

// chunk `c` of the input as values (its parameters looked up by chunk)
template <typename T, typename TIn, bool DEQ>
__device__ __forceinline__ void load_at(const TIn* x, const OperandParams& px, uint32_t c, float (&v)[kE]) {
  float s = 1.0f, o = 0.0f;
  params_at<DEQ>(px, c, s, o);
  operand_chunk<T, TIn, DEQ>(x + (size_t)c * kE, s, o, v);
}

// ---------------------------------------------------------------------------------------------------
// R1: rms_norm over the last `cols` elements + A1:   v = x or T(A2(x)) (per-tensor or per-row parameters);
//     r = rsqrt(sum(v^2) / cols + eps),  z = T((v * r) * w) (no weight: T(v * r)),   codes_j = A1(z; s_j, o_j).
//     The geometry and reduction plan of layer_norm_quantize_kernel (ffq_modules.hip): WPR wavefronts per row, CPL chunks of 8
//     per lane, cols <= 8 * 64 * WPR * CPL; the row is read once and stays in registers.
//     Algorithmic bytes / element: 2 (bf16 input) or 1 (int8 codes) [+ 2 (z)] + 1 per code tensor (+ the weight, cached).
// ---------------------------------------------------------------------------------------------------
template <typename T, typename TIn, bool DEQ, int CPL, int WPR>
__global__ __launch_bounds__(kBlock) void rms_norm_quantize_kernel(const TIn* __restrict__ x, const float* __restrict__ xs,
                                                                   const float* __restrict__ xo, uint32_t per_row,
                                                                   const T* __restrict__ weight, T* __restrict__ out, FanOut f,
                                                                   uint32_t rows, uint32_t chunks_per_row, float cols_f, float eps) {
  constexpr uint32_t LPR = 64u * WPR;
  const uint32_t lane = threadIdx.x % LPR;
  const uint32_t row = blockIdx.x * (kBlock / LPR) + threadIdx.x / LPR;
  if (row >= rows) return;  // block-uniform when WPR == 4
  const size_t base = (size_t)row * chunks_per_row * kE;
  float s = 1.0f, o = 0.0f;
  row_params<DEQ>(xs, xo, per_row, row, s, o);
  float v[CPL][kE];
  float acc = 0.0f;
#pragma unroll
  for (int u = 0; u < CPL; ++u) {
    const uint32_t c = lane + LPR * u;
    if (c >= chunks_per_row) continue;
    operand_chunk<T, TIn, DEQ>(x + base + (size_t)c * kE, s, o, v[u]);
    float part = 0.0f;
#pragma unroll
    for (int i = 0; i < kE; ++i) part = part + v[u][i] * v[u][i];
    acc = acc + part;
  }
  __shared__ float wave_part[kBlock / 64];
  acc = wave_sum(acc);
  if constexpr (WPR > 1) {
    if ((threadIdx.x & 63u) == 0) wave_part[threadIdx.x >> 6] = acc;
    __syncthreads();
    acc = ((wave_part[0] + wave_part[1]) + wave_part[2]) + wave_part[3];
  }
  const float r = rsqrtf(acc / cols_f + eps);
  const FanParams p = load_fan(f);
#pragma unroll
  for (int u = 0; u < CPL; ++u) {
    const uint32_t c = lane + LPR * u;
    if (c >= chunks_per_row) continue;
    float z[kE];
#pragma unroll
    for (int i = 0; i < kE; ++i) z[i] = v[u][i] * r;
    if (weight) {
      Chunk<T, kE> w;
      w.load(weight + (size_t)c * kE);
#pragma unroll
      for (int i = 0; i < kE; ++i) z[i] = z[i] * w.get(i);
    }
    store_chunk<T>(out, f, p, z, base + (size_t)c * kE);
  }
}

// ---------------------------------------------------------------------------------------------------
// U1: exp / sin / cos / pow by a number + A1:   v = x or T(A2(x)) (per-tensor or per-row parameters),   z = T(op(v)),
//     codes_j = A1(z; s_j, o_j). Grid-stride over 8-element chunks (activation_quantize_kernel's plan).
//     Algorithmic bytes / element: 2 (bf16 input) or 1 (int8 codes) [+ 2 (z)] + 1 per code tensor.
// ---------------------------------------------------------------------------------------------------
enum { kOpExp = 0, kOpSin = 1, kOpCos = 2, kOpPow = 3 };  // the ABI's ops (include/ffq.h)
enum { kFExp, kFSin, kFCos, kFOne, kFCopy, kFSquare, kFCube, kFSqrt, kFRsqrt, kFRecip, kFInvSquare, kFPow };  // the device's forms

template <typename T, int FORM>
__device__ __forceinline__ float unary(float v, float e) {
  constexpr int kDt = TypeTag<T>::value;
  if constexpr (FORM == kFExp) return expf(v);
  else if constexpr (FORM == kFSin) return sinf(v);
  else if constexpr (FORM == kFCos) return cosf(v);
  else if constexpr (FORM == kFOne) return 1.0f;
  else if constexpr (FORM == kFCopy) return v;
  else if constexpr (FORM == kFSquare) return v * v;
  else if constexpr (FORM == kFCube) return round_stage(v * v, kDt) * v;
  else if constexpr (FORM == kFSqrt) return sqrtf(v);
  else if constexpr (FORM == kFRsqrt) return rsqrtf(v);
  else if constexpr (FORM == kFRecip) return 1.0f / v;
  else if constexpr (FORM == kFInvSquare) return 1.0f / round_stage(v * v, kDt);
  else return powf(v, e);
}

template <typename T, typename TIn, bool DEQ, int FORM>
__global__ __launch_bounds__(kStreamBlock) void unary_quantize_kernel(const TIn* __restrict__ x, OperandParams px, float exponent,
                                                                      T* __restrict__ out, FanOut f, uint32_t nchunks) {
  const FanParams fp = load_fan(f);
  const uint32_t stride = gridDim.x * (uint32_t)kStreamBlock;
  for (uint32_t c = blockIdx.x * (uint32_t)kStreamBlock + threadIdx.x; c < nchunks; c += stride) {
    float s = 1.0f, o = 0.0f;
    params_at<DEQ>(px, c, s, o);
    float v[kE];
    operand_chunk<T, TIn, DEQ>(x + (size_t)c * kE, s, o, v);
#pragma unroll
    for (int i = 0; i < kE; ++i) v[i] = unary<T, FORM>(v[i], exponent);
    store_chunk<T>(out, f, fp, v, (size_t)c * kE);
  }
}

// ---------------------------------------------------------------------------------------------------
// S: sum over the middle axis of [outer, len, inner] + A1:   z = T(fp32 sum of v),   codes_j = A1(z; s_j, o_j).
//   S1 (inner == 1, outer > 1): WPR wavefronts per row (one for rows of <= 512 elements, a block of four otherwise); each lane sums
//      its chunks in order, the wave by butterfly, the block's waves in order.
//   S2 (inner > 1): a lane per 8 columns of one outer index walks `seg_rows` rows of len in order; with one segment it finishes
//      the sums, with `segments` > 1 it leaves fp32 partials [segments, outer * inner] in the workspace and S3 adds them in order.
//   S4 / S5 (outer == inner == 1, the whole tensor): kAllBlocks blocks leave one fp32 partial each, one block adds them.
//   Every order is fixed by the shape alone: the result is deterministic (no float atomics).
//   Algorithmic bytes / input element: 2 (bf16) or 1 (int8 codes); the output is outer * inner elements.
// ---------------------------------------------------------------------------------------------------
template <typename T, typename TIn, bool DEQ, int WPR>
__global__ __launch_bounds__(kBlock) void reduce_rows_kernel(const TIn* __restrict__ x, OperandParams px, T* __restrict__ out, FanOut f,
                                                             uint32_t rows, uint32_t chunks_per_row) {
  constexpr uint32_t LPR = 64u * WPR;
  const uint32_t lane = threadIdx.x % LPR;
  const uint32_t row = blockIdx.x * (kBlock / LPR) + threadIdx.x / LPR;
  if (row >= rows) return;  // block-uniform when WPR == 4
  const uint32_t first = row * chunks_per_row;
  float acc = 0.0f;
  for (uint32_t c = lane; c < chunks_per_row; c += LPR) {
    float s = 1.0f, o = 0.0f;
    params_at<DEQ>(px, first + c, s, o);
    float v[kE];
    operand_chunk<T, TIn, DEQ>(x + (size_t)(first + c) * kE, s, o, v);
    float part = 0.0f;
#pragma unroll
    for (int i = 0; i < kE; ++i) part = part + v[i];
    acc = acc + part;
  }
  __shared__ float wave_part[kBlock / 64];
  acc = wave_sum(acc);
  if constexpr (WPR > 1) {
    if ((threadIdx.x & 63u) == 0) wave_part[threadIdx.x >> 6] = acc;
    __syncthreads();
    acc = ((wave_part[0] + wave_part[1]) + wave_part[2]) + wave_part[3];
  }
  if (lane == 0) store_one<T>(out, f, load_fan(f), acc, row);
}

struct ColArgs {
  uint32_t ncols;            // outer * inner / 8: lanes per segment
  uint32_t inner_chunks;     // inner / 8
  uint32_t len, seg_rows, segments;
  FastDiv by_ncols, by_inner_chunks;
};

template <typename T, typename TIn, bool DEQ, bool FINAL>
__global__ __launch_bounds__(kBlock) void reduce_cols_kernel(const TIn* __restrict__ x, OperandParams px, ColArgs a, T* __restrict__ out,
                                                             FanOut f, float* __restrict__ partial) {
  const uint32_t t = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  if (t >= a.ncols * a.segments) return;
  const uint32_t seg = fdiv(t, a.by_ncols);
  const uint32_t col = t - seg * a.ncols;
  const uint32_t o_idx = fdiv(col, a.by_inner_chunks);
  const uint32_t ic = col - o_idx * a.inner_chunks;
  const uint32_t l0 = seg * a.seg_rows;
  const uint32_t l1 = min(a.len, l0 + a.seg_rows);
  // chunk index of (o_idx, l, ic): (o_idx * len + l) * inner_chunks + ic
  uint32_t c = (o_idx * a.len + l0) * a.inner_chunks + ic;
  float acc[kE];
#pragma unroll
  for (int i = 0; i < kE; ++i) acc[i] = 0.0f;
  uint32_t l = l0;
  for (; l + kRowsInFlight <= l1; l += kRowsInFlight, c += kRowsInFlight * a.inner_chunks) {
    float v[kRowsInFlight][kE];  // the loads of kRowsInFlight rows first, then the adds in row order
#pragma unroll
    for (int u = 0; u < kRowsInFlight; ++u) load_at<T, TIn, DEQ>(x, px, c + u * a.inner_chunks, v[u]);
#pragma unroll
    for (int u = 0; u < kRowsInFlight; ++u) {
#pragma unroll
      for (int i = 0; i < kE; ++i) acc[i] = acc[i] + v[u][i];
    }
  }
  for (; l < l1; ++l, c += a.inner_chunks) {
    float v[kE];
    load_at<T, TIn, DEQ>(x, px, c, v);
#pragma unroll
    for (int i = 0; i < kE; ++i) acc[i] = acc[i] + v[i];
  }
  if constexpr (FINAL) {
    store_chunk<T>(out, f, load_fan(f), acc, (size_t)col * kE);
  } else {
    Chunk<float, kE> y;
#pragma unroll
    for (int i = 0; i < kE; ++i) y.w[i] = __builtin_bit_cast(uint32_t, acc[i]);
    y.store(partial + ((size_t)seg * a.ncols + col) * kE);
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void reduce_cols_finish_kernel(const float* __restrict__ partial, uint32_t ncols, uint32_t segments,
                                                                    T* __restrict__ out, FanOut f) {
  const uint32_t col = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  if (col >= ncols) return;
  float acc[kE];
#pragma unroll
  for (int i = 0; i < kE; ++i) acc[i] = 0.0f;
  for (uint32_t seg = 0; seg < segments; ++seg) {
    Chunk<float, kE> y;
    y.load(partial + ((size_t)seg * ncols + col) * kE);
#pragma unroll
    for (int i = 0; i < kE; ++i) acc[i] = acc[i] + y.get(i);
  }
  store_chunk<T>(out, f, load_fan(f), acc, (size_t)col * kE);
}

// block-wide sum of one value per lane: butterfly in each wave, the four waves in order (the result is valid in every lane)
__device__ __forceinline__ float block_sum(float acc) {
  __shared__ float wave_part[kBlock / 64];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63u) == 0) wave_part[threadIdx.x >> 6] = acc;
  __syncthreads();
  return ((wave_part[0] + wave_part[1]) + wave_part[2]) + wave_part[3];
}

template <typename T, typename TIn, bool DEQ>
__global__ __launch_bounds__(kBlock) void reduce_all_kernel(const TIn* __restrict__ x, OperandParams px, uint32_t nchunks, float* __restrict__ partial) {
  const uint32_t stride = gridDim.x * (uint32_t)kBlock;
  float acc = 0.0f;
  for (uint32_t c = blockIdx.x * (uint32_t)kBlock + threadIdx.x; c < nchunks; c += stride) {
    float s = 1.0f, o = 0.0f;
    params_at<DEQ>(px, c, s, o);
    float v[kE];
    operand_chunk<T, TIn, DEQ>(x + (size_t)c * kE, s, o, v);
    float part = 0.0f;
#pragma unroll
    for (int i = 0; i < kE; ++i) part = part + v[i];
    acc = acc + part;
  }
  acc = block_sum(acc);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void reduce_all_finish_kernel(const float* __restrict__ partial, uint32_t blocks, T* __restrict__ out, FanOut f) {
  float acc = 0.0f;
  for (uint32_t b = threadIdx.x; b < blocks; b += kBlock) acc = acc + partial[b];
  acc = block_sum(acc);
  if (threadIdx.x == 0) store_one<T>(out, f, load_fan(f), acc, 0);
}

// ---------------------------------------------------------------------------------------------------
// C: cumsum along the middle axis of [outer, len, inner] + A1:   z_l = T(fp32 sum of v_0 .. v_l),   codes_j = A1(z; s_j, o_j).
//   C1 (inner == 1): a block per row walks it in tiles of 256 chunks: each lane scans its 8 values in order, the lanes' totals are
//      scanned across the wave (Hillis-Steele) and across the four waves in order, and the running total of the earlier tiles
//      is carried in a register. Any len % 8 == 0.
//   C2 (inner > 1): a lane per 8 columns of one outer index walks len in order (a sequential fp32 scan).
//   Algorithmic bytes / element: 2 (bf16 input) or 1 (int8 codes) [+ 2 (z)] + 1 per code tensor.
// ---------------------------------------------------------------------------------------------------
template <typename T, typename TIn, bool DEQ>
__global__ __launch_bounds__(kBlock) void scan_rows_kernel(const TIn* __restrict__ x, OperandParams px, T* __restrict__ out, FanOut f,
                                                           uint32_t chunks_per_row) {
  const uint32_t row = blockIdx.x;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t first = row * chunks_per_row;
  const FanParams fp = load_fan(f);
  __shared__ float wave_total[2][kBlock / 64];
  float carry = 0.0f;
  for (uint32_t tile = 0, parity = 0; tile < chunks_per_row; tile += kBlock, parity ^= 1u) {
    const uint32_t c = tile + threadIdx.x;
    float v[kE];
#pragma unroll
    for (int i = 0; i < kE; ++i) v[i] = 0.0f;
    if (c < chunks_per_row) {
      float s = 1.0f, o = 0.0f;
      params_at<DEQ>(px, first + c, s, o);
      operand_chunk<T, TIn, DEQ>(x + (size_t)(first + c) * kE, s, o, v);
    }
#pragma unroll
    for (int i = 1; i < kE; ++i) v[i] = v[i - 1] + v[i];
    // inclusive scan of the lanes' totals across the wave
    float incl = v[kE - 1];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const float y = __shfl_up(incl, d, 64);
      if (lane >= (uint32_t)d) incl = incl + y;
    }
    float excl = __shfl_up(incl, 1, 64);
    if (lane == 0) excl = 0.0f;
    if (lane == 63) wave_total[parity][wave] = incl;
    __syncthreads();  // (double-buffered by tile parity: one barrier per tile)
    float before = carry;
    for (uint32_t w = 0; w < wave; ++w) before = before + wave_total[parity][w];
    const float prefix = before + excl;
    carry = carry + (((wave_total[parity][0] + wave_total[parity][1]) + wave_total[parity][2]) + wave_total[parity][3]);
    if (c < chunks_per_row) {
      float z[kE];
#pragma unroll
      for (int i = 0; i < kE; ++i) z[i] = prefix + v[i];
      store_chunk<T>(out, f, fp, z, (size_t)(first + c) * kE);
    }
  }
}

template <typename T, typename TIn, bool DEQ>
__global__ __launch_bounds__(kBlock) void scan_cols_kernel(const TIn* __restrict__ x, OperandParams px, ColArgs a, T* __restrict__ out, FanOut f) {
  const uint32_t col = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  if (col >= a.ncols) return;
  const uint32_t o_idx = fdiv(col, a.by_inner_chunks);
  const uint32_t ic = col - o_idx * a.inner_chunks;
  const FanParams fp = load_fan(f);
  uint32_t c = o_idx * a.len * a.inner_chunks + ic;
  float acc[kE];
#pragma unroll
  for (int i = 0; i < kE; ++i) acc[i] = 0.0f;
  uint32_t l = 0;
  for (; l + kRowsInFlight <= a.len; l += kRowsInFlight, c += kRowsInFlight * a.inner_chunks) {
    float v[kRowsInFlight][kE];  // the loads of kRowsInFlight rows first, then the scan in row order
#pragma unroll
    for (int u = 0; u < kRowsInFlight; ++u) load_at<T, TIn, DEQ>(x, px, c + u * a.inner_chunks, v[u]);
#pragma unroll
    for (int u = 0; u < kRowsInFlight; ++u) {
#pragma unroll
      for (int i = 0; i < kE; ++i) {
        acc[i] = acc[i] + v[u][i];
        v[u][i] = acc[i];
      }
      store_chunk<T>(out, f, fp, v[u], (size_t)(c + u * a.inner_chunks) * kE);
    }
  }
  for (; l < a.len; ++l, c += a.inner_chunks) {
    float v[kE];
    load_at<T, TIn, DEQ>(x, px, c, v);
#pragma unroll
    for (int i = 0; i < kE; ++i) {
      acc[i] = acc[i] + v[i];
      v[i] = acc[i];
    }
    store_chunk<T>(out, f, fp, v, (size_t)c * kE);
  }
}

static unsigned blocks_for(uint64_t lanes, unsigned block) { return (unsigned)((lanes + block - 1) / block); }

// The plan of a sum: the column reduction's segments, or the full reduction's blocks (workspace = fp32 partials).
struct SumPlan {
  uint32_t segments, seg_rows;
  size_t workspace;
};

static SumPlan sum_plan(int64_t outer, int64_t len, int64_t inner) {
  SumPlan p{1u, (uint32_t)len, 0};
  if (outer * inner == 1) {
    p.workspace = kAllBlocks * sizeof(float);
  } else if (inner > 1) {
    const uint64_t ncols = (uint64_t)(outer * inner / kE);
    uint64_t want = (kTargetLanes + ncols - 1) / ncols;
    const uint64_t most = ((uint64_t)len + kSegmentRows - 1) / kSegmentRows;
    if (want > most) want = most;
    if (want > 1) {
      p.seg_rows = (uint32_t)(((uint64_t)len + want - 1) / want);
      p.segments = (uint32_t)(((uint64_t)len + p.seg_rows - 1) / p.seg_rows);
      p.workspace = (size_t)p.segments * (size_t)(outer * inner) * sizeof(float);
    }
  }
  return p;
}

// shared checks of sum / cumsum: extents, 8-element chunks along the contiguous axis, 32-bit chunk indices
static int check_axes(const char* what, int64_t outer, int64_t len, int64_t inner) {
  if (outer < 0 || len < 0 || inner < 0) return fail(FFQ_ERR_ARG, "negative extent");
  const int64_t numel = outer * len * inner;
  if (numel >= ((int64_t)1 << 35)) return fail(FFQ_ERR_DTYPE, "%s needs numel < 2^35", what);
  if (inner == 1 ? len % kE != 0 : inner % kE != 0)
    return fail(FFQ_ERR_DTYPE, "%s needs 8 | len when inner == 1, else 8 | inner (got [%lld, %lld, %lld])", what, (long long)outer,
                (long long)len, (long long)inner);
  return FFQ_OK;
}

}  // namespace ffq

using namespace ffq;

extern "C" int ffq_rms_norm_quantize(const void* x, int x_dt, const float* x_scale, const float* x_offset, int x_per_row,
                                     const void* weight, int dt, int64_t rows, int64_t cols, double eps, void* out,
                                     const ffq_fanout* fan, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (rows < 0 || cols < 0) return fail(FFQ_ERR_ARG, "negative extent");
  if (!value_dtype(dt)) return fail(FFQ_ERR_DTYPE, "fused rms_norm is built for bf16 / fp16 values");
  int rc = check_operand_form("fused rms_norm", x_dt, x_scale, x_offset, x_per_row != 0, dt);
  if (rc) return rc;
  if (cols == 0) return fail(FFQ_ERR_EMPTY, "rms_norm over an empty row");
  if (cols % kE != 0 || cols > 16384)
    return fail(FFQ_ERR_DTYPE, "fused rms_norm needs cols %% 8 == 0 and cols <= 16384 (got %lld)", (long long)cols);
  if (rows >= ((int64_t)1 << 31)) return fail(FFQ_ERR_ARG, "too many rows");
  FanOut f;
  rc = check_launch_args(fan, rows * cols, rows == 0, x, {x, weight, out}, &f);
  if (rc || rows == 0) return rc;
  const uint32_t cpr = (uint32_t)(cols / kE);
  const uint32_t per_row = x_per_row ? 1u : 0u;
  dispatch_input(dt, x_dt, x_scale != nullptr, [&](auto t, auto tin, auto deq) {
    using T = typename decltype(t)::type;
    using TIn = typename decltype(tin)::type;
    dispatch_row_shape(cpr, [&](auto cpl, auto wpr) {
      rms_norm_quantize_kernel<T, TIn, decltype(deq)::value, decltype(cpl)::value, decltype(wpr)::value>
          <<<row_grid<decltype(wpr)::value>(rows), kBlock, 0, s>>>(static_cast<const TIn*>(x), x_scale, x_offset, per_row, static_cast<const T*>(weight),
                                                                   static_cast<T*>(out), f, (uint32_t)rows, cpr, (float)cols, (float)eps);
    });
  });
  return check_launch("rms_norm_quantize_kernel");
}

extern "C" int ffq_unary_quantize(int op, const void* x, int x_dt, const float* x_scale, const float* x_offset, int64_t param_run,
                                  double exponent, int dt, int64_t numel, void* out, const ffq_fanout* fan, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (numel < 0) return fail(FFQ_ERR_ARG, "negative extent");
  if (op < kOpExp || op > kOpPow) return fail(FFQ_ERR_ARG, "unknown unary op %d (0: exp, 1: sin, 2: cos, 3: pow)", op);
  if (op != kOpPow && exponent != 0.0) return fail(FFQ_ERR_ARG, "the exponent belongs to pow");
  if (!value_dtype(dt)) return fail(FFQ_ERR_DTYPE, "fused exp / sin / cos / pow is built for bf16 / fp16 values");
  if (numel % kE != 0 || numel >= ((int64_t)1 << 35)) return fail(FFQ_ERR_DTYPE, "fused exp / sin / cos / pow needs numel %% 8 == 0 and numel < 2^35");
  int rc = check_operand("fused exp / sin / cos / pow", x_dt, x_scale, x_offset, param_run, dt, numel, 0);
  if (rc) return rc;
  // ATen's branches (pow_Tensor_Scalar_out, then its device kernel): the exact exponent first, then the one converted to dt
  int form = op == kOpExp ? kFExp : op == kOpSin ? kFSin : op == kOpCos ? kFCos : kFPow;
  const float e = round_stage((float)exponent, dt);
  if (op == kOpPow) {
    if (!(exponent == exponent) || fabs(exponent) > 65504.0) return fail(FFQ_ERR_ARG, "the exponent must be finite and within the fp16 range");
    if (exponent == 0.0) form = kFOne;
    else if (exponent == 1.0) form = kFCopy;
    else if (exponent == 0.5) form = kFSqrt;
    else if (exponent == -0.5) form = kFRsqrt;
    else if (exponent == -1.0) form = kFRecip;
    else if (e == 2.0f) form = kFSquare;
    else if (e == 3.0f) form = kFCube;
    else if (e == -2.0f) form = kFInvSquare;
  }
  FanOut f;
  rc = check_launch_args(fan, numel, numel == 0, x, {x, out}, &f);
  if (rc || numel == 0) return rc;
  const uint32_t nchunks = (uint32_t)(numel / kE);
  const OperandParams px = operand_params(x_scale, x_offset, param_run);
  const unsigned grid = blocks_for(nchunks, kStreamBlock);
  dispatch_input(dt, x_dt, x_scale != nullptr, [&](auto t, auto tin, auto deq) {
    using T = typename decltype(t)::type;
    using TIn = typename decltype(tin)::type;
    auto launch = [&](auto f_) {
      unary_quantize_kernel<T, TIn, decltype(deq)::value, decltype(f_)::value><<<grid, kStreamBlock, 0, s>>>(
          static_cast<const TIn*>(x), px, e, static_cast<T*>(out), f, nchunks);
    };
    switch (form) {
      case kFExp: launch(Int<kFExp>{}); break;
      case kFSin: launch(Int<kFSin>{}); break;
      case kFCos: launch(Int<kFCos>{}); break;
      case kFOne: launch(Int<kFOne>{}); break;
      case kFCopy: launch(Int<kFCopy>{}); break;
      case kFSquare: launch(Int<kFSquare>{}); break;
      case kFCube: launch(Int<kFCube>{}); break;
      case kFSqrt: launch(Int<kFSqrt>{}); break;
      case kFRsqrt: launch(Int<kFRsqrt>{}); break;
      case kFRecip: launch(Int<kFRecip>{}); break;
      case kFInvSquare: launch(Int<kFInvSquare>{}); break;
      default: launch(Int<kFPow>{}); break;
    }
  });
  return check_launch("unary_quantize_kernel");
}

extern "C" size_t ffq_sum_quantize_workspace_bytes(int64_t outer, int64_t len, int64_t inner) {
  if (outer <= 0 || len <= 0 || inner <= 0) return 0;
  return sum_plan(outer, len, inner).workspace;
}

extern "C" int ffq_sum_quantize(const void* x, int x_dt, const float* x_scale, const float* x_offset, int64_t param_run, int dt,
                                int64_t outer, int64_t len, int64_t inner, void* out, const ffq_fanout* fan, void* workspace,
                                size_t workspace_bytes, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (!value_dtype(dt)) return fail(FFQ_ERR_DTYPE, "fused sum is built for bf16 / fp16 values");
  int rc = check_axes("fused sum", outer, len, inner);
  if (rc) return rc;
  const int64_t numel = outer * len * inner;
  rc = check_operand("fused sum", x_dt, x_scale, x_offset, param_run, dt, numel, 0);
  if (rc) return rc;
  FanOut f;
  rc = fan_from_abi(fan, outer * inner, &f);
  if (rc) return rc;
  if (outer == 0 || inner == 0) return FFQ_OK;
  if (len == 0) return fail(FFQ_ERR_EMPTY, "a sum over an empty axis is not built (ATen gives zeros)");
  rc = check_buffers(x, {x, inner > 1 ? out : nullptr});  // (inner == 1 stores its results one by one)
  if (rc) return rc;
  const SumPlan plan = sum_plan(outer, len, inner);
  if (plan.workspace && (!workspace || workspace_bytes < plan.workspace || !aligned16(workspace)))
    return fail(FFQ_ERR_WORKSPACE, "fused sum needs %zu bytes of 16-byte aligned workspace", plan.workspace);
  float* partial = static_cast<float*>(workspace);
  const OperandParams px = operand_params(x_scale, x_offset, param_run);
  if (outer * inner == 1) {  // S4 / S5: the whole tensor
    const uint32_t nchunks = (uint32_t)(numel / kE);
    dispatch_input(dt, x_dt, x_scale != nullptr, [&](auto t, auto tin, auto deq) {
      using T = typename decltype(t)::type;
      using TIn = typename decltype(tin)::type;
      reduce_all_kernel<T, TIn, decltype(deq)::value><<<kAllBlocks, kBlock, 0, s>>>(static_cast<const TIn*>(x), px, nchunks, partial);
      reduce_all_finish_kernel<T><<<1, kBlock, 0, s>>>(partial, kAllBlocks, static_cast<T*>(out), f);
    });
    return check_launch("reduce_all_kernel");
  }
  if (inner == 1) {  // S1: rows
    if (outer >= ((int64_t)1 << 31)) return fail(FFQ_ERR_ARG, "too many rows");
    const uint32_t cpr = (uint32_t)(len / kE);
    dispatch_input(dt, x_dt, x_scale != nullptr, [&](auto t, auto tin, auto deq) {
      using T = typename decltype(t)::type;
      using TIn = typename decltype(tin)::type;
      auto launch = [&](auto wpr) {
        reduce_rows_kernel<T, TIn, decltype(deq)::value, decltype(wpr)::value><<<row_grid<decltype(wpr)::value>(outer), kBlock, 0, s>>>(
            static_cast<const TIn*>(x), px, static_cast<T*>(out), f, (uint32_t)outer, cpr);
      };
      if (cpr <= 64) launch(Int<1>{}); else launch(Int<4>{});
    });
    return check_launch("reduce_rows_kernel");
  }
  // S2 / S3: columns
  ColArgs a;
  a.ncols = (uint32_t)(outer * inner / kE);
  a.inner_chunks = (uint32_t)(inner / kE);
  a.len = (uint32_t)len;
  a.seg_rows = plan.seg_rows;
  a.segments = plan.segments;
  a.by_ncols = make_fastdiv(a.ncols);
  a.by_inner_chunks = make_fastdiv(a.inner_chunks);
  const unsigned grid = blocks_for((uint64_t)a.ncols * a.segments, kBlock);
  dispatch_input(dt, x_dt, x_scale != nullptr, [&](auto t, auto tin, auto deq) {
    using T = typename decltype(t)::type;
    using TIn = typename decltype(tin)::type;
    constexpr bool DEQ = decltype(deq)::value;
    if (a.segments == 1) {
      reduce_cols_kernel<T, TIn, DEQ, true><<<grid, kBlock, 0, s>>>(static_cast<const TIn*>(x), px, a, static_cast<T*>(out), f, nullptr);
    } else {
      reduce_cols_kernel<T, TIn, DEQ, false><<<grid, kBlock, 0, s>>>(static_cast<const TIn*>(x), px, a, nullptr, f, partial);
      reduce_cols_finish_kernel<T><<<blocks_for(a.ncols, kBlock), kBlock, 0, s>>>(partial, a.ncols, a.segments, static_cast<T*>(out), f);
    }
  });
  return check_launch("reduce_cols_kernel");
}

extern "C" int ffq_cumsum_quantize(const void* x, int x_dt, const float* x_scale, const float* x_offset, int64_t param_run, int dt,
                                   int64_t outer, int64_t len, int64_t inner, void* out, const ffq_fanout* fan, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (!value_dtype(dt)) return fail(FFQ_ERR_DTYPE, "fused cumsum is built for bf16 / fp16 values");
  int rc = check_axes("fused cumsum", outer, len, inner);
  if (rc) return rc;
  const int64_t numel = outer * len * inner;
  rc = check_operand("fused cumsum", x_dt, x_scale, x_offset, param_run, dt, numel, 0);
  if (rc) return rc;
  FanOut f;
  rc = check_launch_args(fan, numel, numel == 0, x, {x, out}, &f);
  if (rc || numel == 0) return rc;
  const OperandParams px = operand_params(x_scale, x_offset, param_run);
  if (inner == 1) {  // C1: rows
    if (outer >= ((int64_t)1 << 31)) return fail(FFQ_ERR_ARG, "too many rows");
    const uint32_t cpr = (uint32_t)(len / kE);
    dispatch_input(dt, x_dt, x_scale != nullptr, [&](auto t, auto tin, auto deq) {
      using T = typename decltype(t)::type;
      using TIn = typename decltype(tin)::type;
      scan_rows_kernel<T, TIn, decltype(deq)::value><<<(unsigned)outer, kBlock, 0, s>>>(static_cast<const TIn*>(x), px, static_cast<T*>(out), f, cpr);
    });
    return check_launch("scan_rows_kernel");
  }
  ColArgs a;  // C2: columns
  a.ncols = (uint32_t)(outer * inner / kE);
  a.inner_chunks = (uint32_t)(inner / kE);
  a.len = (uint32_t)len;
  a.seg_rows = (uint32_t)len;
  a.segments = 1;
  a.by_ncols = make_fastdiv(a.ncols);
  a.by_inner_chunks = make_fastdiv(a.inner_chunks);
  const unsigned grid = blocks_for(a.ncols, kBlock);
  dispatch_input(dt, x_dt, x_scale != nullptr, [&](auto t, auto tin, auto deq) {
    using T = typename decltype(t)::type;
    using TIn = typename decltype(tin)::type;
    scan_cols_kernel<T, TIn, decltype(deq)::value><<<grid, kBlock, 0, s>>>(static_cast<const TIn*>(x), px, a, static_cast<T*>(out), f);
  });
  return check_launch("scan_cols_kernel");
}
