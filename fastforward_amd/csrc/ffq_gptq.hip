// ffq_gptq.hip — the inner loop of GPTQ for one block of columns.
//
// Reference: gptq(), src/fastforward/quantization/gptq.py:101-136 — for each of the (up to 128) columns of a block:
//   q_j   = dequantize(quantize(w_j))                       (column_quantizer, :149-235: one scale/offset per ROW)
//   e_j   = (w_j - q_j) / Hinv[j, j]
//   w_k  -= e_j * Hinv[j, k]   for the block's remaining columns k > j
// run as ~5 eager launches per column (640 per block, 20 k per 4096-column weight) on [rows] vectors. Rows are
// independent, so one lane owns one row: its block of weights lives in registers (the column loop is fully
// unrolled), the Hinv block lives in LDS and every read of it is a wave-wide broadcast. Each arithmetic step is the
// fp32 operation the eager chain performs (the [rows,1] @ [1,n] update is one multiply and one subtract per element).
//
// gptq_block_kernel takes one (scale, offset) per row (PerTensor / PerChannel(0)). gptq_block_grid_kernel takes the parameters
// from the quantizer's [rows / tile_rows, cols / tile_cols] grid (PerBlock, PerTile, PerChannel(1)), optionally through the
// act-order permutation, and gptq_refit_kernel re-estimates the groups that start in the block (reference :91-99) before it.
#include "ffq_common.h"
#include "ffq_extrema.h"
#include "ffq_vec.h"

#include <math.h>

namespace ffq {

constexpr int kGptqBlock = 128;

struct GptqArgs {
  float* weights;            // [rows, row_stride], the block starts at column col0; updated columns are NOT written back
  float* quantized;          // [rows, row_stride] out: columns col0 .. col0 + bs
  float* errors;             // [rows, row_stride] out: columns col0 .. col0 + bs
  const float* hinv;         // [n, n] upper Cholesky factor of the inverse Hessian; the block is hinv[col0:, col0:]
  const float* scale;        // [rows] or [1]
  const float* offset;       // nullable, [rows] or [1]
  int rows, bs, col0;
  int64_t row_stride, hinv_stride;
  int scale_stride, offset_stride;
  float lo, hi;
};

__global__ __launch_bounds__(kBlock) void gptq_block_kernel(GptqArgs a) {
  __shared__ float h[kGptqBlock * kGptqBlock];  // 64 KiB: row j holds Hinv[col0 + j, col0 + (0..127)]
  for (int idx = threadIdx.x; idx < a.bs * kGptqBlock; idx += kBlock) {
    const int j = idx / kGptqBlock, k = idx - j * kGptqBlock;
    h[idx] = k < a.bs ? a.hinv[(size_t)(a.col0 + j) * a.hinv_stride + a.col0 + k] : 0.0f;
  }
  __syncthreads();
  const int row = blockIdx.x * kBlock + threadIdx.x;
  if (row >= a.rows) return;
  float* wrow = a.weights + (size_t)row * a.row_stride + a.col0;
  float w[kGptqBlock];
#pragma unroll
  for (int k = 0; k < kGptqBlock; ++k) w[k] = k < a.bs ? wrow[k] : 0.0f;
  const float s = a.scale[row * a.scale_stride];
  const float o = a.offset ? rne(a.offset[row * a.offset_stride]) : 0.0f;
  float* qrow = a.quantized + (size_t)row * a.row_stride + a.col0;
  float* erow = a.errors + (size_t)row * a.row_stride + a.col0;
#pragma unroll
  for (int j = 0; j < kGptqBlock; ++j) {
    if (j < a.bs) {  // block-uniform
      const float x = w[j];
      float q = rne(x / s - o);                    // quantize: _quantizer_impl.py:161-162
      q = clamp_nan(q, a.lo, a.hi);
      const float dq = (q + o) * s;                // dequantize: :186
      const float e = (x - dq) / h[j * kGptqBlock + j];
      qrow[j] = dq;
      erow[j] = e;
#pragma unroll
      for (int k = j + 1; k < kGptqBlock; ++k) w[k] = w[k] - e * h[j * kGptqBlock + k];  // columns >= bs carry zeros
    }
  }
}

// ---- parameters from the grid ------------------------------------------------------------------------------------------------
// Column c of the (permuted) weight uses grid column order[c] / tile_cols, row r grid row r / tile_rows. A lane still owns a row;
// one wave per workgroup so that the parameters of all the block's columns for the workgroup's 64 rows fit in LDS beside Hinv:
// they are staged once, read from the table along its rows (consecutive lanes, consecutive columns of one grid row), and each
// column then reads its (scale, offset) from LDS at a per-column offset, lane-consecutive (no strided gather per column).
constexpr int kGridRows = 64;
constexpr int kParamPitch = kGridRows + 1;  // pitch of the staged tables: the staging stores (consecutive j) hit distinct banks

struct GptqGridArgs {
  float* weights;            // [rows, cols], the block starts at column col0; read only
  float* quantized;          // [rows, cols] out: columns col0 .. col0 + bs
  float* errors;             // [rows, cols] out: columns col0 .. col0 + bs
  const float* hinv;         // [n, hinv_stride] upper Cholesky factor of the inverse Hessian
  const float* scale;        // [rows / tile_rows, col_groups]
  const float* offset;       // nullable, same shape
  const int64_t* order;      // nullable (identity): column c of `weights` is column order[c] of the parameters' weight
  int rows, cols, bs, col0, tile_rows, tile_cols, col_groups;
  int64_t hinv_stride;
  float lo, hi;
};

__global__ __launch_bounds__(kGridRows) void gptq_block_grid_kernel(GptqGridArgs a) {
  __shared__ float h[kGptqBlock * kGptqBlock];     // 64 KiB, as in gptq_block_kernel
  __shared__ float ps[kGptqBlock * kParamPitch];   // ps[j * kParamPitch + i]: scale of column j for the workgroup's i-th grid row
  __shared__ float po[kGptqBlock * kParamPitch];   // rne(offset), 0 without one
  __shared__ int group_of[kGptqBlock];
  const int lane = threadIdx.x;
  const int r0 = blockIdx.x * kGridRows;
  const int rg0 = r0 / a.tile_rows;
  const int nrg = (min(r0 + kGridRows, a.rows) - 1) / a.tile_rows - rg0 + 1;  // <= kGridRows
  for (int j = lane; j < a.bs; j += kGridRows) {
    int64_t c = a.order ? a.order[a.col0 + j] : (int64_t)(a.col0 + j);
    c = c < 0 ? 0 : (c >= a.cols ? a.cols - 1 : c);  // a malformed permutation reads wrong parameters, never outside the table
    group_of[j] = (int)(c / a.tile_cols);
  }
#pragma unroll 8
  for (int j = 0; j < a.bs; ++j) {
    const float* src = a.hinv + (size_t)(a.col0 + j) * a.hinv_stride + a.col0;
    h[j * kGptqBlock + lane] = lane < a.bs ? src[lane] : 0.0f;
    h[j * kGptqBlock + kGridRows + lane] = kGridRows + lane < a.bs ? src[kGridRows + lane] : 0.0f;
  }
  __syncthreads();
  for (int idx = lane; idx < nrg * a.bs; idx += kGridRows) {
    const int i = idx / a.bs, j = idx - i * a.bs;
    const size_t p = (size_t)(rg0 + i) * a.col_groups + group_of[j];
    ps[j * kParamPitch + i] = a.scale[p];
    po[j * kParamPitch + i] = a.offset ? rne(a.offset[p]) : 0.0f;
  }
  __syncthreads();
  const int row = r0 + lane;
  if (row >= a.rows) return;
  const int i = row / a.tile_rows - rg0;
  const float* wrow = a.weights + (size_t)row * a.cols + a.col0;
  float w[kGptqBlock];
#pragma unroll
  for (int k = 0; k < kGptqBlock; ++k) w[k] = k < a.bs ? wrow[k] : 0.0f;
  float* qrow = a.quantized + (size_t)row * a.cols + a.col0;
  float* erow = a.errors + (size_t)row * a.cols + a.col0;
#pragma unroll
  for (int j = 0; j < kGptqBlock; ++j) {
    if (j < a.bs) {  // block-uniform
      const float s = ps[j * kParamPitch + i];
      const float o = po[j * kParamPitch + i];
      const float x = w[j];
      float q = rne(x / s - o);                    // the arithmetic of gptq_block_kernel, step for step
      q = clamp_nan(q, a.lo, a.hi);
      const float dq = (q + o) * s;
      const float e = (x - dq) / h[j * kGptqBlock + j];
      qrow[j] = dq;
      erow[j] = e;
#pragma unroll
      for (int k = j + 1; k < kGptqBlock; ++k) w[k] = w[k] - e * h[j * kGptqBlock + k];
    }
  }
}

// ---- group refit: the groups whose first column lies in the block --------------------------------------------------------------
// Reference :91-99 / _ParameterGrid.refit_group: for column group g, min / max over each grid row's tile_rows x tile_cols weights,
// then A5 with ONE one-sided decision for the group (range.py:100 over that group's grid rows), written into the group's column of
// scale / offset. The reference reads the global weights, which within a block still hold their values from the block's start
// (the block's updates go to a clone), so every refit of a block can run before its column loop. blockIdx.x picks the group,
// blockIdx.y a share of its grid rows (kRefitRowsPerBlock at most); teams of kRefitTeam lanes own a grid row at a time and read it
// along its columns. A5 runs per grid row with the group's one decision, never across groups.
constexpr int kRefitBlock = 1024;
constexpr int kRefitTeam = 16;
constexpr int kRefitRowsPerBlock = 4 * (kRefitBlock / kRefitTeam);  // grid rows per workgroup

struct GptqRefitArgs {
  const float* weights;      // [rows, cols]
  float* scale;              // [row_groups, col_groups]
  float* offset;             // nullable, same shape
  int cols, tile_rows, tile_cols, row_groups, col_groups, first_group;
  RangeArgs range;
};

// this lane's share of grid row `rg` of group `g`: running min / max (NaN excluded) and whether a NaN was seen
__device__ __forceinline__ void refit_tile_share(const GptqRefitArgs& a, int rg, int g, int member, float& mn, float& mx, int& nan) {
  const float* base = a.weights + (size_t)rg * a.tile_rows * a.cols + (size_t)g * a.tile_cols;
  for (int r = 0; r < a.tile_rows; ++r) {
    const float* src = base + (size_t)r * a.cols;
    for (int c = member; c < a.tile_cols; c += kRefitTeam) {
      const float v = src[c];
      mn = __builtin_fminf(mn, v);
      mx = __builtin_fmaxf(mx, v);
      nan |= v != v;
    }
  }
}

__global__ __launch_bounds__(kRefitBlock) void gptq_refit_kernel(GptqRefitArgs a) {
  __shared__ int negative_s;
  const int g = a.first_group + blockIdx.x;
  const int team = threadIdx.x / kRefitTeam, member = threadIdx.x % kRefitTeam;
  constexpr int kTeams = kRefitBlock / kRefitTeam;
  int one_sided = 0;
  if (a.range.symmetric && a.range.allow_one_sided) {
    // min over ALL the group's grid-row minima >= 0 (NaN >= 0 is False)   (:100). Every workgroup of the group takes the same
    // decision from the same data; the scan stops at the first negative / NaN tile, i.e. at once for weights of both signs.
    if (threadIdx.x == 0) negative_s = 0;
    __syncthreads();
    int negative = 0;
    for (int base = 0; base < a.row_groups && !negative; base += kTeams) {
      const int rg = base + team;
      if (rg < a.row_groups) {
        float mn = INFINITY, mx = -INFINITY;
        int nan = 0;
        refit_tile_share(a, rg, g, member, mn, mx, nan);
        if (nan || mn < 0.0f) negative_s = 1;
      }
      __syncthreads();
      negative = negative_s;
      __syncthreads();  // (negative_s only ever goes 0 -> 1: no lane may see a later store before every lane has read it)
    }
    one_sided = !negative;
  }
  for (int rg = blockIdx.y * kTeams + team; rg < a.row_groups; rg += gridDim.y * kTeams) {
    float mn = INFINITY, mx = -INFINITY;
    int nan = 0;
    refit_tile_share(a, rg, g, member, mn, mx, nan);
#pragma unroll
    for (int d = kRefitTeam / 2; d >= 1; d >>= 1) {  // within the team (16-lane segments of the wave)
      mn = __builtin_fminf(mn, __shfl_xor(mn, d, kRefitTeam));
      mx = __builtin_fmaxf(mx, __shfl_xor(mx, d, kRefitTeam));
      nan |= __shfl_xor(nan, d, kRefitTeam);
    }
    if (member == 0) {  // torch.min / torch.max propagate NaN
      float scale, offset;
      range_to_parameters(nan ? NAN : mn, nan ? NAN : mx, one_sided, a.range, scale, offset);
      const size_t p = (size_t)rg * a.col_groups + g;
      a.scale[p] = scale;
      if (a.offset) a.offset[p] = offset;  // two-sided symmetric: 0, as update_partial_range writes
    }
  }
}

}  // namespace ffq

using namespace ffq;

extern "C" int ffq_gptq_block(float* weights, float* quantized, float* errors, int64_t rows, int64_t row_stride,
                              int64_t col0, int64_t block_cols, const float* hinv, int64_t hinv_stride, const float* scale,
                              int64_t scale_numel, const float* offset, int64_t offset_numel, double num_bits, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (rows < 0 || block_cols < 0 || col0 < 0) return fail(FFQ_ERR_ARG, "negative extent");
  if (block_cols > kGptqBlock) return fail(FFQ_ERR_DTYPE, "GPTQ block kernel handles at most %d columns per block", kGptqBlock);
  if (rows == 0 || block_cols == 0) return FFQ_OK;
  if (!weights || !quantized || !errors || !hinv || !scale) return fail(FFQ_ERR_ARG, "NULL buffer");
  if ((scale_numel != 1 && scale_numel != rows) || (offset && offset_numel != 1 && offset_numel != rows))
    return fail(FFQ_ERR_PARAM_NUMEL, "GPTQ block kernel takes one scale / offset per row (or one in total)");
  if (rows >= ((int64_t)1 << 31) || col0 + block_cols > row_stride || col0 + block_cols > hinv_stride) return fail(FFQ_ERR_ARG, "block outside the matrix");
  GptqArgs a;
  a.weights = weights; a.quantized = quantized; a.errors = errors; a.hinv = hinv; a.scale = scale; a.offset = offset;
  a.rows = (int)rows; a.bs = (int)block_cols; a.col0 = (int)col0;
  a.row_stride = row_stride; a.hinv_stride = hinv_stride;
  a.scale_stride = scale_numel == 1 ? 0 : 1;
  a.offset_stride = offset_numel == 1 ? 0 : 1;
  const double lo = -pow(2.0, num_bits - 1.0);
  a.lo = (float)lo; a.hi = (float)(-lo - 1.0);
  gptq_block_kernel<<<(unsigned)((rows + kBlock - 1) / kBlock), kBlock, 0, s>>>(a);
  return check_launch("gptq_block_kernel");
}

extern "C" int ffq_gptq_block_grid(float* weights, float* quantized, float* errors, int64_t rows, int64_t cols, int64_t col0,
                                   int64_t block_cols, const float* hinv, int64_t hinv_stride, float* scale, float* offset,
                                   int64_t tile_rows, int64_t tile_cols, const int64_t* column_order, int refit, int symmetric,
                                   int allow_one_sided, double num_bits, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (rows < 0 || cols < 0 || col0 < 0 || block_cols < 0 || tile_rows < 0 || tile_cols < 0) return fail(FFQ_ERR_ARG, "negative extent");
  if (block_cols > kGptqBlock) return fail(FFQ_ERR_DTYPE, "GPTQ block kernel handles at most %d columns per block", kGptqBlock);
  if (rows == 0 || block_cols == 0) return FFQ_OK;
  if (!weights || !quantized || !errors || !hinv || !scale) return fail(FFQ_ERR_ARG, "NULL buffer");
  if (tile_rows == 0 || tile_cols == 0 || rows % tile_rows != 0 || cols % tile_cols != 0)
    return fail(FFQ_ERR_TILE_DIVIDE, "GPTQ parameter tile (%lld, %lld) must divide the weight (%lld, %lld)", (long long)tile_rows,
                (long long)tile_cols, (long long)rows, (long long)cols);
  if (rows >= ((int64_t)1 << 31) || cols >= ((int64_t)1 << 31) || col0 + block_cols > cols || col0 + block_cols > hinv_stride)
    return fail(FFQ_ERR_ARG, "block outside the matrix");
  if (refit) {
    const int64_t first = (col0 + tile_cols - 1) / tile_cols, last = (col0 + block_cols - 1) / tile_cols;  // groups starting in the block
    if (last >= first) {
      GptqRefitArgs r;
      r.weights = weights; r.scale = scale; r.offset = offset;
      r.cols = (int)cols; r.tile_rows = (int)tile_rows; r.tile_cols = (int)tile_cols;
      r.row_groups = (int)(rows / tile_rows); r.col_groups = (int)(cols / tile_cols); r.first_group = (int)first;
      r.range = make_range_args(FFQ_F32, rows / tile_rows, num_bits, symmetric, allow_one_sided, FFQ_F32, FFQ_F32, 0);
      int64_t split = (r.row_groups + kRefitRowsPerBlock - 1) / kRefitRowsPerBlock;
      if (split > 65535) split = 65535;  // (the kernel strides over whatever is left)
      gptq_refit_kernel<<<dim3((unsigned)(last - first + 1), (unsigned)split), kRefitBlock, 0, s>>>(r);
      const int st = check_launch("gptq_refit_kernel");
      if (st != FFQ_OK) return st;
    }
  }
  GptqGridArgs a;
  a.weights = weights; a.quantized = quantized; a.errors = errors; a.hinv = hinv; a.scale = scale; a.offset = offset;
  a.order = column_order;
  a.rows = (int)rows; a.cols = (int)cols; a.bs = (int)block_cols; a.col0 = (int)col0;
  a.tile_rows = (int)tile_rows; a.tile_cols = (int)tile_cols; a.col_groups = (int)(cols / tile_cols);
  a.hinv_stride = hinv_stride;
  const double lo = -pow(2.0, num_bits - 1.0);
  a.lo = (float)lo; a.hi = (float)(-lo - 1.0);
  gptq_block_grid_kernel<<<(unsigned)((rows + kGridRows - 1) / kGridRows), kGridRows, 0, s>>>(a);
  return check_launch("gptq_block_grid_kernel");
}
