// ffq_mx.hip — OCP microscaling formats (include_mx/ffq_mx.h): the MXFP8 / MXFP4 quantizer, its inverse, and a linear on CDNA4's
// block-scaled matrix-core instruction. The reference project has no float-element quantizer: the rule is the OCP MX one as stated in
// the header and docs/numerics.md, and its torch restatement (fastforward_amd/_host.py, mx_quantize / mx_dequantize) decides bit for bit.
//
// Three kernels, each a single launch without workspace:
//   mx_quantize_kernel    one pass: 16 elements per lane, the block's |x| maximum as an integer maximum of the fp32 bit patterns (NaN and
//                         Inf sort above every finite value) across the two lanes of a block by one shuffle; bit arithmetic, no LDS;
//   mx_dequantize_kernel  value(code) * 2^(scale - 127), 16 elements per lane;
//   mx_gemm_kernel        128 x 128 x 128 tiles on v_mfma_scale_f32_32x32x64_f8f6f4, codes global -> LDS by global_load_lds dwordx4 into
//                         two stages, swizzled through the source address.
// Every store is an ordinary vector store from plain C++.
#include "ffq_common.h"
#include "ffq_quantizer_host.h"
#include "ffq_vec.h"

#include "../../include_mx/ffq_mx.h"

namespace ffq {

// ---- the formats ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int mx_emax(int format) { return format == FFQ_MX_E4M3 ? 8 : 2; }

// |y| <= 448 (already clamped), not NaN -> the 7 magnitude bits of e4m3fn, round to nearest even
__device__ __forceinline__ uint32_t e4m3_magnitude(float ay) {
  if (ay < 0.015625f) return (uint32_t)(int)rne(ay * 512.0f);  // below 2^-6: multiples of 2^-9 (8 is the smallest normal's code)
  uint32_t u = __builtin_bit_cast(uint32_t, ay);
  u += 0x7FFFFu + ((u >> 20) & 1u);
  return (u >> 20) - (120u << 3);
}

// |y| <= 6, not NaN -> the 3 magnitude bits of e2m1: the midpoints go to the even code
__device__ __forceinline__ uint32_t e2m1_magnitude(float ay) {
  return (uint32_t)(ay > 0.25f) + (uint32_t)(ay >= 0.75f) + (uint32_t)(ay > 1.25f) + (uint32_t)(ay >= 1.75f) + (uint32_t)(ay > 2.5f) +
         (uint32_t)(ay >= 3.5f) + (uint32_t)(ay > 5.0f);
}

__device__ __forceinline__ uint32_t mx_encode(float x, float mult, int format) {
  const float y = x * mult;  // (exact unless it lands below the fp32 normals, far under half the smallest grid step)
  const uint32_t sign = __builtin_bit_cast(uint32_t, y) >> 31;
  const float ay = __builtin_fabsf(y);
  if (format == FFQ_MX_E4M3) return (sign << 7) | e4m3_magnitude(__builtin_fminf(ay, 448.0f));
  return (sign << 3) | e2m1_magnitude(__builtin_fminf(ay, 6.0f));
}

__device__ __forceinline__ float mx_decode(uint32_t code, int format) {
  float v;
  uint32_t sign;
  if (format == FFQ_MX_E4M3) {
    const uint32_t mag = code & 0x7Fu;
    sign = (code >> 7) & 1u;
    if (mag == 0x7Fu) v = __builtin_bit_cast(float, 0x7FC00000u);
    else if (mag < 8u) v = (float)mag * 0.001953125f;
    else v = __builtin_bit_cast(float, (mag << 20) + (120u << 23));
  } else {
    const uint32_t mag = code & 7u;
    sign = (code >> 3) & 1u;
    v = mag < 2u ? (float)mag * 0.5f : __builtin_bit_cast(float, (((mag >> 1) + 126u) << 23) | ((mag & 1u) << 22));
  }
  return __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, v) | (sign << 31));
}

// 2^(scale - 127) as fp32: subnormal for 0, NaN for 255
__device__ __forceinline__ float mx_scale_value(uint32_t scale) {
  return __builtin_bit_cast(float, scale == 0u ? 0x00400000u : scale == 255u ? 0x7FC00000u : scale << 23);
}

// ---- quantize -------------------------------------------------------------------------------------------------------------------------
struct MxQuantArgs {
  int64_t x_stride;  // elements
  uint32_t items;    // rows * K / 16
  uint32_t K;
  FastDiv items_per_row;  // K / 16
  int format;
};

// An item is 16 consecutive elements of a row: half a block. FAST: 16-byte loads, one 16-byte store of codes, one 8-byte store of packed
// codes; otherwise one element at a time through the same arithmetic.
template <typename T, bool FAST>
__global__ __launch_bounds__(kBlock) void mx_quantize_kernel(const T* __restrict__ x, uint8_t* __restrict__ codes, uint8_t* __restrict__ packed,
                                                             uint8_t* __restrict__ scales, MxQuantArgs a) {
  const uint32_t stride = gridDim.x * (uint32_t)kBlock;
  const uint32_t rounds = (a.items + stride - 1) / stride;
  uint32_t item = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  // every lane of a wave takes every round (the shuffle needs its partner; items is even, so a pair is live or dead together)
  for (uint32_t it = 0; it < rounds; ++it, item += stride) {
    const bool live = item < a.items;
    const uint32_t row = live ? fdiv(item, a.items_per_row) : 0u;
    const uint32_t col = live ? (item - row * a.items_per_row.div) * 16u : 0u;
    const T* src = x + (size_t)row * (size_t)a.x_stride + col;
    float v[16];
    if (live) {
      if constexpr (FAST) {
        constexpr int E = 16 / (int)sizeof(T);
#pragma unroll
        for (int c = 0; c < 16 / E; ++c) {
          Chunk<T, E> in;
          in.load(src + c * E);
#pragma unroll
          for (int i = 0; i < E; ++i) v[c * E + i] = in.get(i);
        }
      } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] = to_f32(src[i]);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i) v[i] = 0.0f;
    }
    uint32_t top = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const uint32_t u = __builtin_bit_cast(uint32_t, v[i]) & 0x7FFFFFFFu;
      top = u > top ? u : top;
    }
    const uint32_t other = (uint32_t)__shfl_xor((int)top, 1, 64);
    top = other > top ? other : top;
    if (!live) continue;
    const int e = (int)(top >> 23);
    const bool poisoned = e == 255;  // a NaN or an Inf in the block
    const int biased = e - mx_emax(a.format);
    const uint32_t scale = poisoned ? 255u : (uint32_t)(biased > 0 ? biased : 0);
    const float mult = __builtin_bit_cast(float, (254u - (poisoned ? 127u : scale)) << 23);  // 2^(127 - scale)
    uint32_t c[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) c[i] = poisoned ? 0u : mx_encode(v[i], mult, a.format);
    const size_t base = (size_t)row * a.K + col;
    if ((col & 31u) == 0u) scales[((size_t)row * a.K + col) >> 5] = (uint8_t)scale;
    if constexpr (FAST) {
      if (codes) {
        u32x4 w;
        w.x = c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24);
        w.y = c[4] | (c[5] << 8) | (c[6] << 16) | (c[7] << 24);
        w.z = c[8] | (c[9] << 8) | (c[10] << 16) | (c[11] << 24);
        w.w = c[12] | (c[13] << 8) | (c[14] << 16) | (c[15] << 24);
        *reinterpret_cast<u32x4*>(codes + base) = w;
      }
      if (packed) {
        u32x2 w;
        w.x = c[0] | (c[1] << 4) | (c[2] << 8) | (c[3] << 12) | (c[4] << 16) | (c[5] << 20) | (c[6] << 24) | (c[7] << 28);
        w.y = c[8] | (c[9] << 4) | (c[10] << 8) | (c[11] << 12) | (c[12] << 16) | (c[13] << 20) | (c[14] << 24) | (c[15] << 28);
        *reinterpret_cast<u32x2*>(packed + (base >> 1)) = w;
      }
    } else {
      if (codes)
#pragma unroll
        for (int i = 0; i < 16; ++i) codes[base + i] = (uint8_t)c[i];
      if (packed)
#pragma unroll
        for (int i = 0; i < 8; ++i) packed[(base >> 1) + i] = (uint8_t)(c[2 * i] | (c[2 * i + 1] << 4));
    }
  }
}

// ---- dequantize -----------------------------------------------------------------------------------------------------------------------
template <typename T, bool FAST>
__global__ __launch_bounds__(kBlock) void mx_dequantize_kernel(const uint8_t* __restrict__ codes, const uint8_t* __restrict__ scales, T* __restrict__ out,
                                                               uint32_t items, int format, int is_packed) {
  const uint32_t stride = gridDim.x * (uint32_t)kBlock;
  for (uint32_t item = blockIdx.x * (uint32_t)kBlock + threadIdx.x; item < items; item += stride) {
    const size_t base = (size_t)item * 16;  // the tensors are dense and K % 32 == 0: the flat block index is base / 32
    const float s = mx_scale_value(scales[base >> 5]);
    uint32_t c[16];
    if constexpr (FAST) {
      if (is_packed) {
        const u32x2 w = *reinterpret_cast<const u32x2*>(codes + (base >> 1));
#pragma unroll
        for (int i = 0; i < 8; ++i) { c[i] = (w.x >> (4 * i)) & 15u; c[8 + i] = (w.y >> (4 * i)) & 15u; }
      } else {
        const u32x4 w = *reinterpret_cast<const u32x4*>(codes + base);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          c[i] = (w.x >> (8 * i)) & 255u; c[4 + i] = (w.y >> (8 * i)) & 255u; c[8 + i] = (w.z >> (8 * i)) & 255u; c[12 + i] = (w.w >> (8 * i)) & 255u;
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i) c[i] = is_packed ? (codes[(base + i) >> 1] >> (4 * (i & 1))) & 15u : codes[base + i];
    }
    T* dst = out + base;
    if constexpr (FAST) {
      constexpr int E = 16 / (int)sizeof(T);
#pragma unroll
      for (int ch = 0; ch < 16 / E; ++ch) {
        float v[E];
#pragma unroll
        for (int i = 0; i < E; ++i) v[i] = mx_decode(c[ch * E + i], format) * s;
        Chunk<T, E> y;
        y.pack(v);
        y.store(dst + ch * E);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i) dst[i] = from_f32<T>(mx_decode(c[i], format) * s);
    }
  }
}

// ---- the GEMM -------------------------------------------------------------------------------------------------------------------------
// The operand map of v_mfma_scale_f32_32x32x64_f8f6f4 (established on the device with exact data: tools/probes/mx_map_probe.hip):
//   lane l, r = l & 31, h = l >> 5 holds row r of A (and of W) of the instruction's 64-deep slice:
//     e2m1  k = 32h .. 32h + 31 in its first four registers, element j at bits [4j, 4j + 4): the packed bytes at rest, unpermuted;
//     e4m3  k = 16h .. 16h + 15 in registers 0-3 and k = 32 + 16h .. 32 + 16h + 15 in registers 4-7, a byte each in memory order: the
//           two halves of a row interleave in 16-byte pieces (NOT 32 consecutive bytes per lane: that form computes other sums);
//   the byte `opsel` of the scale register of lane (r, h) is the E8M0 scale of block h (k = 32h .. 32h + 31) of row r, in both formats —
//   for e4m3 that is not the lane's own data, which spans both blocks;
//   C/D: column (the W row) = l & 31, row (the A row) = (reg & 3) + 8 (reg >> 2) + 4 (l >> 5);
//   an A (or W) scale byte of 255 makes every output of that row (column) NaN; the other outputs keep their bits.
typedef int mx_i32x8 __attribute__((ext_vector_type(8)));
typedef float mx_f32x16 __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(3))) void mx_lds_t;
typedef __attribute__((address_space(1))) const void mx_gbl_t;

constexpr int kMxTile = 128;   // output rows and columns of a workgroup
constexpr int kMxStep = 128;   // elements of K per step: two MFMAs per 32 x 32 tile, four scale bytes = one dword per row

struct MxGemmArgs {
  const uint8_t *a_codes, *a_scales, *w_codes, *w_scales;
  int64_t a_stride, a_scale_stride, w_stride, w_scale_stride;  // bytes
  const void* bias;
  int bias_f32;
  void* out;
  int M, N, K;
  int tiles_m;
};

// FMT: the instruction's format field (0 e4m3, 4 e2m1). A tile row is ROWB bytes = SLOTS 16-byte slots; the slot index is XOR-swizzled
// with the row so that the 32 rows a half-wave reads at one k land on distinct banks.
template <int FMT>
struct MxOperand {
  static constexpr int ROWB = FMT == 4 ? kMxStep / 2 : kMxStep;
  static constexpr int SLOTS = ROWB / 16;                       // 4 | 8
  static constexpr int PER_THREAD = kMxTile * SLOTS / 256;      // 2 | 4 LDS-DMA instructions per thread and stage
  static constexpr int BYTES = kMxTile * ROWB;                  // 8 | 16 KiB per stage
  static constexpr int FRAG = FMT == 4 ? 1 : 2;                 // 16-byte slots of a lane's 32 elements
  // the g-th 16-byte slot of the fragment of lane half h for the kk-th instruction of a step (the operand map below)
  __device__ static __forceinline__ uint32_t frag_slot(uint32_t kk, uint32_t h, uint32_t g) { return FMT == 4 ? 2 * kk + h : 4 * kk + 2 * g + h; }
  __device__ static __forceinline__ uint32_t swz(uint32_t row) { return FMT == 4 ? (row >> 1) & 3u : row & 7u; }
  __device__ static __forceinline__ uint32_t offset(uint32_t row, uint32_t slot) { return row * ROWB + ((slot ^ swz(row)) << 4); }
};

template <int FA, int FB, typename TOut>
__global__ __launch_bounds__(256) void mx_gemm_kernel(MxGemmArgs a) {
  using OA = MxOperand<FA>;
  using OB = MxOperand<FB>;
  __shared__ __attribute__((aligned(16))) uint8_t lds_a[2][OA::BYTES];
  __shared__ __attribute__((aligned(16))) uint8_t lds_b[2][OB::BYTES];

  // XCD-aware tile order (as the int8 GEMM): blocks b, b + 8, ... share an XCD; each XCD gets a contiguous range of tiles
  const uint32_t nblk = gridDim.x;
  const uint32_t xcd = blockIdx.x & 7u, slot_in_xcd = blockIdx.x >> 3;
  const uint32_t q = nblk >> 3, r8 = nblk & 7u;
  const uint32_t tile_id = (xcd < r8 ? xcd * (q + 1) : r8 * (q + 1) + (xcd - r8) * q) + slot_in_xcd;
  const int tn = (int)(tile_id / (uint32_t)a.tiles_m), tm = (int)(tile_id % (uint32_t)a.tiles_m);
  const int m0 = tm * kMxTile, n0 = tn * kMxTile;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 31, fh = lane >> 5;

  mx_f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;

  // the rows whose scales this lane feeds to the instruction; a row beyond the matrix reads the last row's (its
  // outputs are never stored)
  const uint8_t* sa_row[2];
  const uint8_t* sb_row[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int ra = m0 + wm * 64 + i * 32 + fr, rb = n0 + wn * 64 + i * 32 + fr;
    sa_row[i] = a.a_scales + (int64_t)(ra < a.M ? ra : a.M - 1) * a.a_scale_stride;
    sb_row[i] = a.w_scales + (int64_t)(rb < a.N ? rb : a.N - 1) * a.w_scale_stride;
  }

  // Staging: global -> LDS with global_load_lds dwordx4, no register in between. One wave-instruction writes 64 consecutive 16-byte
  // slots of the image (wave-uniform base + lane * 16), so lane i of the p-th instruction of wave w owns PHYSICAL slot p * 256 + tid of
  // the stage; the swizzle goes on the SOURCE: that slot holds logical slot (physical ^ swz(row)) of its row. A row beyond the matrix
  // reads the last row's bytes (in bounds; its outputs are never stored, and rows do not mix inside the instruction).
  const uint8_t* src_a[OA::PER_THREAD];
  const uint8_t* src_b[OB::PER_THREAD];
#pragma unroll
  for (int p = 0; p < OA::PER_THREAD; ++p) {
    const uint32_t s = tid + p * 256, row = s / OA::SLOTS, logical = (s % OA::SLOTS) ^ OA::swz(row);
    const int gr = m0 + (int)row < a.M ? m0 + (int)row : a.M - 1;
    src_a[p] = a.a_codes + (int64_t)gr * a.a_stride + logical * 16;
  }
#pragma unroll
  for (int p = 0; p < OB::PER_THREAD; ++p) {
    const uint32_t s = tid + p * 256, row = s / OB::SLOTS, logical = (s % OB::SLOTS) ^ OB::swz(row);
    const int gr = n0 + (int)row < a.N ? n0 + (int)row : a.N - 1;
    src_b[p] = a.w_codes + (int64_t)gr * a.w_stride + logical * 16;
  }
  uint32_t sa_next[2], sb_next[2];
  auto fetch_scales = [&](int kt) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      sa_next[i] = *reinterpret_cast<const uint32_t*>(sa_row[i] + (int64_t)kt * 4);
      sb_next[i] = *reinterpret_cast<const uint32_t*>(sb_row[i] + (int64_t)kt * 4);
    }
  };
  auto stage_codes = [&](int kt, int stage) {
#pragma unroll
    for (int p = 0; p < OA::PER_THREAD; ++p)
      __builtin_amdgcn_global_load_lds((mx_gbl_t*)(src_a[p] + (int64_t)kt * OA::ROWB), (mx_lds_t*)(&lds_a[stage][(p * 256 + wave * 64) * 16]), 16, 0, 0);
#pragma unroll
    for (int p = 0; p < OB::PER_THREAD; ++p)
      __builtin_amdgcn_global_load_lds((mx_gbl_t*)(src_b[p] + (int64_t)kt * OB::ROWB), (mx_lds_t*)(&lds_b[stage][(p * 256 + wave * 64) * 16]), 16, 0, 0);
  };
  // a lane's 32 elements of MFMA kk of the step
  auto frag_a = [&](int stage, int row, int kk) {
    mx_i32x8 f = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int g = 0; g < OA::FRAG; ++g) {
      const u32x4 w = *reinterpret_cast<const u32x4*>(&lds_a[stage][OA::offset(row, OA::frag_slot(kk, fh, g))]);
      f[4 * g + 0] = (int)w.x; f[4 * g + 1] = (int)w.y; f[4 * g + 2] = (int)w.z; f[4 * g + 3] = (int)w.w;
    }
    return f;
  };
  auto frag_b = [&](int stage, int row, int kk) {
    mx_i32x8 f = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int g = 0; g < OB::FRAG; ++g) {
      const u32x4 w = *reinterpret_cast<const u32x4*>(&lds_b[stage][OB::offset(row, OB::frag_slot(kk, fh, g))]);
      f[4 * g + 0] = (int)w.x; f[4 * g + 1] = (int)w.y; f[4 * g + 2] = (int)w.z; f[4 * g + 3] = (int)w.w;
    }
    return f;
  };

  const int ksteps = a.K / kMxStep;
  fetch_scales(0);
  stage_codes(0, 0);
  __syncthreads();  // (waits for the LDS-DMA of this wave, then for every wave's)
  for (int kt = 0; kt < ksteps; ++kt) {
    const int cur = kt & 1;
    // the step's four scale bytes of a row: blocks 0 .. 3. The lanes of the upper half supply blocks 1 and 3 of their row, so they shift
    // by one byte and byte 0 / byte 2 (opsel 0 / 2) is the right one on both halves for the step's first / second MFMA
    int sa[2], sb[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      sa[i] = (int)(sa_next[i] >> (8 * fh));
      sb[i] = (int)(sb_next[i] >> (8 * fh));
    }
    if (kt + 1 < ksteps) {  // the next step's codes fly into the other stage, whose readers passed the barrier below, under the MFMAs
      stage_codes(kt + 1, cur ^ 1);
      fetch_scales(kt + 1);
    }
    {
      mx_i32x8 fa[2], fb[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) fa[i] = frag_a(cur, wm * 64 + i * 32 + fr, 0);
#pragma unroll
      for (int j = 0; j < 2; ++j) fb[j] = frag_b(cur, wn * 64 + j * 32 + fr, 0);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fa[i], fb[j], acc[i][j], FA, FB, 0, sa[i], 0, sb[j]);
    }
    {
      mx_i32x8 fa[2], fb[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) fa[i] = frag_a(cur, wm * 64 + i * 32 + fr, 1);
#pragma unroll
      for (int j = 0; j < 2; ++j) fb[j] = frag_b(cur, wn * 64 + j * 32 + fr, 1);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fa[i], fb[j], acc[i][j], FA, FB, 2, sa[i], 2, sb[j]);
    }
    __syncthreads();
  }

  TOut* out = static_cast<TOut*>(a.out);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = n0 + wn * 64 + j * 32 + fr;
    if (n >= a.N) continue;
    float b = 0.0f;
    if (a.bias) b = a.bias_f32 ? static_cast<const float*>(a.bias)[n] : to_f32(static_cast<const TOut*>(a.bias)[n]);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int m = m0 + wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * fh;
        if (m < a.M) out[(int64_t)m * a.N + n] = from_f32<TOut>(acc[i][j][e] + b);
      }
    }
  }
}

// ---- host: each rule once ---------------------------------------------------------------------------------------------------------------
static bool mx_format_ok(int f) { return f == FFQ_MX_E4M3 || f == FFQ_MX_E2M1; }
static bool mx_aligned(const void* p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }
static bool mx_extent_ok(int64_t v) { return v >= 0 && v < ((int64_t)1 << 31); }
static int64_t mx_code_row_bytes(int64_t K, int format) { return format == FFQ_MX_E2M1 ? K / 2 : K; }

// rows, K of the quantizer and its inverse, in the order they share
static int mx_check_matrix(const char* who, int64_t rows, int64_t K) {
  if (rows < 0 || K < 0 || (rows > 0 && K > (((int64_t)1 << 35) - 1) / rows))
    return fail(FFQ_ERR_ARG, "%s: bad extent (rows %lld, K %lld; rows * K < 2^35)", who, (long long)rows, (long long)K);
  if (K % FFQ_MX_BLOCK) return fail(FFQ_ERR_ARG, "%s: K %% 32 != 0 (K %lld)", who, (long long)K);
  return FFQ_OK;
}

static unsigned mx_grid(int64_t items) {
  int64_t blocks = (items + kBlock - 1) / kBlock;
  if (blocks > 16384) blocks = 16384;
  return (unsigned)(blocks < 1 ? 1 : blocks);
}

}  // namespace ffq

using namespace ffq;

extern "C" int ffq_mx_quantize(const void* x, int x_dt, int64_t x_stride, int64_t rows, int64_t K, int format, uint8_t* codes, uint8_t* packed,
                               uint8_t* scales, void* stream) {
  static const char* who = "mx_quantize";
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (!is_f32_bf16_f16(x_dt)) return fail(FFQ_ERR_DTYPE, "%s: x holds bf16, fp16 or fp32 values, got dtype %d", who, x_dt);
  if (!mx_format_ok(format)) return fail(FFQ_ERR_ARG, "%s: the element format is FFQ_MX_E4M3 (0) or FFQ_MX_E2M1 (1), got %d", who, format);
  if (int rc = mx_check_matrix(who, rows, K)) return rc;
  if (x_stride < K) return fail(FFQ_ERR_ARG, "%s: the row stride %lld is below the row length %lld", who, (long long)x_stride, (long long)K);
  if (packed && format != FFQ_MX_E2M1) return fail(FFQ_ERR_ARG, "%s: only e2m1 codes have a packed form", who);
  if (rows == 0 || K == 0) return FFQ_OK;
  if (!x || !scales || (!codes && !packed)) return fail(FFQ_ERR_ARG, "%s: NULL buffer (x, scales, or both code outputs)", who);
  if (!mx_aligned(x, (uintptr_t)dt_size(x_dt))) return fail(FFQ_ERR_ARG, "%s: x must be aligned to its element", who);
  MxQuantArgs a;
  a.x_stride = x_stride;
  a.items = (uint32_t)(rows * K / 16);
  a.K = (uint32_t)K;
  a.items_per_row = make_fastdiv((uint32_t)(K / 16));
  a.format = format;
  const bool fast = aligned16(x) && (x_stride * dt_size(x_dt)) % 16 == 0 && mx_aligned(codes, 16) && mx_aligned(packed, 8) && !generic_kernels_forced();
  const unsigned grid = mx_grid(a.items);
  for_dtype<bf16_t, f16_t, float>(x_dt, [&](auto t) {
    using T = typename decltype(t)::type;
    if (fast) mx_quantize_kernel<T, true><<<grid, kBlock, 0, s>>>(static_cast<const T*>(x), codes, packed, scales, a);
    else mx_quantize_kernel<T, false><<<grid, kBlock, 0, s>>>(static_cast<const T*>(x), codes, packed, scales, a);
  });
  return check_launch("mx_quantize_kernel");
}

extern "C" int ffq_mx_dequantize(const uint8_t* codes, int is_packed, const uint8_t* scales, int64_t rows, int64_t K, int format, void* out,
                                 int out_dt, void* stream) {
  static const char* who = "mx_dequantize";
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (!is_f32_bf16_f16(out_dt)) return fail(FFQ_ERR_DTYPE, "%s: the output holds bf16, fp16 or fp32 values, got dtype %d", who, out_dt);
  if (!mx_format_ok(format)) return fail(FFQ_ERR_ARG, "%s: the element format is FFQ_MX_E4M3 (0) or FFQ_MX_E2M1 (1), got %d", who, format);
  if ((is_packed != 0 && is_packed != 1) || (is_packed && format != FFQ_MX_E2M1))
    return fail(FFQ_ERR_ARG, "%s: is_packed is 0 or 1, and 1 only for e2m1 (got %d, format %d)", who, is_packed, format);
  if (int rc = mx_check_matrix(who, rows, K)) return rc;
  if (rows == 0 || K == 0) return FFQ_OK;
  if (!codes || !scales || !out) return fail(FFQ_ERR_ARG, "%s: NULL buffer", who);
  if (!mx_aligned(out, (uintptr_t)dt_size(out_dt))) return fail(FFQ_ERR_ARG, "%s: out must be aligned to its element", who);
  const uint32_t items = (uint32_t)(rows * K / 16);
  const bool fast = aligned16(out) && mx_aligned(codes, is_packed ? 8 : 16) && !generic_kernels_forced();
  const unsigned grid = mx_grid(items);
  for_dtype<bf16_t, f16_t, float>(out_dt, [&](auto t) {
    using T = typename decltype(t)::type;
    if (fast) mx_dequantize_kernel<T, true><<<grid, kBlock, 0, s>>>(codes, scales, static_cast<T*>(out), items, format, is_packed);
    else mx_dequantize_kernel<T, false><<<grid, kBlock, 0, s>>>(codes, scales, static_cast<T*>(out), items, format, is_packed);
  });
  return check_launch("mx_dequantize_kernel");
}

extern "C" int ffq_linear_mx_supported(int64_t M, int64_t N, int64_t K, int a_format, int w_format) {
  if (!mx_format_ok(a_format) || !mx_format_ok(w_format) || (a_format == FFQ_MX_E2M1 && w_format == FFQ_MX_E4M3)) return 0;
  if (M < 1 || N < 1 || K < kMxStep || K % kMxStep) return 0;
  return mx_extent_ok(M) && mx_extent_ok(N) && mx_extent_ok(K) && (M + kMxTile - 1) / kMxTile * ((N + kMxTile - 1) / kMxTile) < ((int64_t)1 << 31);
}

extern "C" int ffq_linear_mx(const uint8_t* a_codes, int64_t a_stride, const uint8_t* a_scales, int64_t a_scale_stride, int a_format,
                             const uint8_t* w_codes, int64_t w_stride, const uint8_t* w_scales, int64_t w_scale_stride, int w_format,
                             const void* bias, int bias_dt, void* out, int out_dt, int64_t M, int64_t N, int64_t K, void* stream) {
  static const char* who = "linear_mx";
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (!mx_format_ok(a_format) || !mx_format_ok(w_format))
    return fail(FFQ_ERR_ARG, "%s: an element format is FFQ_MX_E4M3 (0) or FFQ_MX_E2M1 (1), got A %d, W %d", who, a_format, w_format);
  if (a_format == FFQ_MX_E2M1 && w_format == FFQ_MX_E4M3)
    return fail(FFQ_ERR_ARG, "%s: the pair (A e2m1, W e4m3) is not covered: (e4m3, e4m3), (e4m3, e2m1) and (e2m1, e2m1) are", who);
  if (!is_f32_bf16_f16(out_dt)) return fail(FFQ_ERR_DTYPE, "%s: the output holds fp32, bf16 or fp16 values, got dtype %d", who, out_dt);
  if (bias && bias_dt != FFQ_F32 && bias_dt != out_dt)
    return fail(FFQ_ERR_DTYPE, "%s: the bias is fp32 or of the output's dtype %d, got dtype %d", who, out_dt, bias_dt);
  if (!mx_extent_ok(M) || !mx_extent_ok(N) || !mx_extent_ok(K))
    return fail(FFQ_ERR_ARG, "%s: bad extent (M %lld, N %lld, K %lld)", who, (long long)M, (long long)N, (long long)K);
  if (M == 0 || N == 0) return FFQ_OK;
  if (K == 0 || K % kMxStep) return fail(FFQ_ERR_ARG, "%s: K must be a positive multiple of 128, got %lld", who, (long long)K);
  const int64_t tiles_m = (M + kMxTile - 1) / kMxTile, tiles_n = (N + kMxTile - 1) / kMxTile;
  if (tiles_m * tiles_n >= ((int64_t)1 << 31)) return fail(FFQ_ERR_ARG, "%s: too many output tiles (M %lld, N %lld)", who, (long long)M, (long long)N);
  if (a_stride < mx_code_row_bytes(K, a_format) || w_stride < mx_code_row_bytes(K, w_format) || a_scale_stride < K / 32 || w_scale_stride < K / 32)
    return fail(FFQ_ERR_ARG, "%s: a row stride is below the row's bytes (codes A %lld, W %lld; scales A %lld, W %lld; K %lld)", who, (long long)a_stride,
                (long long)w_stride, (long long)a_scale_stride, (long long)w_scale_stride, (long long)K);
  if (!a_codes || !a_scales || !w_codes || !w_scales || !out) return fail(FFQ_ERR_ARG, "%s: NULL buffer", who);
  if (!aligned16(a_codes) || !aligned16(w_codes) || a_stride % 16 || w_stride % 16)
    return fail(FFQ_ERR_ARG, "%s: code pointers and code row strides must be 16-byte aligned", who);
  if (!mx_aligned(a_scales, 4) || !mx_aligned(w_scales, 4) || a_scale_stride % 4 || w_scale_stride % 4)
    return fail(FFQ_ERR_ARG, "%s: scale pointers and scale row strides must be 4-byte aligned", who);
  if (!mx_aligned(out, (uintptr_t)dt_size(out_dt)) || (bias && !mx_aligned(bias, (uintptr_t)dt_size(bias_dt))))
    return fail(FFQ_ERR_ARG, "%s: out and bias must be aligned to their elements", who);
  MxGemmArgs a;
  a.a_codes = a_codes; a.a_scales = a_scales; a.w_codes = w_codes; a.w_scales = w_scales;
  a.a_stride = a_stride; a.a_scale_stride = a_scale_stride; a.w_stride = w_stride; a.w_scale_stride = w_scale_stride;
  a.bias = bias; a.bias_f32 = bias_dt == FFQ_F32;
  a.out = out;
  a.M = (int)M; a.N = (int)N; a.K = (int)K;
  a.tiles_m = (int)tiles_m;
  const unsigned grid = (unsigned)(tiles_m * tiles_n);
  for_dtype<float, bf16_t, f16_t>(out_dt, [&](auto t) {
    using T = typename decltype(t)::type;
    if (a_format == FFQ_MX_E4M3 && w_format == FFQ_MX_E4M3) mx_gemm_kernel<0, 0, T><<<grid, 256, 0, s>>>(a);
    else if (a_format == FFQ_MX_E4M3) mx_gemm_kernel<0, 4, T><<<grid, 256, 0, s>>>(a);
    else mx_gemm_kernel<4, 4, T><<<grid, 256, 0, s>>>(a);
  });
  return check_launch("mx_gemm_kernel");
}
