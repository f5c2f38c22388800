// ffq_lpbq.hip — LPBQ weights (include/lpbq/ffq_lpbq.h): a W4 block-quantized weight as int8 codes with one scale per output channel.
//
// Reference: LPBQProcessor.grouped_dynamic_quantize, src/fastforward/export/_lpbq.py:138-175 — per output channel
//   m = amax_j s[n, j];  d = m / 2^bits;  q[n, j] = clamp(round(s[n, j] / d), 1, 2^bits)
// so that the block scale reads q * d and code4 * q is an int8 code of a per-channel tensor with scale d: the operand of the int8
// GEMM (ffq_linear.hip), whose epilogue applies per-row weight scales.
//
// Three launches, each a single kernel without workspace:
//   ffq_lpbq_compress_scales  the three lines above, one wave per row;
//   ffq_lpbq_quantize         the weight quantizer of a training / calibration step: compression (q stays in LDS), A1 at `bits` bits
//                             with ffq_affine.h's arithmetic (the codes of ffq_quantize_by_tile, bit for bit) and the product, one pass
//                             over w: 2 B in + 1 B out per element for bf16;
//   ffq_lpbq_expand           4-bit codes at rest (int8 or the nibbles of ffq_pack_int4) times q.
// Every store is an ordinary vector store from plain C++.
#ifndef FFQ_NT_STREAMS
#define FFQ_NT_STREAMS 1  // w is read once: nt loads; the codes are the next launch's GEMM operand: plain stores (ffq_vec.h)
#endif
#include "ffq_affine.h"
#include "ffq_common.h"
#include "ffq_quantizer_host.h"
#include "ffq_vec.h"

#include "../../include/lpbq/ffq_lpbq.h"

#include <math.h>

namespace ffq {

constexpr int kLpbqMaxBlocks = 1024;  // J: a row's q are one LDS line of that many bytes
constexpr int kLpbqWaveRowK = 8192;   // up to here a wave owns a row (<= 16 chunks of 8 per lane) and a workgroup four rows: the
                                      // compression's barriers and divisions are paid once per 8 chunks of a lane at K = 4096, not per 2

// The compression of one row by a team of TEAM lanes (one wave, or the whole workgroup): returns d on every lane of the team. `s` is
// the row's J scales; q goes to `q_row` (LDS, nullable) and `int_scale_row` (global, nullable), d to `*channel_scale` — all of it only
// where `live`. Every thread of the workgroup calls this (barriers inside), whether its row exists or not.
template <int TEAM>
__device__ __forceinline__ float lpbq_compress_row(const float* __restrict__ s, uint32_t J, int bits, bool live, uint32_t lane,
                                                   uint8_t* q_row, uint8_t* __restrict__ int_scale_row, float* __restrict__ channel_scale) {
  float m = -INFINITY;
  if (live)
    for (uint32_t j = lane; j < J; j += TEAM) m = __builtin_fmaxf(m, s[j]);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) m = __builtin_fmaxf(m, __shfl_xor(m, off, 64));
  if constexpr (TEAM == kBlock) {
    __shared__ float wave_max[kBlock / 64];
    if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = m;
    __syncthreads();
    m = __builtin_fmaxf(__builtin_fmaxf(wave_max[0], wave_max[1]), __builtin_fmaxf(wave_max[2], wave_max[3]));
  }
  const float top = (float)(1 << bits);
  const float d = m / top;  // the IEEE quotient (Makefile: correctly rounded divide)
  if (live) {
    for (uint32_t j = lane; j < J; j += TEAM) {
      // fmaxf / fminf: a NaN quotient (0 / 0, Inf / Inf) lands on 1
      const float v = __builtin_fminf(__builtin_fmaxf(rne(s[j] / d), 1.0f), top);
      const uint8_t q = (uint8_t)(int)v;
      if (q_row) q_row[j] = q;
      if (int_scale_row) int_scale_row[j] = q;
    }
    if (lane == 0) *channel_scale = d;
  }
  __syncthreads();  // q_row is read by other lanes
  return d;
}

__global__ __launch_bounds__(kBlock) void lpbq_compress_kernel(const float* __restrict__ scales, int64_t scale_stride, uint32_t N, uint32_t J,
                                                               int bits, uint8_t* __restrict__ int_scale, float* __restrict__ channel_scale) {
  const uint32_t slot = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t row = blockIdx.x * (kBlock / 64) + slot;
  const bool live = row < N;
  const size_t r = live ? row : 0;
  lpbq_compress_row<64>(scales + r * scale_stride, J, bits, live, lane, nullptr, int_scale + r * J, channel_scale + r);
}

struct LpbqArgs {
  uint32_t N, K, J, G;
  int64_t w_stride, scale_stride;  // elements
  int bits, requantize;
  float lo, hi;                // A1's clamp bounds at `bits` bits
  FastDiv chunks_per_group;    // group form: G / 8
};

// four int8 codes of one dword times q, truncated to int8
__device__ __forceinline__ uint32_t lpbq_scale_bytes(uint32_t v, int q) {
  const int b0 = (int)(int8_t)(v & 0xFFu), b1 = (int)(int8_t)((v >> 8) & 0xFFu), b2 = (int)(int8_t)((v >> 16) & 0xFFu), b3 = (int)(int8_t)(v >> 24);
  return pack_bytes(b0 * q, b1 * q, b2 * q, b3 * q);
}

// TEAM lanes per row (64: four rows per workgroup; kBlock: one). GROUP: 8 elements per lane and step (one or two 16-byte loads, one
// 8-byte store), else one element.
template <typename T, int TEAM, bool GROUP>
__global__ __launch_bounds__(kBlock) void lpbq_quantize_kernel(const T* __restrict__ w, const float* __restrict__ scales, int8_t* __restrict__ codes8,
                                                               float* __restrict__ channel_scale, uint8_t* __restrict__ int_scale, LpbqArgs a) {
  constexpr int ROWS = kBlock / TEAM;
  __shared__ uint8_t q_lds[ROWS][kLpbqMaxBlocks];
  const uint32_t slot = threadIdx.x / TEAM, lane = threadIdx.x % TEAM;
  const uint32_t row = blockIdx.x * ROWS + slot;
  const bool live = row < a.N;
  const size_t r = live ? row : 0;
  const float* s = scales + r * a.scale_stride;
  const T* wr = w + r * a.w_stride;
  int8_t* out = codes8 + r * a.K;
  // group form: a lane's first PRE chunks are requested before the compression, whose two barriers and divisions then run under
  // their latency
  constexpr int PRE = 4;
  const uint32_t nchunks = GROUP ? a.K / 8 : 0u;
  Chunk<T, 8> early[PRE];
  if constexpr (GROUP) {
#pragma unroll
    for (int p = 0; p < PRE; ++p)
      if (live && lane + p * TEAM < nchunks) early[p].FFQ_SLOAD(wr + (size_t)(lane + p * TEAM) * 8);
  }
  const float d = lpbq_compress_row<TEAM>(s, a.J, a.bits, live, lane, q_lds[slot], int_scale ? int_scale + r * a.J : nullptr, channel_scale + r);
  if (!live) return;
  if constexpr (GROUP) {
    auto finish = [&](const Chunk<T, 8>& in, uint32_t c) {
      const uint32_t g = fdiv(c, a.chunks_per_group);
      const int q = q_lds[slot][g];
      const float sc = a.requantize ? d * (float)q : s[g];  // (one fp32 rounding: -ffp-contract=off)
      float x[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) x[i] = in.get(i);
      Chunk<int8_t, 8> y;
      quantize_chunk_to_bytes<8>(x, sc, 0.0f, a.lo, a.hi, y);
      y.w[0] = lpbq_scale_bytes(y.w[0], q);
      y.w[1] = lpbq_scale_bytes(y.w[1], q);
      y.store(out + (size_t)c * 8);
    };
#pragma unroll
    for (int p = 0; p < PRE; ++p)
      if (lane + p * TEAM < nchunks) finish(early[p], lane + p * TEAM);
    for (uint32_t c = lane + PRE * TEAM; c < nchunks; c += TEAM) {
      Chunk<T, 8> in;
      in.FFQ_SLOAD(wr + (size_t)c * 8);
      finish(in, c);
    }
  } else {
    for (uint32_t k = lane; k < a.K; k += TEAM) {
      const uint32_t g = k / a.G;
      const int q = q_lds[slot][g];
      const float sc = a.requantize ? d * (float)q : s[g];
      const float x[4] = {to_f32(wr[k]), 0.0f, 0.0f, 0.0f};  // (the chunk arithmetic on one element: the same codes)
      Chunk<int8_t, 4> y;
      quantize_chunk_to_bytes<4>(x, sc, 0.0f, a.lo, a.hi, y);
      out[k] = (int8_t)((int)(int8_t)(y.w[0] & 0xFFu) * q);
    }
  }
}

// ---- expand: codes at rest times q ---------------------------------------------------------------------------------------------------
// Group form. Plain codes: a lane owns 8 codes (8 bytes in, 8 bytes out). Nibbles: a lane owns 8 packed bytes, i.e. 8 codes of the low
// half of a packing block and the 8 at the same place of its high half (8 bytes in, two 8-byte stores). 8 divides G, so each run of 8
// shares one q, and K % G == 0 makes the flat block index e / G the index into int_scale.
template <bool PACKED>
__global__ __launch_bounds__(kBlock) void lpbq_expand_group_kernel(const uint8_t* __restrict__ in, const uint8_t* __restrict__ int_scale,
                                                                   int8_t* __restrict__ out, uint32_t nitems, FastDiv items_per_block,
                                                                   uint32_t block, FastDiv group) {
  const uint32_t stride = gridDim.x * (uint32_t)kBlock;
  for (uint32_t item = blockIdx.x * (uint32_t)kBlock + threadIdx.x; item < nitems; item += stride) {
    if constexpr (!PACKED) {
      const uint32_t e = item * 8;
      const int q = int_scale[fdiv(e, group)];
      Chunk<int8_t, 8> c;
      c.load(reinterpret_cast<const int8_t*>(in) + e);
      c.w[0] = lpbq_scale_bytes(c.w[0], q);
      c.w[1] = lpbq_scale_bytes(c.w[1], q);
      c.store(out + e);
    } else {
      const uint32_t b = fdiv(item, items_per_block);
      const uint32_t j = (item - b * items_per_block.div) * 8;
      const uint32_t e_lo = b * block + j, e_hi = e_lo + block / 2;
      const int q_lo = int_scale[fdiv(e_lo, group)], q_hi = int_scale[fdiv(e_hi, group)];
      Chunk<uint8_t, 8> p;
      p.load(in + (size_t)b * (block / 2) + j);
      Chunk<int8_t, 8> lo, hi;
#pragma unroll
      for (int wd = 0; wd < 2; ++wd) {
        int l[4], h[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const uint32_t byte = (p.w[wd] >> (8 * i)) & 0xFFu;
          l[i] = ((int)(byte & 15u) - 8) * q_lo;
          h[i] = ((int)(byte >> 4) - 8) * q_hi;
        }
        lo.w[wd] = pack_bytes(l[0], l[1], l[2], l[3]);
        hi.w[wd] = pack_bytes(h[0], h[1], h[2], h[3]);
      }
      lo.store(out + e_lo);
      hi.store(out + e_hi);
    }
  }
}

// Element form: any G, block and alignment; one code (nibbles: one byte, two codes) per lane.
template <bool PACKED>
__global__ __launch_bounds__(kBlock) void lpbq_expand_element_kernel(const uint8_t* __restrict__ in, const uint8_t* __restrict__ int_scale,
                                                                     int8_t* __restrict__ out, int64_t nitems, int64_t block, int64_t G) {
  const int64_t stride = (int64_t)gridDim.x * kBlock, half = block / 2;
  for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < nitems; p += stride) {
    if constexpr (!PACKED) {
      out[p] = (int8_t)((int)(int8_t)in[p] * (int)int_scale[p / G]);
    } else {
      const int64_t b = p / half, j = p % half;
      const int64_t e_lo = b * block + j, e_hi = e_lo + half;
      const uint32_t byte = in[p];
      out[e_lo] = (int8_t)(((int)(byte & 15u) - 8) * (int)int_scale[e_lo / G]);
      out[e_hi] = (int8_t)(((int)(byte >> 4) - 8) * (int)int_scale[e_hi / G]);
    }
  }
}

// ---- host: each rule of the three entry points once --------------------------------------------------------------------------------------
static bool lpbq_bits_ok(int bits) { return bits >= 2 && bits <= 4; }
static bool lpbq_extent_ok(int64_t v) { return v >= 0 && v < ((int64_t)1 << 31); }
static bool aligned_to(const void* p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

// N, K, G and the block count of a row, in the order quantize and expand share
static int lpbq_check_matrix(const char* who, int64_t N, int64_t K, int64_t G) {
  if (!lpbq_extent_ok(N) || !lpbq_extent_ok(K) || G < 1) return fail(FFQ_ERR_ARG, "%s: bad extent (N %lld, K %lld, G %lld)", who, (long long)N, (long long)K, (long long)G);
  if (K % G) return fail(FFQ_ERR_ARG, "%s: K %% G != 0 (K %lld, G %lld)", who, (long long)K, (long long)G);
  if (K / G > kLpbqMaxBlocks) return fail(FFQ_ERR_ARG, "%s: K / G = %lld blocks per row, at most %d", who, (long long)(K / G), kLpbqMaxBlocks);
  return FFQ_OK;
}

static unsigned lpbq_grid(int64_t items) {
  int64_t blocks = (items + kBlock - 1) / kBlock;
  if (blocks > 16384) blocks = 16384;
  return (unsigned)(blocks < 1 ? 1 : blocks);
}

}  // namespace ffq

using namespace ffq;

extern "C" int ffq_lpbq_compress_scales(const float* scales, int64_t scale_stride, int64_t N, int64_t J, int bits, uint8_t* int_scale,
                                        float* channel_scale, void* stream) {
  static const char* who = "lpbq_compress_scales";
  if (!lpbq_bits_ok(bits)) return fail(FFQ_ERR_ARG, "%s: bits must be 2, 3 or 4, got %d", who, bits);
  if (!lpbq_extent_ok(N) || J < 0) return fail(FFQ_ERR_ARG, "%s: bad extent (N %lld, J %lld)", who, (long long)N, (long long)J);
  if (J > kLpbqMaxBlocks) return fail(FFQ_ERR_ARG, "%s: J = %lld blocks per row, at most %d", who, (long long)J, kLpbqMaxBlocks);
  if (scale_stride < J) return fail(FFQ_ERR_ARG, "%s: the row stride %lld is below the row length %lld", who, (long long)scale_stride, (long long)J);
  if (N == 0 || J == 0) return FFQ_OK;
  if (!scales || !int_scale || !channel_scale) return fail(FFQ_ERR_ARG, "%s: NULL buffer", who);
  if (!aligned_to(scales, 4) || !aligned_to(channel_scale, 4)) return fail(FFQ_ERR_ARG, "%s: scales and channel_scale must be 4-byte aligned", who);
  const unsigned grid = (unsigned)((N + kBlock / 64 - 1) / (kBlock / 64));
  lpbq_compress_kernel<<<grid, kBlock, 0, static_cast<hipStream_t>(stream)>>>(scales, scale_stride, (uint32_t)N, (uint32_t)J, bits, int_scale, channel_scale);
  return check_launch("lpbq_compress_kernel");
}

extern "C" int ffq_lpbq_quantize(const void* w, int w_dt, int64_t w_stride, const float* scales, int64_t scale_stride, int64_t N, int64_t K,
                                 int64_t G, int bits, int requantize, int8_t* codes8, float* channel_scale, uint8_t* int_scale, void* stream) {
  static const char* who = "lpbq_quantize";
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (!is_f32_bf16_f16(w_dt)) return fail(FFQ_ERR_DTYPE, "%s: w holds bf16, fp16 or fp32 values, got dtype %d", who, w_dt);
  if (!lpbq_bits_ok(bits)) return fail(FFQ_ERR_ARG, "%s: bits must be 2, 3 or 4, got %d", who, bits);
  if (requantize != 0 && requantize != 1) return fail(FFQ_ERR_ARG, "%s: requantize is 0 or 1, got %d", who, requantize);
  if (int rc = lpbq_check_matrix(who, N, K, G)) return rc;
  const int64_t J = K / G;
  if (w_stride < K || scale_stride < J)
    return fail(FFQ_ERR_ARG, "%s: a row stride is below the row length (w %lld < %lld or scales %lld < %lld)", who, (long long)w_stride, (long long)K,
                (long long)scale_stride, (long long)J);
  if (N == 0 || K == 0) return FFQ_OK;
  if (!w || !scales || !codes8 || !channel_scale) return fail(FFQ_ERR_ARG, "%s: NULL buffer", who);
  if (!aligned_to(w, (uintptr_t)dt_size(w_dt)) || !aligned_to(scales, 4) || !aligned_to(channel_scale, 4))
    return fail(FFQ_ERR_ARG, "%s: w must be aligned to its element, scales and channel_scale to 4 bytes", who);
  const ClampBounds bounds = clamp_bounds((double)bits);
  LpbqArgs a;
  a.N = (uint32_t)N; a.K = (uint32_t)K; a.J = (uint32_t)J; a.G = (uint32_t)G;
  a.w_stride = w_stride; a.scale_stride = scale_stride;
  a.bits = bits; a.requantize = requantize;
  a.lo = (float)bounds.lo; a.hi = (float)bounds.hi;
  const bool group = G % 8 == 0 && aligned16(w) && (w_stride * dt_size(w_dt)) % 16 == 0 && aligned_to(codes8, 8) && !generic_kernels_forced();
  a.chunks_per_group = make_fastdiv(group ? (uint32_t)(G / 8) : 1u);
  const bool wave_rows = K <= kLpbqWaveRowK;
  const unsigned grid = wave_rows ? (unsigned)((N + kBlock / 64 - 1) / (kBlock / 64)) : (unsigned)N;
#define FFQ_LPBQ_Q(T, TEAM, GROUP) \
  lpbq_quantize_kernel<T, TEAM, GROUP><<<grid, kBlock, 0, s>>>(static_cast<const T*>(w), scales, codes8, channel_scale, int_scale, a)
  for_dtype<bf16_t, f16_t, float>(w_dt, [&](auto t) {
    using T = typename decltype(t)::type;
    if (wave_rows) {
      if (group) FFQ_LPBQ_Q(T, 64, true); else FFQ_LPBQ_Q(T, 64, false);
    } else {
      if (group) FFQ_LPBQ_Q(T, kBlock, true); else FFQ_LPBQ_Q(T, kBlock, false);
    }
  });
#undef FFQ_LPBQ_Q
  return check_launch("lpbq_quantize_kernel");
}

extern "C" int ffq_lpbq_expand(const void* codes4, int packed, int64_t block, const uint8_t* int_scale, int64_t N, int64_t K, int64_t G,
                               int8_t* codes8, void* stream) {
  static const char* who = "lpbq_expand";
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (packed != 0 && packed != 1) return fail(FFQ_ERR_ARG, "%s: packed is 0 or 1, got %d", who, packed);
  if (int rc = lpbq_check_matrix(who, N, K, G)) return rc;
  const int64_t numel = N * K;
  if (packed && (block < 2 || (block & 1) || numel % block))
    return fail(FFQ_ERR_ARG, "%s: bad block %lld (even, >= 2, a divisor of N * K = %lld)", who, (long long)block, (long long)numel);
  if (numel == 0) return FFQ_OK;
  if (!codes4 || !int_scale || !codes8) return fail(FFQ_ERR_ARG, "%s: NULL buffer", who);
  const uint8_t* in = static_cast<const uint8_t*>(codes4);
  const bool group = G % 8 == 0 && numel < ((int64_t)1 << 32) && aligned_to(codes4, 8) && aligned_to(codes8, 8) && (!packed || block % 16 == 0) &&
                     !generic_kernels_forced();
  if (group) {
    const FastDiv by_group = make_fastdiv((uint32_t)G);
    if (packed) {
      const uint32_t nitems = (uint32_t)(numel / 16);
      lpbq_expand_group_kernel<true><<<lpbq_grid(nitems), kBlock, 0, s>>>(in, int_scale, codes8, nitems, make_fastdiv((uint32_t)(block / 16)), (uint32_t)block, by_group);
    } else {
      const uint32_t nitems = (uint32_t)(numel / 8);
      lpbq_expand_group_kernel<false><<<lpbq_grid(nitems), kBlock, 0, s>>>(in, int_scale, codes8, nitems, make_fastdiv(1u), 0u, by_group);
    }
    return check_launch("lpbq_expand_group_kernel");
  }
  if (packed) lpbq_expand_element_kernel<true><<<lpbq_grid(numel / 2), kBlock, 0, s>>>(in, int_scale, codes8, numel / 2, block, G);
  else lpbq_expand_element_kernel<false><<<lpbq_grid(numel), kBlock, 0, s>>>(in, int_scale, codes8, numel, 0, G);
  return check_launch("lpbq_expand_element_kernel");
}
