// ffq_sdpa_decode.hip — scaled_dot_product_attention for a short query over int8 K / V codes (a quantized KV cache), split over the
// keys: two plain launches, no tickets, no spin waits, no grid barrier (include/ffq_sdpa_decode.h).
//
// sdpa_decode_partial_kernel: one workgroup = 4 waves = one (batch, kv head, key split). The rows = L * (H / HKV) <= 32 query rows
// that read this kv head are the query side of ONE 32x32x16 MFMA tile (row r = g * L + l: query head kvh * G + g, position l), so
// the codes of K and V are read once per (batch, kv head) whatever the GQA group is. A wave walks 32-key tiles of the split (wave w
// takes keys [128 it + 32 w, +32) of it) with its own online softmax; the four waves' (m, l, O) are merged through LDS at the end.
//   * K stays int8 in memory and goes from global memory straight into the MFMA's A operand: lane (key r32, half h) loads the 16
//     codes of columns [(2u + h) * 16, +16) of its key row with one 16-byte load and dequantizes them in registers,
//     (c + rne(o)) * s in fp32, rounded once to the data dtype (transform<F16> of ffq_sdpa.hip: the value the math path contracts).
//     Their first 8 values are the lane's slice of MFMA step 2u, the last 8 of step 2u + 1; the Q fragments use the same slices, so
//     the contraction runs over all of E in an order of its own (fp32 accumulation);
//   * scores transposed, S^T[key][row] = mfma(A = K, B = Q): a lane holds 16 keys of one query row, the row statistics are
//     lane-local plus one cross-half exchange. The raw q values enter the MFMA and sqrt(scale)^2 multiplies the fp32 sum;
//   * V is loaded the same way, dequantized, and written to a wave-private V^T image in LDS ([d][key], 72-byte pitch), from which
//     the A operand of O^T[d][row] = mfma(A = V^T, B = P) is read with two 8-byte loads (load_vt of ffq_sdpa.hip). The image is
//     written ahead of the tile's score chain, so its stores land under the QK^T MFMAs and the softmax. bf16 P carries its rounding
//     residue in a second MFMA, as there;
//   * the next tile's K and V loads are issued before this tile's arithmetic: 8 KiB in flight per wave, 32 KiB per workgroup;
//   * keys >= the split's end (and >= S) are never loaded and score -inf; rows >= `rows` hold zeros and are never stored.
// It writes fp32 partials: O[rows][E], m[rows], l[rows] per (batch, kv head, split). m = -inf (l = 0, O = 0) for a row whose keys
// in the split are all masked, and for a forced split without keys.
//
// sdpa_decode_combine_kernel: one workgroup per (batch, head, position), one lane per column:
// m = max m_i, out = sum e^(m_i - m) O_i / sum e^(m_i - m) l_i in fp32; a split with m_i = -inf contributes nothing, a row with
// every m_i = -inf gives exactly 0 (the safe softmax); then the optional output quantizer on the fp32 value (A1 then A2, QReg::fake
// of ffq_sdpa.hip) and one rounding to the data dtype.
//
// The split plan is a pure function of (B, HKV, S, rows, E): no device state, graph-safe (docs/kernels.md has the sweep).
//
// ffq_kv_decode (include/ffq_kv_cache.h) runs the same two kernels over a preallocated cache: the split COUNT is still a host
// integer, but every batch reads its own key count from `lens` on the device and cuts it over that count by the same rule, and the
// causal mask is bottom-right. Both entry points share the kernels' instantiations: the difference is a launch-uniform null check.
//
// ffq_kv_paged_decode (include/ffq_kv_paged.h) is ffq_kv_decode over K / V held in fixed-size pages of two pools.
// kv_paged_partial_kernel is the partial kernel's body (decode_partial) instantiated with PAGED: a lane finds its key row through
// one int32 load of the sequence's block table per tile (page table[b][key / P], row key % P; P >= 32 makes the page uniform over a
// wave's 32 keys, P = 16 gives two), and the keys of a table entry outside the pool are neither loaded nor scored (-inf, as a bool
// mask would). The key order, the arithmetic, the LDS and the combine kernel are the dense form's: the same bits at the same split count.
//
// ffq_kv_token_decode (include/ffq_kv_token.h) is ffq_kv_decode over codes whose (scale, offset) live per position in an fp32 store
// beside them. kv_token_partial_kernel is decode_partial instantiated with TOKEN: stage_load loads the lane's key position's four
// floats (k_scale, k_offset, v_scale, v_offset) with one 16-byte load beside the K and V codes (zeros for a position that is not
// loaded), and the tile's dks / dko / dvs / dvo come out of those staging registers when the tile is consumed, each lane's own. Nothing
// else differs: the same bits as the dense form wherever the parameters agree.
//
// ffq_kv_paged_token_decode (include/ffq_kv_paged_token.h) is ffq_kv_token_decode over pages. kv_paged_token_partial_kernel is
// decode_partial instantiated with PAGED and TOKEN: the lane's four floats come from row key % P of page table[b][key / P] of the
// parameter pool, one 16-byte load beside the K and V loads under the same `in` flag (the length, the split's end, a page outside the
// pool), so the parameters of a key that is not loaded are not loaded either. At P = 16 a wave's 32 keys span two pages; the page is per
// lane already. The key order, the arithmetic, the LDS and the combine kernel are unchanged.
//
// Host side: the entry points fill one DecodeCall from their own parameter lists, run the shared rules (check_operands,
// check_rows, check_quantizer_and_splits, check_sizes_and_buffers, check_layout_and_workspace) in the order their error tables pin,
// with their own steps in between, and hand the call to enqueue(); launch_partial is the one partial launch (docs/kernels.md).
#include "ffq_affine.h"
#include "ffq_common.h"
#include "ffq_paging.h"
#include "ffq_vec.h"

#include "../../include/ffq_kv_cache.h"
#include "../../include/ffq_kv_paged.h"
#include "../../include/ffq_kv_paged_token.h"
#include "../../include/ffq_kv_token.h"
#include "../../include/ffq_sdpa_decode.h"

#include <math.h>

namespace ffq {
namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 dc_bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 dc_f16x8;
typedef __attribute__((ext_vector_type(16))) float dc_f32x16;
typedef __attribute__((ext_vector_type(4))) short dc_s16x4;
typedef __attribute__((ext_vector_type(4))) float dc_f32x4;

constexpr int kWaves = 4;
constexpr int kThreads = kWaves * 64;
constexpr int kRows = FFQ_SDPA_DECODE_MAX_ROWS;   // query rows of the one MFMA tile
constexpr int kWaveKeys = 32;                     // keys per wave step
constexpr int kTile = FFQ_SDPA_DECODE_KEY_TILE;   // keys per workgroup step: the unit of a split
constexpr int kVtPitch = 72;                      // bytes per column of a wave's V^T image (32 keys + 8 bytes of skew)
static_assert(kTile == kWaves * kWaveKeys, "a workgroup step is one 32-key tile per wave");

enum { MASK_NONE = 0, MASK_CAUSAL, MASK_BOOL, MASK_FLOAT };

struct DecodeArgs {
  const void* q;       // dt or int8 container
  const int8_t* k;
  const int8_t* v;
  const float* deq_s[3];  // q (nullptr: plain) / k / v
  const float* deq_o[3];
  int64_t qs[3], ks[3], vs[3];  // element strides of (batch, head, row)
  int32_t B, H, HKV, L, S;
  int32_t rows, splits, tiles_per_split;
  int32_t q_i8;
  const void* mask;
  int32_t mask_kind, mask_dt;
  int64_t ms[4];
  float c;  // float(sqrt(scale))
  float* ws_o;
  float* ws_m;
  float* ws_l;
  // ffq_kv_decode (include/ffq_kv_cache.h): the key count of every batch on the device. nullptr: S and tiles_per_split above hold
  // for every batch. Else S is S_max, batch b has S_b = clamp(lens[b], 0, S) keys, cut over `splits` by the same rule, and
  // MASK_CAUSAL is bottom-right: row l sees key <= l + (S_b - L)
  const int32_t* lens;
};

template <bool F16>
__device__ __forceinline__ float to_f32(uint16_t h) {
  return F16 ? f16_bits_to_f32(h) : bf16_bits_to_f32(h);
}
template <bool F16>
__device__ __forceinline__ uint16_t from_f32(float f) {
  return F16 ? f32_to_f16_bits(f) : f32_to_bf16_bits(f);
}
template <bool F16>
__device__ __forceinline__ uint32_t pack_pair(float a, float b) {
  if constexpr (F16) return pack2<f16_t>(a, b);
  else return pack2<bf16_t>(a, b);
}

// 4 int8 codes of one dword -> 4 dequantized values in the data dtype (two dwords): (c + o) * s in fp32, one rounding. `w` holds the
// codes with their sign bits flipped (c + 128 as unsigned bytes: one conversion instruction each) and `o` is rne(offset) - 128, so
// (c + 128) + (o - 128) is the one fp32 addition whose exact operands sum to c + rne(offset): the bits of (float)c + rne(offset)
// for every |rne(offset)| < 2^24 - 127, where both operands and the sum are integers below 2^24. At rne(offset) = -(2^24 - 127) the
// bias term -(2^24 + 1) is itself rounded, and from there on the sum may differ from (float)c + rne(offset) by one fp32 ulp before
// the product and the rounding to the data dtype (docs/numerics.md; tests/test_sdpa_decode_cases_cpu.py holds the bound).
template <bool F16>
__device__ __forceinline__ void dequant4(uint32_t w, float s, float o, uint32_t& lo, uint32_t& hi) {
  const float f0 = ((float)(w & 0xFFu) + o) * s;
  const float f1 = ((float)((w >> 8) & 0xFFu) + o) * s;
  const float f2 = ((float)((w >> 16) & 0xFFu) + o) * s;
  const float f3 = ((float)(w >> 24) + o) * s;
  lo = pack_pair<F16>(f0, f1);
  hi = pack_pair<F16>(f2, f3);
}

// 16 codes -> the 8 values of MFMA step 2u (a) and of step 2u + 1 (b); `o` is rne(offset) - 128 (dequant4)
template <bool F16>
__device__ __forceinline__ void dequant16(u32x4 w, float s, float o, u32x4& a, u32x4& b) {
  uint32_t p[8];
  dequant4<F16>(w.x ^ 0x80808080u, s, o, p[0], p[1]);
  dequant4<F16>(w.y ^ 0x80808080u, s, o, p[2], p[3]);
  dequant4<F16>(w.z ^ 0x80808080u, s, o, p[4], p[5]);
  dequant4<F16>(w.w ^ 0x80808080u, s, o, p[6], p[7]);
  a = u32x4{p[0], p[1], p[2], p[3]};
  b = u32x4{p[4], p[5], p[6], p[7]};
}

// 8 values of a value-dtype container: codes dequantized to dt, or the plain values as they are
template <bool F16>
__device__ __forceinline__ u32x4 dequant8(u32x4 w, bool deq, float s, float o) {
  if (!deq) return w;
  uint32_t word[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float x0 = (to_f32<F16>((uint16_t)(word[i] & 0xFFFFu)) + o) * s;
    const float x1 = (to_f32<F16>((uint16_t)(word[i] >> 16)) + o) * s;
    word[i] = pack_pair<F16>(x0, x1);
  }
  return u32x4{word[0], word[1], word[2], word[3]};
}

__device__ __forceinline__ dc_bf16x8 load_vt(const unsigned char* vt, uint32_t d, uint32_t key0) {
  const dc_s16x4 a = *reinterpret_cast<const dc_s16x4*>(vt + d * kVtPitch + key0 * 2);
  const dc_s16x4 b = *reinterpret_cast<const dc_s16x4*>(vt + d * kVtPitch + (key0 + 8) * 2);
  return __builtin_bit_cast(dc_bf16x8, __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7));
}

template <bool F16>
__device__ __forceinline__ dc_f32x16 mfma(dc_bf16x8 a, dc_bf16x8 b, dc_f32x16 c) {
  if constexpr (F16)
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(dc_f16x8, a), __builtin_bit_cast(dc_f16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

template <int E>
struct Lds {
  static constexpr int kVt = kWaves * E * kVtPitch;                        // the four V^T images
  static constexpr int kMerge = (kWaves - 1) * (E / 32) * 16 * 64 * 4;     // waves 1..3 hand their O to wave 0
  static constexpr int kBody = kVt > kMerge ? kVt : kMerge;
  static constexpr int kStats = 2 * kWaves * kRows * 4;                    // m and l of every wave
};

// Paged K / V (include/ffq_kv_paged.h, ffq_paging.h): the codes live in fixed-size pages of two pools, found through a per-sequence
// block table. DecodeArgs::ks / vs are then the (page, head, row) strides of the pools, S is the capacity max_pages * P of a sequence
struct PagedDecodeArgs : DecodeArgs {
  Paging pg;
};

// Per-position parameters (include/ffq_kv_token.h): deq_s[1..2] / deq_o[1..2] are unused, `params` is the fp32 store
// [batch, kv_heads, S, 4] of (k_scale, k_offset, v_scale, v_offset) with the (batch, head, row) strides ps
struct TokenDecodeArgs : DecodeArgs {
  const float* params;
  int64_t ps[3];
};

// Both (include/ffq_kv_paged_token.h): `params` is the parameter pool [num_pages, kv_heads, P, 4] and ps its (page, head, row) strides
struct PagedTokenDecodeArgs : TokenDecodeArgs {
  Paging pg;
};

// The body of the partial kernels. PAGED changes where a lane finds its key row (stage_load) and adds one mask, the keys of a page
// the table does not place inside the pool; the arithmetic and the key order are the dense form's. TOKEN changes where a lane finds
// the (scale, offset) of its key row: staged beside the codes, one 16-byte load per lane and tile (with PAGED: out of the key's page
// of the parameter pool)
template <int E, bool F16, bool PAGED, bool TOKEN = false, typename Args>
__device__ __forceinline__ void decode_partial(const Args& a) {
  constexpr int T = E / 16;   // MFMA k-steps of QK^T
  constexpr int U = E / 32;   // 16-byte loads per key row and lane
  constexpr int DB = E / 32;  // 32-column blocks of O^T
  __shared__ __attribute__((aligned(16))) unsigned char body[Lds<E>::kBody];
  __shared__ float stat_m[kWaves][kRows];
  __shared__ float stat_l[kWaves][kRows];

  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t r32 = lane & 31, h = lane >> 5;
  const uint32_t sp = blockIdx.x % (uint32_t)a.splits, bk = blockIdx.x / (uint32_t)a.splits;
  const uint32_t kvh = bk % (uint32_t)a.HKV, b = bk / (uint32_t)a.HKV;
  const uint32_t G = (uint32_t)a.H / (uint32_t)a.HKV;

  // this batch's keys, tiles per split and causal diagonal: the launch's, or (a cache with device-side lengths) its own
  int32_t S = a.S, per = a.tiles_per_split, diag = 0;
  if (a.lens != nullptr) {
    const int32_t n = a.lens[b];
    S = n < 0 ? 0 : (n < a.S ? n : a.S);
    per = ((S + kTile - 1) / kTile + a.splits - 1) / a.splits;
    diag = S - a.L;
  }
  // the split's keys [k_begin, k_end): whole tiles but for the last split; a forced split may be empty
  const int64_t first = (int64_t)sp * per * kTile;
  const int32_t k_begin = first < S ? (int32_t)first : S;
  const int64_t last = first + (int64_t)per * kTile;
  const int32_t k_end = last < S ? (int32_t)last : S;
  const int32_t iters = (k_end - k_begin + kTile - 1) / kTile;  // the same for the four waves: the barriers below are uniform

  // this lane's query row
  const bool row_ok = (int32_t)r32 < a.rows;
  const uint32_t row = row_ok ? r32 : 0;
  const uint32_t g = row / (uint32_t)a.L, l = row % (uint32_t)a.L;
  const uint32_t head = kvh * G + g;

  const bool deq_q = a.deq_s[0] != nullptr;
  const float dqs = deq_q ? a.deq_s[0][0] : 1.0f, dqo = (deq_q && a.deq_o[0]) ? rne(a.deq_o[0][0]) : 0.0f;
  float dks = 0.0f, dko = 0.0f, dvs = 0.0f, dvo = 0.0f;  // (TOKEN: this lane's key row's, out of the staging registers)
  if constexpr (!TOKEN) {
    dks = a.deq_s[1][0], dko = (a.deq_o[1] ? rne(a.deq_o[1][0]) : 0.0f) - 128.0f;  // (biased: dequant4)
    dvs = a.deq_s[2][0], dvo = (a.deq_o[2] ? rne(a.deq_o[2][0]) : 0.0f) - 128.0f;
  }
  const float alpha = a.c * a.c;

  // ---- Q fragments: step t = 2u + j takes columns [(2u + h) * 16 + 8j, +8) of row `row` (the slices of the K loads)
  dc_bf16x8 qf[T];
  {
    const int64_t at = (int64_t)b * a.qs[0] + (int64_t)head * a.qs[1] + (int64_t)l * a.qs[2];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      u32x4 lo, hi;
      if (a.q_i8) {
        const u32x4 w = *reinterpret_cast<const u32x4*>(static_cast<const int8_t*>(a.q) + at + (2 * u + h) * 16);
        dequant16<F16>(w, dqs, dqo - 128.0f, lo, hi);
      } else {
        const uint16_t* p = static_cast<const uint16_t*>(a.q) + at + (2 * u + h) * 16;
        lo = dequant8<F16>(*reinterpret_cast<const u32x4*>(p), deq_q, dqs, dqo);
        hi = dequant8<F16>(*reinterpret_cast<const u32x4*>(p + 8), deq_q, dqs, dqo);
      }
      if (!row_ok) lo = hi = u32x4{0, 0, 0, 0};
      qf[2 * u] = __builtin_bit_cast(dc_bf16x8, lo);
      qf[2 * u + 1] = __builtin_bit_cast(dc_bf16x8, hi);
    }
  }

  // ---- K / V rows of this lane: key (tile's first) + r32, 16 codes at column (2u + h) * 16; rows >= k_end read nothing
  // paged: the row is (page table[b][key / P], row key % P) of the pools, one table load per lane and tile; a table entry outside
  // [0, num_pages) reads nothing either, and `staged_ok` (bit i: key i of the staged 32 was loaded) masks its keys in the scores
  const int8_t* kbase = a.k + (PAGED ? 0 : (int64_t)b * a.ks[0]) + (int64_t)kvh * a.ks[1] + h * 16;
  const int8_t* vbase = a.v + (PAGED ? 0 : (int64_t)b * a.vs[0]) + (int64_t)kvh * a.vs[1] + h * 16;
  u32x4 sk[U], sv[U];
  uint32_t staged_ok = 0;
  [[maybe_unused]] dc_f32x4 sprm = {0.0f, 0.0f, 0.0f, 0.0f};  // (TOKEN) the staged key row's (k_scale, k_offset, v_scale, v_offset)
  [[maybe_unused]] const float* pbase = nullptr;
  if constexpr (TOKEN) pbase = a.params + (PAGED ? 0 : (int64_t)b * a.ps[0]) + (int64_t)kvh * a.ps[1];
  auto stage_load = [&](int32_t it) {
    const int32_t key = k_begin + it * kTile + (int32_t)wave * kWaveKeys + (int32_t)r32;
    bool in = key < k_end;
    int32_t at = key;                   // the row inside the cache, or inside its page
    int64_t k_page = 0, v_page = 0;     // (paged) where the page starts in each pool
    [[maybe_unused]] int64_t p_page = 0;
    if constexpr (PAGED) {
      const int32_t page = in ? page_of(a.pg, b, key) : -1;
      in = page >= 0;
      at = key & ((1 << a.pg.page_shift) - 1);
      k_page = (int64_t)page * a.ks[0];
      v_page = (int64_t)page * a.vs[0];
      if constexpr (TOKEN) p_page = (int64_t)page * a.ps[0];
      staged_ok = (uint32_t)__ballot(in);  // (both halves of the wave hold the same 32 keys)
    }
    if constexpr (TOKEN) {
      sprm = dc_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      if (in) sprm = *reinterpret_cast<const dc_f32x4*>(pbase + p_page + (int64_t)at * a.ps[2]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      sk[u] = u32x4{0, 0, 0, 0};
      sv[u] = u32x4{0, 0, 0, 0};
      if (in) {
        sk[u] = *reinterpret_cast<const u32x4*>(kbase + k_page + (int64_t)at * a.ks[2] + u * 32);
        sv[u] = *reinterpret_cast<const u32x4*>(vbase + v_page + (int64_t)at * a.vs[2] + u * 32);
      }
    }
  };

  unsigned char* vt = body + wave * (E * kVtPitch);
  const unsigned char* mbase = static_cast<const unsigned char*>(a.mask);
  const int64_t moff = (int64_t)b * a.ms[0] + (int64_t)head * a.ms[1] + (int64_t)l * a.ms[2];

  dc_f32x16 o[DB];
#pragma unroll
  for (int i = 0; i < DB; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) o[i][e] = 0.0f;
  float m_run = -INFINITY, l_run = 0.0f;  // l_run: this lane's half of the row sum

  if (iters > 0) stage_load(0);
  for (int32_t it = 0; it < iters; ++it) {
    // this tile's operands out of the staging registers, the next tile's loads into them
    dc_bf16x8 kf[T];
    u32x4 vw[U][2];
    if constexpr (TOKEN) {  // (the offsets are stored rounded; biased as above)
      dks = sprm.x; dko = sprm.y - 128.0f;
      dvs = sprm.z; dvo = sprm.w - 128.0f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      u32x4 lo, hi;
      dequant16<F16>(sk[u], dks, dko, lo, hi);
      kf[2 * u] = __builtin_bit_cast(dc_bf16x8, lo);
      kf[2 * u + 1] = __builtin_bit_cast(dc_bf16x8, hi);
      dequant16<F16>(sv[u], dvs, dvo, vw[u][0], vw[u][1]);
    }
    const int32_t key0 = k_begin + it * kTile + (int32_t)wave * kWaveKeys;
    const uint32_t tile_ok = staged_ok;
    if (it + 1 < iters) stage_load(it + 1);

    // ---- V^T image of the wave's 32 keys: column d is a row of 32 keys. Written ahead of the score chain, whose MFMAs and softmax
    // then run while the stores land; the barrier after the softmax publishes it
    __syncthreads();  // (the previous tile's reads are done)
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const uint32_t words[4] = {vw[u][half].x, vw[u][half].y, vw[u][half].z, vw[u][half].w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const uint32_t d = (2 * u + h) * 16 + 8 * half + j;
          *reinterpret_cast<uint16_t*>(vt + d * kVtPitch + r32 * 2) = (uint16_t)(words[j >> 1] >> (16 * (j & 1)));
        }
      }

    // ---- S^T of 32 keys x 32 rows
    dc_f32x16 s, s_odd;  // two chains of T / 2 dependent MFMAs instead of one of T
#pragma unroll
    for (int e = 0; e < 16; ++e) s[e] = s_odd[e] = 0.0f;
#pragma unroll
    for (int t = 0; t < T; t += 2) {
      s = mfma<F16>(kf[t], qf[t], s);
      s_odd = mfma<F16>(kf[t + 1], qf[t + 1], s_odd);
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) s[e] += s_odd[e];
    // the masked scores x (keys >= k_end -> -inf): the mask's kind is launch-uniform, so each form is a straight run of 16 elements;
    // a key beyond the split reads the mask at the split's last key (in bounds) and is then discarded
    const bool whole = key0 + kWaveKeys <= k_end;
    auto key_of = [&](int e) { return key0 + (e & 3) + 8 * (e >> 2) + 4 * (int32_t)h; };
#pragma unroll
    for (int e = 0; e < 16; ++e) s[e] *= alpha;
    if (a.mask_kind == MASK_CAUSAL) {
#pragma unroll
      for (int e = 0; e < 16; ++e) s[e] = key_of(e) <= (int32_t)l + diag ? s[e] : -INFINITY;
    } else if (a.mask_kind == MASK_BOOL) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int32_t key = key_of(e) < k_end ? key_of(e) : k_end - 1;
        s[e] = mbase[moff + (int64_t)key * a.ms[3]] ? s[e] : -INFINITY;
      }
    } else if (a.mask_kind == MASK_FLOAT) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int32_t key = key_of(e) < k_end ? key_of(e) : k_end - 1;
        const int64_t at = moff + (int64_t)key * a.ms[3];
        float mv;
        if (a.mask_dt == FFQ_F32) mv = reinterpret_cast<const float*>(mbase)[at];
        else if (a.mask_dt == FFQ_BF16) mv = bf16_bits_to_f32(reinterpret_cast<const uint16_t*>(mbase)[at]);
        else mv = f16_bits_to_f32(reinterpret_cast<const uint16_t*>(mbase)[at]);
        s[e] = s[e] + mv;
      }
    }
    if (!whole) {
#pragma unroll
      for (int e = 0; e < 16; ++e) s[e] = key_of(e) < k_end ? s[e] : -INFINITY;
    }
    if constexpr (PAGED) {
      if (tile_ok != 0xFFFFFFFFu) {  // (wave-uniform) a key without a page in the pool: as if a bool mask hid it
#pragma unroll
        for (int e = 0; e < 16; ++e) s[e] = (tile_ok >> (key_of(e) - key0)) & 1u ? s[e] : -INFINITY;
      }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int e = 0; e < 16; ++e) mx = fmaxf(mx, s[e]);
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float m_new = fmaxf(m_run, mx);
    const float m_use = m_new == -INFINITY ? 0.0f : m_new;
    const float scale_old = m_run == -INFINITY ? 0.0f : __expf(m_run - m_use);
    m_run = m_new;
    l_run *= scale_old;
    if (__any(scale_old != 1.0f)) {  // (wave-uniform: once the running maxima have settled, nothing is rescaled)
#pragma unroll
      for (int i = 0; i < DB; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) o[i][e] *= scale_old;
    }
    // P in the data dtype, two per conversion; pl: (bf16) the rounding residue of P, a second MFMA term
    uint32_t pw[8], lw[8];
    float rs = 0.0f;
#pragma unroll
    for (int e = 0; e < 16; e += 2) {
      const float p0 = __expf(s[e] - m_use), p1 = __expf(s[e + 1] - m_use);
      rs += p0;
      rs += p1;
      const uint32_t w = pack_pair<F16>(p0, p1);
      pw[e >> 1] = w;
      if constexpr (!F16) lw[e >> 1] = pack_pair<false>(p0 - bf16_bits_to_f32((uint16_t)(w & 0xFFFFu)), p1 - bf16_bits_to_f32((uint16_t)(w >> 16)));
    }
    l_run += rs;
    dc_bf16x8 pf[2], pl[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      pf[u] = __builtin_bit_cast(dc_bf16x8, u32x4{pw[4 * u], pw[4 * u + 1], pw[4 * u + 2], pw[4 * u + 3]});
      if constexpr (!F16) pl[u] = __builtin_bit_cast(dc_bf16x8, u32x4{lw[4 * u], lw[4 * u + 1], lw[4 * u + 2], lw[4 * u + 3]});
    }

    __syncthreads();  // (the V^T image is complete)
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const dc_bf16x8 vf = load_vt(vt, 32 * db + r32, 16 * u + 4 * h);
        o[db] = mfma<F16>(vf, pf[u], o[db]);
        if constexpr (!F16) o[db] = mfma<F16>(vf, pl[u], o[db]);
      }
  }

  // ---- merge the four waves: m = max m_w, O = sum e^(m_w - m) O_w, l = sum e^(m_w - m) l_w
  const float l_wave = l_run + __shfl_xor(l_run, 32);
  if (h == 0) {
    stat_m[wave][r32] = m_run;
    stat_l[wave][r32] = l_wave;
  }
  __syncthreads();  // (also: every wave is done with its V^T image, which the merge buffer overlays)
  float m_all = -INFINITY;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) m_all = fmaxf(m_all, stat_m[w][r32]);
  const float m_use = m_all == -INFINITY ? 0.0f : m_all;
  float l_all = 0.0f;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    const float mw = stat_m[w][r32];
    l_all += mw == -INFINITY ? 0.0f : __expf(mw - m_use) * stat_l[w][r32];
  }
  const float mine = m_run == -INFINITY ? 0.0f : __expf(m_run - m_use);
  float* merge = reinterpret_cast<float*>(body);
  if (wave != 0) {
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
      for (int e = 0; e < 16; ++e) merge[(((wave - 1) * DB + db) * 16 + e) * 64 + lane] = o[db][e] * mine;
  }
  __syncthreads();
  if (wave != 0 || !row_ok) return;
#pragma unroll
  for (int db = 0; db < DB; ++db)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      float acc = o[db][e] * mine;
#pragma unroll
      for (int w = 0; w < kWaves - 1; ++w) acc += merge[((w * DB + db) * 16 + e) * 64 + lane];
      o[db][e] = acc;
    }
  // O^T lane (r32 = row, h): d = 32 db + (e & 3) + 8 (e >> 2) + 4 h
  const int64_t part = (int64_t)blockIdx.x * a.rows + r32;
  if (h == 0) {
    a.ws_m[part] = m_all;
    a.ws_l[part] = l_all;
  }
#pragma unroll
  for (int db = 0; db < DB; ++db)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const dc_f32x4 w = {o[db][4 * rr], o[db][4 * rr + 1], o[db][4 * rr + 2], o[db][4 * rr + 3]};
      *reinterpret_cast<dc_f32x4*>(a.ws_o + part * E + 32 * db + 8 * rr + 4 * (int)h) = w;
    }
}

template <int E, bool F16>
__global__ __launch_bounds__(kThreads) void sdpa_decode_partial_kernel(DecodeArgs a) {
  decode_partial<E, F16, false>(a);
}

// (its name holds neither "sdpa_decode_partial_kernel" nor "sdpa_decode_combine_kernel": tests count the dense kernels by those)
template <int E, bool F16>
__global__ __launch_bounds__(kThreads) void kv_paged_partial_kernel(PagedDecodeArgs a) {
  decode_partial<E, F16, true>(a);
}

// (its name holds none of the names the dense and the paged kernels are counted by)
template <int E, bool F16>
__global__ __launch_bounds__(kThreads) void kv_token_partial_kernel(TokenDecodeArgs a) {
  decode_partial<E, F16, false, true>(a);
}

// (its name holds none of the names the other three are counted by)
template <int E, bool F16>
__global__ __launch_bounds__(kThreads) void kv_paged_token_partial_kernel(PagedTokenDecodeArgs a) {
  decode_partial<E, F16, true, true>(a);
}

struct CombineArgs {
  const float* ws_o;
  const float* ws_m;
  const float* ws_l;
  uint16_t* out;
  int32_t H, HKV, L, E, rows, splits;
  const float* out_scale;   // nullptr: no output quantizer
  const float* out_offset;  // nullable
  float lo, hi;
};

template <bool F16>
__global__ __launch_bounds__(128) void sdpa_decode_combine_kernel(CombineArgs a) {
  const uint32_t d = threadIdx.x;
  if ((int32_t)d >= a.E) return;
  const uint32_t l = blockIdx.x % (uint32_t)a.L, bh = blockIdx.x / (uint32_t)a.L;
  const uint32_t head = bh % (uint32_t)a.H, b = bh / (uint32_t)a.H;
  const uint32_t G = (uint32_t)a.H / (uint32_t)a.HKV;
  const uint32_t kvh = head / G, r = (head % G) * (uint32_t)a.L + l;
  const int64_t first = ((int64_t)b * a.HKV + kvh) * a.splits;
  float m = -INFINITY;
  for (int32_t i = 0; i < a.splits; ++i) m = fmaxf(m, a.ws_m[(first + i) * a.rows + r]);
  float x = 0.0f;
  if (m != -INFINITY) {
    float num = 0.0f, den = 0.0f;
    for (int32_t i = 0; i < a.splits; ++i) {
      const int64_t part = (first + i) * a.rows + r;
      const float mi = a.ws_m[part];
      if (mi == -INFINITY) continue;
      const float f = expf(mi - m);
      num += f * a.ws_o[part * a.E + d];
      den += f * a.ws_l[part];
    }
    x = num / den;
  }
  if (a.out_scale) {  // A1 then A2 on the fp32 value
    const float s = a.out_scale[0], o = a.out_offset ? rne(a.out_offset[0]) : 0.0f;
    const float code = __builtin_amdgcn_fmed3f(rne(x / s - o), a.lo, a.hi);
    x = (code + o) * s;
  }
  a.out[(((int64_t)b * a.H + head) * a.L + l) * a.E + d] = from_f32<F16>(x);
}

// ---- the split plan ----------------------------------------------------------------------------------------------------------
constexpr int64_t kCap = FFQ_SDPA_DECODE_MAX_SPLITS;
constexpr int64_t kTargetGroups = 256;    // workgroups wanted: one per CU (E = 128 holds one workgroup per CU; docs/kernels.md: the sweep)
constexpr int64_t kMinTilesPerSplit = 2;  // a split shorter than 256 keys pays more for its merge and its partial than it streams

int64_t tiles_of(int64_t S) { return (S + kTile - 1) / kTile; }

int64_t plan_splits(int64_t batch, int64_t kv_heads, int64_t S) {
  const int64_t tiles = tiles_of(S), groups = batch * kv_heads;
  if (tiles <= 0 || groups <= 0) return 1;
  int64_t want = (kTargetGroups + groups - 1) / groups;
  const int64_t most = tiles / kMinTilesPerSplit;
  if (want > most) want = most;
  if (want > kCap) want = kCap;
  if (want < 1) want = 1;
  const int64_t per = (tiles + want - 1) / want;
  return (tiles + per - 1) / per;  // no split without a key
}

size_t workspace_bytes(int64_t batch, int64_t kv_heads, int64_t rows, int64_t E, int64_t splits) {
  return (size_t)(batch * kv_heads * splits * rows * (E + 2)) * sizeof(float);
}

// ---- one decode call, and each rule of the three entry points once ----------------------------------------------------------------
// What ffq_sdpa_decode, ffq_kv_decode and ffq_kv_paged_decode fill from their own parameter lists: the rules below read it and
// enqueue() launches from it. A member with an initialiser is one that only some entry points have.
struct DecodeCall {
  const void* q;
  const void* k;  // k / v: the codes [B, HKV, keys, E], or (paging) the two pools with the strides of (page, head, row)
  const void* v;
  int q_dt, dt;
  const float* const* deq_scale;
  const float* const* deq_offset;
  int64_t batch, q_heads, kv_heads, L, E, keys;  // keys: S, S_max or max_pages * P
  const int64_t* strides;
  const int32_t* lens = nullptr;  // nullptr: `keys` keys for every batch; else the device-side counts, `keys` their cap, MASK_CAUSAL bottom-right
  const void* mask = nullptr;
  const int64_t* mask_strides = nullptr;
  int mask_kind = MASK_NONE, mask_dt = FFQ_F32;
  double sqrt_scale, out_num_bits;
  const float* out_scale;
  const float* out_offset;
  // splits and plan_len as given (0: the rule, over plan_len or, 0 again, `keys` keys); nsplit: the count check_layout_and_workspace settles
  int64_t splits, plan_len = 0, nsplit = 0;
  void* out;
  void* workspace;
  size_t workspace_bytes;
  const Paging* paging = nullptr;
  const float* params = nullptr;  // (ffq_kv_token_decode, ffq_kv_paged_token_decode) the per-position store or pool and its three strides
  const int64_t* param_strides = nullptr;
};

int64_t rows_of(const DecodeCall& c) { return c.L * (c.q_heads / c.kv_heads); }

// Each rule takes the entry point's name for its message and returns the first failing status; an entry point calls them in the order
// its error table pins (tests/test_sdpa_decode_cpu.py, test_kv_cache_cpu.py, test_kv_paged_cpu.py) with its own steps in between.
// The value dtype, q's container, the argument tables, the scales, E and the extents
int check_operands(const char* name, const DecodeCall& c) {
  if (c.dt != FFQ_BF16 && c.dt != FFQ_F16) return fail(FFQ_ERR_DTYPE, "%s: bf16 or fp16 values", name);
  if (c.q_dt != c.dt && c.q_dt != FFQ_I8) return fail(FFQ_ERR_DTYPE, "%s: q is held in the value dtype or in int8", name);
  if (!c.strides || !c.deq_scale || !c.deq_offset) return fail(FFQ_ERR_ARG, "%s: NULL argument table", name);
  if (c.q_dt == FFQ_I8 && !c.deq_scale[0]) return fail(FFQ_ERR_DTYPE, "%s: int8 q codes need their scale", name);
  if (!c.deq_scale[1] || !c.deq_scale[2]) return fail(FFQ_ERR_ARG, "%s: k and v are int8 codes and need their scales", name);
  if (c.E != 64 && c.E != 128) return fail(FFQ_ERR_ARG, "%s: E must be 64 or 128", name);
  if (c.batch < 0 || c.L < 0 || c.keys < 0 || c.q_heads <= 0 || c.kv_heads <= 0 || c.q_heads % c.kv_heads) return fail(FFQ_ERR_ARG, "%s: bad extent", name);
  return FFQ_OK;
}

// The query rows of one kv head fit the one MFMA tile
int check_rows(const char* name, const DecodeCall& c) {
  if (c.L > kRows || rows_of(c) > kRows) return fail(FFQ_ERR_ARG, "%s: L * (q_heads / kv_heads) must be <= %d", name, kRows);
  return FFQ_OK;
}

// The output quantizer and the forced split count
int check_quantizer_and_splits(const char* name, const DecodeCall& c) {
  if (!c.out_scale && c.out_offset) return fail(FFQ_ERR_ARG, "%s: an output offset needs its scale", name);
  if (c.out_scale && !(c.out_num_bits >= 1.0 && c.out_num_bits <= 8.0 && c.out_num_bits == (double)(int)c.out_num_bits))
    return fail(FFQ_ERR_ARG, "%s: the output quantizer needs an integral bit-width in 1..8", name);
  if (c.splits < 0 || c.splits > kCap) return fail(FFQ_ERR_ARG, "%s: splits must be 0 (the rule) or 1..%d", name, (int)kCap);
  return FFQ_OK;
}

// The sizes the kernels' 32-bit fields hold, then the buffers every entry point has; `others`: the entry point's own are there too
int check_sizes_and_buffers(const char* name, const DecodeCall& c, bool others = true) {
  if (c.keys >= ((int64_t)1 << 30) || c.batch * c.kv_heads >= ((int64_t)1 << 24)) return fail(FFQ_ERR_ARG, "%s: too large", name);
  if (!c.q || !c.k || !c.v || !c.out || !others) return fail(FFQ_ERR_ARG, "%s: NULL buffer", name);
  return FFQ_OK;
}

// Alignment (`words_aligned`, `words`: the entry point's own 4-byte tables and how its message names them), the nine strides, then
// the split count (c.nsplit) and the workspace it needs
int check_layout_and_workspace(const char* name, DecodeCall& c, bool words_aligned = true, const char* words = "") {
  if (!aligned16(c.q) || !aligned16(c.k) || !aligned16(c.v) || !aligned16(c.out) || !words_aligned)
    return fail(FFQ_ERR_ARG, "%s: buffers must be 16-byte aligned%s", name, words);
  const int64_t q_unit = c.q_dt == FFQ_I8 ? 16 : 8;  // elements per 16 bytes
  for (int i = 0; i < 9; ++i)
    if (c.strides[i] < 0 || c.strides[i] % (i < 3 ? q_unit : 16)) return fail(FFQ_ERR_ARG, "%s: strides must be non-negative multiples of 16 bytes", name);
  c.nsplit = c.splits ? c.splits : plan_splits(c.batch, c.kv_heads, c.plan_len ? c.plan_len : c.keys);
  const size_t need = workspace_bytes(c.batch, c.kv_heads, rows_of(c), c.E, c.nsplit);
  if (!c.workspace || !aligned16(c.workspace) || c.workspace_bytes < need)
    return fail(FFQ_ERR_WORKSPACE, "%s: the workspace needs %zu bytes, 16-byte aligned (got %zu)", name, need, c.workspace_bytes);
  return FFQ_OK;
}

// The three strides of the parameter store (c.param_strides), `store` as the entry point names it
int check_param_strides(const char* name, const DecodeCall& c, const char* store) {
  for (int i = 0; i < 3; ++i)
    if (c.param_strides[i] < 0 || c.param_strides[i] % 4)
      return fail(FFQ_ERR_ARG, "%s: the strides of %s must be non-negative multiples of 16 bytes", name, store);
  return FFQ_OK;
}

// one partial launch: `f16` / `bf16` are the two instantiations of one of the four partial kernels at the call's E
template <typename Args>
void launch_partial(void (*f16)(Args), void (*bf16)(Args), bool is_f16, const Args& a, unsigned blocks, hipStream_t s) {
  auto kernel = is_f16 ? f16 : bf16;
  kernel<<<blocks, kThreads, 0, s>>>(a);
}

// the two launches, after an entry point's checks
int enqueue(const DecodeCall& c, hipStream_t s) {
  const int64_t rows = rows_of(c), parts = c.batch * c.kv_heads * c.nsplit;
  PagedDecodeArgs a;  // (the dense kernels take its DecodeArgs)
  a.q = c.q; a.k = static_cast<const int8_t*>(c.k); a.v = static_cast<const int8_t*>(c.v);
  for (int i = 0; i < 3; ++i) {
    a.deq_s[i] = c.deq_scale[i];
    a.deq_o[i] = c.deq_scale[i] ? c.deq_offset[i] : nullptr;
    a.qs[i] = c.strides[i]; a.ks[i] = c.strides[3 + i]; a.vs[i] = c.strides[6 + i];
  }
  a.B = (int32_t)c.batch; a.H = (int32_t)c.q_heads; a.HKV = (int32_t)c.kv_heads; a.L = (int32_t)c.L; a.S = (int32_t)c.keys;
  a.rows = (int32_t)rows; a.splits = (int32_t)c.nsplit; a.tiles_per_split = (int32_t)((tiles_of(c.keys) + c.nsplit - 1) / c.nsplit);
  a.q_i8 = c.q_dt == FFQ_I8;
  a.mask = c.mask; a.mask_kind = c.mask_kind; a.mask_dt = c.mask_dt;
  for (int i = 0; i < 4; ++i) a.ms[i] = c.mask_kind >= MASK_BOOL ? c.mask_strides[i] : 0;
  a.c = (float)c.sqrt_scale;
  a.lens = c.lens;
  a.ws_o = static_cast<float*>(c.workspace);
  a.ws_m = a.ws_o + parts * rows * c.E;
  a.ws_l = a.ws_m + parts * rows;
  a.pg = c.paging ? *c.paging : Paging{};
  const bool f16 = c.dt == FFQ_F16;
  if (c.params) {
    PagedTokenDecodeArgs t;  // (the dense token kernels take its TokenDecodeArgs)
    static_cast<DecodeArgs&>(t) = a;
    t.params = c.params;
    for (int i = 0; i < 3; ++i) t.ps[i] = c.param_strides[i];
    t.pg = a.pg;
    if (c.paging && c.E == 64) launch_partial(kv_paged_token_partial_kernel<64, true>, kv_paged_token_partial_kernel<64, false>, f16, t, (unsigned)parts, s);
    else if (c.paging) launch_partial(kv_paged_token_partial_kernel<128, true>, kv_paged_token_partial_kernel<128, false>, f16, t, (unsigned)parts, s);
    else if (c.E == 64) launch_partial<TokenDecodeArgs>(kv_token_partial_kernel<64, true>, kv_token_partial_kernel<64, false>, f16, t, (unsigned)parts, s);
    else launch_partial<TokenDecodeArgs>(kv_token_partial_kernel<128, true>, kv_token_partial_kernel<128, false>, f16, t, (unsigned)parts, s);
  } else if (c.paging && c.E == 64) launch_partial(kv_paged_partial_kernel<64, true>, kv_paged_partial_kernel<64, false>, f16, a, (unsigned)parts, s);
  else if (c.paging) launch_partial(kv_paged_partial_kernel<128, true>, kv_paged_partial_kernel<128, false>, f16, a, (unsigned)parts, s);
  else if (c.E == 64) launch_partial<DecodeArgs>(sdpa_decode_partial_kernel<64, true>, sdpa_decode_partial_kernel<64, false>, f16, a, (unsigned)parts, s);
  else launch_partial<DecodeArgs>(sdpa_decode_partial_kernel<128, true>, sdpa_decode_partial_kernel<128, false>, f16, a, (unsigned)parts, s);
  if (int rc = check_launch(c.params && c.paging ? "kv_paged_token_partial_kernel" : c.params ? "kv_token_partial_kernel" : c.paging ? "kv_paged_partial_kernel" : "sdpa_decode_partial_kernel")) return rc;

  CombineArgs m;
  m.ws_o = a.ws_o; m.ws_m = a.ws_m; m.ws_l = a.ws_l;
  m.out = static_cast<uint16_t*>(c.out);
  m.H = a.H; m.HKV = a.HKV; m.L = a.L; m.E = (int32_t)c.E; m.rows = a.rows; m.splits = a.splits;
  m.out_scale = c.out_scale; m.out_offset = c.out_scale ? c.out_offset : nullptr;
  const double half = c.out_scale ? ldexp(1.0, (int)c.out_num_bits - 1) : 1.0;
  m.lo = (float)-half; m.hi = (float)(half - 1.0);
  const unsigned cblocks = (unsigned)(c.batch * c.q_heads * c.L);
  if (f16) sdpa_decode_combine_kernel<true><<<cblocks, 128, 0, s>>>(m);
  else sdpa_decode_combine_kernel<false><<<cblocks, 128, 0, s>>>(m);
  return check_launch("sdpa_decode_combine_kernel");
}

}  // namespace
}  // namespace ffq

using namespace ffq;

extern "C" int64_t ffq_sdpa_decode_splits(int64_t batch, int64_t kv_heads, int64_t S, int64_t rows, int64_t E) {
  (void)rows;
  (void)E;  // (in the signature so that the rule can come to depend on them without a new entry point)
  return plan_splits(batch, kv_heads, S);
}

extern "C" size_t ffq_sdpa_decode_workspace_bytes(int64_t batch, int64_t kv_heads, int64_t rows, int64_t E, int64_t splits) {
  if (batch <= 0 || kv_heads <= 0 || rows <= 0 || E <= 0 || splits <= 0) return 0;
  return workspace_bytes(batch, kv_heads, rows, E, splits);
}

extern "C" int ffq_sdpa_decode(const void* q, int q_dt, const void* k, const void* v, int dt, const float* const* deq_scale,
                               const float* const* deq_offset, int64_t batch, int64_t q_heads, int64_t kv_heads, int64_t L, int64_t S,
                               int64_t E, const int64_t* strides, const void* mask, int mask_kind, int mask_dt, const int64_t* mask_strides,
                               double sqrt_scale, const float* out_scale, const float* out_offset, double out_num_bits, int64_t splits,
                               void* out, void* workspace, size_t workspace_bytes_given, void* stream) {
  DecodeCall c;
  c.q = q; c.q_dt = q_dt; c.k = k; c.v = v; c.dt = dt; c.deq_scale = deq_scale; c.deq_offset = deq_offset;
  c.batch = batch; c.q_heads = q_heads; c.kv_heads = kv_heads; c.L = L; c.keys = S; c.E = E; c.strides = strides;
  c.mask = mask; c.mask_kind = mask_kind; c.mask_dt = mask_dt; c.mask_strides = mask_strides;
  c.sqrt_scale = sqrt_scale; c.out_scale = out_scale; c.out_offset = out_offset; c.out_num_bits = out_num_bits;
  c.splits = splits; c.out = out; c.workspace = workspace; c.workspace_bytes = workspace_bytes_given;
  if (int rc = check_operands("sdpa_decode", c)) return rc;
  if (int rc = check_rows("sdpa_decode", c)) return rc;
  if (mask_kind < MASK_NONE || mask_kind > MASK_FLOAT) return fail(FFQ_ERR_ARG, "sdpa_decode: bad mask kind");
  if (mask_kind == MASK_FLOAT && mask_dt != FFQ_F32 && mask_dt != FFQ_BF16 && mask_dt != FFQ_F16) return fail(FFQ_ERR_DTYPE, "sdpa_decode: float mask dtype");
  if (int rc = check_quantizer_and_splits("sdpa_decode", c)) return rc;
  if (batch == 0 || L == 0) return FFQ_OK;
  if (S == 0) return fail(FFQ_ERR_ARG, "sdpa_decode: S must be >= 1");
  if (int rc = check_sizes_and_buffers("sdpa_decode", c)) return rc;
  if (mask_kind >= MASK_BOOL && (!mask || !mask_strides)) return fail(FFQ_ERR_ARG, "sdpa_decode: the mask needs its data and strides");
  if (int rc = check_layout_and_workspace("sdpa_decode", c)) return rc;
  return enqueue(c, static_cast<hipStream_t>(stream));
}

extern "C" int ffq_kv_decode(const void* q, int q_dt, const void* k, const void* v, int dt, const float* const* deq_scale,
                             const float* const* deq_offset, const void* lens, int64_t batch, int64_t q_heads, int64_t kv_heads, int64_t L,
                             int64_t S_max, int64_t E, const int64_t* strides, int causal, double sqrt_scale, const float* out_scale,
                             const float* out_offset, double out_num_bits, int64_t splits, int64_t plan_len, void* out, void* workspace,
                             size_t workspace_bytes_given, void* stream) {
  DecodeCall c;
  c.q = q; c.q_dt = q_dt; c.k = k; c.v = v; c.dt = dt; c.deq_scale = deq_scale; c.deq_offset = deq_offset;
  c.batch = batch; c.q_heads = q_heads; c.kv_heads = kv_heads; c.L = L; c.keys = S_max; c.E = E; c.strides = strides;
  c.lens = static_cast<const int32_t*>(lens); c.mask_kind = causal ? MASK_CAUSAL : MASK_NONE;
  c.sqrt_scale = sqrt_scale; c.out_scale = out_scale; c.out_offset = out_offset; c.out_num_bits = out_num_bits;
  c.splits = splits; c.plan_len = plan_len; c.out = out; c.workspace = workspace; c.workspace_bytes = workspace_bytes_given;
  if (int rc = check_operands("kv_decode", c)) return rc;
  if (int rc = check_rows("kv_decode", c)) return rc;
  if (causal != 0 && causal != 1) return fail(FFQ_ERR_ARG, "kv_decode: causal is 0 (every key) or 1 (bottom-right)");
  if (int rc = check_quantizer_and_splits("kv_decode", c)) return rc;
  if (plan_len < 0 || plan_len > S_max) return fail(FFQ_ERR_ARG, "kv_decode: plan_len must be 0 (S_max) or 1..S_max");
  if (batch == 0 || L == 0) return FFQ_OK;
  if (S_max == 0) return fail(FFQ_ERR_ARG, "kv_decode: S_max must be >= 1");
  if (int rc = check_sizes_and_buffers("kv_decode", c, lens != nullptr)) return rc;
  if (int rc = check_layout_and_workspace("kv_decode", c, aligned4(lens), " (lens: 4-byte)")) return rc;
  return enqueue(c, static_cast<hipStream_t>(stream));
}

extern "C" int ffq_kv_paged_decode(const void* q, int q_dt, const void* k_pool, const void* v_pool, int dt, const float* const* deq_scale,
                                   const float* const* deq_offset, const void* lens, const void* block_table, int64_t batch, int64_t q_heads,
                                   int64_t kv_heads, int64_t L, int64_t num_pages, int64_t P, int64_t max_pages, int64_t table_stride, int64_t E,
                                   const int64_t* strides, int causal, double sqrt_scale, const float* out_scale, const float* out_offset,
                                   double out_num_bits, int64_t splits, int64_t plan_len, void* out, void* workspace,
                                   size_t workspace_bytes_given, void* stream) {
  DecodeCall c;
  c.q = q; c.q_dt = q_dt; c.k = k_pool; c.v = v_pool; c.dt = dt; c.deq_scale = deq_scale; c.deq_offset = deq_offset;
  c.batch = batch; c.q_heads = q_heads; c.kv_heads = kv_heads; c.L = L; c.keys = 0; c.E = E; c.strides = strides;  // (keys: once the geometry is sound)
  c.lens = static_cast<const int32_t*>(lens); c.mask_kind = causal ? MASK_CAUSAL : MASK_NONE;
  c.sqrt_scale = sqrt_scale; c.out_scale = out_scale; c.out_offset = out_offset; c.out_num_bits = out_num_bits;
  c.splits = splits; c.plan_len = plan_len; c.out = out; c.workspace = workspace; c.workspace_bytes = workspace_bytes_given;
  if (int rc = check_operands("kv_paged_decode", c)) return rc;
  if (const char* why = paging_error(num_pages, P, max_pages, table_stride)) return fail(FFQ_ERR_ARG, "kv_paged_decode: %s", why);
  c.keys = max_pages * P;  // a sequence's capacity, in the place of S_max (below 2^30)
  if (int rc = check_rows("kv_paged_decode", c)) return rc;
  if (causal != 0 && causal != 1) return fail(FFQ_ERR_ARG, "kv_paged_decode: causal is 0 (every key) or 1 (bottom-right)");
  if (int rc = check_quantizer_and_splits("kv_paged_decode", c)) return rc;
  if (plan_len < 0 || plan_len > c.keys) return fail(FFQ_ERR_ARG, "kv_paged_decode: plan_len must be 0 (max_pages * P) or 1..max_pages * P");
  if (batch == 0 || L == 0) return FFQ_OK;
  if (int rc = check_sizes_and_buffers("kv_paged_decode", c, lens && block_table)) return rc;
  if (int rc = check_layout_and_workspace("kv_paged_decode", c, aligned4(lens) && aligned4(block_table), " (lens, block_table: 4-byte)")) return rc;
  const Paging paging = {static_cast<const int32_t*>(block_table), table_stride, (int32_t)num_pages, page_shift_of(P)};
  c.paging = &paging;
  return enqueue(c, static_cast<hipStream_t>(stream));
}

extern "C" int ffq_kv_token_decode(const void* q, int q_dt, const void* k, const void* v, int dt, const float* q_scale, const float* q_offset,
                                   const void* params, const void* lens, int64_t batch, int64_t q_heads, int64_t kv_heads, int64_t L, int64_t S_max,
                                   int64_t E, const int64_t* strides, int causal, double sqrt_scale, const float* out_scale, const float* out_offset,
                                   double out_num_bits, int64_t splits, int64_t plan_len, void* out, void* workspace, size_t workspace_bytes_given,
                                   void* stream) {
  // the tables of the shared rules: the query's own pair, and the store in the place of the scales of k and v (it holds them)
  const float* const deq_scale[3] = {q_scale, static_cast<const float*>(params), static_cast<const float*>(params)};
  const float* const deq_offset[3] = {q_offset, nullptr, nullptr};
  DecodeCall c;
  c.q = q; c.q_dt = q_dt; c.k = k; c.v = v; c.dt = dt; c.deq_scale = deq_scale; c.deq_offset = deq_offset;
  c.batch = batch; c.q_heads = q_heads; c.kv_heads = kv_heads; c.L = L; c.keys = S_max; c.E = E; c.strides = strides;
  c.lens = static_cast<const int32_t*>(lens); c.mask_kind = causal ? MASK_CAUSAL : MASK_NONE;
  c.sqrt_scale = sqrt_scale; c.out_scale = out_scale; c.out_offset = out_offset; c.out_num_bits = out_num_bits;
  c.splits = splits; c.plan_len = plan_len; c.out = out; c.workspace = workspace; c.workspace_bytes = workspace_bytes_given;
  c.params = static_cast<const float*>(params); c.param_strides = strides ? strides + 12 : nullptr;
  if (int rc = check_operands("kv_token_decode", c)) return rc;
  if (int rc = check_rows("kv_token_decode", c)) return rc;
  if (causal != 0 && causal != 1) return fail(FFQ_ERR_ARG, "kv_token_decode: causal is 0 (every key) or 1 (bottom-right)");
  if (int rc = check_quantizer_and_splits("kv_token_decode", c)) return rc;
  if (plan_len < 0 || plan_len > S_max) return fail(FFQ_ERR_ARG, "kv_token_decode: plan_len must be 0 (S_max) or 1..S_max");
  if (batch == 0 || L == 0) return FFQ_OK;
  if (S_max == 0) return fail(FFQ_ERR_ARG, "kv_token_decode: S_max must be >= 1");
  if (int rc = check_sizes_and_buffers("kv_token_decode", c, lens != nullptr)) return rc;
  if (int rc = check_param_strides("kv_token_decode", c, "params")) return rc;
  if (int rc = check_layout_and_workspace("kv_token_decode", c, aligned16(params) && aligned4(lens), " (lens: 4-byte)")) return rc;
  return enqueue(c, static_cast<hipStream_t>(stream));
}

extern "C" int ffq_kv_paged_token_decode(const void* q, int q_dt, const void* k_pool, const void* v_pool, int dt, const float* q_scale,
                                         const float* q_offset, const void* param_pool, const void* lens, const void* block_table, int64_t batch,
                                         int64_t q_heads, int64_t kv_heads, int64_t L, int64_t num_pages, int64_t P, int64_t max_pages,
                                         int64_t table_stride, int64_t E, const int64_t* strides, int causal, double sqrt_scale,
                                         const float* out_scale, const float* out_offset, double out_num_bits, int64_t splits, int64_t plan_len,
                                         void* out, void* workspace, size_t workspace_bytes_given, void* stream) {
  // the tables of the shared rules, as in ffq_kv_token_decode: the pool in the place of the scales of k and v (it holds them)
  const float* const deq_scale[3] = {q_scale, static_cast<const float*>(param_pool), static_cast<const float*>(param_pool)};
  const float* const deq_offset[3] = {q_offset, nullptr, nullptr};
  DecodeCall c;
  c.q = q; c.q_dt = q_dt; c.k = k_pool; c.v = v_pool; c.dt = dt; c.deq_scale = deq_scale; c.deq_offset = deq_offset;
  c.batch = batch; c.q_heads = q_heads; c.kv_heads = kv_heads; c.L = L; c.keys = 0; c.E = E; c.strides = strides;  // (keys: once the geometry is sound)
  c.lens = static_cast<const int32_t*>(lens); c.mask_kind = causal ? MASK_CAUSAL : MASK_NONE;
  c.sqrt_scale = sqrt_scale; c.out_scale = out_scale; c.out_offset = out_offset; c.out_num_bits = out_num_bits;
  c.splits = splits; c.plan_len = plan_len; c.out = out; c.workspace = workspace; c.workspace_bytes = workspace_bytes_given;
  c.params = static_cast<const float*>(param_pool); c.param_strides = strides ? strides + 12 : nullptr;
  if (int rc = check_operands("kv_paged_token_decode", c)) return rc;
  if (const char* why = paging_error(num_pages, P, max_pages, table_stride)) return fail(FFQ_ERR_ARG, "kv_paged_token_decode: %s", why);
  c.keys = max_pages * P;  // a sequence's capacity, in the place of S_max (below 2^30)
  if (int rc = check_rows("kv_paged_token_decode", c)) return rc;
  if (causal != 0 && causal != 1) return fail(FFQ_ERR_ARG, "kv_paged_token_decode: causal is 0 (every key) or 1 (bottom-right)");
  if (int rc = check_quantizer_and_splits("kv_paged_token_decode", c)) return rc;
  if (plan_len < 0 || plan_len > c.keys) return fail(FFQ_ERR_ARG, "kv_paged_token_decode: plan_len must be 0 (max_pages * P) or 1..max_pages * P");
  if (batch == 0 || L == 0) return FFQ_OK;
  if (int rc = check_sizes_and_buffers("kv_paged_token_decode", c, lens && block_table)) return rc;
  if (int rc = check_param_strides("kv_paged_token_decode", c, "param_pool")) return rc;
  if (int rc = check_layout_and_workspace("kv_paged_token_decode", c, aligned16(param_pool) && aligned4(lens) && aligned4(block_table),
                                          " (lens, block_table: 4-byte)"))
    return rc;
  const Paging paging = {static_cast<const int32_t*>(block_table), table_stride, (int32_t)num_pages, page_shift_of(P)};
  c.paging = &paging;
  return enqueue(c, static_cast<hipStream_t>(stream));
}
