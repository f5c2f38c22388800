// ffq_sdpa.hip — ff.nn.functional.scaled_dot_product_attention with its eight quantizers in one launch, plus a small first one
// that writes the scaled-K codes when that quantizer is active (reference
// nn/functional/custom/sdpa.py:116-285, ATen's math SDPA after an fp32 upcast with a quantizer after every step). The chain
// materialises the [B, H, L, S] fp32 scores five to seven times; here nothing of that size leaves the registers.
//
// One workgroup = 4 waves = 128 query rows of one (batch, query head); a wave owns 32 rows. K (and V) tiles of 64 keys are
// register-staged: the next tile's loads are in flight while this tile's matrix work runs (one LDS buffer, two barriers per tile).
//   * scores transposed, as in ffq_attention.hip: S^T[key][query] = mfma_32x32x16(A = K rows, B = Q rows), so a lane holds one
//     query row's 32 keys of the tile and the row statistics are lane-local plus one cross-half exchange;
//   * context transposed: O^T[d][query] = mfma(A = V^T, B = P) with P in the score registers and V^T from a transposed LDS image
//     (written once per staged tile, read with two 8-byte loads per fragment);
//   * every elementwise quantizer acts in registers with the arithmetic of ffq_affine.h on fp32 values: scaled q (once, on the
//     Q fragments) and scaled k (once per call, by sdpa_key_codes_kernel), scores, mask and masked scores (per score);
//   * with a scaled-q / scaled-k quantizer the MFMA receives the codes (|code| <= 128: exact in bf16 and fp16 for any offset); the
//     offsets enter through per-row / per-key sums of the codes, and the scales multiply the fp32 sum afterwards. The probability
//     integers code + round(offset) of the weights / dropout quantizers are split into up to three exact parts (one MFMA each) when
//     the quantizer's range goes beyond the integers the dtype holds exactly (bf16: 256, fp16: 2048) — decided in the kernel from
//     the parameters, so the choice is graph-safe;
//   * MODE 0 (no weights and no dropout quantizer): online softmax, one pass over the keys, O / l at the end;
//     MODE 1: pass 1 takes each row's max m and sum l of exp(x - m), pass 2 recomputes the scores and forms p = exp(x - m) / l,
//     quantizes it (weights, then dropout) and accumulates P V — about 1.5x the flops of MODE 0, in the same launch;
//   * the safe softmax: a row whose masked scores are all <= neg_inf gives exactly 0; keys >= S and query rows >= L are masked
//     out in registers (no out-of-bounds access);
//   * causal (top-left tril): tiles entirely above a wave's rows are skipped when their masked value is -inf (no mask /
//     masked-scores quantizer, neg_inf = -inf) and a probability of 0 stays 0 through the weights / dropout quantizers;
//     heavy query blocks are dispatched first.
#include "ffq_affine.h"
#include "ffq_common.h"
#include "ffq_vec.h"

#include <math.h>

namespace ffq {
namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 sd_bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 sd_f16x8;
typedef __attribute__((ext_vector_type(16))) float sd_f32x16;
typedef __attribute__((ext_vector_type(4))) short sd_s16x4;

constexpr int kWaves = 4;
constexpr int kThreads = kWaves * 64;
constexpr int kRows = 32;                 // query rows per wave
constexpr int kQBlock = kWaves * kRows;   // 128 query rows per workgroup
constexpr int kKeys = 64;                 // keys per tile
constexpr int kKPitch = 256;              // bytes per K row in LDS (16 swizzled 16-byte slots; E = 64 uses the first 8 columns)
constexpr int kVtPitch = 136;             // bytes per column of the V^T image in LDS (64 keys + 8 bytes of skew)
constexpr int kNQ = FFQ_SDPA_QUANTIZERS;  // quantizer slots, in the order of include/ffq.h

enum {
  QS_SCORES = FFQ_SDPA_SCORES, QS_MASK = FFQ_SDPA_MASK, QS_MASKED = FFQ_SDPA_MASKED, QS_WEIGHTS = FFQ_SDPA_WEIGHTS,
  QS_QUERY = FFQ_SDPA_QUERY, QS_KEY = FFQ_SDPA_KEY, QS_DROPOUT = FFQ_SDPA_DROPOUT, QS_OUTPUT = FFQ_SDPA_OUTPUT
};
enum { MASK_NONE = 0, MASK_CAUSAL, MASK_BOOL, MASK_FLOAT };

struct Quant {
  const float* scale;   // nullptr: inactive
  const float* offset;  // nullable
  float lo, hi;
};

struct SdpaArgs {
  const uint16_t* q;
  const uint16_t* k;
  const uint16_t* v;
  const float* deq_s[3];  // q / k / v codes: per-tensor dequantization (nullptr: plain values)
  const float* deq_o[3];
  int64_t qs[3], ks[3], vs[3];  // element strides of (batch, head, row)
  int32_t B, H, HKV, L, S;
  int32_t nqb;
  const void* mask;
  int32_t mask_kind, mask_dt;
  int64_t ms[4];  // element strides of the mask expanded to [B, H, L, S]
  float c;        // float(sqrt(scale))
  float neg_inf;  // float(neg_inf)
  int32_t skip;   // causal tiles above the diagonal may be skipped
  int32_t k_coded;  // k holds the scaled-K codes of sdpa_key_codes_kernel (contiguous): staged as they are
  Quant qz[kNQ];
  uint16_t* out;   // nullable: [B, H, L, E] in dt
  int8_t* codes;   // nullable: [B, H, L, E] codes of the output quantizer
};

// one active quantizer in registers: A1 then A2, both in fp32 (ffq_affine.h: rne(x / s - round(o)), clamp; (c + round(o)) * s)
struct QReg {
  float s, o, lo, hi;
  bool on;
  __device__ __forceinline__ void load(const Quant& q) {
    on = q.scale != nullptr;
    s = on ? q.scale[0] : 1.0f;
    o = (on && q.offset) ? rne(q.offset[0]) : 0.0f;
    lo = q.lo;
    hi = q.hi;
  }
  __device__ __forceinline__ float code(float x) const { return __builtin_amdgcn_fmed3f(rne(x / s - o), lo, hi); }
  __device__ __forceinline__ float integer(float x) const { return code(x) + o; }   // an integer; not always a small one
  __device__ __forceinline__ float fake(float x) const { return on ? integer(x) * s : x; }
};

// a row's flag from both lane halves (the exchange runs in every lane: no short-circuit around the shuffle)
__device__ __forceinline__ bool both_halves(bool flag) {
  const int other = __shfl_xor((int)flag, 32);
  return flag && other;
}

__device__ __forceinline__ float QReg_fake(const Quant& q, float x) {
  QReg r;
  r.load(q);
  return r.fake(x);
}

template <bool F16>
__device__ __forceinline__ float to_f32(uint16_t h) {
  return F16 ? f16_bits_to_f32(h) : bf16_bits_to_f32(h);
}
template <bool F16>
__device__ __forceinline__ uint16_t from_f32(float f) {
  return F16 ? f32_to_f16_bits(f) : f32_to_bf16_bits(f);
}

// the 8 values of one 16-byte slot as the MFMA gets them: codes of a quantized operand dequantized to dt, then (if `qz` is on)
// the CODE of the scaled value (|code| <= 128 for <= 8 bits: exact in bf16 and fp16 whatever the offset), else the value itself
template <bool F16>
__device__ __forceinline__ u32x4 transform(u32x4 w, bool deq, float ds, float dof, const QReg& qz, float c) {
  if (!deq && !qz.on) return w;
  uint32_t word[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    uint16_t h[2] = {(uint16_t)(word[i] & 0xFFFFu), (uint16_t)(word[i] >> 16)};
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      float x = to_f32<F16>(h[j]);
      if (deq) x = to_f32<F16>(from_f32<F16>((x + dof) * ds));  // the dequantized operand in its dtype
      if (qz.on) x = qz.code(x * c);                             // mul(x, sqrt(scale)) in fp32, then A1
      h[j] = from_f32<F16>(x);
    }
    word[i] = (uint32_t)h[0] | ((uint32_t)h[1] << 16);
  }
  return u32x4{word[0], word[1], word[2], word[3]};
}

// V^T fragment of one MFMA: lane (d, h) takes keys base + 4h + {0..3, 8..11} of column d — the keys its P fragment holds
// (the score layout of S^T): two 8-byte reads from the V^T image
// sum of the 8 values of one slot in fp32 (integers: exact)
template <bool F16>
__device__ __forceinline__ float sum8(u32x4 w) {
  const uint32_t word[4] = {w.x, w.y, w.z, w.w};
  float acc = 0.0f;
#pragma unroll
  for (int i = 0; i < 4; ++i) acc += to_f32<F16>((uint16_t)(word[i] & 0xFFFFu)) + to_f32<F16>((uint16_t)(word[i] >> 16));
  return acc;
}

// An integer n of the probability codes (code + round(offset)) as up to three MFMA operands whose sum is n exactly. parts and the
// power-of-two pre-scale (fp16 only: keeps every part below its largest finite value) follow from the quantizer's bound
// max(|lo + o|, |hi + o|): one part while every integer up to the bound is exact in the dtype (bf16: 256, fp16: 2048).
struct PSplit {
  int parts;
  float prescale;  // applied to n before the split; the epilogue divides it out
  template <bool F16>
  __device__ __forceinline__ void plan(const QReg& q) {
    const float bound = fmaxf(fabsf(q.lo + q.o), fabsf(q.hi + q.o));
    const int m = F16 ? 11 : 8;  // significant bits of the dtype
    int nb = 1;
    while (nb < 25 && ldexpf(1.0f, nb) <= bound) ++nb;  // |n| < 2^nb
    parts = bound <= ldexpf(1.0f, m) ? 1 : (nb + m - 1) / m;
    parts = parts > 3 ? 3 : parts;
    prescale = (F16 && bound > 32768.0f) ? ldexpf(1.0f, 15 - nb) : 1.0f;
  }
};

__device__ __forceinline__ sd_bf16x8 load_vt(const unsigned char* vbuf, uint32_t d, uint32_t key0) {
  const sd_s16x4 a = *reinterpret_cast<const sd_s16x4*>(vbuf + d * kVtPitch + key0 * 2);
  const sd_s16x4 b = *reinterpret_cast<const sd_s16x4*>(vbuf + d * kVtPitch + (key0 + 8) * 2);
  return __builtin_bit_cast(sd_bf16x8, __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7));
}

template <bool F16>
__device__ __forceinline__ sd_f32x16 mfma(sd_bf16x8 a, sd_bf16x8 b, sd_f32x16 c) {
  if constexpr (F16)
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(sd_f16x8, a), __builtin_bit_cast(sd_f16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

template <int D, int MODE, bool F16>
__global__ __launch_bounds__(kThreads) void sdpa_quantize_kernel(SdpaArgs a) {
  constexpr int T = D / 16;                    // MFMA k-steps of QK^T
  constexpr int DB = D / 32;                   // 32-column blocks of O^T
  constexpr int SLOTS = D / 8;                 // 16-byte slots per row
  constexpr int ROWS_PER_PASS = kThreads / SLOTS;
  constexpr int PASSES = kKeys / ROWS_PER_PASS;
  __shared__ __attribute__((aligned(16))) unsigned char kbuf[kKeys * kKPitch];
  __shared__ __attribute__((aligned(16))) unsigned char vbuf[128 * kVtPitch];
  __shared__ float ksum[kKeys];  // (scaled-q quantizer) sum over E of each staged key row as the MFMA sees it

  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t r32 = lane & 31, h = lane >> 5;

  // blockIdx -> (query block, heaviest first; batch; head)
  const uint32_t bh_count = (uint32_t)a.B * (uint32_t)a.H;
  const uint32_t qb = (uint32_t)a.nqb - 1 - blockIdx.x / bh_count;
  const uint32_t bh = blockIdx.x % bh_count;
  const uint32_t b = bh / (uint32_t)a.H, head = bh % (uint32_t)a.H;
  const uint32_t kvh = head / ((uint32_t)a.H / (uint32_t)a.HKV);
  const int32_t q0 = (int32_t)qb * kQBlock;
  const int32_t qw0 = q0 + (int32_t)wave * kRows;
  const int32_t qi = qw0 + (int32_t)r32;
  const bool row_ok = qi < a.L;
  const int32_t q_end = q0 + kQBlock < a.L ? q0 + kQBlock : a.L;
  // a skipped key must contribute nothing: its probability 0 has to stay 0 through the weights / dropout quantizers
  const float zero_image = QReg_fake(a.qz[QS_DROPOUT], QReg_fake(a.qz[QS_WEIGHTS], 0.0f));
  const bool skip = a.skip && zero_image == 0.0f;
  const int32_t key_end = (skip && q_end < a.S) ? q_end : a.S;
  const int32_t ntiles = (key_end + kKeys - 1) / kKeys;

  QReg qz[kNQ];
#pragma unroll
  for (int i = 0; i < kNQ; ++i) qz[i].load(a.qz[i]);
  const bool deq_q = a.deq_s[0] != nullptr, deq_k = a.deq_s[1] != nullptr, deq_v = a.deq_s[2] != nullptr;
  const float dqs = deq_q ? a.deq_s[0][0] : 1.0f, dqo = (deq_q && a.deq_o[0]) ? rne(a.deq_o[0][0]) : 0.0f;
  const float dks = deq_k ? a.deq_s[1][0] : 1.0f, dko = (deq_k && a.deq_o[1]) ? rne(a.deq_o[1][0]) : 0.0f;
  const float dvs = deq_v ? a.deq_s[2][0] : 1.0f, dvo = (deq_v && a.deq_o[2]) ? rne(a.deq_o[2][0]) : 0.0f;
  const QReg off{1.0f, 0.0f, 0.0f, 0.0f, false};
  const QReg& kquant = a.k_coded ? off : qz[QS_KEY];  // the scaled-K quantizer, unless its codes were written by the pre-pass
  const bool kdeq = deq_k && !a.k_coded;
  // The MFMA contracts y_q . y_k, where y is a side's code (quantizer on) or its plain value. With shifts o = round(offset) (0 for a
  // plain side) the integers of the chain are y + o, and
  //   sum (y_q + o_q)(y_k + o_k) = acc + o_k * sum(y_q) + o_q * sum(y_k) + E * o_q * o_k,
  // each term exact in fp32 for codes. The scores are that times alpha: each side's quantizer scale, or sqrt(scale) for a plain side.
  const float alpha = (qz[QS_QUERY].on ? qz[QS_QUERY].s : a.c) * (qz[QS_KEY].on ? qz[QS_KEY].s : a.c);
  const float shift_q = qz[QS_QUERY].o, shift_k = qz[QS_KEY].o;  // 0 when the quantizer is off
  // the two values of a causal / bool bias and their images under the mask quantizer
  const float b_keep = qz[QS_MASK].fake(0.0f), b_drop = qz[QS_MASK].fake(a.neg_inf);

  // ---- Q fragments: lane (r32, h) holds columns [(2t+h)*8, +8) of row qi
  sd_bf16x8 qf[T];
  float qsum = 0.0f;  // sum over E of this lane's half of its query row as the MFMA sees it
  {
    const uint16_t* qrow = a.q + (int64_t)b * a.qs[0] + (int64_t)head * a.qs[1] + (int64_t)(row_ok ? qi : 0) * a.qs[2];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      u32x4 w = *reinterpret_cast<const u32x4*>(qrow + (2 * t + h) * 8);
      w = transform<F16>(w, deq_q, dqs, dqo, qz[QS_QUERY], a.c);
      if (!row_ok) w = u32x4{0, 0, 0, 0};
      if (qz[QS_KEY].on) qsum += sum8<F16>(w);
      qf[t] = __builtin_bit_cast(sd_bf16x8, w);
    }
  }
  // the row's correction term of the scores (see alpha): o_k * sum(y_q) + E * o_q * o_k
  const float row_term = shift_k * (qsum + __shfl_xor(qsum, 32)) + (float)D * shift_q * shift_k;

  // ---- staging: thread -> (row srow + ROWS_PER_PASS p, slot sslot); rows >= S read nothing and stage zeros
  const uint32_t srow = tid / SLOTS, sslot = tid % SLOTS;
  const uint16_t* kbase = a.k + (int64_t)b * a.ks[0] + (int64_t)kvh * a.ks[1] + sslot * 8;
  const uint16_t* vbase = a.v + (int64_t)b * a.vs[0] + (int64_t)kvh * a.vs[1] + sslot * 8;
  u32x4 sk[PASSES], sv[PASSES];
  auto stage_load = [&](int32_t tile, bool with_v) {
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      const int32_t row = tile * kKeys + (int32_t)srow + ROWS_PER_PASS * p;
      sk[p] = u32x4{0, 0, 0, 0};
      sv[p] = u32x4{0, 0, 0, 0};
      if (row < a.S) {
        sk[p] = *reinterpret_cast<const u32x4*>(kbase + (int64_t)row * a.ks[2]);
        if (with_v) sv[p] = *reinterpret_cast<const u32x4*>(vbase + (int64_t)row * a.vs[2]);
      }
    }
  };
  auto stage_store = [&](int32_t tile, bool with_v) {
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      const uint32_t row = srow + ROWS_PER_PASS * p;
      const bool in = tile * kKeys + (int32_t)row < a.S;
      u32x4 kw = transform<F16>(sk[p], kdeq, dks, dko, kquant, a.c);
      if (!in) kw = u32x4{0, 0, 0, 0};
      *reinterpret_cast<u32x4*>(kbuf + row * kKPitch + ((sslot ^ (row & 15)) << 4)) = kw;
      if (qz[QS_QUERY].on) {  // the key row's sum over E: the SLOTS consecutive lanes of one row (every lane shuffles)
        float part = sum8<F16>(kw);
#pragma unroll
        for (int m = 1; m < SLOTS; m <<= 1) part += __shfl_xor(part, m);
        if (sslot == 0) ksum[row] = part;
      }
      if (with_v) {  // V^T image: column d of the tile is a row of 64 keys
        const u32x4 vw = transform<F16>(sv[p], deq_v, dvs, dvo, off, 1.0f);
        const uint32_t words[4] = {vw.x, vw.y, vw.z, vw.w};
#pragma unroll
        for (int j = 0; j < 8; ++j)
          *reinterpret_cast<uint16_t*>(vbuf + (sslot * 8 + j) * kVtPitch + row * 2) = (uint16_t)(words[j >> 1] >> (16 * (j & 1)));
      }
    }
  };

  // masked scores x of the tile in registers (keys >= S -> -inf); `all_masked` collects x <= neg_inf over the row's keys
  auto scores = [&](int32_t tile, sd_f32x16 (&s)[2], bool& all_masked) {
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
      for (int e = 0; e < 16; ++e) s[sub][e] = 0.0f;
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
        const uint32_t krow = 32 * sub + r32;
        const sd_bf16x8 kf = *reinterpret_cast<const sd_bf16x8*>(kbuf + krow * kKPitch + (((2 * t + h) ^ (krow & 15)) << 4));
        s[sub] = mfma<F16>(kf, qf[t], s[sub]);
      }
    const int32_t kv0 = tile * kKeys;
    const int32_t mrow = row_ok ? qi : 0;
    const unsigned char* mbase = static_cast<const unsigned char*>(a.mask);
    const int64_t moff = (int64_t)b * a.ms[0] + (int64_t)head * a.ms[1] + (int64_t)mrow * a.ms[2];
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int32_t kl = 32 * sub + (e & 3) + 8 * (e >> 2) + 4 * (int32_t)h, key = kv0 + kl;
        const float corr = qz[QS_QUERY].on ? row_term + shift_q * ksum[kl] : row_term;
        float x = (s[sub][e] + corr) * alpha;
        x = qz[QS_SCORES].fake(x);
        float bias = b_keep;
        if (a.mask_kind == MASK_CAUSAL) {
          bias = key <= qi ? b_keep : b_drop;
        } else if (key < a.S && a.mask_kind == MASK_BOOL) {
          bias = mbase[moff + (int64_t)key * a.ms[3]] ? b_keep : b_drop;
        } else if (key < a.S && a.mask_kind == MASK_FLOAT) {
          const int64_t at = moff + (int64_t)key * a.ms[3];
          float m;
          if (a.mask_dt == FFQ_F32) m = reinterpret_cast<const float*>(mbase)[at];
          else if (a.mask_dt == FFQ_BF16) m = bf16_bits_to_f32(reinterpret_cast<const uint16_t*>(mbase)[at]);
          else m = f16_bits_to_f32(reinterpret_cast<const uint16_t*>(mbase)[at]);
          bias = qz[QS_MASK].fake(m);
        }
        x = qz[QS_MASKED].fake(x + bias);
        const bool valid = key < a.S;
        all_masked = all_masked && (!valid || x <= a.neg_inf);
        s[sub][e] = valid ? x : -INFINITY;
      }
  };


  sd_f32x16 o[DB];
#pragma unroll
  for (int i = 0; i < DB; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) o[i][e] = 0.0f;
  float m_run = -INFINITY, l_run = 0.0f;  // l_run: this lane's half of the row sum
  bool all_masked = true;

  // a tile is above every row of this wave: skipped (only when its masked scores are -inf, a.skip)
  auto wave_skips = [&](int32_t tile) { return skip && tile * kKeys > qw0 + kRows - 1; };

  // online (m, l) update with the tile's x; returns the scale applied to what was accumulated before
  auto update = [&](const sd_f32x16 (&s)[2]) {
    float mx = -INFINITY;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
      for (int e = 0; e < 16; ++e) mx = fmaxf(mx, s[sub][e]);
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float m_new = fmaxf(m_run, mx);
    const float m_use = m_new == -INFINITY ? 0.0f : m_new;
    const float scale_old = m_run == -INFINITY ? 0.0f : expf(m_run - m_use);
    m_run = m_new;
    return make_float2(scale_old, m_use);
  };

  if constexpr (MODE == 1) {
    // ---- pass 1: row max and sum of exp(x - max), K only
    stage_load(0, false);
    for (int32_t tile = 0; tile < ntiles; ++tile) {
      __syncthreads();
      stage_store(tile, false);
      __syncthreads();
      if (tile + 1 < ntiles) stage_load(tile + 1, false);
      if (wave_skips(tile)) continue;
      sd_f32x16 s[2];
      scores(tile, s, all_masked);
      const float2 u = update(s);
      float rs = 0.0f;
#pragma unroll
      for (int sub = 0; sub < 2; ++sub)
#pragma unroll
        for (int e = 0; e < 16; ++e) rs += expf(s[sub][e] - u.y);
      l_run = l_run * u.x + rs;
    }
  }
  // (MODE 1) the final row statistics: p = exp(x - m) / l, and whether the row is masked everywhere
  const float l_pass1 = l_run + __shfl_xor(l_run, 32);
  const float m_pass1 = m_run == -INFINITY ? 0.0f : m_run;
  const bool masked_pass1 = both_halves(all_masked);

  // ---- main pass: P V
  PSplit ps{1, 1.0f};
  if constexpr (MODE == 1) ps.plan<F16>(qz[QS_DROPOUT].on ? qz[QS_DROPOUT] : qz[QS_WEIGHTS]);
  stage_load(0, true);
  for (int32_t tile = 0; tile < ntiles; ++tile) {
    __syncthreads();
    stage_store(tile, true);
    __syncthreads();
    if (tile + 1 < ntiles) stage_load(tile + 1, true);
    if (wave_skips(tile)) continue;
    sd_f32x16 s[2];
    // pl: (bf16, MODE 0) the rounding residue of P, a second MFMA term; (MODE 1) pl / pl2: the further parts of wide integers
    sd_bf16x8 pf[2][2], pl[2][2], pl2[2][2];
    if constexpr (MODE == 0) {
      scores(tile, s, all_masked);
      const float2 u = update(s);
      l_run *= u.x;
#pragma unroll
      for (int i = 0; i < DB; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) o[i][e] *= u.x;
      float rs = 0.0f;
#pragma unroll
      for (int sub = 0; sub < 2; ++sub)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const float p = __expf(s[sub][e] - u.y);
          rs += p;
          const uint16_t bits = from_f32<F16>(p);
          reinterpret_cast<uint16_t*>(&pf[sub][e >> 3])[e & 7] = bits;
          if constexpr (!F16) reinterpret_cast<uint16_t*>(&pl[sub][e >> 3])[e & 7] = from_f32<false>(p - to_f32<false>(bits));
        }
      l_run += rs;
    } else {
      bool unused = true;
      scores(tile, s, unused);
#pragma unroll
      for (int sub = 0; sub < 2; ++sub)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const float p = masked_pass1 ? 0.0f : expf(s[sub][e] - m_pass1) / l_pass1;
          // weights quantizer, dropout (p == 0: the identity), dropout quantizer; the MFMA takes the last one's integers
          const float n = qz[QS_DROPOUT].on ? qz[QS_DROPOUT].integer(qz[QS_WEIGHTS].fake(p)) : qz[QS_WEIGHTS].integer(p);
          // n = hi + mid + lo exactly (each residue is exact in fp32 and has at most 8 / 11 significant bits left)
          float r = n * ps.prescale;
          const uint16_t hi = from_f32<F16>(r);
          r -= to_f32<F16>(hi);
          const uint16_t mid = from_f32<F16>(r);
          r -= to_f32<F16>(mid);
          reinterpret_cast<uint16_t*>(&pf[sub][e >> 3])[e & 7] = hi;
          reinterpret_cast<uint16_t*>(&pl[sub][e >> 3])[e & 7] = mid;
          reinterpret_cast<uint16_t*>(&pl2[sub][e >> 3])[e & 7] = from_f32<F16>(r);
        }
    }
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
      for (int sub = 0; sub < 2; ++sub)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
        {
          const sd_bf16x8 vf = load_vt(vbuf, 32 * db + r32, 32 * sub + 16 * u + 4 * h);
          o[db] = mfma<F16>(vf, pf[sub][u], o[db]);
          // bf16 P carries 8 bits: its residue keeps the one-pass form within the math path's error (fp16 P carries 11)
          if constexpr (MODE == 0 && !F16) o[db] = mfma<F16>(vf, pl[sub][u], o[db]);
          if constexpr (MODE == 1) {  // wave-uniform: the parts of the probability integers beyond the first
            if (ps.parts > 1) o[db] = mfma<F16>(vf, pl[sub][u], o[db]);
            if (ps.parts > 2) o[db] = mfma<F16>(vf, pl2[sub][u], o[db]);
          }
        }
        }
  }

  // ---- epilogue: O^T lane (r32 = query, h): d = 32 db + (e & 3) + 8 (e >> 2) + 4 h
  const bool row_masked = both_halves(all_masked);
  const float l_tot = l_run + __shfl_xor(l_run, 32);
  if (!row_ok) return;
  // MODE 1: the scale of the integers in P, the split's pre-scale divided out (a power of two: exact)
  const float mul = (qz[QS_DROPOUT].on ? qz[QS_DROPOUT].s : qz[QS_WEIGHTS].s) / ps.prescale;
  const int64_t obase = (((int64_t)b * a.H + head) * a.L + qi) * D;
  const QReg& oq = qz[QS_OUTPUT];
#pragma unroll
  for (int db = 0; db < DB; ++db)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      float y[4];
      uint32_t cw = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float x = MODE == 0 ? (row_masked ? 0.0f : o[db][4 * rr + i] / l_tot) : o[db][4 * rr + i] * mul;
        if (oq.on) {
          const float c = oq.code(x);
          cw |= ((uint32_t)(uint8_t)(int8_t)(int)c) << (8 * i);
          x = (c + oq.o) * oq.s;
        }
        y[i] = x;
      }
      const int d = 32 * db + 8 * rr + 4 * (int)h;
      if (a.out) {
        u32x2 w;
        w.x = (uint32_t)from_f32<F16>(y[0]) | ((uint32_t)from_f32<F16>(y[1]) << 16);
        w.y = (uint32_t)from_f32<F16>(y[2]) | ((uint32_t)from_f32<F16>(y[3]) << 16);
        *reinterpret_cast<u32x2*>(a.out + obase + d) = w;
      }
      if (a.codes) *reinterpret_cast<uint32_t*>(a.codes + obase + d) = cw;
    }
}

}  // namespace
}  // namespace ffq

using namespace ffq;

namespace {
// The scaled-K codes, written once per call ([B][kv heads][S][E] in dt) instead of per staged tile by every query block: the
// quantizer's IEEE division per element then runs B * kv_heads * S * E times, not that times the number of query blocks
// (docs/kernels.md has the measurement). One thread per 16-byte slot.
template <bool F16>
__global__ __launch_bounds__(256) void sdpa_key_codes_kernel(const uint16_t* k, int64_t ks0, int64_t ks1, int64_t ks2, int32_t HKV, int32_t S,
                                                             int32_t slots, int64_t total, const float* ds, const float* dof, Quant kq, float c,
                                                             uint16_t* out) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int64_t slot = idx % slots, row = idx / slots;
  const int64_t s = row % S, bh = row / S, h = bh % HKV, b = bh / HKV;
  const u32x4 w = *reinterpret_cast<const u32x4*>(k + b * ks0 + h * ks1 + s * ks2 + slot * 8);
  QReg q;
  q.load(kq);
  const float dsv = ds ? ds[0] : 1.0f, dov = (ds && dof) ? rne(dof[0]) : 0.0f;
  *reinterpret_cast<u32x4*>(out + row * slots * 8 + slot * 8) = transform<F16>(w, ds != nullptr, dsv, dov, q, c);
}

template <int D, int MODE>
void launch(const SdpaArgs& a, bool f16, int64_t blocks, hipStream_t s) {
  if (f16) sdpa_quantize_kernel<D, MODE, true><<<(unsigned)blocks, kThreads, 0, s>>>(a);
  else sdpa_quantize_kernel<D, MODE, false><<<(unsigned)blocks, kThreads, 0, s>>>(a);
}
}  // namespace

extern "C" int ffq_sdpa_quantize(const void* q, const void* k, const void* v, int dt, const float* const* deq_scale,
                                 const float* const* deq_offset, int64_t batch, int64_t q_heads, int64_t kv_heads, int64_t L,
                                 int64_t S, int64_t E, const int64_t* strides, const void* mask, int mask_kind, int mask_dt,
                                 const int64_t* mask_strides, double sqrt_scale, double neg_inf, const ffq_sdpa_quantizer* quantizers,
                                 int skip_above_diagonal, void* out, int8_t* codes_out, void* key_codes, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (dt != FFQ_BF16 && dt != FFQ_F16) return fail(FFQ_ERR_DTYPE, "sdpa: bf16 or fp16 operands");
  if (E != 64 && E != 128) return fail(FFQ_ERR_ARG, "sdpa: E must be 64 or 128");
  if (batch < 0 || L < 0 || S < 0 || q_heads <= 0 || kv_heads <= 0 || q_heads % kv_heads) return fail(FFQ_ERR_ARG, "sdpa: bad extent");
  if (mask_kind < MASK_NONE || mask_kind > MASK_FLOAT) return fail(FFQ_ERR_ARG, "sdpa: bad mask kind");
  if (!strides || !quantizers || !deq_scale || !deq_offset) return fail(FFQ_ERR_ARG, "sdpa: NULL argument table");
  if (batch == 0 || L == 0) return FFQ_OK;
  if (S == 0) return fail(FFQ_ERR_ARG, "sdpa: S must be >= 1");
  if (!q || !k || !v || (!out && !codes_out)) return fail(FFQ_ERR_ARG, "sdpa: NULL buffer");
  if (mask_kind >= MASK_BOOL && (!mask || !mask_strides)) return fail(FFQ_ERR_ARG, "sdpa: the mask needs its data and strides");
  if (mask_kind == MASK_FLOAT && mask_dt != FFQ_F32 && mask_dt != FFQ_BF16 && mask_dt != FFQ_F16) return fail(FFQ_ERR_DTYPE, "sdpa: float mask dtype");
  if (codes_out && !quantizers[QS_OUTPUT].scale) return fail(FFQ_ERR_ARG, "sdpa: codes need the output quantizer");
  if (!aligned16(q) || !aligned16(k) || !aligned16(v) || (out && !aligned16(out)) || (codes_out && !aligned16(codes_out)))
    return fail(FFQ_ERR_ARG, "sdpa: buffers must be 16-byte aligned");
  for (int i = 0; i < 9; ++i)  // rows of 16-byte aligned runs: every stride a multiple of 8 elements
    if (strides[i] < 0 || strides[i] % 8) return fail(FFQ_ERR_ARG, "sdpa: strides must be non-negative multiples of 8 elements");
  if (L >= ((int64_t)1 << 30) || S >= ((int64_t)1 << 30) || batch * q_heads >= ((int64_t)1 << 30)) return fail(FFQ_ERR_ARG, "sdpa: too large");
  SdpaArgs a;
  a.q = static_cast<const uint16_t*>(q); a.k = static_cast<const uint16_t*>(k); a.v = static_cast<const uint16_t*>(v);
  for (int i = 0; i < 3; ++i) {
    a.deq_s[i] = deq_scale[i];
    a.deq_o[i] = deq_scale[i] ? deq_offset[i] : nullptr;
    a.qs[i] = strides[i]; a.ks[i] = strides[3 + i]; a.vs[i] = strides[6 + i];
  }
  a.B = (int32_t)batch; a.H = (int32_t)q_heads; a.HKV = (int32_t)kv_heads; a.L = (int32_t)L; a.S = (int32_t)S;
  a.nqb = (int32_t)((L + kQBlock - 1) / kQBlock);
  a.mask = mask; a.mask_kind = mask_kind; a.mask_dt = mask_dt;
  for (int i = 0; i < 4; ++i) a.ms[i] = mask_kind >= MASK_BOOL ? mask_strides[i] : 0;
  a.c = (float)sqrt_scale; a.neg_inf = (float)neg_inf;
  a.skip = mask_kind == MASK_CAUSAL && skip_above_diagonal;
  bool probs = false;
  for (int i = 0; i < kNQ; ++i) {
    const ffq_sdpa_quantizer& z = quantizers[i];
    if (z.scale && !(z.num_bits >= 1.0 && z.num_bits <= 8.0 && z.num_bits == (double)(int)z.num_bits))
      return fail(FFQ_ERR_ARG, "sdpa: quantizers need an integral bit-width in 1..8");
    const double half = z.scale ? ldexp(1.0, (int)z.num_bits - 1) : 1.0;
    a.qz[i] = Quant{z.scale, z.scale ? z.offset : nullptr, (float)-half, (float)(half - 1.0)};
    if (z.scale && (i == QS_WEIGHTS || i == QS_DROPOUT)) probs = true;
  }
  a.out = static_cast<uint16_t*>(out); a.codes = codes_out;
  a.k_coded = 0;
  const bool f16 = dt == FFQ_F16;
  if (quantizers[QS_KEY].scale) {  // the scaled-K codes, once: k is then read from key_codes
    if (!key_codes || !aligned16(key_codes)) return fail(FFQ_ERR_ARG, "sdpa: a scaled-key quantizer needs key_codes (B * kv_heads * S * E, 16-byte aligned)");
    const int64_t total = batch * kv_heads * S * (E / 8);
    const unsigned kblocks = (unsigned)((total + 255) / 256);
    if (f16) sdpa_key_codes_kernel<true><<<kblocks, 256, 0, s>>>(a.k, a.ks[0], a.ks[1], a.ks[2], a.HKV, a.S, (int32_t)(E / 8), total, deq_scale[1],
                                                                 deq_offset[1], a.qz[QS_KEY], a.c, static_cast<uint16_t*>(key_codes));
    else sdpa_key_codes_kernel<false><<<kblocks, 256, 0, s>>>(a.k, a.ks[0], a.ks[1], a.ks[2], a.HKV, a.S, (int32_t)(E / 8), total, deq_scale[1],
                                                              deq_offset[1], a.qz[QS_KEY], a.c, static_cast<uint16_t*>(key_codes));
    const int rc = check_launch("sdpa_key_codes_kernel");
    if (rc != FFQ_OK) return rc;
    a.k = static_cast<const uint16_t*>(key_codes);
    a.ks[0] = kv_heads * S * E; a.ks[1] = S * E; a.ks[2] = E;
    a.deq_s[1] = nullptr; a.deq_o[1] = nullptr;
    a.k_coded = 1;
  }
  const int64_t blocks = (int64_t)a.nqb * batch * q_heads;
  if (blocks >= ((int64_t)1 << 31)) return fail(FFQ_ERR_ARG, "sdpa: too many workgroups");
  if (E == 64) probs ? launch<64, 1>(a, f16, blocks, s) : launch<64, 0>(a, f16, blocks, s);
  else probs ? launch<128, 1>(a, f16, blocks, s) : launch<128, 0>(a, f16, blocks, s);
  return check_launch("sdpa_quantize_kernel");
}
