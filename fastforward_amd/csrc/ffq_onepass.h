// ffq_onepass.h — what the one-pass quantized families share: ffq_modules.hip (LayerNorm / Embedding / ReLU / SiLU),
// ffq_elementwise.hip (add / sub / mul / div, softmax, sigmoid, GELU), ffq_math.hip (rms_norm, pow, exp, sin, cos, sum, cumsum),
// ffq_pool.hip (the pools, nearest interpolate), ffq_concat.hip (cat, pad), ffq_index.hip (index_add, permute) and ffq_unfold.hip
// (unfold).
//
// The arithmetic contract of every kernel in those files:
//   A2  an operand given as codes is dequantized in registers as ffq_dequantize.hip does: (q + round(o)) * s in fp32 (two roundings,
//       no FMA), rounded once to the data dtype T — exactly the intermediate tensor of the reference's chain. A plain operand is T.
//   op  ATen's device formula in fp32 (stated at each kernel), rounded ONCE to T.
//   A1  the rounded value goes through the arithmetic of ffq_affine.h for up to FFQ_MAX_FANOUT static per-tensor quantizers
//       (ffq_fanout.h); the value itself is stored only when the caller asks (`out` != NULL).
// Chunks are 8 elements: 16 B per lane for bf16 / fp16 values, 8 B for int8 codes.
// A translation unit picks its nt policy (FFQ_NT_STREAMS, ffq_vec.h) before it includes this header.
#pragma once

#include "ffq_affine.h"
#include "ffq_common.h"
#include "ffq_fanout.h"
#include "ffq_vec.h"

#include <initializer_list>
#include <math.h>
#include <type_traits>

namespace ffq {

constexpr int kE = 8;  // elements per chunk

// ---- device: operands ------------------------------------------------------------------------------------------------------

template <typename T>
__device__ __forceinline__ void unpack(const Chunk<T, kE>& h, float (&v)[kE]) {
#pragma unroll
  for (int i = 0; i < kE; ++i) v[i] = h.get(i);
}

// A2 of one chunk of codes, before the rounding to the data dtype. `o` is already rounded.
template <typename TIn>
__device__ __forceinline__ void a2_chunk(const Chunk<TIn, kE>& q, float s, float o, float (&v)[kE]) {
#pragma unroll
  for (int i = 0; i < kE; ++i) {
    const float a = q.get(i) + o;
    v[i] = a * s;
  }
}

// One chunk of an operand as values of the data dtype T held in fp32: plain T, or A2 of codes TIn.
// NT: a streamed operand (the unit's nt hint); one that is re-read (a broadcast `other`, an embedding row) stays in the caches.
template <typename T, typename TIn, bool DEQ, bool NT = true>
__device__ __forceinline__ void operand_chunk(const TIn* p, float s, float o, float (&v)[kE]) {
  Chunk<T, kE> h;
  if constexpr (DEQ) {
    Chunk<TIn, kE> q;
    if constexpr (NT) q.FFQ_SLOAD(p); else q.load(p);
    a2_chunk(q, s, o, v);
    h.pack(v);
  } else {
    if constexpr (NT) h.FFQ_SLOAD(reinterpret_cast<const T*>(p)); else h.load(reinterpret_cast<const T*>(p));
  }
  unpack(h, v);
}

// ... the same, left packed (the kernels that keep a row, or look values up, as T).
template <typename T, typename TIn, bool DEQ, bool NT = true>
__device__ __forceinline__ Chunk<T, kE> operand_packed(const TIn* p, float s, float o) {
  Chunk<T, kE> h;
  if constexpr (DEQ) {
    Chunk<TIn, kE> q;
    if constexpr (NT) q.FFQ_SLOAD(p); else q.load(p);
    float v[kE];
    a2_chunk(q, s, o, v);
    h.pack(v);
  } else {
    if constexpr (NT) h.FFQ_SLOAD(reinterpret_cast<const T*>(p)); else h.load(reinterpret_cast<const T*>(p));
  }
  return h;
}

// A2 of one code (ffq_pool.hip's gathers, ffq_concat.hip's element forms). `o` is already rounded.
template <typename T>
__device__ __forceinline__ float a2_value(float q, float s, float o) {
  const float a = q + o;
  float m = a * s;
  // (the product in a register of its own: hipcc otherwise folds the multiply and the fp16 conversion into v_fma_mixlo_f16 with a
  // +0 addend, which turns the -0.0 of a code -0.0 under an offset -0.0 into +0.0; seen on the MI355X against the chain's A2)
  asm volatile("" : "+v"(m));
  return round_stage(m, TypeTag<T>::value);
}

// Parameters of a streamed operand: one pair, or one per run of `by_run.div` chunks (a row of the last dimension).
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

// The row kernels' prologue: the pair of the tensor or of `row`.
template <bool DEQ>
__device__ __forceinline__ void row_params(const float* xs, const float* xo, uint32_t per_row, uint32_t row, float& s, float& o) {
  if constexpr (DEQ) {
    const uint32_t p = per_row ? row : 0u;
    s = xs[p];
    o = xo ? rne(xo[p]) : 0.0f;
  }
}

// ---- device: results -------------------------------------------------------------------------------------------------------

// 8 fp32 results -> the data dtype (the one rounding), stored when asked, with their codes.
template <typename T>
__device__ __forceinline__ void store_chunk(T* out, const FanOut& f, const FanParams& p, float (&z)[kE], size_t at) {
  Chunk<T, kE> y;
  y.pack(z);
  if (out) y.FFQ_SSTORE(out + at);
  unpack(y, z);
  fan_store(f, p, z, at);
}

// The value and the codes of ONE result (a reduction, the tail of a pooled map): quantize_chunk_to_bytes' arithmetic for E = 1.
template <typename T>
__device__ __forceinline__ void store_one(T* out, const FanOut& f, const FanParams& p, float acc, size_t at) {
  const float z[1] = {round_stage(acc, TypeTag<T>::value)};  // the one rounding to the data dtype
  if (out) out[at] = from_f32<T>(z[0]);
  const int ilo = (int)f.lo, ihi = (int)f.hi;
#pragma unroll
  for (int j = 0; j < FFQ_MAX_FANOUT; ++j) {
    if (j >= f.n) break;
    const Divider<1> d(p.s[j]);
    float r[1];
    quantize_chunk_with<1, 1>(d, z, p.o[j], r);
    int v = (int)r[0];  // v_cvt_i32_f32 saturates and maps NaN to 0, as finalize_chunk
    v = v < ilo ? ilo : (v > ihi ? ihi : v);
    f.codes[j][at] = (int8_t)v;
  }
}

// ---- device: one value or one group that only moves (ffq_concat.hip, ffq_index.hip, ffq_unfold.hip) ----------------------------

// The codes of ONE value of the data dtype (store_one's arithmetic without its store: a plain element keeps its own bits).
__device__ __forceinline__ void fan_one(const FanOut& f, const FanParams& p, float z, size_t at) {
  const float one[1] = {z};
  const int ilo = (int)f.lo, ihi = (int)f.hi;
#pragma unroll
  for (int j = 0; j < FFQ_MAX_FANOUT; ++j) {
    if (j >= f.n) break;
    const Divider<1> d(p.s[j]);
    float r[1];
    quantize_chunk_with<1, 1>(d, one, p.o[j], r);
    int v = (int)r[0];  // v_cvt_i32_f32 saturates and maps NaN to 0, as finalize_chunk
    v = v < ilo ? ilo : (v > ihi ? ihi : v);
    f.codes[j][at] = (int8_t)v;
  }
}

// Element `i` of an operand as a value of T: its own bits when plain, A2 of the code otherwise.
template <typename T, typename TIn, bool DEQ>
__device__ __forceinline__ T element(const TIn* x, size_t i, float s, float o) {
  if constexpr (DEQ) return from_f32<T>(a2_value<T>(to_f32(x[i]), s, o));
  else return reinterpret_cast<const T*>(x)[i];
}

template <typename T>
__device__ __forceinline__ void put_one(T* out, const FanOut& f, const FanParams& p, T v, size_t at) {
  if (out) out[at] = v;
  if (f.n) fan_one(f, p, to_f32(v), at);
}

template <typename T>
__device__ __forceinline__ void put_group(T* out, const FanOut& f, const FanParams& p, const Chunk<T, kE>& h, size_t at) {
  if (out) h.store(out + at);
  if (f.n) {
    float v[kE];
    unpack(h, v);
    fan_store(f, p, v, at);
  }
}

// ---- device: reductions ----------------------------------------------------------------------------------------------------

// Sum of one value per lane over a wave (butterfly: every lane gets the same, deterministic sum).
__device__ __forceinline__ float wave_sum(float acc) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) acc = acc + __shfl_xor(acc, d, 64);
  return acc;
}

// ---- host: checks ----------------------------------------------------------------------------------------------------------

static bool value_dtype(int dt) { return dt == FFQ_BF16 || dt == FFQ_F16; }

// The form of an operand: plain `dt` (no parameters), or codes of int8 / `dt` with a scale.
static int check_operand_form(const char* what, int x_dt, const float* scale, const float* offset, bool per_row, int dt) {
  if (scale ? (x_dt != FFQ_I8 && x_dt != dt) : (x_dt != dt || offset || per_row))
    return fail(FFQ_ERR_DTYPE, "%s: a plain operand of the value dtype, or int8 / value-dtype codes with a scale", what);
  return FFQ_OK;
}

// ... of a streamed operand with one parameter pair or one per run of `run` elements (run % 8 == 0, run divides numel, fewer than
// `row_limit` runs; 0: no limit).
static int check_operand(const char* what, int x_dt, const float* scale, const float* offset, int64_t run, int dt, int64_t numel,
                         int64_t row_limit) {
  if (run < 0) return fail(FFQ_ERR_ARG, "%s: negative parameter run", what);
  const int rc = check_operand_form(what, x_dt, scale, offset, run != 0, dt);
  if (rc) return rc;
  if (run && (run % kE != 0 || numel % run != 0 || (row_limit && numel / run >= row_limit)))
    return fail(FFQ_ERR_DTYPE, "%s: per-row parameters need a row length that divides numel and is a multiple of 8", what);
  return FFQ_OK;
}

constexpr int64_t kRowLimit = (int64_t)1 << 31;  // rows a 32-bit parameter index reaches

static OperandParams operand_params(const float* scale, const float* offset, int64_t run) {
  OperandParams p;
  p.scale = scale;
  p.offset = offset;
  p.per_row = run ? 1u : 0u;
  p.by_run = make_fastdiv(run ? (uint32_t)(run / kE) : 1u);
  return p;
}

// The buffers of a launch: the input there, every vector-accessed buffer 16-byte aligned (a NULL optional one passes).
static int check_buffers(const void* x, std::initializer_list<const void*> vectors) {
  if (!x) return fail(FFQ_ERR_ARG, "NULL buffer");
  for (const void* p : vectors)
    if (!aligned16(p)) return fail(FFQ_ERR_ARG, "buffers must be 16-byte aligned");
  return FFQ_OK;
}

// The common tail of an entry point's checks, in the order every entry keeps: the fan-out of `fan_numel` results, then an empty
// extent (FFQ_OK with nothing to launch: the caller returns on `rc || empty`), then the buffers.
static int check_launch_args(const ffq_fanout* fan, int64_t fan_numel, bool empty, const void* x, std::initializer_list<const void*> vectors,
                             FanOut* f) {
  const int rc = fan_from_abi(fan, fan_numel, f);
  if (rc || empty) return rc;
  return check_buffers(x, vectors);
}

// ---- host: launch dispatch -------------------------------------------------------------------------------------------------

template <typename T>
struct Tag {
  using type = T;
};
template <int N>
using Int = std::integral_constant<int, N>;

// launch(Tag<TIn>, bool_constant<DEQ>) for an operand of the value dtype T: plain, int8 codes or T codes.
template <typename T, typename F>
static void dispatch_form(int x_dt, bool deq, F&& launch) {
  if (!deq) launch(Tag<T>{}, std::false_type{});
  else if (x_dt == FFQ_I8) launch(Tag<int8_t>{}, std::true_type{});
  else launch(Tag<T>{}, std::true_type{});
}

// launch(Tag<T>) for the value dtype `dt` (bf16 | fp16: the caller has checked value_dtype).
template <typename F>
static void dispatch_dtype(int dt, F&& launch) {
  if (dt == FFQ_BF16) launch(Tag<bf16_t>{}); else launch(Tag<f16_t>{});
}

// launch(Tag<T>, Tag<TIn>, bool_constant<DEQ>): value dtype x input form, the six instantiations every family builds.
template <typename F>
static void dispatch_input(int dt, int x_dt, bool deq, F&& launch) {
  dispatch_dtype(dt, [&](auto t) {
    dispatch_form<typename decltype(t)::type>(x_dt, deq, [&](auto tin, auto d) { launch(t, tin, d); });
  });
}

// launch(Int<CPL>, Int<WPR>) for a row of `cpr` chunks held in registers: WPR wavefronts per row (1: four rows per block), CPL
// chunks per lane, cpr <= 64 * WPR * CPL.
template <typename F>
static void dispatch_row_shape(uint32_t cpr, F&& launch) {
  if (cpr <= 64) launch(Int<1>{}, Int<1>{});
  else if (cpr <= 256) launch(Int<1>{}, Int<4>{});
  else if (cpr <= 512) launch(Int<2>{}, Int<4>{});
  else if (cpr <= 1024) launch(Int<4>{}, Int<4>{});
  else launch(Int<8>{}, Int<4>{});
}

// blocks of the row kernels: kBlock / (64 * WPR) rows each
template <int WPR>
static unsigned row_grid(int64_t rows) { return (unsigned)((rows + 4 / WPR - 1) / (4 / WPR)); }

}  // namespace ffq
