// ffq_conv_transpose.hip — the W8A8 transposed convolution (conv_transpose1d / conv_transpose2d) as a phase-split int8 implicit
// GEMM on the matrix cores of gfx950.
//
// Replaces fallback.conv_transpose1d / fallback.conv_transpose2d, src/fastforward/_gen/fallback.py:346-449: the reference
// dequantizes the input codes and the weight codes, runs a float transposed convolution and optionally re-quantizes. Here the
// codes are contracted exactly in int32 and the affine parameters are applied once per output element (include/ffq.h,
// ffq_conv_transpose2d_w8a8):
//
//   y[b,n,p] = sx * sw[n'] * ( acc + ox * rsw(n,p) + ow[n'] * rsx(b,p) + C * |V(p)| * ox * ow[n'] )  (+ bias[n])
//
// V(p) is the set of taps (kh, kw) for which stride divides o + pad - k * dil on both axes and the quotient lies inside the input.
//
// Phase decomposition. Output rows oh = rh (mod stride_h) use exactly the taps kh with stride_h | rh + pad_h - kh * dil_h; they are
// kh = k0 + a * (stride_h / g), g = gcd(stride_h, dil_h), and tap a reads input row i + off0 - a * (dil_h / g) for oh = rh +
// stride_h * i. Columns alike. Every tap belongs to exactly one phase (rh, rw); inside a phase the operation is a dense stride-1
// correlation over the phase's taps. A phase may have no tap at all (its outputs are the bias).
//
// Two launches:
//   * convt_reorder_kernel — the input codes NCHW -> NHWC with C padded to Cp = 16 * ceil(C / 16) (skipped for a channels-last
//     input), the weight codes [C, OC, KH, KW] -> [OC, Kp] with the taps permuted phase-major (each phase's K range is one
//     contiguous [k_begin, k_end) of every row, 16-channel runs innermost), the per-tap weight sums tapsum[n, t] in that order
//     and the per-(phase, n) totals. A weight thread owns one (16-channel group, n * taps + t) with n * taps + t fastest: torch's
//     transposed layout [C, OC, KH, KW] makes each of its 16 byte loads 64 consecutive bytes per wave.
//   * convt_w8a8_kernel — conv_w8a8_kernel's tile (128 x 128 x 64, register-staged, double-buffered swizzled LDS, 2 x 2 waves of
//     v_mfma_i32_32x32x32_i8, XCD-aware tile order), the weight on the A side, output positions on the B side. Every 128-position
//     tile lies inside one phase (a host-built table gives each phase's tile prefix, K range and per-axis taps); its K loop runs
//     over that phase's taps only. Stores go to NCHW at ow = rw + stride_w * j.
#include "ffq_conv_host.h"
#include "ffq_conv_tile.h"

namespace ffq {
namespace {

constexpr int TBM = 128, TBN = 128, TBK = 64;
constexpr int kTileBytes = TBM * TBK;
constexpr int kMaxPhases = 64;                 // stride_h * stride_w: the size of the phase table

// One residue of one axis: the taps k0, k0 + kstep, ... (n of them); tap a reads input index i + off0 - a * ostep.
struct AxisPhase { int k0, n, off0, extent; };  // extent: the number of outputs o = r (mod stride) below the output size

// The phase table. Phase p = rh * sw + rw; its positions are [B, ah[rh].extent, aw[rw].extent], its tiles [tile_end[p - 1],
// tile_end[p]), its taps the product ah[rh] x aw[rw] (w fastest) at [tap_begin[p], tap_begin[p] + ah[rh].n * aw[rw].n) of the
// phase-major order.
struct PhaseTable {
  int tile_end[kMaxPhases];
  int tap_begin[kMaxPhases];
  AxisPhase ah[kMaxPhases], aw[kMaxPhases];
  int kstep_h, ostep_h, kstep_w, ostep_w;
};

struct ConvtArgs {
  const int8_t* wq;       // [OC, Kp]: weight codes, taps phase-major, Kp = KH * KW * Cp
  const int8_t* xq;       // [B, H, W, Cp]
  const int32_t* tapsum;  // [OC, KH * KW] (phase-major taps) then [nph, OC] phase totals
  const float* x_scale; const float* x_offset;
  const float* w_scale; const float* w_offset; int w_per_row;
  const void* bias; int bias_dt;
  void* out;  // [B, OC, OH, OW]
  const float* out_scale; const float* out_offset;
  float out_lo, out_hi;
  int y_dt;
  int B, OC, C, Cp, H, W, OH, OW, taps;
  int sh, sw, nph;
  int Kp;
  int tiles_m;
};

// [lo, hi) of the taps a < n with 0 <= o0 - a * m < extent (m >= 1)
__device__ __forceinline__ void tap_range_down(int o0, int m, int n, int extent, int& lo, int& hi) {
  hi = o0 < 0 ? 0 : o0 / m + 1;
  hi = hi < n ? hi : n;
  const int over = o0 - extent + 1;  // a * m >= over
  lo = over <= 0 ? 0 : (over + m - 1) / m;
  if (hi < lo) hi = lo;
}

__device__ __forceinline__ int pos_mod(int v, int m) {
  const int r = v % m;
  return r < 0 ? r + m : r;
}

// -------------------------------------------------------------------------------------------------
// Reorder pass. Threads [0, n_in) move the input as conv_layout_kernel's input half does. Threads [n_in, n_in + n_w) move the
// weight: one (16-channel group g, n * taps + t) each with n * taps + t fastest, t in the SOURCE order (kh, kw). The 16 codes
// wq[g * 16 + k, n, t] leave as one store at the tap's phase-major place in row n; their sum goes into tapsum[n, place] and
// into the total of (phase, n) (both zeroed ahead of the launch).
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void convt_reorder_kernel(const int8_t* __restrict__ x, int8_t* __restrict__ xn, int64_t n_in, int C,
                                                            int64_t HW, int groups, const int8_t* __restrict__ w, int8_t* __restrict__ wn,
                                                            int64_t n_w, int taps, int KW, int OC, int sh, int sw, int ph, int pw, int dh,
                                                            int dw, int32_t* __restrict__ tapsum, PhaseTable tab) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int Cp = groups * 16;
  if (idx < n_in) {
    nchw_to_nhwc16(x, xn, idx, C, HW, groups);
    return;
  }
  const int64_t j = idx - n_in;
  if (j >= n_w) return;
  const int64_t row_taps = (int64_t)OC * taps;
  const int64_t row_tap = j % row_taps;  // n * taps + t
  const int g = (int)(j / row_taps);
  const int t = (int)(row_tap % taps);
  const int64_t n = row_tap / taps;
  const int kh = t / KW, kw = t - kh * KW;
  // the tap's phase and its place in the phase: stride | r + pad - k * dil, so r = k * dil - pad (mod stride)
  const int rh = pos_mod(kh * dh - ph, sh), rw = pos_mod(kw * dw - pw, sw);
  const int p = rh * sw + rw;
  const int place = tab.tap_begin[p] + (kh / tab.kstep_h) * tab.aw[rw].n + kw / tab.kstep_w;
  uint8_t v[16];
  int sum = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int c = g * 16 + k;
    const int8_t q = c < C ? w[(int64_t)c * row_taps + row_tap] : (int8_t)0;
    v[k] = (uint8_t)q;
    sum += q;
  }
  *reinterpret_cast<u32x4*>(wn + (n * taps + place) * Cp + g * 16) = pack16(v);
  if (sum != 0) {
    atomicAdd(tapsum + n * taps + place, sum);
    atomicAdd(tapsum + row_taps + (int64_t)p * OC + n, sum);
  }
}

// -------------------------------------------------------------------------------------------------
// The implicit GEMM of one phase per tile: [OC, phase's K range] weight codes x the gathered matrix [phase's positions, that K
// range], block tile 128 x 128 x 64. A lane stages two B rows (output positions of the phase's grid) and one 16-byte slot of each;
// the slot's tap (a, b) of the phase and its channel offset c0 advance by 64 k-bytes per step with no division. With weight
// offsets the lanes also sum the B rows' codes as they pass through their registers.
// -------------------------------------------------------------------------------------------------
template <typename TOut, bool REQUANT>
__global__ __launch_bounds__(256) void convt_w8a8_kernel(ConvtArgs a, PhaseTable tab) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[2][2][kTileBytes];
  __shared__ int rsx_s[TBN];

  // XCD-aware tile order, as conv_w8a8_kernel: blocks b, b+8, ... share an XCD and get a contiguous range of tiles
  const uint32_t nblk = gridDim.x;
  const uint32_t xcd = blockIdx.x & 7u, slot_in_xcd = blockIdx.x >> 3;
  const uint32_t q = nblk >> 3, r = nblk & 7u;
  const uint32_t tile_id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot_in_xcd;
  const int tn = tile_id / a.tiles_m, tm = tile_id % a.tiles_m;
  const int m0 = tm * TBM;

  // the tile's phase (block-uniform): the first whose tile prefix lies above tn
  int p = 0;
  while (p + 1 < a.nph && tn >= tab.tile_end[p]) ++p;
  const int rh = p / a.sw, rw = p - rh * a.sw;
  const AxisPhase fh = tab.ah[rh], fw = tab.aw[rw];
  const int n0 = (tn - (p ? tab.tile_end[p - 1] : 0)) * TBN;  // the tile's first position inside the phase
  const int grid_hw = fh.extent * fw.extent;                  // >= 1: a phase without positions has no tile
  const int npos = a.B * grid_hw;
  const int klen = fh.n * fw.n * a.Cp;  // the phase's K range [kbeg, kbeg + klen) of every weight row
  const int64_t kbeg = (int64_t)tab.tap_begin[p] * a.Cp;
  const int mh = -tab.ostep_h, mw = -tab.ostep_w;  // input rows / columns one tap further back, >= 1

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int s_row0 = tid >> 2, s_slot = tid & 3;
  const int s_row1 = s_row0 + 64;

  // the two staged output positions: image base (in bytes of the NHWC codes) and the input pixel of the phase's first tap
  int64_t pbase[2];
  int pih[2], piw[2];
  bool pok[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int n = n0 + (h ? s_row1 : s_row0);
    pok[h] = n < npos;
    const int nn = pok[h] ? n : 0;
    const int b = nn / grid_hw, pp = nn - b * grid_hw;
    const int i = pp / fw.extent, j = pp - i * fw.extent;
    pbase[h] = (int64_t)b * a.H * a.W * a.Cp;
    pih[h] = i + fh.off0;
    piw[h] = j + fw.off0;
  }
  // this lane's slot: k-byte s_slot * 16 of the step, as (tap ta of the rows, tap tb of the columns, c0)
  int c0 = s_slot * 16, tb = 0, ta = 0;
  auto normalize = [&]() {
    while (c0 >= a.Cp) {
      c0 -= a.Cp;
      if (++tb == fw.n) { tb = 0; ++ta; }
    }
  };
  normalize();

  v16i acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0;

  const int ksteps = (klen + TBK - 1) / TBK;  // 0 for a phase without taps
  const bool want_rsx = a.w_offset != nullptr;
  u32x4 ra0, ra1, rb0, rb1;
  int rs0 = 0, rs1 = 0;
  auto add_rowsums = [&]() {
    if (want_rsx) {
      const uint32_t w0[4] = {rb0.x, rb0.y, rb0.z, rb0.w}, w1[4] = {rb1.x, rb1.y, rb1.z, rb1.w};
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        rs0 = __builtin_amdgcn_sdot4((int)w0[d], 0x01010101, rs0, false);
        rs1 = __builtin_amdgcn_sdot4((int)w1[d], 0x01010101, rs1, false);
      }
    }
  };
  auto load_a = [&](int row, int kb) {
    u32x4 v = {0u, 0u, 0u, 0u};
    if (row < a.OC && kb < klen) v = *reinterpret_cast<const u32x4*>(a.wq + (size_t)row * a.Kp + kbeg + kb);
    return v;
  };
  auto gather = [&](int h) {
    u32x4 v = {0u, 0u, 0u, 0u};
    const int ih = pih[h] - ta * mh, iw = piw[h] - tb * mw;
    if (pok[h] && ta < fh.n && (unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W)
      v = *reinterpret_cast<const u32x4*>(a.xq + pbase[h] + ((int64_t)ih * a.W + iw) * a.Cp + c0);
    return v;
  };
  auto fetch = [&](int kt) {  // called for kt = 0, 1, 2, ... in order: the slot's tap state advances here
    const int kb = kt * TBK + s_slot * 16;
    ra0 = load_a(m0 + s_row0, kb);
    ra1 = load_a(m0 + s_row1, kb);
    rb0 = gather(0);
    rb1 = gather(1);
    c0 += TBK;
    normalize();
  };
  auto stash = [&](int stage) {
    *reinterpret_cast<u32x4*>(&lds[stage][0][conv_swizzled(s_row0, s_slot)]) = ra0;
    *reinterpret_cast<u32x4*>(&lds[stage][0][conv_swizzled(s_row1, s_slot)]) = ra1;
    *reinterpret_cast<u32x4*>(&lds[stage][1][conv_swizzled(s_row0, s_slot)]) = rb0;
    *reinterpret_cast<u32x4*>(&lds[stage][1][conv_swizzled(s_row1, s_slot)]) = rb1;
  };

  if (ksteps > 0) {  // block-uniform
    fetch(0);
    add_rowsums();
    stash(0);
  }
  __syncthreads();

  const uint32_t frag_row = lane & 31, frag_g = lane >> 5;
  for (int kt = 0; kt < ksteps; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < ksteps) fetch(kt + 1);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      v4i fa[2], fb[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const uint32_t row = wm * 64 + i * 32 + frag_row;
        fa[i] = *reinterpret_cast<const v4i*>(&lds[cur][0][conv_swizzled(row, kk * 2 + frag_g)]);
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const uint32_t row = wn * 64 + j * 32 + frag_row;
        fb[j] = *reinterpret_cast<const v4i*>(&lds[cur][1][conv_swizzled(row, kk * 2 + frag_g)]);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[i], fb[j], acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < ksteps) { add_rowsums(); stash(cur ^ 1); }
    __syncthreads();
  }
  if (want_rsx) {  // the four lanes that staged a position's four slots meet; block-uniform branch
    rs0 += __shfl_xor(rs0, 1, 64); rs0 += __shfl_xor(rs0, 2, 64);
    rs1 += __shfl_xor(rs1, 1, 64); rs1 += __shfl_xor(rs1, 2, 64);
    if (s_slot == 0) { rsx_s[s_row0] = rs0; rsx_s[s_row1] = rs1; }
    __syncthreads();
  }

  // epilogue: C/D layout of the 32x32 MFMA: col (position) = lane & 31, row (channel) = (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5)
  TOut* out = static_cast<TOut*>(a.out);
  // the block's 128 channel parameters through LDS (the operand slots are free after the loop's last barrier), read per
  // accumulator register from an index the compiler cannot hoist, as conv_w8a8_kernel does
  float* colp = reinterpret_cast<float*>(&lds[0][0][0]);  // [4][128]: weight scale, rounded weight offset, bias, the phase's weight sum
  if (tid < TBM) {
    int m = m0 + tid;
    m = m < a.OC ? m : a.OC - 1;
    colp[tid] = a.w_scale[a.w_per_row ? m : 0];
    colp[TBM + tid] = a.w_offset ? rne(a.w_offset[a.w_per_row ? m : 0]) : 0.0f;
    colp[2 * TBM + tid] = a.bias ? (float)load_any(a.bias, a.bias_dt, m) : 0.0f;
    colp[3 * TBM + tid] = (float)a.tapsum[(int64_t)a.OC * a.taps + (int64_t)p * a.OC + m];
  }
  __syncthreads();
  const float sx = a.x_scale[0];
  const float ox = a.x_offset ? rne(a.x_offset[0]) : 0.0f;
  float oscale = 1.0f, ooff = 0.0f;
  if constexpr (REQUANT) {
    oscale = a.out_scale[0];
    ooff = a.out_offset ? rne(a.out_offset[0]) : 0.0f;
  }
  const int64_t ohw = (int64_t)a.OH * a.OW;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int col = wn * 64 + j * 32 + (lane & 31);
    const int n = n0 + col;
    if (n >= npos) continue;
    const int b = n / grid_hw, pp = n - b * grid_hw;
    const int gi = pp / fw.extent, gj = pp - gi * fw.extent;
    int ta_lo, ta_hi, tb_lo, tb_hi;
    tap_range_down(gi + fh.off0, mh, fh.n, a.H, ta_lo, ta_hi);
    tap_range_down(gj + fw.off0, mw, fw.n, a.W, tb_lo, tb_hi);
    const bool full = ta_lo == 0 && ta_hi == fh.n && tb_lo == 0 && tb_hi == fw.n;
    const float cnt = (float)(a.C * (ta_hi - ta_lo) * (tb_hi - tb_lo));  // C * |V(p)| < 131072: exact
    const float rsx = want_rsx ? (float)rsx_s[col] : 0.0f;
    const size_t out_base = (size_t)b * a.OC * ohw + (size_t)(rh + a.sh * gi) * a.OW + (rw + a.sw * gj);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int m = m0 + wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
        if (m >= a.OC) continue;
        int c = m - m0;
        asm volatile("" : "+v"(c));
        const float sw = colp[c], ow = colp[TBM + c], bias = colp[2 * TBM + c];
        float rsw = 0.0f;
        if (ox != 0.0f) {  // sum of the weight codes over the phase's taps inside the input (the phase total away from the border)
          if (full) {
            rsw = colp[3 * TBM + c];
          } else {
            const int32_t* ts = a.tapsum + (int64_t)m * a.taps + tab.tap_begin[p];
            int s = 0;
            for (int y = ta_lo; y < ta_hi; ++y)
              for (int x = tb_lo; x < tb_hi; ++x) s += ts[y * fw.n + x];
            rsw = (float)s;
          }
        }
        const float y = conv_affine(acc[i][j][e], ox, rsw, ow, rsx, cnt, sx, sw, a.bias != nullptr, bias);
        conv_store<TOut, REQUANT>(out + out_base + (size_t)m * ohw, y, a.y_dt, oscale, ooff, a.out_lo, a.out_hi);
      }
    }
  }
}

struct ConvtGeometry {
  int64_t OH, OW, Cp, taps, Kp, nph;
  ConvWorkspace ws;
};

int64_t gcd64(int64_t x, int64_t y) {
  while (y) { const int64_t t = x % y; x = y; y = t; }
  return x;
}

// One axis of the phase table: for every residue r < s the taps k < K with s | r + pad - k * d and the outputs o = r (mod s)
void axis_phases(int64_t K, int64_t s, int64_t pad, int64_t d, int64_t O, AxisPhase* out, int* kstep, int* ostep) {
  const int64_t g = gcd64(s, d);
  *kstep = (int)(s / g);
  *ostep = (int)(-(d / g));
  for (int64_t r = 0; r < s; ++r) {
    int64_t k0 = -1;
    for (int64_t k = 0; k < K && k < s / g; ++k)
      if ((r + pad - k * d) % s == 0) { k0 = k; break; }
    AxisPhase& f = out[r];
    f.k0 = k0 < 0 ? 0 : (int)k0;
    f.n = k0 < 0 ? 0 : (int)((K - k0 + s / g - 1) / (s / g));
    f.off0 = k0 < 0 ? 0 : (int)((r + pad - k0 * d) / s);
    f.extent = r < O ? (int)((O - r + s - 1) / s) : 0;
  }
}

// 0 with the geometry filled in, else the status of the first check that fails (no HIP call is made here)
int convt_geometry(int64_t B, int64_t C, int64_t OC, const int64_t* in, const int64_t* k, const int64_t* s, const int64_t* p, const int64_t* op,
                   const int64_t* d, int x_nhwc, ConvtGeometry* g) {
  int rc = check_conv_axes("transposed convolution", 2, B, C, OC, in, k, s, p, d);
  if (rc) return rc;
  if (op[0] < 0 || op[1] < 0 || op[0] >= (s[0] > d[0] ? s[0] : d[0]) || op[1] >= (s[1] > d[1] ? s[1] : d[1]))
    return fail(FFQ_ERR_ARG, "output padding must be >= 0 and smaller than either stride or dilation");
  if (s[0] * s[1] > kMaxPhases)
    return fail(FFQ_ERR_ARG, "stride_h * stride_w = %lld exceeds %d (the phase table)", (long long)(s[0] * s[1]), kMaxPhases);
  rc = check_conv_reduction(C, 2, k);
  if (rc) return rc;
  if (x_nhwc && C % 16 != 0) return fail(FFQ_ERR_DTYPE, "channels-last input codes need C %% 16 == 0");
  if (in[0] < 1 || in[1] < 1) return fail(FFQ_ERR_ARG, "a transposed convolution of an empty image");
  g->OH = (in[0] - 1) * s[0] - 2 * p[0] + d[0] * (k[0] - 1) + op[0] + 1;
  g->OW = (in[1] - 1) * s[1] - 2 * p[1] + d[1] * (k[1] - 1) + op[1] + 1;
  if (g->OH < 1 || g->OW < 1) return fail(FFQ_ERR_ARG, "the padding leaves no output (%lld x %lld)", (long long)g->OH, (long long)g->OW);
  g->Cp = (C + 15) / 16 * 16;
  g->taps = k[0] * k[1];
  g->Kp = g->taps * g->Cp;
  g->nph = s[0] * s[1];
  const int64_t o[2] = {g->OH, g->OW};
  const int64_t npos = product_capped(B, 2, o), voxels = product_capped(B, 2, in);
  if (g->OH > ((int64_t)1 << 30) || g->OW > ((int64_t)1 << 30) || npos >= ((int64_t)1 << 31) - kMaxPhases * TBN ||
      mul_capped(voxels, g->Cp, kConvBig) >= kConvBig || OC >= ((int64_t)1 << 31) || mul_capped(npos, OC, kConvBig) >= kConvBig ||
      mul_capped(OC, g->taps * (g->Cp / 16), kConvBig) >= kConvBig)
    return fail(FFQ_ERR_ARG, "extent too large for one launch");
  g->ws = conv_workspace(voxels * g->Cp, x_nhwc, OC * g->Kp, OC * g->taps + OC * kMaxPhases);
  return FFQ_OK;
}

}  // namespace
}  // namespace ffq

using namespace ffq;

extern "C" size_t ffq_conv_transpose2d_w8a8_workspace_bytes(int64_t B, int64_t C, int64_t H, int64_t W, int64_t OC, int64_t KH,
                                                            int64_t KW, int x_nhwc) {
  const int64_t in[2] = {H, W}, k[2] = {KH, KW};
  return conv_workspace_query(B, C, OC, 2, in, k, x_nhwc, kMaxPhases);
}

extern "C" int ffq_conv_transpose2d_w8a8(const int8_t* xq, int x_nhwc, const int8_t* wq, const float* x_scale, const float* x_offset,
                                         const float* w_scale, const float* w_offset, int w_per_channel, const void* bias, int bias_dt,
                                         void* out, int out_dt, const float* out_scale, const float* out_offset, double out_num_bits,
                                         int y_dt, int64_t B, int64_t C, int64_t H, int64_t W, int64_t OC, int64_t KH, int64_t KW,
                                         int64_t stride_h, int64_t stride_w, int64_t pad_h, int64_t pad_w, int64_t out_pad_h,
                                         int64_t out_pad_w, int64_t dil_h, int64_t dil_w, void* workspace, size_t workspace_bytes,
                                         void* stream) {
  ConvtGeometry g;
  const int64_t in[2] = {H, W}, k[2] = {KH, KW}, st[2] = {stride_h, stride_w}, pd[2] = {pad_h, pad_w};
  const int64_t op[2] = {out_pad_h, out_pad_w}, dl[2] = {dil_h, dil_w};
  int rc = convt_geometry(B, C, OC, in, k, st, pd, op, dl, x_nhwc, &g);
  if (rc) return rc;
  const bool requant = out_scale != nullptr;
  rc = check_conv_output("transposed convolution", bias, bias_dt, requant, out_dt, out_num_bits, y_dt);
  if (rc) return rc;
  if (B == 0 || OC == 0) return FFQ_OK;
  rc = check_conv_buffers("transposed convolution", xq, x_nhwc, wq, x_scale, w_scale, out, workspace, workspace_bytes, g.ws.total());
  if (rc) return rc;

  // the phase table: per-axis residues, then per phase the tile prefix and the first tap of the phase-major order
  PhaseTable tab = {};
  axis_phases(KH, stride_h, pad_h, dil_h, g.OH, tab.ah, &tab.kstep_h, &tab.ostep_h);
  axis_phases(KW, stride_w, pad_w, dil_w, g.OW, tab.aw, &tab.kstep_w, &tab.ostep_w);
  int64_t tiles = 0, tap = 0;
  for (int64_t rh = 0; rh < stride_h; ++rh)
    for (int64_t rw = 0; rw < stride_w; ++rw) {
      const int64_t p = rh * stride_w + rw;
      tiles += (B * tab.ah[rh].extent * tab.aw[rw].extent + TBN - 1) / TBN;
      tab.tile_end[p] = (int)tiles;
      tab.tap_begin[p] = (int)tap;
      tap += (int64_t)tab.ah[rh].n * tab.aw[rw].n;
    }
  const int64_t tiles_m = (OC + TBM - 1) / TBM;
  if (tiles * tiles_m >= ((int64_t)1 << 31)) return fail(FFQ_ERR_ARG, "extent too large for one launch");

  hipStream_t s = static_cast<hipStream_t>(stream);
  ConvBuffers buf;
  rc = carve_conv_workspace(xq, x_nhwc, workspace, g.ws, OC * g.taps + OC * g.nph, s, &buf);
  if (rc) return rc;
  const int groups = (int)(g.Cp / 16);
  const int64_t n_in = x_nhwc ? 0 : B * H * W * groups;
  const int64_t n_w = OC * g.taps * groups;
  const int64_t threads = n_in + n_w;
  if ((threads + 255) / 256 >= ((int64_t)1 << 31)) return fail(FFQ_ERR_ARG, "extent too large for one launch");
  convt_reorder_kernel<<<(unsigned)((threads + 255) / 256), 256, 0, s>>>(xq, buf.xn, n_in, (int)C, H * W, groups, wq, buf.wn, n_w,
                                                                          (int)g.taps, (int)KW, (int)OC, (int)stride_h, (int)stride_w,
                                                                          (int)pad_h, (int)pad_w, (int)dil_h, (int)dil_w, buf.tapsum, tab);
  rc = check_launch("convt_reorder_kernel");
  if (rc) return rc;

  ConvtArgs a;
  a.wq = buf.wn; a.xq = buf.xn; a.tapsum = buf.tapsum;
  fill_conv_operands(a, x_scale, x_offset, w_scale, w_offset, w_per_channel, bias, bias_dt, out, out_scale, out_offset, out_num_bits, y_dt);
  a.B = (int)B; a.OC = (int)OC; a.C = (int)C; a.Cp = (int)g.Cp; a.H = (int)H; a.W = (int)W;
  a.OH = (int)g.OH; a.OW = (int)g.OW; a.taps = (int)g.taps;
  a.sh = (int)stride_h; a.sw = (int)stride_w; a.nph = (int)g.nph;
  a.Kp = (int)g.Kp;
  a.tiles_m = (int)tiles_m;
  const unsigned grid = (unsigned)(tiles * tiles_m);
  dispatch_conv_output(requant, out_dt, [&](auto t, auto q) {
    convt_w8a8_kernel<typename decltype(t)::type, decltype(q)::value><<<grid, 256, 0, s>>>(a, tab);
  });
  return check_launch("convt_w8a8_kernel");
}
