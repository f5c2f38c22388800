// ffq_conv.hip — the W8A8 convolution (QuantizedConv1d / QuantizedConv2d) as an int8 implicit GEMM on the matrix cores of gfx950.
//
// Replaces fallback.conv1d / fallback.conv2d, src/fastforward/_gen/fallback.py:116-214: the reference dequantizes the input
// codes and the weight codes into data-dtype tensors, runs a float convolution and optionally re-quantizes. Here the codes are
// contracted exactly in int32 and the affine parameters are applied once per output element (include/ffq.h, ffq_conv2d_w8a8):
//
//   y[b,n,p] = sx * sw[n'] * ( acc + ox * rsw(n,p) + ow[n'] * rsx(b,p) + C * |V(p)| * ox * ow[n'] )  (+ bias[n])
//
// V(p) is the set of filter taps whose input pixel lies inside the image. The reference pads the DEQUANTIZED input with 0.0,
// whose code (-ox) need not fit the container; here out-of-image taps read code 0 and the offset terms count only V(p).
// Channels padded up to a multiple of 16 hold code 0 as well and contribute to nothing.
//
// Two launches:
//   * conv_layout_kernel — the input codes NCHW -> NHWC with C padded to Cp = 16 * ceil(C / 16) (skipped for a channels-last
//     input with C % 16 == 0), the weight codes [OC, C, KH, KW] -> [OC, KH, KW, Cp], and the per-tap weight sums
//     tapsum[n, t] = sum_c wq[n, c, t] with their totals sum_t tapsum[n, t]: one grid, the two halves side by side.
//   * conv_w8a8_kernel — the tail kernel of ffq_linear.hip (128 x 128 x 64, register-staged, double-buffered LDS, 2 x 2 waves
//     of v_mfma_i32_32x32x32_i8) with the WEIGHT on the A side (rows = output channels, K = (kh, kw, c)) and the OUTPUT
//     POSITIONS on the B side: every 16-byte staging slot of a B row is one 16-channel run of one tap of the im2col matrix,
//     gathered from the NHWC codes (zeros outside the image). The B row lands on lane & 31 of the accumulator, so one
//     accumulator register over 32 lanes is 32 consecutive output positions of one channel: the epilogue stores NCHW directly.
#include "ffq_conv_host.h"
#include "ffq_conv_tile.h"

namespace ffq {
namespace {

constexpr int CBM = 128, CBN = 128, CBK = 64;
constexpr int kConvTileBytes = CBM * CBK;

struct ConvArgs {
  const int8_t* wq;       // [OC, Kp]: weight codes reordered to (kh, kw, c), Kp = KH * KW * Cp
  const int8_t* xq;       // [B, H, W, Cp]: input codes, channels innermost
  const int32_t* tapsum;  // [OC, KH * KW] then [OC] totals
  const float* x_scale; const float* x_offset;
  const float* w_scale; const float* w_offset; int w_per_row;
  const void* bias; int bias_dt;
  void* out;  // [B, OC, OH, OW]
  const float* out_scale; const float* out_offset;
  float out_lo, out_hi;
  int y_dt;
  int OC, C, Cp, H, W, KH, KW, OH, OW;
  int sh, sw, ph, pw, dh, dw;
  int Kp, npos, ohw;
  int tiles_m, tiles_n;
};

// -------------------------------------------------------------------------------------------------
// Layout pass. Threads [0, n_in) move the input: one (b, 16-channel group, pixel) each, pixel fastest so that each of the 16
// byte loads of a wave reads 64 consecutive bytes of one channel plane; the 16 bytes leave as one store. Threads
// [n_in, n_in + n_w) move the weight: one (n, tap, 16-channel group) each, and add the group's code sum into tapsum[n, tap] and
// into the total of row n (zeroed ahead of the launch).
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void conv_layout_kernel(const int8_t* __restrict__ x, int8_t* __restrict__ xn, int64_t n_in, int C,
                                                          int64_t HW, int groups, const int8_t* __restrict__ w, int8_t* __restrict__ wn,
                                                          int64_t n_w, int taps, int OC, int32_t* __restrict__ tapsum) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int Cp = groups * 16;
  if (idx < n_in) {
    nchw_to_nhwc16(x, xn, idx, C, HW, groups);
    return;
  }
  const int64_t j = idx - n_in;
  if (j >= n_w) return;
  weight_to_taps16(w, wn, j, C, groups, Cp, taps, OC, tapsum);
}

// -------------------------------------------------------------------------------------------------
// The implicit GEMM: [OC, Kp] weight codes x the im2col matrix of the NHWC codes [npos, Kp], block tile 128 x 128 x 64.
// A lane stages two B rows (output positions) and one 16-byte slot of each; the slot's tap (kh, kw) and channel offset c0
// advance by 64 k-bytes per step with no division. With weight offsets the lanes also sum the B rows' codes as they pass through
// their registers (rsx: zeros outside the image add nothing).
// -------------------------------------------------------------------------------------------------
template <typename TOut, bool REQUANT>
__global__ __launch_bounds__(256) void conv_w8a8_kernel(ConvArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[2][2][kConvTileBytes];
  __shared__ int rsx_s[CBN];

  // XCD-aware tile order, as the linear's tail kernel: blocks b, b+8, ... share an XCD and get a contiguous range of tiles
  const uint32_t nblk = gridDim.x;
  const uint32_t xcd = blockIdx.x & 7u, slot_in_xcd = blockIdx.x >> 3;
  const uint32_t q = nblk >> 3, r = nblk & 7u;
  const uint32_t tile_id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot_in_xcd;
  // position-major inside a group of tiles_m channel tiles: neighbours share the gathered activation panel
  const int tn = tile_id / a.tiles_m, tm = tile_id % a.tiles_m;
  const int m0 = tm * CBM, n0 = tn * CBN;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int s_row0 = tid >> 2, s_slot = tid & 3;
  const int s_row1 = s_row0 + 64;

  // the two staged output positions: image base (in bytes of the NHWC codes) and top-left input pixel; ok = inside npos
  int64_t pbase[2];
  int pih[2], piw[2];
  bool pok[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int n = n0 + (h ? s_row1 : s_row0);
    pok[h] = n < a.npos;
    const int nn = pok[h] ? n : 0;
    const int b = nn / a.ohw, p = nn - b * a.ohw;
    const int oh = p / a.OW, ow = p - oh * a.OW;
    pbase[h] = (int64_t)b * a.H * a.W * a.Cp;
    pih[h] = oh * a.sh - a.ph;
    piw[h] = ow * a.sw - a.pw;
  }
  // this lane's slot: k-byte s_slot * 16 of the step, as (kh, kw, c0)
  int c0 = s_slot * 16, kw = 0, kh = 0;
  auto normalize = [&]() {
    while (c0 >= a.Cp) {
      c0 -= a.Cp;
      if (++kw == a.KW) { kw = 0; ++kh; }
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

  const int ksteps = (a.Kp + CBK - 1) / CBK;
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
    if (row < a.OC && kb < a.Kp) v = *reinterpret_cast<const u32x4*>(a.wq + (size_t)row * a.Kp + kb);
    return v;
  };
  auto gather = [&](int h) {
    u32x4 v = {0u, 0u, 0u, 0u};
    const int ih = pih[h] + kh * a.dh, iw = piw[h] + kw * a.dw;
    if (pok[h] && kh < a.KH && (unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W)
      v = *reinterpret_cast<const u32x4*>(a.xq + pbase[h] + ((int64_t)ih * a.W + iw) * a.Cp + c0);
    return v;
  };
  auto fetch = [&](int kt) {  // called for kt = 0, 1, 2, ... in order: the slot's tap state advances here
    const int kb = kt * CBK + s_slot * 16;
    ra0 = load_a(m0 + s_row0, kb);
    ra1 = load_a(m0 + s_row1, kb);
    rb0 = gather(0);
    rb1 = gather(1);
    c0 += CBK;
    normalize();
  };
  auto stash = [&](int stage) {
    *reinterpret_cast<u32x4*>(&lds[stage][0][conv_swizzled(s_row0, s_slot)]) = ra0;
    *reinterpret_cast<u32x4*>(&lds[stage][0][conv_swizzled(s_row1, s_slot)]) = ra1;
    *reinterpret_cast<u32x4*>(&lds[stage][1][conv_swizzled(s_row0, s_slot)]) = rb0;
    *reinterpret_cast<u32x4*>(&lds[stage][1][conv_swizzled(s_row1, s_slot)]) = rb1;
  };

  fetch(0);
  add_rowsums();
  stash(0);
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
  const int taps = a.KH * a.KW;
  // the block's 128 channel parameters through LDS (the operand slots are free after the loop's last barrier): read per
  // accumulator register from an index the compiler cannot hoist, or the 32 unrolled registers' loads all go up front (spills)
  float* colp = reinterpret_cast<float*>(&lds[0][0][0]);  // [4][128]: weight scale, rounded weight offset, bias, weight row sum
  if (tid < CBM) {
    int m = m0 + tid;
    m = m < a.OC ? m : a.OC - 1;
    colp[tid] = a.w_scale[a.w_per_row ? m : 0];
    colp[CBM + tid] = a.w_offset ? rne(a.w_offset[a.w_per_row ? m : 0]) : 0.0f;
    colp[2 * CBM + tid] = a.bias ? (float)load_any(a.bias, a.bias_dt, m) : 0.0f;
    colp[3 * CBM + tid] = (float)a.tapsum[(int64_t)a.OC * taps + m];
  }
  __syncthreads();
  const float sx = a.x_scale[0];
  const float ox = a.x_offset ? rne(a.x_offset[0]) : 0.0f;
  float oscale = 1.0f, ooff = 0.0f;
  if constexpr (REQUANT) {
    oscale = a.out_scale[0];
    ooff = a.out_offset ? rne(a.out_offset[0]) : 0.0f;
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int col = wn * 64 + j * 32 + (lane & 31);
    const int n = n0 + col;
    if (n >= a.npos) continue;
    const int b = n / a.ohw, p = n - b * a.ohw;
    const int oh = p / a.OW, ow_ = p - oh * a.OW;
    int kh_lo, kh_hi, kw_lo, kw_hi;
    tap_range(oh * a.sh - a.ph, a.dh, a.KH, a.H, kh_lo, kh_hi);
    tap_range(ow_ * a.sw - a.pw, a.dw, a.KW, a.W, kw_lo, kw_hi);
    const bool full = kh_lo == 0 && kh_hi == a.KH && kw_lo == 0 && kw_hi == a.KW;
    const float cnt = (float)(a.C * (kh_hi - kh_lo) * (kw_hi - kw_lo));  // C * |V(p)| < 131072: exact
    const float rsx = want_rsx ? (float)rsx_s[col] : 0.0f;
    const size_t out_base = (size_t)b * a.OC * a.ohw + p;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int m = m0 + wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
        if (m >= a.OC) continue;
        int c = m - m0;
        asm volatile("" : "+v"(c));
        const float sw = colp[c], ow = colp[CBM + c], bias = colp[2 * CBM + c];
        float rsw = 0.0f;
        if (ox != 0.0f) {  // sum of the weight codes over the taps inside the image (the whole row away from the border)
          if (full) {
            rsw = colp[3 * CBM + c];
          } else {
            int s = 0;
            for (int y = kh_lo; y < kh_hi; ++y)
              for (int x = kw_lo; x < kw_hi; ++x) s += a.tapsum[(int64_t)m * taps + y * a.KW + x];
            rsw = (float)s;
          }
        }
        const float y = conv_affine(acc[i][j][e], ox, rsw, ow, rsx, cnt, sx, sw, a.bias != nullptr, bias);
        conv_store<TOut, REQUANT>(out + out_base + (size_t)m * a.ohw, y, a.y_dt, oscale, ooff, a.out_lo, a.out_hi);
      }
    }
  }
}

}  // namespace
}  // namespace ffq

using namespace ffq;

extern "C" size_t ffq_conv2d_w8a8_workspace_bytes(int64_t B, int64_t C, int64_t H, int64_t W, int64_t OC, int64_t KH, int64_t KW,
                                                  int x_nhwc) {
  const int64_t in[2] = {H, W}, k[2] = {KH, KW};
  return conv_workspace_query(B, C, OC, 2, in, k, x_nhwc, 1);
}

extern "C" int ffq_conv2d_w8a8(const int8_t* xq, int x_nhwc, const int8_t* wq, const float* x_scale, const float* x_offset,
                               const float* w_scale, const float* w_offset, int w_per_channel, const void* bias, int bias_dt, void* out,
                               int out_dt, const float* out_scale, const float* out_offset, double out_num_bits, int y_dt, int64_t B,
                               int64_t C, int64_t H, int64_t W, int64_t OC, int64_t KH, int64_t KW, int64_t stride_h, int64_t stride_w,
                               int64_t pad_h, int64_t pad_w, int64_t dil_h, int64_t dil_w, void* workspace, size_t workspace_bytes,
                               void* stream) {
  ConvGeometry g;
  const int64_t in[2] = {H, W}, k[2] = {KH, KW}, st[2] = {stride_h, stride_w}, pd[2] = {pad_h, pad_w}, dl[2] = {dil_h, dil_w};
  int rc = conv_geometry(2, B, C, OC, in, k, st, pd, dl, x_nhwc, &g);
  if (rc) return rc;
  const bool requant = out_scale != nullptr;
  rc = check_conv_output("convolution", bias, bias_dt, requant, out_dt, out_num_bits, y_dt);
  if (rc) return rc;
  if (B == 0 || OC == 0) return FFQ_OK;
  rc = check_conv_buffers("convolution", xq, x_nhwc, wq, x_scale, w_scale, out, workspace, workspace_bytes, g.ws.total());
  if (rc) return rc;

  hipStream_t s = static_cast<hipStream_t>(stream);
  ConvBuffers buf;
  rc = carve_conv_workspace(xq, x_nhwc, workspace, g.ws, OC * g.taps + OC, s, &buf);
  if (rc) return rc;
  const int groups = (int)(g.Cp / 16);
  const int64_t n_in = x_nhwc ? 0 : g.voxels * groups;
  const int64_t n_w = OC * g.taps * groups;
  const int64_t threads = n_in + n_w;
  conv_layout_kernel<<<(unsigned)((threads + 255) / 256), 256, 0, s>>>(xq, buf.xn, n_in, (int)C, H * W, groups, wq, buf.wn, n_w,
                                                                        (int)g.taps, (int)OC, buf.tapsum);
  rc = check_launch("conv_layout_kernel");
  if (rc) return rc;

  ConvArgs a;
  a.wq = buf.wn; a.xq = buf.xn; a.tapsum = buf.tapsum;
  fill_conv_operands(a, x_scale, x_offset, w_scale, w_offset, w_per_channel, bias, bias_dt, out, out_scale, out_offset, out_num_bits, y_dt);
  a.OC = (int)OC; a.C = (int)C; a.Cp = (int)g.Cp; a.H = (int)H; a.W = (int)W; a.KH = (int)KH; a.KW = (int)KW;
  a.OH = (int)g.o[0]; a.OW = (int)g.o[1];
  a.sh = (int)stride_h; a.sw = (int)stride_w; a.ph = (int)pad_h; a.pw = (int)pad_w; a.dh = (int)dil_h; a.dw = (int)dil_w;
  a.Kp = (int)g.Kp; a.npos = (int)g.npos; a.ohw = (int)(g.o[0] * g.o[1]);
  a.tiles_m = (int)((OC + CBM - 1) / CBM);
  a.tiles_n = (int)((g.npos + CBN - 1) / CBN);
  const unsigned grid = (unsigned)((int64_t)a.tiles_m * a.tiles_n);
  dispatch_conv_output(requant, out_dt, [&](auto t, auto q) {
    conv_w8a8_kernel<typename decltype(t)::type, decltype(q)::value><<<grid, 256, 0, s>>>(a);
  });
  return check_launch("conv_w8a8_kernel");
}
