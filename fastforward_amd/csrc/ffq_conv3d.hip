// ffq_conv3d.hip — the W8A8 3-D convolution (QuantizedConv3d) as an int8 implicit GEMM on the matrix cores of gfx950.
//
// Replaces fallback.conv3d, src/fastforward/_gen/fallback.py:218-265: the reference dequantizes the input codes and the weight
// codes into data-dtype tensors, runs a float convolution and optionally re-quantizes. Here the codes are contracted exactly in
// int32 and the affine parameters are applied once per output element (include/ffq_3d.h, ffq_conv3d_w8a8), as ffq_conv.hip does in
// two dimensions:
//
//   y[b,n,p] = sx * sw[n'] * ( acc + ox * rsw(n,p) + ow[n'] * rsx(b,p) + C * |V(p)| * ox * ow[n'] )  (+ bias[n])
//
// V(p) is the set of filter taps (kd, kh, kw) whose input voxel lies inside D x H x W: out-of-volume taps read code 0 and the
// offset terms count only V(p). Channels padded up to a multiple of 16 hold code 0 and contribute to nothing.
//
// Two launches, the plan of ffq_conv.hip with one more axis:
//   * conv3d_layout_kernel — the layout pass of the 2-D convolution with HW := D * H * W voxels per plane and taps := KD * KH * KW
//     (its two halves are ffq_conv_tile.h's): NCDHW -> NDHWC with C padded to Cp (skipped for a channels_last_3d input with
//     C % 16 == 0), the weight [OC, C, KD, KH, KW] -> [OC, KD, KH, KW, Cp], the per-tap weight sums and their totals.
//   * conv3d_w8a8_kernel — the 128 x 128 x 64 tile of conv_w8a8_kernel (register-staged, double-buffered LDS, 2 x 2 waves of
//     v_mfma_i32_32x32x32_i8, XCD-aware tile order) with K = (kd, kh, kw, c): every 16-byte staging slot of a B row is one
//     16-channel run of one tap, gathered from [B, D, H, W, Cp] (zeros outside the volume). One accumulator register over 32 lanes
//     is 32 consecutive output positions of one channel: the epilogue stores NCDHW directly.
#include "ffq_conv_host.h"
#include "ffq_conv_tile.h"

#include "../../include/ffq_3d.h"

namespace ffq {
namespace {

constexpr int CBM = 128, CBN = 128, CBK = 64;
constexpr int kConvTileBytes = CBM * CBK;

struct Conv3dArgs {
  const int8_t* wq;       // [OC, Kp]: weight codes reordered to (kd, kh, kw, c), Kp = KD * KH * KW * Cp
  const int8_t* xq;       // [B, D, H, W, Cp]: input codes, channels innermost
  const int32_t* tapsum;  // [OC, KD * KH * KW] then [OC] totals
  const float* x_scale; const float* x_offset;
  const float* w_scale; const float* w_offset; int w_per_row;
  const void* bias; int bias_dt;
  void* out;  // [B, OC, OD, OH, OW]
  const float* out_scale; const float* out_offset;
  float out_lo, out_hi;
  int y_dt;
  int OC, C, Cp, D, H, W, KD, KH, KW, OH, OW;
  int sd, sh, sw, pd, ph, pw, dd, dh, dw;
  int Kp, npos, ovol, ohw;  // ovol = OD * OH * OW, ohw = OH * OW
  int tiles_m, tiles_n;
};

__global__ __launch_bounds__(256) void conv3d_layout_kernel(const int8_t* __restrict__ x, int8_t* __restrict__ xn, int64_t n_in, int C,
                                                            int64_t DHW, int groups, const int8_t* __restrict__ w, int8_t* __restrict__ wn,
                                                            int64_t n_w, int taps, int OC, int32_t* __restrict__ tapsum) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int Cp = groups * 16;
  if (idx < n_in) {
    nchw_to_nhwc16(x, xn, idx, C, DHW, groups);
    return;
  }
  const int64_t j = idx - n_in;
  if (j >= n_w) return;
  weight_to_taps16(w, wn, j, C, groups, Cp, taps, OC, tapsum);
}

// -------------------------------------------------------------------------------------------------
// The implicit GEMM: [OC, Kp] weight codes x the im2col matrix of the NDHWC codes [npos, Kp], block tile 128 x 128 x 64.
// A lane stages two B rows (output positions) and one 16-byte slot of each; the slot's tap (kd, kh, kw) and channel offset c0
// advance by 64 k-bytes per step with no division. With weight offsets the lanes also sum the B rows' codes as they pass through
// their registers (rsx: zeros outside the volume add nothing).
// -------------------------------------------------------------------------------------------------
template <typename TOut, bool REQUANT>
__global__ __launch_bounds__(256) void conv3d_w8a8_kernel(Conv3dArgs a) {
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

  // the two staged output positions: volume base (in bytes of the NDHWC codes) and front-top-left input voxel; ok = inside npos
  int64_t pbase[2];
  int pid[2], pih[2], piw[2];
  bool pok[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int n = n0 + (h ? s_row1 : s_row0);
    pok[h] = n < a.npos;
    const int nn = pok[h] ? n : 0;
    const int b = nn / a.ovol, p = nn - b * a.ovol;
    const int od = p / a.ohw, p2 = p - od * a.ohw;
    const int oh = p2 / a.OW, ow = p2 - oh * a.OW;
    pbase[h] = (int64_t)b * a.D * a.H * a.W * a.Cp;
    pid[h] = od * a.sd - a.pd;
    pih[h] = oh * a.sh - a.ph;
    piw[h] = ow * a.sw - a.pw;
  }
  // this lane's slot: k-byte s_slot * 16 of the step, as (kd, kh, kw, c0)
  int c0 = s_slot * 16, kw = 0, kh = 0, kd = 0;
  auto normalize = [&]() {
    while (c0 >= a.Cp) {
      c0 -= a.Cp;
      if (++kw == a.KW) {
        kw = 0;
        if (++kh == a.KH) { kh = 0; ++kd; }
      }
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
  auto gather = [&](int h) {  // kd < KD: the slot is inside Kp (the ragged last k-step reads zeros), so c0 + 16 <= Cp of a real tap
    u32x4 v = {0u, 0u, 0u, 0u};
    const int id = pid[h] + kd * a.dd, ih = pih[h] + kh * a.dh, iw = piw[h] + kw * a.dw;
    if (pok[h] && kd < a.KD && (unsigned)id < (unsigned)a.D && (unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W)
      v = *reinterpret_cast<const u32x4*>(a.xq + pbase[h] + (((int64_t)id * a.H + ih) * a.W + iw) * a.Cp + c0);
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
  const int taps_hw = a.KH * a.KW, taps = a.KD * taps_hw;
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
    const int b = n / a.ovol, p = n - b * a.ovol;
    const int od = p / a.ohw, p2 = p - od * a.ohw;
    const int oh = p2 / a.OW, ow_ = p2 - oh * a.OW;
    int kd_lo, kd_hi, kh_lo, kh_hi, kw_lo, kw_hi;
    tap_range(od * a.sd - a.pd, a.dd, a.KD, a.D, kd_lo, kd_hi);
    tap_range(oh * a.sh - a.ph, a.dh, a.KH, a.H, kh_lo, kh_hi);
    tap_range(ow_ * a.sw - a.pw, a.dw, a.KW, a.W, kw_lo, kw_hi);
    const bool full = kd_lo == 0 && kd_hi == a.KD && kh_lo == 0 && kh_hi == a.KH && kw_lo == 0 && kw_hi == a.KW;
    const float cnt = (float)(a.C * (kd_hi - kd_lo) * (kh_hi - kh_lo) * (kw_hi - kw_lo));  // C * |V(p)| < 131072: exact
    const float rsx = want_rsx ? (float)rsx_s[col] : 0.0f;
    const size_t out_base = (size_t)b * a.OC * a.ovol + p;
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
        if (ox != 0.0f) {  // sum of the weight codes over the taps inside the volume (the whole row away from the border)
          if (full) {
            rsw = colp[3 * CBM + c];
          } else {
            const int32_t* row = a.tapsum + (int64_t)m * taps;
            int s = 0;
            for (int z = kd_lo; z < kd_hi; ++z)
              for (int y = kh_lo; y < kh_hi; ++y)
                for (int x = kw_lo; x < kw_hi; ++x) s += row[z * taps_hw + y * a.KW + x];
            rsw = (float)s;
          }
        }
        const float y = conv_affine(acc[i][j][e], ox, rsw, ow, rsx, cnt, sx, sw, a.bias != nullptr, bias);
        conv_store<TOut, REQUANT>(out + out_base + (size_t)m * a.ovol, y, a.y_dt, oscale, ooff, a.out_lo, a.out_hi);
      }
    }
  }
}

}  // namespace
}  // namespace ffq

using namespace ffq;

extern "C" size_t ffq_conv3d_w8a8_workspace_bytes(int64_t B, int64_t C, int64_t D, int64_t H, int64_t W, int64_t OC, int64_t KD, int64_t KH,
                                                  int64_t KW, int x_ndhwc) {
  const int64_t in[3] = {D, H, W}, k[3] = {KD, KH, KW};
  return conv_workspace_query(B, C, OC, 3, in, k, x_ndhwc, 1);
}

extern "C" int ffq_conv3d_w8a8(const int8_t* xq, int x_ndhwc, const int8_t* wq, const float* x_scale, const float* x_offset,
                               const float* w_scale, const float* w_offset, int w_per_channel, const void* bias, int bias_dt, void* out,
                               int out_dt, const float* out_scale, const float* out_offset, double out_num_bits, int y_dt, int64_t B,
                               int64_t C, int64_t D, int64_t H, int64_t W, int64_t OC, int64_t KD, int64_t KH, int64_t KW, int64_t stride_d,
                               int64_t stride_h, int64_t stride_w, int64_t pad_d, int64_t pad_h, int64_t pad_w, int64_t dil_d, int64_t dil_h,
                               int64_t dil_w, void* workspace, size_t workspace_bytes, void* stream) {
  ConvGeometry g;
  const int64_t in[3] = {D, H, W}, k[3] = {KD, KH, KW};
  const int64_t st[3] = {stride_d, stride_h, stride_w}, pd[3] = {pad_d, pad_h, pad_w}, dl[3] = {dil_d, dil_h, dil_w};
  int rc = conv_geometry(3, B, C, OC, in, k, st, pd, dl, x_ndhwc, &g);
  if (rc) return rc;
  const bool requant = out_scale != nullptr;
  rc = check_conv_output("convolution", bias, bias_dt, requant, out_dt, out_num_bits, y_dt);
  if (rc) return rc;
  if (B == 0 || OC == 0) return FFQ_OK;
  rc = check_conv_buffers("3-D convolution", xq, x_ndhwc, wq, x_scale, w_scale, out, workspace, workspace_bytes, g.ws.total());
  if (rc) return rc;

  hipStream_t s = static_cast<hipStream_t>(stream);
  ConvBuffers buf;
  rc = carve_conv_workspace(xq, x_ndhwc, workspace, g.ws, OC * g.taps + OC, s, &buf);
  if (rc) return rc;
  const int groups = (int)(g.Cp / 16);
  const int64_t n_in = x_ndhwc ? 0 : g.voxels * groups;
  const int64_t n_w = OC * g.taps * groups;
  const int64_t threads = n_in + n_w;
  conv3d_layout_kernel<<<(unsigned)((threads + 255) / 256), 256, 0, s>>>(xq, buf.xn, n_in, (int)C, D * H * W, groups, wq, buf.wn, n_w,
                                                                          (int)g.taps, (int)OC, buf.tapsum);
  rc = check_launch("conv3d_layout_kernel");
  if (rc) return rc;

  Conv3dArgs a;
  a.wq = buf.wn; a.xq = buf.xn; a.tapsum = buf.tapsum;
  fill_conv_operands(a, x_scale, x_offset, w_scale, w_offset, w_per_channel, bias, bias_dt, out, out_scale, out_offset, out_num_bits, y_dt);
  a.OC = (int)OC; a.C = (int)C; a.Cp = (int)g.Cp; a.D = (int)D; a.H = (int)H; a.W = (int)W; a.KD = (int)KD; a.KH = (int)KH; a.KW = (int)KW;
  a.OH = (int)g.o[1]; a.OW = (int)g.o[2];
  a.sd = (int)stride_d; a.sh = (int)stride_h; a.sw = (int)stride_w;
  a.pd = (int)pad_d; a.ph = (int)pad_h; a.pw = (int)pad_w;
  a.dd = (int)dil_d; a.dh = (int)dil_h; a.dw = (int)dil_w;
  a.Kp = (int)g.Kp; a.npos = (int)g.npos; a.ovol = (int)(g.o[0] * g.o[1] * g.o[2]); a.ohw = (int)(g.o[1] * g.o[2]);
  a.tiles_m = (int)((OC + CBM - 1) / CBM);
  a.tiles_n = (int)((g.npos + CBN - 1) / CBN);
  const unsigned grid = (unsigned)((int64_t)a.tiles_m * a.tiles_n);
  dispatch_conv_output(requant, out_dt, [&](auto t, auto q) {
    conv3d_w8a8_kernel<typename decltype(t)::type, decltype(q)::value><<<grid, 256, 0, s>>>(a);
  });
  return check_launch("conv3d_w8a8_kernel");
}
