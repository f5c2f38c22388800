// mx_map_probe.hip — the operand map of v_mfma_scale_f32_32x32x64_f8f6f4, established with exact data on the device.
//
// One wave, one instruction per case. The operands are filled under the map the GEMM of csrc/ffq_mx.hip uses:
//   lane l, r = l & 31, h = l >> 5 holds row r of A (B: of W): e2m1 k = 32h .. 32h + 31, element j at bits [4j, 4j + 4) of the first four
//   registers; e4m3 k = 16h .. 16h + 15 in registers 0-3 and k = 32 + 16h .. 32 + 16h + 15 in registers 4-7, a byte each;
//   the byte `opsel` of the scale register of lane (r, h) is the E8M0 scale of block h (k = 32h .. 32h + 31) of row r;
//   C/D: col = l & 31 (the B row), row = (reg & 3) + 8 (reg >> 2) + 4 (l >> 5) (the A row).
// (With e4m3 lanes holding 32 CONSECUTIVE k, the first guess, three quarters of the outputs of these cases are wrong.)
// Element values are small integers (e4m3) or any grid value (e2m1), the scale codes 126 .. 129 differ per row and block and the other
// three bytes of every scale register hold decoys, so a wrong row, k order, nibble order or scale byte cannot give the expected sums.
// Every sum is exact in fp32. Prints the number of mismatches per case (0 = the map holds) and what a scale byte of 255 does; with an
// argument, writes the raw operands and results of every case to that file.
//
//   hipcc --offload-arch=gfx950 -O2 -o mx_map_probe mx_map_probe.hip && ./mx_map_probe [dump.bin]
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

template <int FA, int FB, int OA, int OB>
__global__ void one_mfma(const i32x8* a, const i32x8* b, const int* sa, const int* sb, f32x16* c) {
  const int l = threadIdx.x;
  f32x16 acc = {};
  acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a[l], b[l], acc, FA, FB, OA, sa[l], OB, sb[l]);
  c[l] = acc;
}

static const float kE2M1[8] = {0.0f, 0.5f, 1.0f, 1.5f, 2.0f, 3.0f, 4.0f, 6.0f};
static double e2m1_value(unsigned c) { return (c & 8 ? -1.0 : 1.0) * kE2M1[c & 7]; }
static double e4m3_value(unsigned c) {
  const int e = (c >> 3) & 15, m = c & 7;
  const double v = e ? ldexp(1.0 + m / 8.0, e - 7) : ldexp(m / 8.0, -6);
  return c & 0x80 ? -v : v;
}
static unsigned e4m3_of_int(int v) {  // |v| <= 15: exact
  for (unsigned c = 0; c < 256; ++c)
    if ((c & 0x7F) != 0x7F && e4m3_value(c) == (double)v && !(v == 0 && c)) return c;
  abort();
}

static uint32_t rng_state = 12345u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

struct Case {
  unsigned a_code[32][64], b_code[32][64];  // element codes, [row][k]
  unsigned a_scale[32][2], b_scale[32][2];  // E8M0 codes, [row][block]
};

static void fill(Case& c, int fa, int fb) {
  for (int r = 0; r < 32; ++r)
    for (int k = 0; k < 64; ++k) {
      c.a_code[r][k] = fa == 4 ? rnd() % 16 : e4m3_of_int((int)(rnd() % 31) - 15);
      c.b_code[r][k] = fb == 4 ? rnd() % 16 : e4m3_of_int((int)(rnd() % 31) - 15);
    }
  for (int r = 0; r < 32; ++r)
    for (int h = 0; h < 2; ++h) {
      c.a_scale[r][h] = 127 + rnd() % 3;
      c.b_scale[r][h] = 126 + rnd() % 3;
    }
}

static void pack(const unsigned code[32][64], int fmt, i32x8* regs) {
  for (int l = 0; l < 64; ++l) {
    uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int r = l & 31, h = l >> 5;
    for (int j = 0; j < 32; ++j) {
      const unsigned v = fmt == 4 ? code[r][32 * h + j] : code[r][16 * h + (j % 16) + 32 * (j / 16)];
      if (fmt == 4) w[j / 8] |= v << (4 * (j % 8));
      else w[j / 4] |= v << (8 * (j % 4));
    }
    for (int i = 0; i < 8; ++i) regs[l][i] = (int)w[i];
  }
}

static void pack_scales(const unsigned scale[32][2], int opsel, int* regs) {
  for (int l = 0; l < 64; ++l) {
    uint32_t w = 0;
    for (int b = 0; b < 4; ++b) w |= (b == opsel ? scale[l & 31][l >> 5] : 120u + (rnd() % 16)) << (8 * b);
    regs[l] = (int)w;
  }
}

template <int FA, int FB, int OA, int OB>
static int run_case(const char* name, FILE* dump, bool nan_scale) {
  static Case c;
  fill(c, FA, FB);
  if (nan_scale) c.a_scale[3][1] = 255;
  i32x8 ha[64], hb[64];
  int hsa[64], hsb[64];
  float hc[64][16];
  pack(c.a_code, FA, ha);
  pack(c.b_code, FB, hb);
  pack_scales(c.a_scale, OA, hsa);
  pack_scales(c.b_scale, OB, hsb);
  i32x8 *da, *db;
  int *dsa, *dsb;
  f32x16* dc;
  if (hipMalloc(&da, sizeof ha) || hipMalloc(&db, sizeof hb) || hipMalloc(&dsa, sizeof hsa) || hipMalloc(&dsb, sizeof hsb) || hipMalloc(&dc, sizeof hc)) return -1;
  hipMemcpy(da, ha, sizeof ha, hipMemcpyHostToDevice);
  hipMemcpy(db, hb, sizeof hb, hipMemcpyHostToDevice);
  hipMemcpy(dsa, hsa, sizeof hsa, hipMemcpyHostToDevice);
  hipMemcpy(dsb, hsb, sizeof hsb, hipMemcpyHostToDevice);
  one_mfma<FA, FB, OA, OB><<<1, 64>>>(da, db, dsa, dsb, dc);
  if (hipMemcpy(hc, dc, sizeof hc, hipMemcpyDeviceToHost) != hipSuccess) { printf("%s: launch failed\n", name); return -1; }
  int bad = 0, nans = 0, nan_rows = 0;
  for (int m = 0; m < 32; ++m) {
    int row_nans = 0;
    for (int n = 0; n < 32; ++n) {
      double want = 0.0;
      for (int k = 0; k < 64; ++k) {
        const double av = FA == 4 ? e2m1_value(c.a_code[m][k]) : e4m3_value(c.a_code[m][k]);
        const double bv = FB == 4 ? e2m1_value(c.b_code[n][k]) : e4m3_value(c.b_code[n][k]);
        want += av * bv * ldexp(1.0, (int)c.a_scale[m][k / 32] - 127) * ldexp(1.0, (int)c.b_scale[n][k / 32] - 127);
      }
      // row m = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5), col n = lane & 31
      const int reg = (m & 3) + 4 * (m >> 3), lane = n + 32 * ((m >> 2) & 1);
      const float got = hc[lane][reg];
      if (got != got) { ++nans; ++row_nans; }
      if (nan_scale && m == 3) continue;
      if ((double)got != want) {
        if (bad < 4) printf("  %s: out[%d][%d] = %g, expected %g\n", name, m, n, got, want);
        ++bad;
      }
    }
    nan_rows += row_nans == 32;
  }
  if (nan_scale) {
    printf("%s: scale byte 255 on A row 3, block 1: %d NaN outputs, %d whole NaN rows, row 3 holds %s; other rows: %d mismatches\n", name, nans, nan_rows,
           hc[3][3] != hc[3][3] ? "NaN" : "numbers", bad);
    printf("  row 3 sample: %g %g %g\n", hc[0][3], hc[1][3], hc[31][3]);
  } else {
    printf("%s: %d mismatches of 1024\n", name, bad);
  }
  if (dump) {
    fwrite(ha, sizeof ha, 1, dump); fwrite(hb, sizeof hb, 1, dump); fwrite(hsa, sizeof hsa, 1, dump); fwrite(hsb, sizeof hsb, 1, dump);
    fwrite(hc, sizeof hc, 1, dump);
  }
  hipFree(da); hipFree(db); hipFree(dsa); hipFree(dsb); hipFree(dc);
  return bad;
}

int main(int argc, char** argv) {
  FILE* dump = argc > 1 ? fopen(argv[1], "wb") : nullptr;
  int bad = 0;
  bad |= run_case<0, 0, 0, 0>("e4m3 x e4m3, opsel 0/0", dump, false);
  bad |= run_case<0, 0, 2, 2>("e4m3 x e4m3, opsel 2/2", dump, false);
  bad |= run_case<0, 4, 0, 0>("e4m3 x e2m1, opsel 0/0", dump, false);
  bad |= run_case<0, 4, 2, 2>("e4m3 x e2m1, opsel 2/2", dump, false);
  bad |= run_case<4, 4, 0, 0>("e2m1 x e2m1, opsel 0/0", dump, false);
  bad |= run_case<4, 4, 2, 2>("e2m1 x e2m1, opsel 2/2", dump, false);
  bad |= run_case<0, 0, 1, 3>("e4m3 x e4m3, opsel 1/3", dump, false);
  bad |= run_case<4, 4, 0, 0>("e2m1 x e2m1, NaN scale", dump, true);
  bad |= run_case<0, 0, 2, 2>("e4m3 x e4m3, NaN scale", dump, true);
  if (dump) fclose(dump);
  printf(bad ? "MAP DOES NOT HOLD\n" : "MAP HOLDS\n");
  return bad ? 1 : 0;
}
