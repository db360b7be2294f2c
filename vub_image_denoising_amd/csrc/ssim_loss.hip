// The SSIM term of combined_loss (gfx950): pytorch_msssim.ssim v1.0.0 -- 11-tap Gaussian
// window (sigma 1.5, normalised), applied separably with valid padding to x, y, x^2, y^2
// and xy (products formed in fp32 before filtering), C1 = (0.01 R)^2, C2 = (0.03 R)^2,
// mean of the SSIM map over [n, c, h-10, w-10] -- and its gradient by x.
//
// Forward: one block = one 32x32 tile of the valid map of one plane.  The 42x42 halos of
// x and y go to LDS (14 KiB), the five fields are filtered along x into LDS (42 rows x
// 32 columns each, 26 KiB), then along y into registers, four output rows per thread.
// Per pixel, with m1, m2, q, r, p the filtered x, y, x^2, y^2, xy:
//   A1 = 2 m1 m2 + C1     B1 = m1^2 + m2^2 + C1
//   A2 = 2 (p - m1 m2) + C2     B2 = (q - m1^2) + (r - m2^2) + C2     S = A1 A2 / (B1 B2)
// The block sums S in a fixed order into one fp32 partial; a one-block kernel sums the
// partials in float64 (no atomics: the same call gives the same bits).  For the backward
// the forward keeps the derivatives of S by the three filtered fields that depend on x:
//   Gq = dS/dq  = -S / B2
//   Gp = dS/dp  = 2 A1 / (B1 B2)
//   Gm = dS/dm1 = 2 m2 (A2 - A1) / (B1 B2) + 2 m1 S (1/B2 - 1/B1)
// (dA1 = 2 m2, dA2 = -2 m2, dB1 = 2 m1, dB2 = -2 m1 by m1).
//
// Backward: one block = one 32x32 tile of dx.  m1 = F x, q = F x^2, p = F xy, so
//   dx = scale (F'Gm + 2 x F'Gq + y F'Gp),  scale = gout weight / (n c (h-10) (w-10)),
// where F' is the transposed filter: the window is symmetric, so it is the same taps over
// the map padded with 10 zeros on every side.  The three 42x42 halos (positions outside
// the valid map read 0) and their row-filtered forms take 36 KiB of LDS.
//
// Both are HBM/LDS-bound stencil passes: 4-byte accesses coalesced along x (rows of an
// arbitrary W are not 16-byte aligned), 64-bit plane offsets.
#include "rdn_pointwise.h"

#include <math.h>

namespace {

constexpr int kWin = 11, kPad = kWin - 1, kTile = 32, kHalo = kTile + kPad, kRows = 4;

struct SsimTaps {
  float g[kWin];
};

// the window as the torch code builds it: exp in fp32, divided by the fp32 sum
static SsimTaps make_taps() {
  SsimTaps t;
  float s = 0.f;
  for (int i = 0; i < kWin; ++i) {
    const float c = (float)(i - kWin / 2);
    t.g[i] = expf(-(c * c) / 4.5f);
    s += t.g[i];
  }
  for (int i = 0; i < kWin; ++i) t.g[i] /= s;
  return t;
}

// rows r0 .. r0+3 of column c of a row-filtered field [kHalo][kTile], filtered along y
__device__ __forceinline__ void filter_y(const float (*f)[kTile], int r0, int c, const SsimTaps& t, float* acc) {
#pragma unroll
  for (int o = 0; o < kRows; ++o) acc[o] = 0.f;
#pragma unroll
  for (int j = 0; j < kRows + kPad; ++j) {
    const float v = f[r0 + j][c];
#pragma unroll
    for (int o = 0; o < kRows; ++o)
      if (j - o >= 0 && j - o < kWin) acc[o] += t.g[j - o] * v;
  }
}

__global__ __launch_bounds__(256) void ssim_fwd_kernel(const float* __restrict__ x, const float* __restrict__ y, int h, int w,
                                                       SsimTaps taps, float c1, float c2, float* __restrict__ coef,
                                                       int64_t cstride, float* __restrict__ part) {
  __shared__ float sx[kHalo][kHalo], sy[kHalo][kHalo];
  __shared__ float hf[5][kHalo][kTile];
  __shared__ float red[4];
  const int tid = threadIdx.x;
  const int oh = h - kPad, ow = w - kPad;
  const int ty0 = blockIdx.y * kTile, tx0 = blockIdx.x * kTile;
  const int64_t plane = blockIdx.z;
  const float* __restrict__ xp = x + plane * h * (int64_t)w;
  const float* __restrict__ yp = y + plane * h * (int64_t)w;
  for (int i = tid; i < kHalo * kHalo; i += 256) {
    const int r = i / kHalo, c = i - r * kHalo;
    const int gy = ty0 + r, gx = tx0 + c;
    const bool ok = gy < h && gx < w;
    const int64_t off = (int64_t)gy * w + gx;
    sx[r][c] = ok ? xp[off] : 0.f;
    sy[r][c] = ok ? yp[off] : 0.f;
  }
  __syncthreads();
  for (int i = tid; i < kHalo * kTile; i += 256) {
    const int r = i / kTile, c = i % kTile;
    float m1 = 0.f, m2 = 0.f, q = 0.f, rr = 0.f, p = 0.f;
#pragma unroll
    for (int k = 0; k < kWin; ++k) {
      const float a = sx[r][c + k], b = sy[r][c + k], g = taps.g[k];
      m1 += g * a;
      m2 += g * b;
      q += g * (a * a);
      rr += g * (b * b);
      p += g * (a * b);
    }
    hf[0][r][c] = m1; hf[1][r][c] = m2; hf[2][r][c] = q; hf[3][r][c] = rr; hf[4][r][c] = p;
  }
  __syncthreads();
  const int c = tid % kTile, r0 = (tid / kTile) * kRows;
  float m1[kRows], m2[kRows], q[kRows], rr[kRows], p[kRows];
  filter_y(hf[0], r0, c, taps, m1);
  filter_y(hf[1], r0, c, taps, m2);
  filter_y(hf[2], r0, c, taps, q);
  filter_y(hf[3], r0, c, taps, rr);
  filter_y(hf[4], r0, c, taps, p);
  float sum = 0.f;
  const int64_t cplane = plane * oh * (int64_t)ow;
#pragma unroll
  for (int o = 0; o < kRows; ++o) {
    const int oy = ty0 + r0 + o, ox = tx0 + c;
    if (oy < oh && ox < ow) {
      const float mm = m1[o] * m2[o], m11 = m1[o] * m1[o], m22 = m2[o] * m2[o];
      const float a1 = 2.f * mm + c1, a2 = 2.f * (p[o] - mm) + c2;
      const float b1 = m11 + m22 + c1, b2 = (q[o] - m11) + (rr[o] - m22) + c2;
      const float ib1 = 1.f / b1, ib2 = 1.f / b2, ib = ib1 * ib2;
      const float s = a1 * a2 * ib;
      sum += s;
      if (coef) {
        const int64_t off = cplane + (int64_t)oy * ow + ox;
        coef[off] = 2.f * m2[o] * (a2 - a1) * ib + 2.f * m1[o] * s * (ib2 - ib1);   // Gm
        coef[cstride + off] = -s * ib2;                                            // Gq
        coef[2 * cstride + off] = 2.f * a1 * ib;                                   // Gp
      }
    }
  }
  block_wave_sums(sum, red);
  if (tid == 0)
    part[((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void ssim_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                       const float* __restrict__ coef, int64_t cstride, int h, int w,
                                                       SsimTaps taps, float weight, double count,
                                                       const float* __restrict__ gout, float* __restrict__ dx, int accumulate) {
  __shared__ float sg[3][kHalo][kHalo];
  __shared__ float hf[3][kHalo][kTile];
  const int tid = threadIdx.x;
  const int oh = h - kPad, ow = w - kPad;
  const int ty0 = blockIdx.y * kTile, tx0 = blockIdx.x * kTile;
  const int64_t plane = blockIdx.z;
  const float* __restrict__ cp = coef + plane * oh * (int64_t)ow;
  for (int i = tid; i < kHalo * kHalo; i += 256) {
    const int r = i / kHalo, c = i - r * kHalo;
    const int oy = ty0 - kPad + r, ox = tx0 - kPad + c;
    const bool ok = oy >= 0 && oy < oh && ox >= 0 && ox < ow;
    const int64_t off = ok ? (int64_t)oy * ow + ox : 0;
#pragma unroll
    for (int f = 0; f < 3; ++f) sg[f][r][c] = ok ? cp[f * cstride + off] : 0.f;
  }
  __syncthreads();
  for (int i = tid; i < kHalo * kTile; i += 256) {
    const int r = i / kTile, c = i % kTile;
    float a[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < kWin; ++k) {
#pragma unroll
      for (int f = 0; f < 3; ++f) a[f] += taps.g[k] * sg[f][r][c + k];
    }
#pragma unroll
    for (int f = 0; f < 3; ++f) hf[f][r][c] = a[f];
  }
  __syncthreads();
  const int c = tid % kTile, r0 = (tid / kTile) * kRows;
  float fm[kRows], fq[kRows], fp[kRows];
  filter_y(hf[0], r0, c, taps, fm);
  filter_y(hf[1], r0, c, taps, fq);
  filter_y(hf[2], r0, c, taps, fp);
  const float scale = (float)((double)gout[0] * (double)weight / count);
  const int64_t poff = plane * h * (int64_t)w;
#pragma unroll
  for (int o = 0; o < kRows; ++o) {
    const int gy = ty0 + r0 + o, gx = tx0 + c;
    if (gy < h && gx < w) {
      const int64_t off = poff + (int64_t)gy * w + gx;
      const float v = scale * (fm[o] + 2.f * x[off] * fq[o] + y[off] * fp[o]);
      dx[off] = accumulate ? dx[off] + v : v;
    }
  }
}

// shape checks shared by the three entry points; the tile grids of both kernels (the
// backward's, over h x w, is the larger) must fit one launch
static int check_shape(const char* what, int n, int c, int h, int w) {
  if (n < 1) { rdn_set_error("%s: n=%d must be >= 1", what, n); return RDN_E_ARG; }
  if (c < 1) { rdn_set_error("%s: c=%d must be >= 1", what, c); return RDN_E_ARG; }
  if ((int64_t)n * c > 65535) {   // the planes are the launches' grid.z
    rdn_set_error("%s: n*c=%lld planes must be <= 65535", what, (long long)n * c);
    return RDN_E_ARG;
  }
  if (h < kWin) { rdn_set_error("%s: h=%d must be >= %d", what, h, kWin); return RDN_E_ARG; }
  if (w < kWin) { rdn_set_error("%s: w=%d must be >= %d", what, w, kWin); return RDN_E_ARG; }
  if (h > (1 << 21)) { rdn_set_error("%s: h=%d must be <= 2^21", what, h); return RDN_E_ARG; }   // rows of tiles: grid.y
  const int64_t blocks = (int64_t)n * c * ((h + kTile - 1) / kTile) * ((w + kTile - 1) / kTile);
  if (blocks > (1 << 23)) {
    rdn_set_error("%s: n=%d c=%d h=%d w=%d are %lld tiles, more than 2^23", what, n, c, h, w, (long long)blocks);
    return RDN_E_ARG;
  }
  return RDN_OK;
}

static dim3 tile_grid(int n, int c, int rows, int cols) {
  return dim3((unsigned)((cols + kTile - 1) / kTile), (unsigned)((rows + kTile - 1) / kTile), (unsigned)(n * c));
}

}  // namespace

extern "C" int64_t rdn_ssim_workspace_size(int32_t n, int32_t c, int32_t h, int32_t w) {
  if (check_shape("rdn_ssim_workspace_size", n, c, h, w)) return 0;
  const dim3 g = tile_grid(n, c, h - kPad, w - kPad);
  return (int64_t)g.x * g.y * g.z * (int64_t)sizeof(float);
}

extern "C" int rdn_ssim_fwd(const float* x, const float* y, int32_t n, int32_t c, int32_t h, int32_t w, float data_range,
                            float* coef, float* ws, float* out, void* stream) {
  if (!x) { rdn_set_error("rdn_ssim_fwd: x is a null pointer"); return RDN_E_ARG; }
  if (!y) { rdn_set_error("rdn_ssim_fwd: y is a null pointer"); return RDN_E_ARG; }
  if (!ws) { rdn_set_error("rdn_ssim_fwd: ws is a null pointer"); return RDN_E_ARG; }
  if (!out) { rdn_set_error("rdn_ssim_fwd: out is a null pointer"); return RDN_E_ARG; }
  if (const int rc = check_shape("rdn_ssim_fwd", n, c, h, w)) return rc;
  const int oh = h - kPad, ow = w - kPad;
  const int64_t count = (int64_t)n * c * oh * ow;
  // (K R)^2 in double, rounded once, as the Python scalars of the torch code are
  const float c1 = (float)((0.01 * data_range) * (0.01 * data_range)), c2 = (float)((0.03 * data_range) * (0.03 * data_range));
  const dim3 grid = tile_grid(n, c, oh, ow);
  const int nb = (int)(grid.x * grid.y * grid.z);
  ssim_fwd_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(x, y, h, w, make_taps(), c1, c2, coef, count, ws);
  mean_final_kernel<1><<<1, 256, 0, (hipStream_t)stream>>>(ws, nb, (double)count, out);
  return rdn_check_launch("rdn_ssim_fwd");
}

extern "C" int rdn_ssim_bwd(const float* x, const float* y, const float* coef, int32_t n, int32_t c, int32_t h, int32_t w,
                            float weight, const float* gout, float* dx, int32_t accumulate, void* stream) {
  if (!x) { rdn_set_error("rdn_ssim_bwd: x is a null pointer"); return RDN_E_ARG; }
  if (!y) { rdn_set_error("rdn_ssim_bwd: y is a null pointer"); return RDN_E_ARG; }
  if (!coef) { rdn_set_error("rdn_ssim_bwd: coef is a null pointer"); return RDN_E_ARG; }
  if (!gout) { rdn_set_error("rdn_ssim_bwd: gout is a null pointer"); return RDN_E_ARG; }
  if (!dx) { rdn_set_error("rdn_ssim_bwd: dx is a null pointer"); return RDN_E_ARG; }
  if (const int rc = check_shape("rdn_ssim_bwd", n, c, h, w)) return rc;
  const int64_t count = (int64_t)n * c * (h - kPad) * (w - kPad);
  ssim_bwd_kernel<<<tile_grid(n, c, h, w), 256, 0, (hipStream_t)stream>>>(x, y, coef, count, h, w, make_taps(), weight,
                                                                           (double)count, gout, dx, accumulate);
  return rdn_check_launch("rdn_ssim_bwd");
}
