// Whole-image denoising by overlapping tiles (gfx950): the tile grid, the gather of a
// batch of fixed-shape tiles out of an fp32 NCHW image (reflect padding at the bottom /
// right edge) and the windowed blend of the denoised tiles back into the image.
//
// Grid, per axis (extent n, requested tile, overlap); restated in sampling.plan_tiles:
//   t    = min(tile, ceil8(n))            tile extent
//   npad = max(n, t)                      > n only when n < t; then npad - n <= 7
//   s    = t - overlap                    stride (only used when there is more than 1 tile)
//   k    = npad == t ? 0 : ceil((npad - t) / s)
//   o_i  = min(i*s, npad - t), i = 0..k   the last tile is clamped to end at npad
// Both kernels derive the origins from these scalars; there is no device-side table.
// They are HBM-bound pointwise passes: 4-byte accesses coalesced along x (rows of an
// arbitrary W are not 16-byte aligned), 64-bit element offsets, one block per 256
// pixels of one row.
//
// Geometric self-ensemble (rdn_tile_gather_d4 / rdn_tile_accum_d4): every tile of the same
// grid is denoised under the first n_ens of the 8 flips and transposes of the square, d =
// 0..n_ens-1 (bit 0 flips x, bit 1 flips y, bit 2 transposes after the flips), and the tile
// the blend sees is e_g = (((v_0 + v_1) + v_2) + ... + v_{n_ens-1}) * (1/n_ens) with
// v_d = T_d^-1(sampler(T_d(tile_g))): an fp32 sum in ascending d, not contracted, scaled by
// an exact power of two.  The gather applies T_d, the accumulate T_d^-1 and the running
// mean; the definitions are with the kernels below.
#include "rdn_common.h"

namespace {

struct TileAxis {
  int n, t, npad, s, k, overlap;
};

static TileAxis make_axis(int n, int tile, int overlap) {
  TileAxis a;
  const int n8 = (n + 7) / 8 * 8;
  a.n = n;
  a.t = tile < n8 ? tile : n8;
  a.npad = n > a.t ? n : a.t;
  a.s = a.t - overlap;
  a.k = a.npad == a.t ? 0 : (a.npad - a.t + a.s - 1) / a.s;   // npad > t only with t == tile: s >= tile/2 > 0
  a.overlap = overlap;
  return a;
}

__device__ __forceinline__ int tile_origin(const TileAxis& a, int i) {
  const int o = i * a.s, last = a.npad - a.t;
  return o < last ? o : last;
}

// tiles covering position p (< n): i in [lo, hi].  The regular tiles i < k start at i*s;
// tile k is clamped to npad - t and may overlap two of them, so up to 3 tiles cover p.
__device__ __forceinline__ void tile_cover(const TileAxis& a, int p, int& lo, int& hi) {
  if (a.k == 0) { lo = hi = 0; return; }
  lo = p < a.t ? 0 : (p - a.t) / a.s + 1;
  hi = p >= a.npad - a.t ? a.k : p / a.s;
}

// w(i) = min(1, min(i+1, t-i) / (overlap+1)), an IEEE fp32 division
__device__ __forceinline__ float tile_window(const TileAxis& a, int i) {
  const int m = i + 1 < a.t - i ? i + 1 : a.t - i;
  const float w = __fdiv_rn((float)m, (float)(a.overlap + 1));
  return w < 1.f ? w : 1.f;
}

// reflect (torch 'reflect') of a padded position p >= n
__device__ __forceinline__ int tile_reflect(int p, int n) { return p < n ? p : 2 * (n - 1) - p; }

// one block row = one row of one channel of one tile; blockIdx.y walks x in steps of 256
__global__ __launch_bounds__(256) void tile_gather_kernel(const float* __restrict__ img, int c, TileAxis ay, TileAxis ax,
                                                          int64_t first, int64_t total, float* __restrict__ tiles) {
  const int x = blockIdx.y * 256 + threadIdx.x;
  if (x >= ax.t) return;
  const int r = blockIdx.x;                       // (j*c + ch)*th + yy
  const int yy = r % ay.t, jc = r / ay.t;
  const int ch = jc % c, j = jc / c;
  int64_t g = first + j;
  if (g > total - 1) g = total - 1;               // past the end: the last tile again
  const int nx = ax.k + 1, ny = ay.k + 1;
  const int kx = (int)(g % nx);
  const int64_t gy = g / nx;
  const int ky = (int)(gy % ny);
  const int64_t b = gy / ny;
  const int sy = tile_reflect(tile_origin(ay, ky) + yy, ay.n);
  const int sx = tile_reflect(tile_origin(ax, kx) + x, ax.n);
  tiles[(int64_t)r * ax.t + x] = img[((b * c + ch) * ay.n + sy) * (int64_t)ax.n + sx];
}

// one thread per output element.  Sum of wy*wx*v over the covering tiles in ascending ky,
// then ascending kx, divided by the same sum of weights; a pixel under exactly one tile
// takes that tile's value unchanged.
__global__ __launch_bounds__(256) void tile_blend_kernel(const float* __restrict__ tiles, int c, TileAxis ay, TileAxis ax,
                                                         float* __restrict__ out) {
#pragma clang fp contract(off)
  const int x = blockIdx.y * 256 + threadIdx.x;
  if (x >= ax.n) return;
  const int r = blockIdx.x;                       // (b*c + ch)*h + y
  const int y = r % ay.n, bc = r / ay.n;
  const int ch = bc % c, b = bc / c;
  int ylo, yhi, xlo, xhi;
  tile_cover(ay, y, ylo, yhi);
  tile_cover(ax, x, xlo, xhi);
  const int nx = ax.k + 1, ny = ay.k + 1;
  const int64_t plane = (int64_t)ay.t * ax.t;
  float v;
  if (ylo == yhi && xlo == xhi) {
    const int64_t g = ((int64_t)b * ny + ylo) * nx + xlo;
    v = tiles[(g * c + ch) * plane + (int64_t)(y - tile_origin(ay, ylo)) * ax.t + (x - tile_origin(ax, xlo))];
  } else {
    float acc = 0.f, wsum = 0.f;
    for (int ky = ylo; ky <= yhi; ++ky) {
      const int ty = y - tile_origin(ay, ky);
      const float wy = tile_window(ay, ty);
      for (int kx = xlo; kx <= xhi; ++kx) {
        const int tx = x - tile_origin(ax, kx);
        const float w = wy * tile_window(ax, tx);
        const int64_t g = ((int64_t)b * ny + ky) * nx + kx;
        acc += w * tiles[(g * c + ch) * plane + (int64_t)ty * ax.t + tx];
        wsum += w;
      }
    }
    v = __fdiv_rn(acc, wsum);
  }
  out[(int64_t)r * ax.n + x] = v;
}

// ---------------------------------------------------------------- geometric self-ensemble
// d in 0..7: bit 0 flips x, bit 1 flips y, bit 2 transposes (after the flips):
//   T_d(u)[y', x'] = u[sy, sx],  (y, x) = d&4 ? (x', y') : (y', x'),
//   sy = d&2 ? th-1-y : y,  sx = d&1 ? tw-1-x : x;  T_d(u) is tw x th when d&4.
// A pass is the transforms d0 .. d0+nd-1 of one tile shape; work item w = g*nd + (d - d0)
// (tile-major).  Both kernels move 32 x 32 patches through LDS rows of 33 floats: the side
// that runs along a source row writes patch[r][lane], the other side reads patch[r][lane]
// or, under a transpose, patch[lane][r] (bank (33*lane + r) % 32: conflict-free), so global
// loads and stores are both coalesced along x.  Flips only reverse an index inside the row.
// Tile extents are multiples of 8, so edge patches are partial: loads and stores are
// masked, and every thread of a block reaches every barrier.
constexpr int D4_PATCH = 32;

__device__ __forceinline__ int d4_flip(int i, int t, int on) { return on ? t - 1 - i : i; }

// one block = one patch of one channel of one output tile j; patches are counted on the output
__global__ __launch_bounds__(256) void tile_gather_d4_kernel(const float* __restrict__ img, int c, TileAxis ay, TileAxis ax,
                                                             int d0, int nd, int64_t first, int64_t total, int npy, int npx,
                                                             float* __restrict__ tiles) {
  __shared__ float patch[D4_PATCH][D4_PATCH + 1];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  int blk = blockIdx.x;                           // ((j*c + ch)*npy + py)*npx + px
  const int px = blk % npx; blk /= npx;
  const int py = blk % npy; blk /= npy;
  const int ch = blk % c, j = blk / c;
  int64_t w = first + j;
  if (w > total - 1) w = total - 1;               // past the end: the last work item again
  const int d = d0 + (int)(w % nd);
  const int64_t g = w / nd;
  const int nx = ax.k + 1, ny = ay.k + 1;
  const int kx = (int)(g % nx);
  const int64_t gy = g / nx;
  const int ky = (int)(gy % ny);
  const int64_t b = gy / ny;
  const bool tr = d & 4;
  const int oh = tr ? ax.t : ay.t, ow = tr ? ay.t : ax.t;
  const int oy0 = py * D4_PATCH, ox0 = px * D4_PATCH;
  const int y0 = tr ? ox0 : oy0, x0 = tr ? oy0 : ox0;       // the patch in tile coordinates (y, x)
  const float* plane = img + (b * c + ch) * ay.n * (int64_t)ax.n;
  const int x = x0 + tx;
#pragma unroll
  for (int k = 0; k < D4_PATCH / 8; ++k) {
    const int r = ty + 8 * k, y = y0 + r;
    if (y < ay.t && x < ax.t) {
      const int sy = tile_reflect(tile_origin(ay, ky) + d4_flip(y, ay.t, d & 2), ay.n);
      const int sx = tile_reflect(tile_origin(ax, kx) + d4_flip(x, ax.t, d & 1), ax.n);
      patch[r][tx] = plane[sy * (int64_t)ax.n + sx];
    }
  }
  __syncthreads();
  float* dst = tiles + ((int64_t)j * c + ch) * oh * (int64_t)ow;
  const int ox = ox0 + tx;
#pragma unroll
  for (int k = 0; k < D4_PATCH / 8; ++k) {
    const int r = ty + 8 * k, oy = oy0 + r;
    if (oy < oh && ox < ow) dst[oy * (int64_t)ow + ox] = tr ? patch[tx][r] : patch[r][tx];
  }
}

// one block = one patch of one channel of one tile of acc that the items [first, end) touch.
// A thread owns 4 elements of the patch and walks the tile's items in ascending d:
//   v_d[Y, X] = T_d^-1(src_d)[Y, X] = d&4 ? src_d[fx(X), fy(Y)] : src_d[fy(Y), fx(X)]
// with fy / fx the flips of bit 1 / bit 0.  d == 0 stores without reading acc, any other
// first d of the range adds to the stored partial sum, d == n_ens-1 scales by 1/n_ens.
__global__ __launch_bounds__(256) void tile_accum_d4_kernel(const float* __restrict__ src, float* __restrict__ acc, int c,
                                                            int th, int tw, int d0, int nd, int n_ens, int64_t first,
                                                            int64_t end, int npy, int npx) {
#pragma clang fp contract(off)
  __shared__ float patch[D4_PATCH][D4_PATCH + 1];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  int blk = blockIdx.x;                           // ((gi*c + ch)*npy + py)*npx + px
  const int px = blk % npx; blk /= npx;
  const int py = blk % npy; blk /= npy;
  const int ch = blk % c, gi = blk / c;
  const int64_t g = first / nd + gi;
  const int64_t wlo = g * nd > first ? g * nd : first;
  const int64_t whi = (g + 1) * nd < end ? (g + 1) * nd : end;      // wlo < whi: the host launches touched tiles only
  const int Y0 = py * D4_PATCH, X0 = px * D4_PATCH;
  const int64_t plane = (int64_t)th * tw;
  float* dst = acc + (g * c + ch) * plane;
  const int X = X0 + tx;
  float sum[D4_PATCH / 8] = {};
  for (int64_t w = wlo; w < whi; ++w) {           // block-uniform trip count
    const int d = d0 + (int)(w - g * nd);
    const bool tr = d & 4;
    const int sw = tr ? th : tw;                  // src_d is tw x th under a transpose
    const float* s = src + ((w - first) * c + ch) * plane;
#pragma unroll
    for (int k = 0; k < D4_PATCH / 8; ++k) {      // the lane runs along the source row
      const int r = ty + 8 * k;
      const int ly = Y0 + (tr ? tx : r), lx = X0 + (tr ? r : tx);
      if (ly < th && lx < tw) {
        const int fy = d4_flip(ly, th, d & 2), fx = d4_flip(lx, tw, d & 1);
        patch[r][tx] = tr ? s[fx * (int64_t)sw + fy] : s[fy * (int64_t)sw + fx];
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < D4_PATCH / 8; ++k) {
      const int r = ty + 8 * k, Y = Y0 + r;
      if (Y < th && X < tw) {
        const float v = tr ? patch[tx][r] : patch[r][tx];
        if (w > wlo) sum[k] += v;
        else if (d == 0) sum[k] = v;
        else sum[k] = dst[Y * (int64_t)tw + X] + v;
      }
    }
    __syncthreads();                              // the patch is rewritten by the next d
  }
  const bool done = d0 + (int)(whi - 1 - g * nd) == n_ens - 1;
  const float scale = 1.f / (float)n_ens;         // a power of two: exact
#pragma unroll
  for (int k = 0; k < D4_PATCH / 8; ++k) {
    const int Y = Y0 + ty + 8 * k;
    if (Y < th && X < tw) dst[Y * (int64_t)tw + X] = done ? sum[k] * scale : sum[k];
  }
}

// the grid's validity (header, rdn_tile_grid); c < 0: not checked
static int check_grid(const char* what, int h, int w, int tile, int overlap, int c) {
  if (tile < 16 || tile % 8) {
    rdn_set_error("%s: tile=%d must be a multiple of 8 and >= 16", what, tile);
    return RDN_E_ARG;
  }
  if (overlap < 0 || overlap > tile / 2) {
    rdn_set_error("%s: overlap=%d must be in [0, tile/2 = %d]", what, overlap, tile / 2);
    return RDN_E_ARG;
  }
  if (h < 8) { rdn_set_error("%s: h=%d must be >= 8", what, h); return RDN_E_ARG; }
  if (w < 8) { rdn_set_error("%s: w=%d must be >= 8", what, w); return RDN_E_ARG; }
  if (h > (1 << 23) || w > (1 << 23)) {   // 256-pixel row pieces are the launches' grid.y (< 65536)
    rdn_set_error("%s: h=%d / w=%d must be <= 2^23", what, h, w);
    return RDN_E_ARG;
  }
  if (c >= 0 && (c < 1 || c > 8)) { rdn_set_error("%s: c=%d must be in [1, 8]", what, c); return RDN_E_ARG; }
  return RDN_OK;
}

// a pass d0 .. d0+nd-1 on th x tw tiles (header, rdn_tile_gather_d4)
static int check_pass(const char* what, int d0, int nd, int th, int tw) {
  if (nd < 1) { rdn_set_error("%s: nd=%d must be >= 1", what, nd); return RDN_E_ARG; }
  if (d0 < 0) { rdn_set_error("%s: d0=%d must be >= 0", what, d0); return RDN_E_ARG; }
  if (d0 > 8 - nd) { rdn_set_error("%s: d0=%d + nd=%d must be <= 8", what, d0, nd); return RDN_E_ARG; }
  if (th != tw && d0 < 4 && d0 + nd > 4) {
    rdn_set_error("%s: the pass d0=%d, nd=%d straddles d = 4 on %d x %d tiles (one tile shape per pass)", what, d0, nd, th, tw);
    return RDN_E_ARG;
  }
  return RDN_OK;
}

// blocks of a 32 x 32-patch launch over `items` planes of oh x ow; 0: too many for one launch
static int64_t d4_blocks(int64_t items, int oh, int ow, int& npy, int& npx) {
  npy = (oh + D4_PATCH - 1) / D4_PATCH;
  npx = (ow + D4_PATCH - 1) / D4_PATCH;
  const int64_t per = (int64_t)npy * npx;
  return items > 0x7fffffffLL / per ? 0 : items * per;
}

}  // namespace

extern "C" int rdn_tile_grid(int32_t h, int32_t w, int32_t tile, int32_t overlap, int32_t out[4]) {
  if (!out) { rdn_set_error("rdn_tile_grid: out is a null pointer"); return RDN_E_ARG; }
  if (const int rc = check_grid("rdn_tile_grid", h, w, tile, overlap, -1)) return rc;
  const TileAxis ay = make_axis(h, tile, overlap), ax = make_axis(w, tile, overlap);
  out[0] = ay.t; out[1] = ax.t; out[2] = ay.k + 1; out[3] = ax.k + 1;
  return RDN_OK;
}

extern "C" int rdn_tile_gather(const float* img, int32_t n, int32_t c, int32_t h, int32_t w, int32_t tile, int32_t overlap,
                               int64_t first, int32_t count, float* tiles, void* stream) {
  if (!img) { rdn_set_error("rdn_tile_gather: img is a null pointer"); return RDN_E_ARG; }
  if (!tiles) { rdn_set_error("rdn_tile_gather: tiles is a null pointer"); return RDN_E_ARG; }
  if (const int rc = check_grid("rdn_tile_gather", h, w, tile, overlap, c)) return rc;
  if (n < 1) { rdn_set_error("rdn_tile_gather: n=%d must be >= 1", n); return RDN_E_ARG; }
  if (first < 0) { rdn_set_error("rdn_tile_gather: first=%lld must be >= 0", (long long)first); return RDN_E_ARG; }
  if (count < 1) { rdn_set_error("rdn_tile_gather: count=%d must be >= 1", count); return RDN_E_ARG; }
  const TileAxis ay = make_axis(h, tile, overlap), ax = make_axis(w, tile, overlap);
  const int64_t total = (int64_t)n * (ay.k + 1) * (ax.k + 1);
  const int64_t rows = (int64_t)count * c * ay.t;
  if (rows > 0x7fffffffLL) { rdn_set_error("rdn_tile_gather: count=%d tiles are too many rows for one launch", count); return RDN_E_SHAPE; }
  const dim3 grid((unsigned)rows, (unsigned)((ax.t + 255) / 256));
  tile_gather_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(img, c, ay, ax, first, total, tiles);
  return rdn_check_launch("rdn_tile_gather");
}

extern "C" int rdn_tile_blend(const float* tiles, int32_t n, int32_t c, int32_t h, int32_t w, int32_t tile, int32_t overlap,
                              float* out, void* stream) {
  if (!tiles) { rdn_set_error("rdn_tile_blend: tiles is a null pointer"); return RDN_E_ARG; }
  if (!out) { rdn_set_error("rdn_tile_blend: out is a null pointer"); return RDN_E_ARG; }
  if (const int rc = check_grid("rdn_tile_blend", h, w, tile, overlap, c)) return rc;
  if (n < 1) { rdn_set_error("rdn_tile_blend: n=%d must be >= 1", n); return RDN_E_ARG; }
  const TileAxis ay = make_axis(h, tile, overlap), ax = make_axis(w, tile, overlap);
  const int64_t rows = (int64_t)n * c * h;
  if (rows > 0x7fffffffLL) { rdn_set_error("rdn_tile_blend: n=%d images are too many rows for one launch", n); return RDN_E_SHAPE; }
  const dim3 grid((unsigned)rows, (unsigned)((w + 255) / 256));
  tile_blend_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(tiles, c, ay, ax, out);
  return rdn_check_launch("rdn_tile_blend");
}

extern "C" int rdn_tile_gather_d4(const float* img, int32_t n, int32_t c, int32_t h, int32_t w, int32_t tile, int32_t overlap,
                                  int32_t d0, int32_t nd, int64_t first, int32_t count, float* tiles, void* stream) {
  const char* what = "rdn_tile_gather_d4";
  if (!img) { rdn_set_error("%s: img is a null pointer", what); return RDN_E_ARG; }
  if (!tiles) { rdn_set_error("%s: tiles is a null pointer", what); return RDN_E_ARG; }
  if (const int rc = check_grid(what, h, w, tile, overlap, c)) return rc;
  if (n < 1) { rdn_set_error("%s: n=%d must be >= 1", what, n); return RDN_E_ARG; }
  const TileAxis ay = make_axis(h, tile, overlap), ax = make_axis(w, tile, overlap);
  if (const int rc = check_pass(what, d0, nd, ay.t, ax.t)) return rc;
  if (first < 0) { rdn_set_error("%s: first=%lld must be >= 0", what, (long long)first); return RDN_E_ARG; }
  if (count < 1) { rdn_set_error("%s: count=%d must be >= 1", what, count); return RDN_E_ARG; }
  const int64_t total = (int64_t)n * (ay.k + 1) * (ax.k + 1) * nd;
  const bool tr = d0 >= 4;                        // a pass that mixes both has th == tw
  int npy, npx;
  const int64_t blocks = d4_blocks((int64_t)count * c, tr ? ax.t : ay.t, tr ? ay.t : ax.t, npy, npx);
  if (!blocks) { rdn_set_error("%s: count=%d tiles are too many patches for one launch", what, count); return RDN_E_SHAPE; }
  tile_gather_d4_kernel<<<dim3((unsigned)blocks), 256, 0, (hipStream_t)stream>>>(img, c, ay, ax, d0, nd, first, total, npy, npx,
                                                                              tiles);
  return rdn_check_launch(what);
}

extern "C" int rdn_tile_accum_d4(const float* src, float* acc, int64_t n_tiles, int32_t c, int32_t th, int32_t tw, int32_t d0,
                                 int32_t nd, int32_t n_ens, int64_t first, int32_t count, void* stream) {
  const char* what = "rdn_tile_accum_d4";
  if (!src) { rdn_set_error("%s: src is a null pointer", what); return RDN_E_ARG; }
  if (!acc) { rdn_set_error("%s: acc is a null pointer", what); return RDN_E_ARG; }
  if (c < 1 || c > 8) { rdn_set_error("%s: c=%d must be in [1, 8]", what, c); return RDN_E_ARG; }
  if (th < 8 || th % 8 || th > (1 << 23)) { rdn_set_error("%s: th=%d must be a multiple of 8 in [8, 2^23]", what, th); return RDN_E_ARG; }
  if (tw < 8 || tw % 8 || tw > (1 << 23)) { rdn_set_error("%s: tw=%d must be a multiple of 8 in [8, 2^23]", what, tw); return RDN_E_ARG; }
  if (const int rc = check_pass(what, d0, nd, th, tw)) return rc;
  if (n_ens != 1 && n_ens != 2 && n_ens != 4 && n_ens != 8) {
    rdn_set_error("%s: n_ens=%d must be 1, 2, 4 or 8", what, n_ens);
    return RDN_E_ARG;
  }
  if (d0 + nd > n_ens) { rdn_set_error("%s: d0=%d + nd=%d must be <= n_ens=%d", what, d0, nd, n_ens); return RDN_E_ARG; }
  if (n_tiles < 1 || n_tiles > (1LL << 40)) { rdn_set_error("%s: n_tiles=%lld must be in [1, 2^40]", what, (long long)n_tiles); return RDN_E_ARG; }
  if (first < 0) { rdn_set_error("%s: first=%lld must be >= 0", what, (long long)first); return RDN_E_ARG; }
  if (count < 1) { rdn_set_error("%s: count=%d must be >= 1", what, count); return RDN_E_ARG; }
  const int64_t total = n_tiles * nd;
  if (first >= total) return RDN_OK;              // surplus items only
  const int64_t end = first + count < total ? first + count : total;
  const int64_t touched = (end - 1) / nd - first / nd + 1;
  int npy, npx;
  const int64_t blocks = d4_blocks(touched * c, th, tw, npy, npx);
  if (!blocks) { rdn_set_error("%s: count=%d tiles are too many patches for one launch", what, count); return RDN_E_SHAPE; }
  tile_accum_d4_kernel<<<dim3((unsigned)blocks), 256, 0, (hipStream_t)stream>>>(src, acc, c, th, tw, d0, nd, n_ens, first, end,
                                                                             npy, npx);
  return rdn_check_launch(what);
}
