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
