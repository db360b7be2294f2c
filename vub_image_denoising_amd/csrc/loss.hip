// Pixel losses of the train step (gfx950): Charbonnier + MSE (combined_loss) and L1
// (nn.L1Loss, mean), forward and backward.  Each is a single pass over HBM; the forward
// sums are the two-level sum of rdn_pointwise.h, so the same call gives the same bits.
#include "rdn_pointwise.h"

namespace {

__global__ __launch_bounds__(256) void charb_partial_kernel(const float* __restrict__ p, const float* __restrict__ t,
                                                            int64_t n, float eps2, float* __restrict__ part) {
  float s[2] = {0.f, 0.f};   // Charbonnier, squared error
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float d = p[i] - t[i];
    s[0] += sqrtf(d * d + eps2);
    s[1] += d * d;
  }
  __shared__ float sh[2][4];
  block_wave_sums(s, sh);
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = sh[0][0] + sh[0][1] + sh[0][2] + sh[0][3];
    part[2 * blockIdx.x + 1] = sh[1][0] + sh[1][1] + sh[1][2] + sh[1][3];
  }
}

__global__ void charb_bwd_kernel(const float* __restrict__ p, const float* __restrict__ t, int64_t n, float eps2,
                                 float wc, float wm, const float* __restrict__ gout, float* __restrict__ dp) {
  const float g = gout[0] / (float)n;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float d = p[i] - t[i];
    dp[i] = g * (wc * (d / sqrtf(d * d + eps2)) + wm * 2.f * d);
  }
}

// L1: the same two levels.  n4 16-byte units go through 128-bit loads (0 when a pointer
// is not 16-byte aligned), the rest element by element; every thread's addition order is
// fixed by (n, n4, grid), so the sum does not depend on timing.
__global__ __launch_bounds__(256) void l1_partial_kernel(const float* __restrict__ p, const float* __restrict__ t,
                                                         int64_t n, int64_t n4, float* __restrict__ part) {
  float s = 0.f;
  vec4_loop(n, n4, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x, [&](int64_t i) {
    const f32x4 a = ((const f32x4*)p)[i], b = ((const f32x4*)t)[i];
    s += (fabsf(a[0] - b[0]) + fabsf(a[1] - b[1])) + (fabsf(a[2] - b[2]) + fabsf(a[3] - b[3]));
  }, [&](int64_t i) { s += fabsf(p[i] - t[i]); });
  __shared__ float sh[4];
  block_wave_sums(s, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

// torch.sign: -1, 0, +1 (0 for a tie, -0.0 against 0.0 included, and for NaN)
__device__ __forceinline__ float l1_sgn(float d) { return (float)((d > 0.f) - (d < 0.f)); }

__global__ __launch_bounds__(256) void l1_bwd_kernel(const float* __restrict__ p, const float* __restrict__ t, int64_t n,
                                                     int64_t n4, const float* __restrict__ gout, float* __restrict__ dp) {
  const float g = gout[0] / (float)n;
  vec4_loop(n, n4, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x, [&](int64_t i) {
    const f32x4 a = ((const f32x4*)p)[i], b = ((const f32x4*)t)[i];
    f32x4 o;
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q] = g * l1_sgn(a[q] - b[q]);
    ((f32x4*)dp)[i] = o;
  }, [&](int64_t i) { dp[i] = g * l1_sgn(p[i] - t[i]); });
}

}  // namespace

extern "C" int64_t rdn_reduce_workspace_size(int64_t) { return 2 * kRedBlocks * (int64_t)sizeof(float); }

extern "C" int rdn_charbonnier_fwd(const float* pred, const float* target, int64_t count, float eps, float* ws,
                                   float* out, void* stream) {
  if (!pred || !target || !ws || !out || count <= 0) { rdn_set_error("rdn_charbonnier_fwd: bad arguments"); return RDN_E_ARG; }
  const int nb = grid_for(count, 256 * 8, kRedBlocks);
  charb_partial_kernel<<<nb, 256, 0, RDN_STREAM>>>(pred, target, count, eps * eps, ws);
  mean_final_kernel<2><<<1, 256, 0, RDN_STREAM>>>(ws, nb, (double)count, out);
  return rdn_check_launch("rdn_charbonnier_fwd");
}

extern "C" int rdn_charbonnier_bwd(const float* pred, const float* target, int64_t count, float eps, float wc, float wm,
                                   const float* gout, float* dpred, void* stream) {
  if (!pred || !target || !gout || !dpred || count <= 0) { rdn_set_error("rdn_charbonnier_bwd: bad arguments"); return RDN_E_ARG; }
  charb_bwd_kernel<<<grid_for(count, 256 * 4), 256, 0, RDN_STREAM>>>(pred, target, count, eps * eps, wc, wm, gout, dpred);
  return rdn_check_launch("rdn_charbonnier_bwd");
}

extern "C" int rdn_l1_fwd(const float* pred, const float* target, int64_t count, float* ws, float* out, void* stream) {
  if (!pred || !target || !ws || !out || count <= 0) { rdn_set_error("rdn_l1_fwd: bad arguments"); return RDN_E_ARG; }
  const int nb = grid_for(count, 256 * 8, kRedBlocks);
  l1_partial_kernel<<<nb, 256, 0, RDN_STREAM>>>(pred, target, count, vec4_plan(count, pred, target).n4, ws);
  mean_final_kernel<1><<<1, 256, 0, RDN_STREAM>>>(ws, nb, (double)count, out);
  return rdn_check_launch("rdn_l1_fwd");
}

extern "C" int rdn_l1_bwd(const float* pred, const float* target, int64_t count, const float* gout, float* dpred,
                          void* stream) {
  if (!pred || !target || !gout || !dpred || count <= 0) { rdn_set_error("rdn_l1_bwd: bad arguments"); return RDN_E_ARG; }
  l1_bwd_kernel<<<grid_for(count, 256 * 8, 2048), 256, 0, RDN_STREAM>>>(pred, target, count,
                                                                        vec4_plan(count, pred, target, dpred).n4, gout, dpred);
  return rdn_check_launch("rdn_l1_bwd");
}
