// PReLU backward as a pass of its own (gfx950): dY -> dYpre in the storage type, with the
// per-channel dalpha / dbias sums as per-block partials and a finalize launch.
#include "rdn_pointwise.h"

namespace {

constexpr int RDN_PRELU_PU = 4;   // pixel iterations per trip of the NHWC fast path

// dyp = dy * (pre > 0 ? 1 : a);  dalpha += sum_{pre<=0} pre*dy;  dbias += sum dyp
// (aten prelu backward: mask = input > 0, Activation.cpp; conv grad_bias = sum
// over N,H,W of grad_output).  Thread = 16-byte channel group of one pixel.
// (The element rule is rdn_prelu_bwd1's, written out in both loops with the channel mask:
// through the helper the masked form compiles to different code.)
template <typename T>
// (<= 64 VGPRs: one wave per SIMD still fits beside a two-wave weight-gradient block of
// the side stream -- 2 x 218 of 512 -- so the pass is not confined to the CUs the
// side stream leaves free)
__global__ __launch_bounds__(256, 1) void prelu_bwd_kernel(int64_t pixels, int H, int W, int C, int cpad,
                                                        const T* __restrict__ dy, int64_t dy_ps, int dy_c0,
                                                        int64_t dy_pl, const float* __restrict__ dy_nchw, const T* __restrict__ pre,
                                                        int64_t pre_ps, const float* __restrict__ alpha, T* __restrict__ dyp,
                                                        float* __restrict__ part) {
  constexpr int VEC = TypeInfo<T>::VEC;
  const int G = cpad / VEC;                 // groups per pixel
  const int ppb = 256 / G;                  // pixels per block iteration
  const int tid = threadIdx.x;
  const int grp = tid % G, pl = tid / G;
  const bool active = pl < ppb;
  float sa[VEC], sb[VEC], al[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    sa[k] = 0.f; sb[k] = 0.f;
    const int c = grp * VEC + k;
    al[k] = (active && c < C) ? alpha[c] : 0.f;
  }
  const int64_t stride = (int64_t)gridDim.x * ppb;
  int64_t p0 = (int64_t)blockIdx.x * ppb + pl;
  const int64_t dy_cf = rdn_coff(dy_c0 + grp * VEC, dy_ps, dy_pl);   // channel offset of this thread's unit
  // NHWC fast path: 4 pixel iterations per trip with all 8 loads issued first
  // (unconditional, from a clamped valid pixel) -- the plain loop exposes one
  // HBM round trip per pixel, which is what the small level-2/3 passes pay
  if (active && !dy_nchw && ((dy_ps | dy_c0) % VEC) == 0) {
    for (; p0 < pixels; p0 += RDN_PRELU_PU * stride) {
      u32x4 gv[RDN_PRELU_PU], xv[RDN_PRELU_PU];
#pragma unroll
      for (int u = 0; u < RDN_PRELU_PU; ++u) {
        const int64_t pu = p0 + u * stride;
        const int64_t pc = pu < pixels ? pu : p0;
        gv[u] = *(const u32x4*)(dy + pc * dy_ps + dy_cf);
        xv[u] = *(const u32x4*)(pre + pc * pre_ps + grp * VEC);
      }
#pragma unroll
      for (int u = 0; u < RDN_PRELU_PU; ++u) {
        const int64_t pu = p0 + u * stride;
        if (pu >= pixels) break;
        float g[VEC], x[VEC], o[VEC];
        Unit16<T>::unpack(gv[u], g);
        Unit16<T>::unpack(xv[u], x);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          const int c = grp * VEC + k;
          const bool valid = c < C;
          const bool pos = x[k] > 0.f;
          o[k] = valid ? (pos ? g[k] : al[k] * g[k]) : 0.f;
          if (valid && !pos) sa[k] += x[k] * g[k];
          sb[k] += o[k];
        }
        *(u32x4*)(dyp + pu * cpad + grp * VEC) = Unit16<T>::pack(o);
      }
    }
  }
  if (active) {
    for (int64_t p = p0; p < pixels; p += stride) {
      float g[VEC], x[VEC], o[VEC];
      if (dy_nchw) {
        const int64_t hw = (int64_t)H * W;
        const int64_t nimg = p / hw, r = p - nimg * hw;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          const int c = grp * VEC + k;
          g[k] = c < C ? dy_nchw[(nimg * C + c) * hw + r] : 0.f;
        }
      } else {
        const T* src = dy + p * dy_ps + dy_cf;
        if (((dy_ps | dy_c0) % VEC) == 0) {
          Unit16<T>::unpack(*(const u32x4*)src, g);
        } else {
#pragma unroll
          for (int k = 0; k < VEC; ++k) g[k] = to_f32(src[k]);
        }
      }
      Unit16<T>::unpack(*(const u32x4*)(pre + p * pre_ps + grp * VEC), x);
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const int c = grp * VEC + k;
        const bool valid = c < C;
        const bool pos = x[k] > 0.f;
        o[k] = valid ? (pos ? g[k] : al[k] * g[k]) : 0.f;
        if (valid && !pos) sa[k] += x[k] * g[k];
        sb[k] += o[k];
      }
      *(u32x4*)(dyp + p * cpad + grp * VEC) = Unit16<T>::pack(o);
    }
  }
  // block reduction per channel: LDS [ppb][cpad] x 2, then one partial per
  // (block, channel) -- no atomics (one address per channel would serialise
  // thousands of blocks); prelu_finalize_kernel sums the partials.
  __shared__ float red[2][256 * 8];
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    red[0][tid * VEC + k] = active ? sa[k] : 0.f;
    red[1][tid * VEC + k] = active ? sb[k] : 0.f;
  }
  __syncthreads();
  for (int c = tid; c < C; c += 256) {
    const int gg = c / VEC, kk = c % VEC;
    float a = 0.f, b = 0.f;
    for (int q = 0; q < ppb; ++q) {
      a += red[0][(q * G + gg) * VEC + kk];
      b += red[1][(q * G + gg) * VEC + kk];
    }
    part[(int64_t)blockIdx.x * 2 * C + c] = a;
    part[(int64_t)blockIdx.x * 2 * C + C + c] = b;
  }
}

// one block per (channel, {alpha, bias}): sum the per-block partials in a
// fixed order and add into the fp32 gradient
__global__ __launch_bounds__(256) void prelu_finalize_kernel(const float* __restrict__ part, int nblk, int C,
                                                             float* __restrict__ dalpha, float* __restrict__ dbias) {
  const int c = blockIdx.x % C, which = blockIdx.x / C;
  float s = 0.f;
  for (int b = threadIdx.x; b < nblk; b += 256) s += part[(int64_t)b * 2 * C + which * C + c];
  __shared__ float sh[4];
  block_wave_sums(s, sh);
  if (threadIdx.x == 0) {
    float* dst = which ? dbias : dalpha;
    if (dst) dst[c] += (sh[0] + sh[1]) + (sh[2] + sh[3]);
  }
}

}  // namespace

extern "C" int32_t rdn_prelu_bwd_blocks(int32_t dtype, int64_t pixels, int32_t cpad) {
  const int vec = dtype == RDN_BF16 ? 8 : 4;
  const int G = cpad / vec, ppb = 256 / G;
  return grid_for(pixels, ppb * 8, 1024);
}

extern "C" int64_t rdn_prelu_bwd_workspace_size(int32_t dtype, int64_t pixels, int32_t C, int32_t cpad) {
  return (int64_t)rdn_prelu_bwd_blocks(dtype, pixels, cpad) * 2 * C * (int64_t)sizeof(float);
}

extern "C" int rdn_prelu_bwd(int32_t dtype, int64_t pixels, int32_t n, int32_t h, int32_t w, int32_t C, int32_t cpad,
                             const void* dy, int64_t dy_ps, int32_t dy_c0, int64_t dy_pl, const float* dy_nchw, const void* pre,
                             int64_t pre_ps, const float* alpha, void* dyp, float* dalpha, float* dbias, float* ws,
                             void* stream) {
  const int vec = dtype == RDN_BF16 ? 8 : 4;
  if ((!dy && !dy_nchw) || !pre || !alpha || !dyp || !ws) { rdn_set_error("rdn_prelu_bwd: null pointer"); return RDN_E_ARG; }
  if (C <= 0 || cpad < C || cpad % vec || cpad / vec > 256 || pre_ps % vec || pixels != (int64_t)n * h * w) {
    rdn_set_error("rdn_prelu_bwd: bad shape C=%d cpad=%d pre_ps=%lld", C, cpad, (long long)pre_ps);
    return RDN_E_SHAPE;
  }
  const int blocks = rdn_prelu_bwd_blocks(dtype, pixels, cpad);
  RDN_LAUNCH_T(dtype, prelu_bwd_kernel<T><<<blocks, 256, 0, RDN_STREAM>>>(pixels, h, w, C, cpad, (const T*)dy, dy_ps, dy_c0, dy_pl,
                                                                          dy_nchw, (const T*)pre, pre_ps, alpha, (T*)dyp, ws));
  if (dalpha || dbias) prelu_finalize_kernel<<<2 * C, 256, 0, RDN_STREAM>>>(ws, blocks, C, dalpha, dbias);
  return rdn_check_launch("rdn_prelu_bwd");
}
