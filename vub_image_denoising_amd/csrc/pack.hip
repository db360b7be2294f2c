// Data movement of the train / sample step (gfx950): the diffusion input (interpolation,
// NCHW fp32 -> padded NHWC), weight packing (single and batched), the NCHW <-> NHWC copies,
// slice zeroing and the sampler's combine.  Single passes over HBM.
#include "rdn_pointwise.h"

namespace {

// ------------------------------------------------------------------ interp / pack input
__global__ void interp_kernel(const float* __restrict__ clean, const float* __restrict__ noisy,
                              const float* __restrict__ tn, int batch, int64_t per, float* __restrict__ x) {
  const int64_t n4 = per / 4;
  const int64_t total = (int64_t)batch * n4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int b = (int)(i / n4);
    const float a = tn[b];
    const f32x4 c = ((const f32x4*)clean)[i], n = ((const f32x4*)noisy)[i];
    ((f32x4*)x)[i] = a * n + (1.f - a) * c;
  }
}

template <typename T>
__global__ void pack_input_kernel(const float* __restrict__ x, int N, int C, int H, int W, const float* __restrict__ t,
                                  int64_t t_sb, int64_t t_sh, int64_t t_sw, int has_t, T* __restrict__ out, int cpad) {
  const int64_t HW = (int64_t)H * W, P = (int64_t)N * HW;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < P; p += (int64_t)gridDim.x * blockDim.x) {
    const int64_t n = p / HW, r = p - n * HW;
    const int y = (int)(r / W), xx = (int)(r - (int64_t)y * W);
    T* o = out + p * cpad;
    for (int c = 0; c < cpad; ++c) {
      float v = 0.f;
      if (c < C) v = x[(n * C + c) * HW + r];
      else if (c == C && has_t) v = t[n * t_sb + y * t_sh + xx * t_sw];
      o[c] = from_f32<T>(v);
    }
  }
}

// ------------------------------------------------------------------ weight packing
__device__ __forceinline__ float pack_value(int mode, const float* __restrict__ w, int d0, int d1, int kh, int kw,
                                            int pad0, int pad1, int kc, int ck, int r, int k) {
  const int taps = kh * kw;
  if (mode == RDN_PACK_CONV_FWD) {  // P[a][tap*pad1 + b] = W[a][b][tap]  (chunked when ck > 0)
    int tap, b;
    if (ck > 0) { const int ch = k / kc, rem = k - ch * kc; tap = rem / ck; b = ch * ck + (rem - tap * ck); }
    else { tap = k / pad1; b = k - tap * pad1; }
    const int a = r;
    if (a < d0 && b < d1 && tap < taps) return w[((int64_t)a * d1 + b) * taps + tap];
  } else if (mode == RDN_PACK_CONV_DGRAD) {  // P[b][tap'*pad0 + a] = W[a][b][flip(tap')]
    int tp, a;
    if (ck > 0) { const int ch = k / kc, rem = k - ch * kc; tp = rem / ck; a = ch * ck + (rem - tp * ck); }
    else { tp = k / pad0; a = k - tp * pad0; }
    const int b = r;
    if (a < d0 && b < d1 && tp < taps) {
      const int ky = kh - 1 - tp / kw, kx = kw - 1 - tp % kw;
      return w[((int64_t)a * d1 + b) * taps + ky * kw + kx];
    }
  } else {  // GEMM_T: P[tap*d1 + b][a] = W[a][b][tap], K = pad0 >= d0
    const int tap = r / d1, b = r - tap * d1, a = k;
    if (tap < taps && a < d0) return w[((int64_t)a * d1 + b) * taps + tap];
  }
  return 0.f;
}

static inline int chunk_sk(int dtype) { return dtype == RDN_BF16 ? 64 : 32; }
static inline int chunk_kc(int ck, int dtype) {
  const int sk = chunk_sk(dtype);
  return ck > 0 ? (9 * ck + sk - 1) / sk * sk : 0;
}

template <typename T>
__global__ void pack_weights_kernel(int mode, const float* __restrict__ w, int d0, int d1, int kh, int kw, int pad0,
                                    int pad1, T* __restrict__ out, int rows_pad, int kp, int ck, int kc) {
  const int64_t total = (int64_t)rows_pad * kp;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(i / kp), k = (int)(i - (int64_t)r * kp);
    out[i] = from_f32<T>(pack_value(mode, w, d0, d1, kh, kw, pad0, pad1, kc, ck, r, k));
  }
}

// one thread = one 16-byte unit of packed output (kp is a multiple of 64, so a unit
// never straddles two rows); 32-bit index math (rows_pad * kp < 2^31 per pack).
// Measured per train step (r02): one element per thread with 64-bit divisions
// 133 us -> 72 us.  What remains is the gather: consecutive k of a packed row read
// weights 9 floats apart (OIHW -> [co][tap][ci]); a flattened index space over all
// packs (per-pack prefix in LDS) was slower (85 us).
template <typename T>
__global__ __launch_bounds__(256) void pack_weights_batched_kernel(const rdn_pack_item* __restrict__ items, int sk) {
  constexpr int VEC = TypeInfo<T>::VEC;
  const rdn_pack_item it = items[blockIdx.y];
  const int kc = it.ck > 0 ? (9 * it.ck + sk - 1) / sk * sk : 0;
  const int units = it.rows_pad * (it.kp / VEC);
  T* __restrict__ out = (T*)it.out;
  for (int u = blockIdx.x * 256 + threadIdx.x; u < units; u += gridDim.x * 256) {
    const int e = u * VEC, r = e / it.kp, k0 = e - r * it.kp;
    float v[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q)
      v[q] = pack_value(it.mode, it.w, it.d0, it.d1, it.kh, it.kw, it.pad0, it.pad1, kc, it.ck, r, k0 + q);
    *(u32x4*)(out + e) = Unit16<T>::pack(v);
  }
}

// x_tilde = (1-a)*f1 + a*y; x_tilde_prev = (1-ap)*f2 + ap*y; x = x - x_tilde + x_tilde_prev
// (diffusion_RDUnet.py:45-49), each product rounded separately as torch does.
__global__ void sampling_combine_kernel(float* __restrict__ x, const float* __restrict__ f1, const float* __restrict__ f2,
                                        const float* __restrict__ y, int64_t n, float c1, float a, float c2, float ap) {
#pragma clang fp contract(off)
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float xt = c1 * f1[i] + a * y[i];
    const float xp = c2 * f2[i] + ap * y[i];
    x[i] = (x[i] - xt) + xp;
  }
}

template <typename T>
__global__ void nchw_to_nhwc_kernel(const float* __restrict__ s, int N, int C, int H, int W, T* __restrict__ d,
                                    int64_t ps, int c0, int64_t pl, int acc) {
  const int64_t HW = (int64_t)H * W, total = (int64_t)N * C * HW;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = i / C;
    const int c = (int)(i - p * C);
    const int64_t n = p / HW, r = p - n * HW;
    T* const o = d + p * ps + rdn_coff(c0 + c, ps, pl);
    const float v = s[(n * C + c) * HW + r];
    *o = from_f32<T>(acc ? to_f32(*o) + v : v);
  }
}

template <typename T>
__global__ void nhwc_to_nchw_kernel(const T* __restrict__ s, int64_t ps, int c0, int64_t pl, int N, int C, int H, int W,
                                    float* __restrict__ d, int acc) {
  const int64_t HW = (int64_t)H * W, total = (int64_t)N * C * HW;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i % HW, nc = i / HW;
    const int c = (int)(nc % C);
    const int64_t n = nc / C;
    const float v = to_f32(s[(n * HW + r) * ps + rdn_coff(c0 + c, ps, pl)]);
    d[i] = acc ? d[i] + v : v;
  }
}

template <typename T>
__global__ void zero_slice_kernel(T* __restrict__ d, int64_t pixels, int64_t ps, int c0, int cols) {
  const int64_t total = pixels * cols;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = i / cols;
    const int c = (int)(i - p * cols);
    d[p * ps + c0 + c] = from_f32<T>(0.f);
  }
}

}  // namespace

extern "C" int rdn_interp(const float* clean, const float* noisy, const float* tnorm, int32_t batch, int64_t per,
                          float* x, void* stream) {
  if (!clean || !noisy || !tnorm || !x || per % 4 || ((uintptr_t)clean | (uintptr_t)noisy | (uintptr_t)x) & 15) {
    rdn_set_error("rdn_interp: bad arguments"); return RDN_E_ARG;
  }
  interp_kernel<<<grid_for(batch * per / 4, 256), 256, 0, RDN_STREAM>>>(clean, noisy, tnorm, batch, per, x);
  return rdn_check_launch("rdn_interp");
}

extern "C" int rdn_pack_input(int32_t dtype, const float* x, int32_t n, int32_t c, int32_t h, int32_t w, const float* t,
                              int64_t t_sb, int64_t t_sh, int64_t t_sw, int32_t has_t, void* out, int32_t cpad,
                              void* stream) {
  if (!x || !out || (has_t && !t) || cpad < c + (has_t ? 1 : 0)) { rdn_set_error("rdn_pack_input: bad arguments"); return RDN_E_ARG; }
  const int64_t P = (int64_t)n * h * w;
  RDN_LAUNCH_T(dtype, pack_input_kernel<T><<<grid_for(P, 256), 256, 0, RDN_STREAM>>>(x, n, c, h, w, t, t_sb, t_sh, t_sw, has_t,
                                                                                   (T*)out, cpad));
  return rdn_check_launch("rdn_pack_input");
}

extern "C" int rdn_pack_weights_batched(const rdn_pack_item* items, int32_t n, int32_t dtype, void* stream) {
  if (!items || n <= 0 || n > 65535) { rdn_set_error("rdn_pack_weights_batched: bad arguments"); return RDN_E_ARG; }
  dim3 grid(96, n);   // 96 x 256 units per pass: the largest pack (level-3 conv_3) in ~8 passes
  RDN_LAUNCH_T(dtype, pack_weights_batched_kernel<T><<<grid, 256, 0, RDN_STREAM>>>(items, chunk_sk(dtype)));
  return rdn_check_launch("rdn_pack_weights_batched");
}

extern "C" int rdn_pack_weights(int32_t mode, int32_t dtype, const float* w, int32_t d0, int32_t d1, int32_t kh,
                                int32_t kw, int32_t pad0, int32_t pad1, void* out, int32_t rows_pad, int32_t kp,
                                int32_t ck, void* stream) {
  if (!w || !out || mode < 0 || mode > 2 || kp % 64 || rows_pad % 128) { rdn_set_error("rdn_pack_weights: bad arguments"); return RDN_E_ARG; }
  const int taps = kh * kw;
  const int kc = chunk_kc(ck, dtype);
  if (ck > 0) {
    const int kside = mode == RDN_PACK_CONV_FWD ? pad1 : pad0;
    if (taps != 9 || mode == RDN_PACK_GEMM_T || kside % ck || (kside / ck) * kc > kp) {
      rdn_set_error("rdn_pack_weights: chunked pack needs a 3x3 conv mode and kp >= %d", (kside / ck) * kc);
      return RDN_E_SHAPE;
    }
  } else if ((mode == RDN_PACK_CONV_FWD && (pad1 < d1 || rows_pad < d0 || taps * pad1 > kp)) ||
      (mode == RDN_PACK_CONV_DGRAD && (pad0 < d0 || rows_pad < d1 || taps * pad0 > kp)) ||
      (mode == RDN_PACK_GEMM_T && (pad0 < d0 || pad0 > kp || rows_pad < taps * d1))) {
    rdn_set_error("rdn_pack_weights: shape (mode=%d d0=%d d1=%d pad0=%d pad1=%d rows=%d kp=%d)", mode, d0, d1, pad0, pad1,
                  rows_pad, kp);
    return RDN_E_SHAPE;
  }
  const int64_t total = (int64_t)rows_pad * kp;
  RDN_LAUNCH_T(dtype, pack_weights_kernel<T><<<grid_for(total, 256), 256, 0, RDN_STREAM>>>(mode, w, d0, d1, kh, kw, pad0, pad1,
                                                                                         (T*)out, rows_pad, kp, ck, kc));
  return rdn_check_launch("rdn_pack_weights");
}

extern "C" int rdn_sampling_combine(float* x, const float* f1, const float* f2, const float* y, int64_t count, float c1,
                                    float a, float c2, float ap, void* stream) {
  if (!x || !f1 || !f2 || !y || count <= 0) { rdn_set_error("rdn_sampling_combine: bad arguments"); return RDN_E_ARG; }
  sampling_combine_kernel<<<grid_for(count, 256 * 4), 256, 0, RDN_STREAM>>>(x, f1, f2, y, count, c1, a, c2, ap);
  return rdn_check_launch("rdn_sampling_combine");
}

extern "C" int rdn_nchw_to_nhwc(int32_t dtype, const float* src, int32_t n, int32_t c, int32_t h, int32_t w, void* dst,
                                int64_t dst_ps, int32_t dst_c0, int64_t dst_pl, int32_t accumulate, void* stream) {
  if (!src || !dst || dst_ps <= 0) { rdn_set_error("rdn_nchw_to_nhwc: null / bad stride"); return RDN_E_ARG; }
  const int64_t total = (int64_t)n * c * h * w;
  RDN_LAUNCH_T(dtype, nchw_to_nhwc_kernel<T><<<grid_for(total, 256 * 4), 256, 0, RDN_STREAM>>>(src, n, c, h, w, (T*)dst, dst_ps,
                                                                                             dst_c0, dst_pl, accumulate));
  return rdn_check_launch("rdn_nchw_to_nhwc");
}

extern "C" int rdn_nhwc_to_nchw(int32_t dtype, const void* src, int64_t src_ps, int32_t src_c0, int64_t src_pl, int32_t n,
                                int32_t c, int32_t h, int32_t w, float* dst, int32_t accumulate, void* stream) {
  if (!src || !dst || src_ps <= 0) { rdn_set_error("rdn_nhwc_to_nchw: null / bad stride"); return RDN_E_ARG; }
  const int64_t total = (int64_t)n * c * h * w;
  RDN_LAUNCH_T(dtype, nhwc_to_nchw_kernel<T><<<grid_for(total, 256 * 4), 256, 0, RDN_STREAM>>>((const T*)src, src_ps, src_c0, src_pl,
                                                                                             n, c, h, w, dst, accumulate));
  return rdn_check_launch("rdn_nhwc_to_nchw");
}

extern "C" int rdn_zero_slice(int32_t dtype, void* dst, int64_t pixels, int64_t ps, int32_t c0, int32_t cols, void* stream) {
  if (!dst || pixels < 0 || cols < 0) { rdn_set_error("rdn_zero_slice: bad arguments"); return RDN_E_ARG; }
  if (pixels == 0 || cols == 0) return RDN_OK;
  RDN_LAUNCH_T(dtype, zero_slice_kernel<T><<<grid_for(pixels * cols, 256 * 4), 256, 0, RDN_STREAM>>>((T*)dst, pixels, ps, c0, cols));
  return rdn_check_launch("rdn_zero_slice");
}
