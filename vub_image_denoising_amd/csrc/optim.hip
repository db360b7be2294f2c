// The parameter update of the train step (gfx950) over the flat fp32 buffers: gradient
// norm and clip (device-side coefficient), Adam / AdamW and Adadelta with and without the
// weight EMA in the same launch, and the stand-alone EMA update.  Single passes over HBM.
#include "rdn_pointwise.h"

namespace {

__global__ __launch_bounds__(256) void sq_partial_kernel(const float* __restrict__ g, int64_t n, float* __restrict__ part) {
  float s = 0.f;
  vec4_loop(n, n / 4, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x, [&](int64_t i) {
    const f32x4 v = ((const f32x4*)g)[i];
    s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
  }, [&](int64_t i) { s += g[i] * g[i]; });
  __shared__ float sh[4];
  block_wave_sums(s, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

// pre: a scale the caller has not applied to g yet (the data-parallel 1/world average,
// ddp.GradSync.defer_average): the norm is that of pre*g and out[1] carries pre; for a
// power-of-two pre both are exactly what scaling g first would give
__global__ __launch_bounds__(256) void sq_final_kernel(const float* __restrict__ part, int nb, float max_norm,
                                                       float pre, float* __restrict__ out) {
  double sq[1];
  if (final_sums(part, nb, sq)) {
    const float tot = (float)(sqrt(sq[0]) * (double)pre);
    out[0] = tot;
    const float coef = max_norm / (tot + 1e-6f);
    out[1] = pre * (coef < 1.f ? coef : 1.f);
  }
}

__global__ void scale_kernel(float* __restrict__ g, int64_t n, const float* __restrict__ coef) {
  const float c = coef[0];
  vec4_loop(n, n / 4, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x,
            [&](int64_t i) { ((f32x4*)g)[i] *= c; }, [&](int64_t i) { g[i] *= c; });
}

// torch.optim.Adam/AdamW single-tensor math (torch/optim/adam.py, _single_tensor_adam),
// with every scalar rounded to fp32 from the same double torch computes it in:
//   AdamW: p *= (1 - lr*wd) ; Adam: g += wd*p
//   m = lerp(m, g, 1-b1) ; v = v*b2 + (1-b2)*g*g
//   p += -(lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps),  bc_i = 1 - b_i^step
struct AdamScalars {
  float decay, wd, omb1, b2, omb2, step_size, bc2s, eps;
};
__host__ __device__ inline AdamScalars adam_scalars(double lr, double b1, double b2, double eps, double wd,
                                                    int decoupled, double step) {
  AdamScalars a;
  const double bc1 = 1.0 - pow(b1, step), bc2 = 1.0 - pow(b2, step);
  a.decay = decoupled ? (float)(1.0 - lr * wd) : 1.f;
  a.wd = decoupled ? 0.f : (float)wd;
  a.omb1 = (float)(1.0 - b1);
  a.b2 = (float)b2;
  a.omb2 = (float)(1.0 - b2);
  a.step_size = (float)(lr / bc1);
  a.bc2s = (float)sqrt(bc2);
  a.eps = (float)eps;
  return a;
}

// Exponential moving average of the weights (no reference counterpart): one element is
//   e = fmaf(w, p - e, e),  w = (float)(1 - d)
// with d = decay, or with warm-up d = min(decay, (1 + n) / (10 + n)) for the update after
// n earlier ones.  w is rounded once from double, on the host for a host-known n and on
// the device, from the same double expression, when n is read from device memory (a
// replayed graph).  In the flat layout's padding gaps p = e = 0, so e stays 0.
__host__ __device__ inline float ema_weight(double decay, int warmup, int64_t n) {
  double d = decay;
  if (warmup) {
    const double r = (1.0 + (double)n) / (10.0 + (double)n);
    d = r < d ? r : d;
  }
  return (float)(1.0 - d);
}

__device__ __forceinline__ void ema_elem(float& e, float p, float w) {
#pragma clang fp contract(off)
  e = fmaf(w, p - e, e);
}

// what an update kernel needs to keep the average: host_w is the weight of a host-known
// count; with n_dev != nullptr (warm-up in a replayable step) the count is read from
// device memory by thread 0 of every block -- nothing in the launch writes it (the
// counter is advanced by rdn_counter_inc behind the launch, stream-ordered)
struct EmaArgs {
  float* e;
  float host_w;
  double decay;
  const int64_t* n_dev;
};

__device__ __forceinline__ float ema_block_weight(const EmaArgs& a) {
  __shared__ float w_s;
  if (!a.n_dev) return a.host_w;
  if (threadIdx.x == 0) w_s = ema_weight(a.decay, 1, *a.n_dev);
  __syncthreads();
  return w_s;
}

// host_sc: the scalars of a host-known step; with step_dev != nullptr the step count
// is read from device memory (graph-replayable optimizer step) and the scalars are
// derived on the device in double, exactly as on the host
__device__ __forceinline__ AdamScalars adam_block_scalars(const AdamScalars& host_sc,
                                                          const int64_t* __restrict__ step_dev, double lr, double b1,
                                                          double b2, double eps, double wd, int decoupled) {
  __shared__ AdamScalars sc_s;
  AdamScalars sc = host_sc;
  if (step_dev) {
    if (threadIdx.x == 0) sc_s = adam_scalars(lr, b1, b2, eps, wd, decoupled, (double)*step_dev);
    __syncthreads();
    sc = sc_s;
  }
  return sc;
}

// EMA: the average of the just-computed p is updated in the same pass (e in the layout of
// p, weight ew).  tid / stride: the grid-stride geometry, read in the __global__ functions
// themselves (read in an inlined body, blockDim compiles to the slower generic load).
template <bool EMA>
__device__ __forceinline__ void adam_loop(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                          float* __restrict__ v, int64_t n, const AdamScalars& sc, float gs,
                                          float* __restrict__ e, float ew, int64_t tid, int64_t stride) {
  for (int64_t i = tid; i < n; i += stride) {
    float pi = p[i], gi = g[i] * gs;
    pi *= sc.decay;
    gi += sc.wd * pi;
    const float mi = m[i] + (gi - m[i]) * sc.omb1;   // lerp form used by torch
    const float vi = v[i] * sc.b2 + sc.omb2 * gi * gi;
    m[i] = mi;
    v[i] = vi;
    pi += -sc.step_size * (mi / (sqrtf(vi) / sc.bc2s + sc.eps));
    p[i] = pi;
    if constexpr (EMA) {
      float ei = e[i];
      ema_elem(ei, pi, ew);
      e[i] = ei;
    }
  }
}

__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                            float* __restrict__ v, int64_t n, AdamScalars host_sc, const int64_t* __restrict__ step_dev,
                            double lr, double b1, double b2, double eps, double wd, int decoupled, float gs) {
  const AdamScalars sc = adam_block_scalars(host_sc, step_dev, lr, b1, b2, eps, wd, decoupled);
  adam_loop<false>(p, g, m, v, n, sc, gs, nullptr, 0.f, (int64_t)blockIdx.x * blockDim.x + threadIdx.x,
                   (int64_t)gridDim.x * blockDim.x);
}

__global__ void adam_ema_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                float* __restrict__ v, int64_t n, AdamScalars host_sc,
                                const int64_t* __restrict__ step_dev, double lr, double b1, double b2, double eps,
                                double wd, int decoupled, float gs, EmaArgs ema) {
  const AdamScalars sc = adam_block_scalars(host_sc, step_dev, lr, b1, b2, eps, wd, decoupled);
  const float ew = ema_block_weight(ema);
  adam_loop<true>(p, g, m, v, n, sc, gs, ema.e, ew, (int64_t)blockIdx.x * blockDim.x + threadIdx.x,
                  (int64_t)gridDim.x * blockDim.x);
}

// torch.optim.Adadelta single-tensor math (torch/optim/adadelta.py, _single_tensor_adadelta),
// one rounding per torch op (its `self + alpha*x` kernels contract to one fma; nothing else
// is contracted), every scalar rounded to fp32 from double:
//   g = g*gs (+ wd*p) ; sq = sq*rho + (1-rho)*g*g
//   delta = sqrt(acc + eps) / sqrt(sq + eps) * g ; acc = acc*rho + (1-rho)*delta*delta
//   p += -lr * delta
// Nothing depends on the step count: the launch is graph-replayable as it is.  In the
// flat layout's padding gaps p = g = 0, so delta = 0 and p stays 0.
struct AdadeltaScalars {
  float rho, omr, eps, neg_lr, wd;
};

__device__ __forceinline__ void adadelta_elem(float& p, float g, float& sq, float& acc, const AdadeltaScalars& sc,
                                              float gs) {
#pragma clang fp contract(off)
  g = g * gs;
  if (sc.wd != 0.f) g = fmaf(sc.wd, p, g);        // grad.add(param, alpha=wd)
  sq = sq * sc.rho;                               // mul_(rho)
  sq = fmaf(sc.omr, g * g, sq);                   // addcmul_(g, g, value=1-rho): self + value*(t1*t2)
  const float std_ = sqrtf(sq + sc.eps);
  float d = sqrtf(acc + sc.eps);
  d = d / std_;
  d = d * g;
  acc = acc * sc.rho;
  acc = fmaf(sc.omr, d * d, acc);
  p = fmaf(sc.neg_lr, d, p);                      // add_(delta, alpha=-lr)
}
template <bool EMA>
__device__ __forceinline__ void adadelta_body(float* __restrict__ p, const float* __restrict__ g,
                                              float* __restrict__ sq, float* __restrict__ acc, int64_t n, int64_t n4,
                                              const AdadeltaScalars& sc, float gs, float* __restrict__ e, float ew,
                                              int64_t tid, int64_t stride) {
  vec4_loop(n, n4, tid, stride, [&](int64_t i) {
    f32x4 pv = ((f32x4*)p)[i], sv = ((f32x4*)sq)[i], av = ((f32x4*)acc)[i];
    const f32x4 gv = ((const f32x4*)g)[i];
    f32x4 ev;
    if constexpr (EMA) ev = ((f32x4*)e)[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float pk = pv[k], sk = sv[k], ak = av[k];
      adadelta_elem(pk, gv[k], sk, ak, sc, gs);
      pv[k] = pk; sv[k] = sk; av[k] = ak;
      if constexpr (EMA) {
        float ek = ev[k];
        ema_elem(ek, pk, ew);
        ev[k] = ek;
      }
    }
    ((f32x4*)p)[i] = pv;
    ((f32x4*)sq)[i] = sv;
    ((f32x4*)acc)[i] = av;
    if constexpr (EMA) ((f32x4*)e)[i] = ev;
  }, [&](int64_t i) {
    adadelta_elem(p[i], g[i], sq[i], acc[i], sc, gs);
    if constexpr (EMA) ema_elem(e[i], p[i], ew);
  });
}

__global__ __launch_bounds__(256) void adadelta_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                       float* __restrict__ sq, float* __restrict__ acc, int64_t n,
                                                       int64_t n4, AdadeltaScalars sc, float gs) {
  adadelta_body<false>(p, g, sq, acc, n, n4, sc, gs, nullptr, 0.f, (int64_t)blockIdx.x * blockDim.x + threadIdx.x,
                       (int64_t)gridDim.x * blockDim.x);
}

__global__ __launch_bounds__(256) void adadelta_ema_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                           float* __restrict__ sq, float* __restrict__ acc, int64_t n,
                                                           int64_t n4, AdadeltaScalars sc, float gs, EmaArgs ema) {
  const float ew = ema_block_weight(ema);
  adadelta_body<true>(p, g, sq, acc, n, n4, sc, gs, ema.e, ew, (int64_t)blockIdx.x * blockDim.x + threadIdx.x,
                      (int64_t)gridDim.x * blockDim.x);
}

// the stand-alone average update (optimizers that are not fused)
__global__ __launch_bounds__(256) void ema_kernel(const float* __restrict__ p, int64_t n, int64_t n4, EmaArgs ema) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const float ew = ema_block_weight(ema);
  float* __restrict__ e = ema.e;
  vec4_loop(n, n4, tid, stride, [&](int64_t i) {
    const f32x4 pv = ((const f32x4*)p)[i];
    f32x4 ev = ((f32x4*)e)[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float ek = ev[k];
      ema_elem(ek, pv[k], ew);
      ev[k] = ek;
    }
    ((f32x4*)e)[i] = ev;
  }, [&](int64_t i) { ema_elem(e[i], p[i], ew); });
}

// the average's arguments as an entry point receives them
struct EmaSpec {
  float* ema;
  double decay;
  int32_t warmup;
  int64_t n;
  const int64_t* n_dev;
};

// validates them and fills the kernel's EmaArgs (false: the error is set)
bool ema_args(const char* who, const EmaSpec& s, EmaArgs* out) {
  if (!s.ema) { rdn_set_error("%s: null ema buffer", who); return false; }
  if (!(s.decay >= 0.0 && s.decay <= 1.0)) { rdn_set_error("%s: decay %g outside [0, 1]", who, s.decay); return false; }
  if (s.n < 0 && !(s.warmup && s.n_dev)) { rdn_set_error("%s: update count %lld < 0", who, (long long)s.n); return false; }
  out->e = s.ema;
  out->host_w = ema_weight(s.decay, s.warmup != 0, s.n < 0 ? 0 : s.n);
  out->decay = s.decay;
  out->n_dev = s.warmup ? s.n_dev : nullptr;
  return true;
}

// rdn_adam_step (ema == nullptr) and rdn_adam_step_ema; who: the entry point called
int adam_launch(const char* who, float* p, const float* g, float* m, float* v, int64_t count, double lr, double beta1,
                double beta2, double eps, double wd, int32_t decoupled, int64_t step, const int64_t* step_dev,
                float grad_scale, const EmaSpec* ema, void* stream) {
  if (!(p && g && m && v && count > 0 && (step_dev || step >= 1) && beta1 >= 0 && beta1 < 1 && beta2 >= 0 && beta2 < 1)) {
    rdn_set_error("%s: bad arguments", who);
    return RDN_E_ARG;
  }
  EmaArgs ea;
  if (ema && !ema_args(who, *ema, &ea)) return RDN_E_ARG;
  const AdamScalars sc = adam_scalars(lr, beta1, beta2, eps, wd, decoupled, (double)(step < 1 ? 1 : step));
  const int blocks = grid_for(count, 256 * 4);
  if (ema)
    adam_ema_kernel<<<blocks, 256, 0, RDN_STREAM>>>(p, g, m, v, count, sc, step_dev, lr, beta1, beta2, eps, wd, decoupled,
                                                    grad_scale, ea);
  else
    adam_kernel<<<blocks, 256, 0, RDN_STREAM>>>(p, g, m, v, count, sc, step_dev, lr, beta1, beta2, eps, wd, decoupled,
                                                grad_scale);
  return rdn_check_launch(who);
}

// rdn_adadelta_step (ema == nullptr) and rdn_adadelta_step_ema
int adadelta_launch(const char* who, float* p, const float* g, float* square_avg, float* acc_delta, int64_t count,
                    double lr, double rho, double eps, double weight_decay, float grad_scale, const EmaSpec* ema,
                    void* stream) {
  if (!p || !g || !square_avg || !acc_delta) { rdn_set_error("%s: null pointer", who); return RDN_E_ARG; }
  if (count < 0) { rdn_set_error("%s: count %lld < 0", who, (long long)count); return RDN_E_ARG; }
  EmaArgs ea;
  if (ema && !ema_args(who, *ema, &ea)) return RDN_E_ARG;
  if (count == 0) return RDN_OK;
  const AdadeltaScalars sc = {(float)rho, (float)(1.0 - rho), (float)eps, (float)(-lr), (float)weight_decay};
  const Vec4Plan v4 = vec4_plan(count, p, g, square_avg, acc_delta, ema ? ema->ema : nullptr);
  const int blocks = grid_for(v4.items, 256 * 4);
  if (ema)
    adadelta_ema_kernel<<<blocks, 256, 0, RDN_STREAM>>>(p, g, square_avg, acc_delta, count, v4.n4, sc, grad_scale, ea);
  else
    adadelta_kernel<<<blocks, 256, 0, RDN_STREAM>>>(p, g, square_avg, acc_delta, count, v4.n4, sc, grad_scale);
  return rdn_check_launch(who);
}

}  // namespace

extern "C" int rdn_sqnorm_scaled(const float* g, int64_t count, float max_norm, float pre_scale, float* ws, float* out,
                                 void* stream) {
  if (!g || !ws || !out || count <= 0 || ((uintptr_t)g & 15) || !(pre_scale > 0.f)) {
    rdn_set_error("rdn_sqnorm: bad arguments");
    return RDN_E_ARG;
  }
  const int nb = grid_for(count, 256 * 16, kRedBlocks);
  sq_partial_kernel<<<nb, 256, 0, RDN_STREAM>>>(g, count, ws);
  sq_final_kernel<<<1, 256, 0, RDN_STREAM>>>(ws, nb, max_norm, pre_scale, out);
  return rdn_check_launch("rdn_sqnorm");
}

extern "C" int rdn_sqnorm(const float* g, int64_t count, float max_norm, float* ws, float* out, void* stream) {
  return rdn_sqnorm_scaled(g, count, max_norm, 1.f, ws, out, stream);
}

extern "C" int rdn_clip_scale(float* g, int64_t count, const float* coef, void* stream) {
  if (!g || !coef || count <= 0 || ((uintptr_t)g & 15)) { rdn_set_error("rdn_clip_scale: bad arguments"); return RDN_E_ARG; }
  scale_kernel<<<grid_for(count / 4 + 1, 256 * 4), 256, 0, RDN_STREAM>>>(g, count, coef);
  return rdn_check_launch("rdn_clip_scale");
}

extern "C" int rdn_adam_step(float* p, const float* g, float* m, float* v, int64_t count, double lr, double beta1,
                             double beta2, double eps, double wd, int32_t decoupled, int64_t step,
                             const int64_t* step_dev, float grad_scale, void* stream) {
  return adam_launch("rdn_adam_step", p, g, m, v, count, lr, beta1, beta2, eps, wd, decoupled, step, step_dev, grad_scale,
                     nullptr, stream);
}

extern "C" int rdn_adam_step_ema(float* p, const float* g, float* m, float* v, int64_t count, double lr, double beta1,
                                 double beta2, double eps, double wd, int32_t decoupled, int64_t step,
                                 const int64_t* step_dev, float grad_scale, float* ema, double decay, int32_t warmup,
                                 int64_t n, const int64_t* n_dev, void* stream) {
  const EmaSpec es = {ema, decay, warmup, n, n_dev};
  return adam_launch("rdn_adam_step_ema", p, g, m, v, count, lr, beta1, beta2, eps, wd, decoupled, step, step_dev,
                     grad_scale, &es, stream);
}

extern "C" int rdn_adadelta_step(float* p, const float* g, float* square_avg, float* acc_delta, int64_t count,
                                 double lr, double rho, double eps, double weight_decay, float grad_scale,
                                 void* stream) {
  return adadelta_launch("rdn_adadelta_step", p, g, square_avg, acc_delta, count, lr, rho, eps, weight_decay, grad_scale,
                         nullptr, stream);
}

extern "C" int rdn_adadelta_step_ema(float* p, const float* g, float* square_avg, float* acc_delta, int64_t count,
                                     double lr, double rho, double eps, double weight_decay, float grad_scale,
                                     float* ema, double decay, int32_t warmup, int64_t n, const int64_t* n_dev,
                                     void* stream) {
  const EmaSpec es = {ema, decay, warmup, n, n_dev};
  return adadelta_launch("rdn_adadelta_step_ema", p, g, square_avg, acc_delta, count, lr, rho, eps, weight_decay,
                         grad_scale, &es, stream);
}

extern "C" int rdn_ema_update(float* ema, const float* p, int64_t count, double decay, int32_t warmup, int64_t n,
                              const int64_t* n_dev, void* stream) {
  if (!p) { rdn_set_error("rdn_ema_update: null parameter buffer"); return RDN_E_ARG; }
  if (count < 0) { rdn_set_error("rdn_ema_update: count %lld < 0", (long long)count); return RDN_E_ARG; }
  EmaArgs ea;
  if (!ema_args("rdn_ema_update", {ema, decay, warmup, n, n_dev}, &ea)) return RDN_E_ARG;
  if (count == 0) return RDN_OK;
  const Vec4Plan v4 = vec4_plan(count, ema, p);
  ema_kernel<<<grid_for(v4.items, 256 * 4), 256, 0, RDN_STREAM>>>(p, count, v4.n4, ea);
  return rdn_check_launch("rdn_ema_update");
}
