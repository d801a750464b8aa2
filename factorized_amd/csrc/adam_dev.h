// The Adam update of the library, written once: every kernel that applies it (adam_kernel, adam_dev_kernel, adam_ext_spans_kernel,
// the fused all-reduce of p2p.hip) calls adam_update / adam_update4, every launcher forms its coefficients with adam_coef.  The
// entry points promise each other's results (include/mfm_hip.h) and data-parallel replicas must compute the same bits, so the
// roundings are fixed here and not left to each caller's floating-point contraction.
#pragma once
#include <math.h>
#include "common.h"

namespace mfm {

struct AdamCoef {
  float beta1, beta2, eps;
  float step_size;     // lr / (1 - beta1^step)
  float bc2_sqrt;      // sqrt(1 - beta2^step)
};

// The bias corrections of the 1-based step count `step`, in double precision (host launchers; thread 0 of adam_dev_kernel).
__host__ __device__ inline AdamCoef adam_coef(float lr, float beta1, float beta2, float eps, int step) {
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  return AdamCoef{beta1, beta2, eps, (float)((double)lr / bc1), (float)sqrt(bc2)};
}

// One element.  `g` is the raw gradient, `grad_scale` its scale (negative: maximize).  A decoupled weight decay is applied to p
// by the caller beforehand.  Uniform options of adam_ext.hip: `l2` adds l2_decay * p to the scaled gradient (torch:
// grad.add(param, alpha=weight_decay)), `amsgrad` keeps the running maximum of v in *vmax and divides by it.  With neither, the
// operations are those of the plain update -- three fused, as written; nothing else may fuse.
__device__ __forceinline__ void adam_update(float& p, float& m, float& v, float g, const AdamCoef& c, float grad_scale,
                                            bool l2 = false, float l2_decay = 0.0f, bool amsgrad = false, float* vmax = nullptr) {
#pragma clang fp contract(off)
  float gg = g * grad_scale;
  float d;
  if (l2) {
    gg = fmaf(l2_decay, p, gg);
    d = gg - m;
  } else {
    d = fmaf(grad_scale, g, -m);
  }
  m = fmaf(1.0f - c.beta1, d, m);
  v = fmaf(c.beta2, v, gg * ((1.0f - c.beta2) * gg));
  float s = v;
  if (amsgrad) {
    // torch.maximum: a NaN on either side stays a NaN
    *vmax = (v > *vmax || v != v) ? v : *vmax;
    s = *vmax;
  }
  const float denom = sqrtf(s) / c.bc2_sqrt + c.eps;
  p = p - c.step_size * m / denom;
}

// Four elements (vector elements do not bind to references: hence the copies).  *vmax is touched only with `amsgrad`.
__device__ __forceinline__ void adam_update4(f32x4& p, f32x4& m, f32x4& v, const f32x4 g, const AdamCoef& c, float grad_scale,
                                             bool l2 = false, float l2_decay = 0.0f, bool amsgrad = false, f32x4* vmax = nullptr) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float pj = p[j], mj = m[j], vj = v[j], xj = amsgrad ? (*vmax)[j] : 0.0f;
    adam_update(pj, mj, vj, g[j], c, grad_scale, l2, l2_decay, amsgrad, &xj);
    p[j] = pj; m[j] = mj; v[j] = vj;
    if (amsgrad) (*vmax)[j] = xj;
  }
}

}  // namespace mfm
