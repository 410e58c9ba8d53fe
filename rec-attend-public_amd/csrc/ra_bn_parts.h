// What the float4 BatchNorm kernels of ra_bn.hip and ra_bn_wide.hip share: a channel quad's constants and the gradient of one
// pooling window (nnlib.py:111-119,250-253 differentiated).  One copy, so that the two files cannot drift apart in arithmetic.
#pragma once
#include "ra_common.h"

namespace ra {
namespace train {
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct BnConst {
  f32x4 mu, g, be, rstd;
};
__device__ inline BnConst bn_const(const float *mean, const float *var, const float *gamma, const float *beta, float eps,
                                   int c0) {
  BnConst k;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float rstd = var ? rsqrtf(var[c0 + i] + eps) : 1.f;
    k.rstd[i] = rstd;
    k.g[i] = (gamma ? gamma[c0 + i] : 1.f) * rstd;
    k.mu[i] = mean ? mean[c0 + i] : 0.f;
    k.be[i] = beta ? beta[c0 + i] : 0.f;
  }
  return k;
}
// dv of every pixel of the window (dy routed to the FIRST maximum, masked by the ReLU) and xhat
template <int POOL>
__device__ inline void window_grad(const f32x4 (&w)[POOL * POOL], const f32x4 dyv, const BnConst &k, float lo, int relu,
                                   f32x4 (&dv)[POOL * POOL], f32x4 (&xh)[POOL * POOL]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float best = -__builtin_inff();
    int arg = 0;
    float v[POOL * POOL];
#pragma unroll
    for (int q = 0; q < POOL * POOL; ++q) {
      xh[q][i] = (w[q][i] - k.mu[i]) * k.rstd[i];
      v[q] = (w[q][i] - k.mu[i]) * k.g[i] + k.be[i];
      const float a = fmaxf(v[q], lo);
      if (a > best) {
        best = a;
        arg = q;
      }
    }
#pragma unroll
    for (int q = 0; q < POOL * POOL; ++q) dv[q][i] = (q == arg && !(relu && v[q] <= 0.f)) ? dyv[i] : 0.f;
  }
}

}  // namespace train
}  // namespace ra
