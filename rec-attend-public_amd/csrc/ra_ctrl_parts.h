// What the controller kernels share (ra_ctrl.hip, ra_ctrl_split.hip, ra_ctrl_train.hip): device code only.
// The GEMV routines of the two one-workgroup kernels (ctrl::gemv, ctrlt::gemv_cols) are NOT here: their part caps and
// bias order differ, and merging them would change bits.
#pragma once
#include "ra_common.h"

namespace ra {

constexpr int kCtrlWgThreads = 1024;  // the one-workgroup kernels (inference and training): 16 waves per image

__device__ inline float sigm(float z) { return 1.0f / (1.0f + expf(-z)); }

// max or sum over the 16 waves of a one-workgroup kernel, wave results added in wave order; red: 16 floats of LDS.
// (ra_ctrl_split.hip's 4-wave version sums (a + b) + (c + d) and stays there.)
__device__ inline float block_reduce16(float v, bool is_max, float *red) {
  const int t = threadIdx.x;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float other = __shfl_xor(v, o);
    v = is_max ? fmaxf(v, other) : v + other;
  }
  __syncthreads();
  if ((t & 63) == 0) red[t >> 6] = v;
  __syncthreads();
  float r = red[0];
  for (int w = 1; w < kCtrlWgThreads / 64; ++w) r = is_max ? fmaxf(r, red[w]) : r + red[w];
  __syncthreads();
  return r;
}

// glimpse[c] = sum_g feat[g, c] * map[g]   (full_model.py:680), one workgroup of kCtrlWgThreads: threads = (channel, part
// of the positions), partial sums in red [parts * Cf], then out[c] for c < Cf (Cf <= 1024).  feat in LDS or global memory.
__device__ __forceinline__ void glimpse_readout(const float *feat, const float *gm, int G, int Cf, float *red, float *out) {
  const int t = threadIdx.x;
  const int parts = kCtrlWgThreads / Cf;
  const int c = t % Cf, part = t / Cf;
  if (part < parts) {
    float s = 0.0f;
    for (int g = part; g < G; g += parts) s += feat[(size_t)g * Cf + c] * gm[g];
    red[part * Cf + c] = s;
  }
  __syncthreads();
  if (t < Cf) {
    float s = 0.0f;
    for (int p = 0; p < parts; ++p) s += red[p * Cf + t];
    out[t] = s;
  }
  __syncthreads();
}

// The 9 controller outputs co -> one image's attention record rec [RA_ATTN_STRIDE]: centre (0, 1), size (2, 3), log-variance
// (4, 5), gammas (6..8), the normalised centre and log-size (9..12), zeros (13..15).  One thread calls.
__device__ __forceinline__ void store_attn_record(const ra_ctrl_desc &d, const float *co, float *r) {
  float cn[2] = {co[0], co[1]}, ls[2] = {co[2], co[3]};
  if (d.squash) {  // full_model.py:695-697
    cn[0] = tanhf(cn[0]);
    cn[1] = tanhf(cn[1]);
    ls[0] = -log1pf(expf(ls[0]));
    ls[1] = -log1pf(expf(ls[1]));
  }
  const float dim[2] = {(float)d.H, (float)d.W}, fs[2] = {(float)d.Fh, (float)d.Fw};
  for (int k = 0; k < 2; ++k) {
    const float ctr = (cn[k] + 1.0f) * (dim[k] / 2.0f);  // modellib.py:761-763
    const float size = expf(ls[k]) * dim[k];             // modellib.py:821-823
    float lv = d.fixed_var ? 0.0f : logf(size) - logf(fs[k]);  // modellib.py:791-792
    if (d.dynamic_var) lv = co[4 + k];
    r[0 + k] = ctr;
    r[2 + k] = size;
    r[4 + k] = lv;
    r[9 + k] = cn[k];
    r[11 + k] = ls[k];
  }
  r[6] = d.fixed_gamma ? 1.0f : expf(co[6]);  // full_model.py:711-719
  r[7] = expf(co[7]);
  r[8] = d.fixed_gamma ? 2.0f : co[8];
  r[13] = r[14] = r[15] = 0.0f;
}

}  // namespace ra
