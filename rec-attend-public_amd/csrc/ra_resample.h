// The per-pixel arithmetic of upsample_single (postprocess.py:93-106, fg_model_eval.py:106-117): cv2.resize(a, (W, H),
// INTER_LINEAR) and cv2.bilateralFilter(b, 5, sigma_color, sigma_space), as inline device functions.  ra_eval.hip's plane
// kernels (resize_linear_kernel, bilateral5_kernel) and ra_fg_eval.hip's fused threshold sweep call the SAME functions, so the
// value of a full-size pixel does not depend on which kernel evaluated it.
//   resize: pixel centres aligned — source coordinate (d + 0.5) * (src / dst) - 0.5, clamped to the image, two-tap linear
//   weights in float32 (cv2's float path; its 8-bit path uses fixed-point coefficients): the row pair first, then the rows;
//   bilateral: d = 5 -> radius 2, the CIRCULAR neighbourhood dy^2 + dx^2 <= 4 (13 pixels), weight
//   exp(-(dy^2 + dx^2) / (2 sigma_space^2) - (v - v0)^2 / (2 sigma_color^2)) as ONE expf of the summed exponent, borders
//   reflected without the edge pixel (BORDER_REFLECT_101).  cv2 evaluates the colour weight from an interpolated table; this
//   is the formula the table approximates (the two cannot be compared here: cv2 is not part of this stack).
#pragma once
#include <cmath>

#include <hip/hip_runtime.h>

namespace ra {
namespace resample {

__device__ inline int reflect101(int i, int n) {
  if (n == 1) return 0;
  while (i < 0 || i >= n) i = i < 0 ? -i : 2 * (n - 1) - i;
  return i;
}

// One axis of cv2.resize's float path with the source coordinate in DOUBLE, as cv2 evaluates it: pixel d of n_dst reads the taps
// i0, i1 of n_src with the weights 1 - w, w (scale = n_src / n_dst in double; the fraction is rounded to float once, taps
// clamped to the image).  A float coordinate is a few 1e-6 off at non-integer ratios; the semantic-map kernels
// (ra_instance_class.hip, ra_pixel_eval.hip) use this one, resize_linear_at below keeps its float coordinate.
__device__ __forceinline__ void tap(int d, int n_src, double scale, int &i0, int &i1, float &w) {
  const double f = ((double)d + 0.5) * scale - 0.5;
  int i = (int)floor(f);
  float fr = (float)(f - (double)i);
  if (i < 0) i = 0, fr = 0.f;
  if (i >= n_src - 1) i = n_src - 1, fr = 0.f;
  i0 = i;
  i1 = i + 1 < n_src ? i + 1 : i;
  w = fr;
}

// The channel holding the FIRST maximum (numpy.argmax) at pixel (r, c) of the H x W resize of the channel-last map semb
// [Hs,Ws,C] of one image; sy = Hs / H and sx = Ws / W in double.  All channels go through one loop body with the pixel's taps
// and weights, every product and sum rounded on its own, so channels that are equal at the four taps give exactly equal values
// and the lower index wins.  The label image of the semantic map (ra_pixel_eval.hip) and the orientation image
// (ra_render.hip) both call this one.
__device__ __forceinline__ int argmax_channel_at(const float *semb, int Hs, int Ws, int C, double sy, double sx, int r, int c) {
#pragma clang fp contract(off)
  int y0, y1, x0, x1;
  float fy, fx;
  tap(r, Hs, sy, y0, y1, fy);
  tap(c, Ws, sx, x0, x1, fx);
  const float *p00 = semb + ((size_t)y0 * Ws + x0) * C, *p01 = semb + ((size_t)y0 * Ws + x1) * C;
  const float *p10 = semb + ((size_t)y1 * Ws + x0) * C, *p11 = semb + ((size_t)y1 * Ws + x1) * C;
  const float gx = 1.f - fx, gy = 1.f - fy;
  float best = 0.f;
  int arg = 0;
  for (int ch = 0; ch < C; ++ch) {
    const float top = p00[ch] * gx + p01[ch] * fx;
    const float bot = p10[ch] * gx + p11[ch] * fx;
    const float v = top * gy + bot * fy;
    if (ch == 0 || v > best) best = v, arg = ch;  // strict: the first maximum, like numpy.argmax
  }
  return arg;
}

// pixel (r, c) of the H x W resize of the plane p [Hs, Ws]
__device__ inline float resize_linear_at(const float *p, int Hs, int Ws, int H, int W, int r, int c) {
  const float sy = (float)Hs / (float)H, sx = (float)Ws / (float)W;
  float fy = ((float)r + 0.5f) * sy - 0.5f, fx = ((float)c + 0.5f) * sx - 0.5f;
  int y0 = (int)floorf(fy), x0 = (int)floorf(fx);
  fy -= (float)y0;
  fx -= (float)x0;
  if (y0 < 0) y0 = 0, fy = 0.f;
  if (y0 >= Hs - 1) y0 = Hs - 1, fy = 0.f;
  if (x0 < 0) x0 = 0, fx = 0.f;
  if (x0 >= Ws - 1) x0 = Ws - 1, fx = 0.f;
  const int y1 = y0 + 1 < Hs ? y0 + 1 : y0, x1 = x0 + 1 < Ws ? x0 + 1 : x0;
  const float top = p[y0 * Ws + x0] * (1.f - fx) + p[y0 * Ws + x1] * fx;
  const float bot = p[y1 * Ws + x0] * (1.f - fx) + p[y1 * Ws + x1] * fx;
  return top * (1.f - fy) + bot * fy;
}

// gs = -0.5 / sigma_space^2, gc = -0.5 / sigma_color^2
__device__ inline float bilateral_gain(float sigma) { return -0.5f / (sigma * sigma); }

// The filtered value of a pixel whose own value is v0; at(dy, dx) is the (border-reflected) neighbour at that offset.  The 13
// taps are visited row by row (dy outer, dx inner), numerator and denominator each one running float32 sum.
template <typename At>
__device__ inline float bilateral5_at(At at, float v0, float gs, float gc) {
  float num = 0.f, den = 0.f;
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy)
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      if (dy * dy + dx * dx > 4) continue;
      const float v = at(dy, dx);
      const float w = expf((float)(dy * dy + dx * dx) * gs + (v - v0) * (v - v0) * gc);
      num += w * v;
      den += w;
    }
  return num / den;
}

}  // namespace resample
}  // namespace ra
