// K22 — the image stage in front of the label stage: the colour image x at network size from the full-size 8-bit image
// (data_api/ins_seg_assembler.py:116, cv2.resize(img, inp_shape, interpolation=cv2.INTER_CUBIC), read back as
// x / 255 by ins_seg_dataset.py:149), and the row filters of the PNG files those images come in.  cv2 is not part of this
// stack: its fixed-point recipe for 8-bit images is RESTATED here (include/recattend.h has the definition), all in
// integers once the two axes' tables exist, so the result is the same bits wherever it runs.
//
//   tables    host code: per destination index the first tap's source index and four 11-bit weights, float32 arithmetic in
//             cv2's order, built without contraction to fused multiply-adds (the Makefile says so for this file).
//   resize    a workgroup of 256 threads owns 4 rows x 64 columns of the output.  It needs at most 16 source rows (four taps
//             per output row; the rows of the span itself when those are fewer, as at every ratio below 4).
//               stage       the bytes of those rows that the tile's columns touch, 16 bytes per lane into LDS — when every
//                           source row starts on a 16-byte boundary (Ws * C % 16 == 0) and the span fits; otherwise the next
//                           step reads its taps from global memory byte by byte;
//               horizontal  thread (row j, column d): sum of 4 taps per channel, int32 into LDS (23 bits);
//               vertical    thread (row r, 4 consecutive channel values): 4 taps out of LDS, + 2^21 >> 22, clamp, and the
//                           stores — one 32-bit word of dst_u8, 16 bytes of dst_f32 — when W * C % 4 == 0 and the outputs
//                           are aligned; element stores otherwise.
//             At an integer ratio of 4 the taps of neighbouring outputs do not overlap: every source byte is read once.
//   unfilter  host code: PNG specification 9.2, a plain loop over the scanlines.
//
// Every tap index is clamped to the image inside the kernel, and every index into the staged bytes and rows to the buffer:
// tables that do not belong to the shape give wrong pixels, never an access outside src or LDS.
#include <cmath>
#include <cstdint>
#include <cstring>

#include "ra_common.h"

namespace ra {
namespace img {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
constexpr int kTW = 64;           // output columns per workgroup: one wave = one row of the horizontal pass
constexpr int kTH = 4;            // output rows per workgroup: 28 KB of LDS, five workgroups per CU.  Measured against 2 and
                                  // 8 rows (profiles/image_stage.txt): 2 the same, 8 slower
constexpr int kRows = 4 * kTH;    // source rows a tile can need
constexpr int kPitch = 1024;      // bytes of one staged row: 64 columns at ratio 4 x 3 channels = 777, + alignment
constexpr int kCoefBits = 11;     // cv2's INTER_RESIZE_COEF_BITS
constexpr int kMaxN = 65535;      // the grid's y extent

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The horizontal pass of one thread: column d of the rows j = j0, j0 + 4, ...  row(j): the bytes of source row j, counted from
// the byte the offsets xb are relative to (the row's first byte in global memory, byte b0 of it in the staged copy)
template <int C, typename RowPtr>
__device__ __forceinline__ void horizontal(RowPtr row, int j0, int nrows, int d, const int (&xb)[4], const int (&q)[4], int *hbuf) {
  for (int j = j0; j < nrows; j += 4) {
    const unsigned char *p = row(j);
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
      int h = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) h += q[k] * (int)p[xb[k] + ch];
      hbuf[j * (kTW * C) + d * C + ch] = h;
    }
  }
}

// Workgroup (tile, n): tile = ty * ntx + tx owns the output rows ty * kTH .. and columns tx * kTW .. of image n.
// stage_ok: Ws * C % 16 == 0 and src 16-byte aligned.  VEC: W * C % 4 == 0, dst_u8 4-byte and dst_f32 16-byte aligned.
template <int C, bool VEC>
__global__ __launch_bounds__(256) void resize_cubic_kernel(const unsigned char *src, int Hs, int Ws, int H, int W, int ntx,
                                                            const int *ofs_y, const short *coef_y, const int *ofs_x,
                                                            const short *coef_x, int stage_ok, unsigned char *dst_u8,
                                                            float *dst_f32) {
  constexpr int TWC = kTW * C;
  __shared__ __attribute__((aligned(16))) int hbuf[kRows * TWC];
  __shared__ __attribute__((aligned(16))) unsigned char stage[kRows * kPitch];
  __shared__ int row_src[kRows];  // the source row of h-row j
  __shared__ int vidx[kRows];     // [r][k]: the h-row of output row r's tap k
  __shared__ int vq[kRows];       // [r][k]: its weight
  const int tid = threadIdx.x, n = blockIdx.y;
  const int ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
  const int r0 = ty * kTH, c0 = tx * kTW;
  const int nr = H - r0 < kTH ? H - r0 : kTH, nc = W - c0 < kTW ? W - c0 : kTW;
  // the rows: the span of the tile's taps when it has at most kRows rows, else the 4 taps of every output row
  const int lo = clampi(ofs_y[r0] - 1, 0, Hs - 1), hi = clampi(ofs_y[r0 + nr - 1] + 2, 0, Hs - 1);
  const bool span_mode = hi >= lo && hi - lo < kRows;
  const int nrows = span_mode ? hi - lo + 1 : 4 * nr;
  if (tid < 4 * nr) {
    const int r = tid >> 2, k = tid & 3;
    const int sr = clampi(ofs_y[r0 + r] - 1 + k, 0, Hs - 1);
    vidx[tid] = span_mode ? clampi(sr - lo, 0, nrows - 1) : tid;
    vq[tid] = coef_y[(size_t)(r0 + r) * 4 + k];
    if (!span_mode) row_src[tid] = sr;
  }
  if (span_mode && tid < nrows) row_src[tid] = lo + tid;
  // the columns: bytes [b0, b1) of a source row, widened to 16-byte boundaries (b1 <= Ws * C since that is a multiple of 16)
  const int xlo = clampi(ofs_x[c0] - 1, 0, Ws - 1), xhi = clampi(ofs_x[c0 + nc - 1] + 2, 0, Ws - 1);
  const int b0 = (xlo * C) & ~15, b1 = ((xhi + 1) * C + 15) & ~15;
  const bool staged = stage_ok && b1 > b0 && b1 - b0 <= kPitch;
  __syncthreads();
  const size_t row_bytes = (size_t)Ws * C;
  const unsigned char *img = src + (size_t)n * Hs * row_bytes;
  if (staged) {
    const int nv = (b1 - b0) >> 4, total = nrows * nv;
#pragma unroll 4
    for (int i = tid; i < total; i += 256) {
      const int j = i / nv, v = i - j * nv;
      const u32x4 w = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(img + (size_t)row_src[j] * row_bytes + b0 + 16 * v));
      *reinterpret_cast<u32x4 *>(stage + j * kPitch + 16 * v) = w;
    }
    __syncthreads();
  }
  const int d = tid & 63;
  if (d < nc) {
    const int s = ofs_x[c0 + d];
    int xb[4], q[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      q[k] = coef_x[(size_t)(c0 + d) * 4 + k];
      xb[k] = clampi(s - 1 + k, 0, Ws - 1) * C;
    }
    if (staged) {
#pragma unroll
      for (int k = 0; k < 4; ++k) xb[k] = clampi(xb[k] - b0, 0, kPitch - C);
      horizontal<C>([&](int j) { return stage + j * kPitch; }, tid >> 6, nrows, d, xb, q, hbuf);
    } else {
      horizontal<C>([&](int j) { return img + (size_t)row_src[j] * row_bytes; }, tid >> 6, nrows, d, xb, q, hbuf);
    }
  }
  __syncthreads();
  const size_t out0 = (((size_t)n * H + r0) * W + c0) * C;  // the tile's first element
  const int ncC = nc * C;
  if (VEC) {
    constexpr int QW = TWC / 4;  // quads per tile row
    for (int e = tid; e < nr * QW; e += 256) {
      const int r = e / QW, qd = 4 * (e - r * QW);
      if (qd >= ncC) continue;  // ncC % 4 == 0
      i32x4 v = {0, 0, 0, 0};
#pragma unroll
      for (int k = 0; k < 4; ++k) v += vq[4 * r + k] * *reinterpret_cast<const i32x4 *>(hbuf + vidx[4 * r + k] * TWC + qd);
      unsigned pack = 0;
      f32x4 f;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int level = clampi((v[u] + (1 << (2 * kCoefBits - 1))) >> (2 * kCoefBits), 0, 255);
        pack |= (unsigned)level << (8 * u);
        f[u] = __fdiv_rn((float)level, 255.0f);
      }
      const size_t o = out0 + (size_t)r * W * C + qd;
      if (dst_u8) *reinterpret_cast<unsigned *>(dst_u8 + o) = pack;
      if (dst_f32) *reinterpret_cast<f32x4 *>(dst_f32 + o) = f;
    }
  } else {
    for (int e = tid; e < nr * TWC; e += 256) {
      const int r = e / TWC, qd = e - r * TWC;
      if (qd >= ncC) continue;
      int v = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) v += vq[4 * r + k] * hbuf[vidx[4 * r + k] * TWC + qd];
      const int level = clampi((v + (1 << (2 * kCoefBits - 1))) >> (2 * kCoefBits), 0, 255);
      const size_t o = out0 + (size_t)r * W * C + qd;
      if (dst_u8) dst_u8[o] = (unsigned char)level;
      if (dst_f32) dst_f32[o] = __fdiv_rn((float)level, 255.0f);
    }
  }
}

template <int C>
int launch(const unsigned char *src, int N, int Hs, int Ws, int H, int W, const int *ofs_y, const short *coef_y,
           const int *ofs_x, const short *coef_x, unsigned char *dst_u8, float *dst_f32, hipStream_t st) {
  const int ntx = ceil_div(W, kTW), nty = ceil_div(H, kTH);  // ntx * nty <= H * W < 2^31
  const int stage_ok = ((size_t)Ws * C) % 16 == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0;
  const bool vec = (W * C) % 4 == 0 && (reinterpret_cast<uintptr_t>(dst_u8) & 3) == 0 && (reinterpret_cast<uintptr_t>(dst_f32) & 15) == 0;
  const dim3 grid((unsigned)(ntx * nty), N);
  if (vec)
    hipLaunchKernelGGL((resize_cubic_kernel<C, true>), grid, dim3(256), 0, st, src, Hs, Ws, H, W, ntx, ofs_y, coef_y, ofs_x, coef_x,
                       stage_ok, dst_u8, dst_f32);
  else
    hipLaunchKernelGGL((resize_cubic_kernel<C, false>), grid, dim3(256), 0, st, src, Hs, Ws, H, W, ntx, ofs_y, coef_y, ofs_x, coef_x,
                       stage_ok, dst_u8, dst_f32);
  return launch_status("ra_resize_cubic_u8");
}

// cv2's interpolateCubic, float32, in its order of operations
inline void cubic_weights(float t, float *c) {
  const float A = -0.75f;
  c[0] = ((A * (t + 1) - 5 * A) * (t + 1) + 8 * A) * (t + 1) - 4 * A;
  c[1] = ((A + 2) * t - (A + 3)) * t * t + 1;
  c[2] = ((A + 2) * (1 - t) - (A + 3)) * (1 - t) * (1 - t) + 1;
  c[3] = 1.f - c[0] - c[1] - c[2];
}

inline unsigned char paeth(int a, int b, int c) {
  const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
  return (unsigned char)((pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c));
}

}  // namespace img
}  // namespace ra

using namespace ra;

extern "C" int ra_resize_cubic_tables(int S, int D, int *ofs, short *coef) {
  if (!ofs || !coef || S < 1 || D < 1) return fail(RA_E_SHAPE, "ra_resize_cubic_tables: S=%d D=%d (S >= 1, D >= 1, tables not null)", S, D);
  const double scale = (double)S / (double)D;
  for (int d = 0; d < D; ++d) {
    float f = (float)((d + 0.5) * scale - 0.5);
    const int s = (int)floorf(f);
    f -= (float)s;
    float c[4];
    img::cubic_weights(f, c);
    ofs[d] = s;
    for (int k = 0; k < 4; ++k) coef[4 * d + k] = (short)lrintf(c[k] * (float)(1 << img::kCoefBits));  // half to even
  }
  return 0;
}

extern "C" int ra_resize_cubic_u8(const unsigned char *src, int N, int Hs, int Ws, int C, int H, int W, const int *ofs_y,
                                  const short *coef_y, const int *ofs_x, const short *coef_x, unsigned char *dst_u8,
                                  float *dst_f32, void *stream) {
  const long long lim = 1ll << 31;
  if (!src || !ofs_y || !coef_y || !ofs_x || !coef_x || N < 1 || N > img::kMaxN || (C != 1 && C != 3) || Hs < 1 || Ws < 1 || H < 1 ||
      W < 1 || (long long)Hs * Ws * C >= lim || (long long)H * W * C * (dst_f32 ? 4 : 1) >= lim)
    return fail(RA_E_SHAPE, "ra_resize_cubic_u8: N=%d %dx%d -> %dx%d C=%d src%s tables%s (1 <= N <= %d, C = 1 | 3, every size >= 1, "
                "Hs * Ws * C < 2^31, the bytes of an output plane < 2^31, src and the tables not null)", N, Hs, Ws, H, W, C,
                src ? "" : "=null", (ofs_y && coef_y && ofs_x && coef_x) ? "" : "=null", img::kMaxN);
  if (!dst_u8 && !dst_f32) return 0;
  hipStream_t st = as_stream(stream);
  return C == 3 ? img::launch<3>(src, N, Hs, Ws, H, W, ofs_y, coef_y, ofs_x, coef_x, dst_u8, dst_f32, st)
                : img::launch<1>(src, N, Hs, Ws, H, W, ofs_y, coef_y, ofs_x, coef_x, dst_u8, dst_f32, st);
}

extern "C" int ra_png_unfilter_u8(const unsigned char *raw, int H, int stride, int bpp, unsigned char *out) {
  if (!raw || !out || H < 1 || stride < 1 || bpp < 1 || bpp > 8 || stride % bpp)
    return fail(RA_E_SHAPE, "ra_png_unfilter_u8: H=%d stride=%d bpp=%d (H >= 1, 1 <= bpp <= 8, stride a positive multiple of bpp, "
                "buffers not null)", H, stride, bpp);
  for (int r = 0; r < H; ++r)
    if (raw[(size_t)r * (stride + 1)] > 4)
      return fail(RA_E_SHAPE, "ra_png_unfilter_u8: row %d has filter type %d", r, (int)raw[(size_t)r * (stride + 1)]);
  for (int r = 0; r < H; ++r) {
    const unsigned char *x = raw + (size_t)r * (stride + 1) + 1;
    unsigned char *o = out + (size_t)r * stride;
    const unsigned char *up = r ? o - stride : nullptr;  // a zero row above the first (9.2)
    const int lead = bpp < stride ? bpp : stride;        // the bytes with nothing to their left
    switch (x[-1]) {
      case 0:
        memcpy(o, x, stride);
        break;
      case 1:
        memcpy(o, x, lead);
        for (int i = bpp; i < stride; ++i) o[i] = (unsigned char)(x[i] + o[i - bpp]);
        break;
      case 2:
        for (int i = 0; i < stride; ++i) o[i] = (unsigned char)(x[i] + (up ? up[i] : 0));
        break;
      case 3:
        for (int i = 0; i < lead; ++i) o[i] = (unsigned char)(x[i] + ((up ? up[i] : 0) >> 1));
        for (int i = bpp; i < stride; ++i) o[i] = (unsigned char)(x[i] + ((o[i - bpp] + (up ? up[i] : 0)) >> 1));
        break;
      default:
        for (int i = 0; i < lead; ++i) o[i] = (unsigned char)(x[i] + img::paeth(0, up ? up[i] : 0, 0));
        for (int i = bpp; i < stride; ++i)
          o[i] = (unsigned char)(x[i] + img::paeth(o[i - bpp], up ? up[i] : 0, up ? up[i - bpp] : 0));
        break;
    }
  }
  return 0;
}
