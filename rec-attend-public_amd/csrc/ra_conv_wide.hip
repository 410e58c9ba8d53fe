// K1-wide — the wide 3x3 layer: K1's fused layer (ra_conv.hip) for Cout 129 .. 512 and C0 + C1 up to 1024, the channel
// widths of fg_model's inner layers (fg_model.py:112-160 through nnlib.cnn / nnlib.dcnn).  Same layer: 3x3 SAME conv, or
// SAME conv2d_transpose stride 1 | 2 as a conv of the (zero-stuffed) input with the flipped, in/out-swapped filter,
// two sources for concat(prev, skip), bias + BN(eval) + ReLU + 2x2 max-pool in the epilogue, NHWC float32.
//
// GEMM view: D[pixel, cout] = sum_k A[pixel, k] B[k, cout], k = (chunk of 16 channels, tap, channel).  Exact float32 on
// v_mfma_f32_16x16x4_f32.  K1 keeps a chunk's B operand in registers; at these widths it cannot (1024 x 512 x 9 floats
// = 18 MB), so BOTH operands go through LDS and the Cout range is split over workgroups:
//   workgroup = 4 waves, tile = 8 x 8 conv pixels x 64 output channels (grid.y = Cout slices of 64, ragged last);
//   wave (wm, wn) owns 32 pixels x 32 channels = 2 x 2 MFMA tiles: four independent accumulators, which is what the
//   40-cycle dependent latency of the 32-cycle instruction asks for.  Where that grid has fewer workgroups than the chip has
//   CUs (the 4 x 8 .. 8 x 16 maps) a workgroup takes 32 channels, half a slice: four waves of 16 pixels x 32 channels;
//   per chunk LDS holds the 10 x 10 halo pixels as [pixel][ksub][cg] (channel 4 cg + ksub: one ds_read_b128 is a lane's A
//   operands of the tap's 4 k-steps) and the slice's filter as [tap][ksub][cout 64][cg] (again one ds_read_b128 per tap
//   and MFMA column tile), which is the packed order in memory, so staging B is a straight 16-byte copy.
// Numerics: a chunk's 144 products are chained inside the MFMA (k-ordered fmaf); the chunk sums are then added to the
// running totals with v_add — blocked summation, so a k chain of 9216 carries the rounding of 144 + 64 terms, not of 9216.
// The order is fixed: results are identical from run to run.
// Epilogue: scale / shift / ReLU in registers, the 64 x 64 tile goes through LDS so that the pool is a max over four
// LDS rows and every global store is a 16-byte piece of a pixel's channel run.
#include "ra_common.h"

namespace ra {
namespace convw {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int CK = 16;                  // channels per chunk
constexpr int TS = 8;                   // tile side (conv pixels)
constexpr int LS = TS + 2;              // with halo
constexpr int NS = 64;                  // output channels per slice of the packed filter
constexpr int A_FLOATS = LS * LS * CK;  // 1600
constexpr int B_FLOATS = 9 * CK * NS;   // 9216 = one (slice, chunk) of the packed filter
// NW = output channels per workgroup: 64 (waves 2 x 2, each 2 x 2 MFMA tiles), or 32 — half a slice, waves 4 x 1, each 1 x 2
// tiles — where 64 would leave most CUs without a workgroup (the 4 x 8 .. 8 x 16 maps with 512 channels)
template <int NW>
struct Geo {
  static constexpr int WN = NW / 32, WM = 4 / WN, MI = 4 / WM;  // waves along channels / pixels, pixel tiles per wave
  static constexpr int BW = 9 * CK * NW;                        // filter floats in LDS
  static constexpr int OUT_LD = NW + 4;                         // epilogue tile row (padded: rows 16 B apart in bank space)
  static_assert(TS * TS * OUT_LD <= A_FLOATS + BW, "the epilogue tile reuses the operands' LDS");
};

struct Args {
  const float *src0, *src1, *wp, *scale, *shift;
  float *y;
  int C0, C1, Hs, Ws, H, W, ups, Cout, relu, pool, Ho, Wo, tiles_x, tiles_y, nchunk;
};

template <int NW>
__global__ __launch_bounds__(256) void conv3x3_wide(const Args a) {
  typedef Geo<NW> G;
  constexpr int MI = G::MI, OUT_LD = G::OUT_LD;
  __shared__ __attribute__((aligned(16))) float lds[A_FLOATS + G::BW];
  float *la = lds, *lb = lds + A_FLOATS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave / G::WN, wn = wave % G::WN;
  int t = blockIdx.x;
  const int tx = t % a.tiles_x;
  t /= a.tiles_x;
  const int ty = t % a.tiles_y, b = t / a.tiles_y;
  const int y0 = ty * TS, x0 = tx * TS;
  const int slice = blockIdx.y / (NS / NW), part = blockIdx.y % (NS / NW), co0 = slice * NS + part * NW;  // first output channel
  const int Cin = a.C0 + a.C1;
  const int m = lane & 15, ksub = lane >> 4;

  f32x4 tot[MI][2];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) tot[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // LDS float offset of this lane's A record for pixel tile i at tap (0, 0): pixel p = (MI wm + i) * 16 + m -> row p / 8, col p % 8
  int aoff[MI];
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int p = (MI * wm + i) * 16 + m;
    aoff[i] = ((p >> 3) * LS + (p & 7)) * CK + ksub * 4;
  }
  const int boff = (ksub * NW + wn * 32 + m) * 4;  // + tap * 4 * NW * 4, + j * 16 * 4

  const float *wslice = a.wp + (size_t)slice * a.nchunk * B_FLOATS;
  for (int ch = 0; ch < a.nchunk; ++ch) {
    __syncthreads();  // the previous chunk's reads are done
    // ---- stage A: halo pixel hp = r * LS + c, channel quad q (channels ch * 16 + 4 q ..+3 = cg q, ksub 0..3)
    for (int e = tid; e < LS * LS * 4; e += 256) {
      const int hp = e >> 2, q = e & 3, r = hp / LS, c = hp - r * LS;
      int yy = y0 + r - 1, xx = x0 + c - 1;
      bool ok = yy >= 0 && yy < a.H && xx >= 0 && xx < a.W;
      if (a.ups) {  // zero-stuffed U[2 i + 1, 2 j + 1] = src[i, j]
        ok = ok && (yy & 1) && (xx & 1);
        yy >>= 1;
        xx >>= 1;
      }
      const int cc = ch * CK + 4 * q;
      f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
      if (ok && cc < Cin) {
        const size_t pix = ((size_t)b * a.Hs + yy) * a.Ws + xx;
        const float *p = cc < a.C0 ? a.src0 + pix * a.C0 + cc : a.src1 + pix * a.C1 + (cc - a.C0);
        v = *reinterpret_cast<const f32x4 *>(p);
      }
      float *d = la + hp * CK + q;
      d[0] = v.x;
      d[4] = v.y;
      d[8] = v.z;
      d[12] = v.w;
    }
    // ---- stage B: the 36 (tap, ksub) rows of the slice's chunk, NW of a row's 64 channels (NW = 64: 9216 contiguous floats)
    {
      const f32x4 *g = reinterpret_cast<const f32x4 *>(wslice + (size_t)ch * B_FLOATS + part * NW * 4);
      f32x4 *d = reinterpret_cast<f32x4 *>(lb);
      constexpr int NP = G::BW / 4;  // 16-byte pieces, NW per row; all loads of a thread in flight together
      f32x4 v[(NP + 255) / 256];
#pragma unroll
      for (int e = 0; e < (NP + 255) / 256; ++e) {
        const int q = tid + e * 256;
        if (q < NP) v[e] = g[(q / NW) * NS + q % NW];
      }
#pragma unroll
      for (int e = 0; e < (NP + 255) / 256; ++e)
        if (tid + e * 256 < NP) d[tid + e * 256] = v[e];
    }
    __syncthreads();
    f32x4 acc[MI][2];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int ky = tap / 3, kx = tap % 3;
      f32x4 av[MI], bv[2];
#pragma unroll
      for (int i = 0; i < MI; ++i) av[i] = *reinterpret_cast<const f32x4 *>(la + aoff[i] + (ky * LS + kx) * CK);
#pragma unroll
      for (int j = 0; j < 2; ++j) bv[j] = *reinterpret_cast<const f32x4 *>(lb + boff + tap * (4 * NW * 4) + j * 64);
#pragma unroll
      for (int cg = 0; cg < 4; ++cg)
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i][cg], bv[j][cg], acc[i][j], 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) tot[i][j] += acc[i][j];
  }

  // ---- epilogue: D register r of a lane = pixel row 4 * (lane >> 4) + r, channel column lane & 15
  __syncthreads();
  float *lo = lds;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int cl = wn * 32 + j * 16 + m, co = co0 + cl;
    const float sc = co < a.Cout ? a.scale[co] : 0.f, sh = co < a.Cout ? a.shift[co] : 0.f;
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = tot[i][j][r] * sc + sh;
        if (a.relu) v = fmaxf(v, 0.f);
        lo[((MI * wm + i) * 16 + ksub * 4 + r) * OUT_LD + cl] = v;
      }
  }
  __syncthreads();
  if (a.pool == 1) {
    for (int e = tid; e < TS * TS * (NW / 4); e += 256) {
      const int p = e / (NW / 4), c4 = (e % (NW / 4)) * 4, yy = y0 + (p >> 3), xx = x0 + (p & 7), co = co0 + c4;
      if (yy < a.H && xx < a.W && co < a.Cout)
        *reinterpret_cast<f32x4 *>(a.y + (((size_t)b * a.Ho + yy) * a.Wo + xx) * a.Cout + co) =
            *reinterpret_cast<const f32x4 *>(lo + p * OUT_LD + c4);
    }
  } else if (tid < 16 * (NW / 4)) {
    const int p = tid / (NW / 4), c4 = (tid % (NW / 4)) * 4, py = p >> 2, px = p & 3, co = co0 + c4;
    const int oy = (y0 >> 1) + py, ox = (x0 >> 1) + px;
    if (oy < a.Ho && ox < a.Wo && co < a.Cout) {
      const float *s = lo + ((2 * py) * TS + 2 * px) * OUT_LD + c4;
      const f32x4 v0 = *reinterpret_cast<const f32x4 *>(s), v1 = *reinterpret_cast<const f32x4 *>(s + OUT_LD),
                  v2 = *reinterpret_cast<const f32x4 *>(s + TS * OUT_LD), v3 = *reinterpret_cast<const f32x4 *>(s + (TS + 1) * OUT_LD);
      f32x4 v;
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = fmaxf(fmaxf(v0[k], v1[k]), fmaxf(v2[k], v3[k]));
      *reinterpret_cast<f32x4 *>(a.y + (((size_t)b * a.Ho + oy) * a.Wo + ox) * a.Cout + co) = v;
    }
  }
}

// ---- the head (fg_model.py:179-194): one thread per pixel
struct HeadArgs {
  const float *logits;
  float *y_out, *d_out;
  const float *x;  // packed destination only
  float *packed, *canvas;
  size_t npix;
  int nsc, no, quant, D, Cp;
};

__device__ inline float quantise(float v, int q) { return q ? floorf(v * 255.f) / 255.f : v; }

template <int N>
__device__ inline void softmax_n(float *v, int n) {
  float mx = v[0];
  for (int k = 1; k < n; ++k) mx = fmaxf(mx, v[k]);
  float s = 0.f;
  for (int k = 0; k < n; ++k) {
    v[k] = expf(v[k] - mx);
    s += v[k];
  }
  for (int k = 0; k < n; ++k) v[k] = v[k] / s;
}

__global__ __launch_bounds__(256) void fg_head(const HeadArgs a) {
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= a.npix) return;
  const int C = a.nsc + a.no;
  const float *l = a.logits + p * C;
  float ys[16], ds[8];  // runtime-indexed: a few scratch words per pixel, nothing beside the conv in front of it
  for (int k = 0; k < 16; ++k) ys[k] = k < a.nsc ? l[k] : 0.f;
  for (int k = 0; k < 8; ++k) ds[k] = k < a.no ? l[a.nsc + k] : 0.f;
  if (a.nsc == 1)
    ys[0] = 1.f / (1.f + expf(-ys[0]));
  else
    softmax_n<16>(ys, a.nsc);
  if (a.no) softmax_n<8>(ds, a.no);
#pragma unroll
  for (int k = 0; k < 16; ++k)
    if (k < a.nsc) {
      ys[k] = quantise(ys[k], a.quant);
      a.y_out[p * a.nsc + k] = ys[k];
    }
#pragma unroll
  for (int k = 0; k < 8; ++k)
    if (k < a.no) {
      ds[k] = quantise(ds[k], a.quant);
      a.d_out[p * a.no + k] = ds[k];
    }
  if (a.packed) {  // [x (D) | canvas = 0 | d_in (no) | y_in (nsc) | 0 ...]: ra_pack_input_plane_f32's pixel
    float *o = a.packed + p * a.Cp;
    for (int c = 0; c < a.Cp; ++c) {
      float w = 0.f;
      if (c < a.D) w = a.x[p * a.D + c];
      o[c] = w;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (k < a.no) o[a.D + 1 + k] = ds[k];
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (k < a.nsc) o[a.D + 1 + a.no + k] = ys[k];
    if (a.canvas) a.canvas[p] = 0.f;
  }
}

// ra_conv_wide_pack_weights on the device, for the output channels [co_first, co_first + co_count) of the filter: one thread per
// packed float, the host loop's index arithmetic.  nslice / nchunk are those of the packed slice (Cin, co_count).
__global__ __launch_bounds__(256) void pack_wide_kernel(const float *w, int Cin_w, int Cout, int Cin, const int *chan_map, int tr,
                                                        int co_first, int co_count, int nchunk, size_t total, float *out) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  size_t r = e;
  const int cg = r & 3;
  r >>= 2;
  const int n = r % NS;
  r /= NS;
  const int ksub = r & 3;
  r >>= 2;
  const int tap = r % 9;
  r /= 9;
  const int ch = r % nchunk, s = (int)(r / nchunk);
  const int c = ch * CK + 4 * cg + ksub, col = s * NS + n, co = co_first + col, ky = tap / 3, kx = tap % 3;
  float v = 0.f;
  const int src_c = c < Cin ? (chan_map ? chan_map[c] : c) : -1;
  if (col < co_count && src_c >= 0 && src_c < Cin_w)
    v = tr ? w[(((size_t)(2 - ky) * 3 + (2 - kx)) * Cout + co) * Cin_w + src_c] : w[(((size_t)ky * 3 + kx) * Cin_w + src_c) * Cout + co];
  out[e] = v;
}

}  // namespace convw
}  // namespace ra

using namespace ra;

extern "C" int ra_conv_wide_supported(int Cin, int Cout) {
  return Cin > 0 && Cin <= 1024 && Cin % 4 == 0 && Cout > 128 && Cout <= 512 && Cout % 16 == 0;
}

extern "C" size_t ra_conv_wide_packed_floats(int Cin, int Cout) {
  if (!ra_conv_wide_supported(Cin, Cout)) return 0;
  return (size_t)ceil_div(Cout, convw::NS) * ceil_div(Cin, convw::CK) * convw::B_FLOATS;
}

// Packed order: [slice = co / 64][chunk = c / 16][tap = ky * 3 + kx][ksub][n = co % 64][cg], channel c = chunk * 16 + 4 cg + ksub;
// channels past Cin and output channels past Cout hold zeros.
extern "C" int ra_conv_wide_pack_weights(const float *w, int Cin_w, int Cout, int Cin, const int *chan_map, int flags, float *out) {
  if (!w || !out || Cin_w <= 0) return fail(RA_E_INVALID, "ra_conv_wide_pack_weights: bad argument");
  if (!ra_conv_wide_supported(Cin, Cout))
    return fail(RA_E_SHAPE, "ra_conv_wide_pack_weights: Cin %d (%% 4, <= 1024) or Cout %d (129 .. 512, %% 16)", Cin, Cout);
  if (!chan_map && Cin_w != Cin) return fail(RA_E_SHAPE, "ra_conv_wide_pack_weights: Cin_w != Cin without map");
  const int nchunk = ceil_div(Cin, convw::CK), nslice = ceil_div(Cout, convw::NS);
  const bool tr = flags & RA_CONV_TRANSPOSED;
  for (int c = 0; c < Cin; ++c) {
    const int src_c = chan_map ? chan_map[c] : c;
    if (src_c >= Cin_w) return fail(RA_E_SHAPE, "ra_conv_wide_pack_weights: chan_map[%d] = %d", c, src_c);
  }
  for (int s = 0; s < nslice; ++s)
    for (int ch = 0; ch < nchunk; ++ch)
      for (int tap = 0; tap < 9; ++tap)
        for (int ksub = 0; ksub < 4; ++ksub)
          for (int n = 0; n < convw::NS; ++n)
            for (int cg = 0; cg < 4; ++cg) {
              const int c = ch * convw::CK + 4 * cg + ksub, co = s * convw::NS + n, ky = tap / 3, kx = tap % 3;
              float v = 0.f;
              const int src_c = c < Cin ? (chan_map ? chan_map[c] : c) : -1;
              if (co < Cout && src_c >= 0)
                v = tr ? w[(((size_t)(2 - ky) * 3 + (2 - kx)) * Cout + co) * Cin_w + src_c]
                       : w[(((size_t)ky * 3 + kx) * Cin_w + src_c) * Cout + co];
              out[(((((size_t)s * nchunk + ch) * 9 + tap) * 4 + ksub) * convw::NS + n) * 4 + cg] = v;
            }
  return 0;
}

extern "C" int ra_conv_wide_pack_weights_dev(const float *w, int Cin_w, int Cout, int Cin, const int *chan_map, int flags, int co_first,
                                             int co_count, float *out, void *stream) {
  if (!w || !out || Cin_w <= 0 || Cout <= 0 || co_first < 0 || co_count <= 0)
    return fail(RA_E_INVALID, "ra_conv_wide_pack_weights_dev: bad argument");
  if (!ra_conv_wide_supported(Cin, co_count))
    return fail(RA_E_SHAPE, "ra_conv_wide_pack_weights_dev: Cin %d (%% 4, <= 1024) or co_count %d (129 .. 512, %% 16)", Cin, co_count);
  if (co_first + co_count > Cout) return fail(RA_E_SHAPE, "ra_conv_wide_pack_weights_dev: channels [%d, %d) of %d", co_first, co_first + co_count, Cout);
  if (!chan_map && Cin_w != Cin) return fail(RA_E_SHAPE, "ra_conv_wide_pack_weights_dev: Cin_w != Cin without map");
  const size_t total = ra_conv_wide_packed_floats(Cin, co_count);
  hipLaunchKernelGGL(convw::pack_wide_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), w, Cin_w, Cout, Cin,
                     chan_map, (flags & RA_CONV_TRANSPOSED) ? 1 : 0, co_first, co_count, ceil_div(Cin, convw::CK), total, out);
  return launch_status("ra_conv_wide_pack_weights_dev");
}

extern "C" int ra_conv3x3_wide_f32(const float *src0, int C0, const float *src1, int C1, int B, int Hs, int Ws, int upsample,
                                   const float *wpacked, const float *scale, const float *shift, int Cout, int relu, int pool,
                                   float *y, void *stream) {
  if (!src0 || !wpacked || !scale || !shift || !y || B <= 0 || Hs <= 0 || Ws <= 0 || C0 <= 0 || C1 < 0 || (C1 > 0 && !src1))
    return fail(RA_E_INVALID, "ra_conv3x3_wide_f32: bad argument");
  if (C0 % 4 || C1 % 4 || !ra_conv_wide_supported(C0 + C1, Cout))
    return fail(RA_E_SHAPE, "ra_conv3x3_wide_f32: C0=%d C1=%d (each %% 4, sum <= 1024), Cout=%d (129 .. 512, %% 16)", C0, C1, Cout);
  if (pool != 1 && pool != 2) return fail(RA_E_SHAPE, "ra_conv3x3_wide_f32: pool %d", pool);
  convw::Args a;
  a.src0 = src0, a.src1 = src1, a.wp = wpacked, a.scale = scale, a.shift = shift, a.y = y;
  a.C0 = C0, a.C1 = C1, a.Hs = Hs, a.Ws = Ws, a.ups = upsample ? 1 : 0;
  a.H = Hs * (1 + a.ups), a.W = Ws * (1 + a.ups);
  if (pool == 2 && ((a.H | a.W) & 1)) return fail(RA_E_SHAPE, "ra_conv3x3_wide_f32: odd size with pool 2");
  a.Cout = Cout, a.relu = relu ? 1 : 0, a.pool = pool, a.Ho = a.H / pool, a.Wo = a.W / pool;
  a.tiles_x = ceil_div(a.W, convw::TS), a.tiles_y = ceil_div(a.H, convw::TS), a.nchunk = ceil_div(C0 + C1, convw::CK);
  const size_t tiles = (size_t)a.tiles_x * a.tiles_y * B;
  if (tiles >= (1ull << 31)) return fail(RA_E_SHAPE, "ra_conv3x3_wide_f32: too many tiles");
  // fewer workgroups than CUs at 64 channels each: half slices
  if (tiles * ceil_div(Cout, convw::NS) < 256)
    hipLaunchKernelGGL(convw::conv3x3_wide<32>, dim3((unsigned)tiles, ceil_div(Cout, 32)), dim3(256), 0, as_stream(stream), a);
  else
    hipLaunchKernelGGL(convw::conv3x3_wide<64>, dim3((unsigned)tiles, ceil_div(Cout, convw::NS)), dim3(256), 0, as_stream(stream), a);
  return launch_status("ra_conv3x3_wide_f32");
}

extern "C" int ra_fg_head_f32(const float *logits, size_t npix, int nsc, int no, int quantise, float *y_out, float *d_out,
                              const float *x, int D, float *packed, int Cp, float *canvas_plane, void *stream) {
  if (!logits || !y_out || npix == 0 || (no && !d_out)) return fail(RA_E_INVALID, "ra_fg_head_f32: bad argument");
  if (nsc < 1 || nsc > 16 || (no != 0 && no != 8)) return fail(RA_E_SHAPE, "ra_fg_head_f32: nsc %d (1 .. 16), no %d (0 | 8)", nsc, no);
  if (packed && (!x || D <= 0 || Cp % 4 || Cp < D + 1 + no + nsc))
    return fail(RA_E_SHAPE, "ra_fg_head_f32: packed image of %d channels for D %d + 1 + %d + %d", Cp, D, no, nsc);
  convw::HeadArgs a;
  a.logits = logits, a.y_out = y_out, a.d_out = d_out, a.x = x, a.packed = packed, a.canvas = packed ? canvas_plane : nullptr;
  a.npix = npix, a.nsc = nsc, a.no = no, a.quant = quantise ? 1 : 0, a.D = D, a.Cp = Cp;
  hipLaunchKernelGGL(convw::fg_head, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, as_stream(stream), a);
  return launch_status("ra_fg_head_f32");
}
