// The parts the two stream formats of the device PNG encoder share (ra_png.hip: K27, the fixed-Huffman segments; ra_png_dyn.hip:
// K28, one dynamic-Huffman block per image): the length symbols of RFC 1951, the workgroup scans, the row staging, the stretch
// analysis of a thread's chunk, the token walk (the bits of a token come from a Coder), the row scan, the argument checks and the
// sequential bit writer of the host entries.  One copy of each.
#pragma once
#include <cstdint>
#include <cstring>

#include "ra_common.h"
#include "ra_ragged.h"

namespace ra {
namespace png {

constexpr int kThreads = 256;
constexpr unsigned kAdler = 65521u;
constexpr int kRowPad = 16;  // segment byte i waits at LDS byte kRowPad - 1 + i: the row's bytes start 16-byte aligned
constexpr int kRowsPerWave = 4, kCompactRows = kRowsPerWave * (kThreads / kWave);

// ---- the code tables of RFC 1951 3.2.5 / 3.2.6 as closed forms; a token is returned LSB-first, as it is packed -------------
__host__ __device__ inline unsigned rev_bits(unsigned v, int nb) { return __builtin_bitreverse32(v) >> (32 - nb); }

__host__ __device__ inline unsigned literal_token(unsigned v, int *nb) {
  if (v < 144u) {
    *nb = 8;
    return rev_bits(0x30u + v, 8);
  }
  *nb = 9;
  return rev_bits(0x190u + (v - 144u), 9);
}

// the length symbol (257 .. 285) of a match of len (3 .. 258) bytes, the number of its extra bits and their value
__host__ __device__ inline int length_symbol(int len, int *xb, int *extra) {
  *xb = 0, *extra = 0;
  if (len <= 10) return 257 + (len - 3);
  if (len == 258) return 285;
  const int l = len - 3;                    // 8 .. 254
  *xb = 29 - __builtin_clz((unsigned)l);    // floor(log2 l) - 2: 1 .. 5 extra bits
  *extra = l & ((1 << *xb) - 1);
  return 261 + 4 * *xb + ((l >> *xb) & 3);
}

// a match of length len (3 .. 258) at distance d (1 or 3): length code, its extra bits, the 5-bit distance code (0 or 2)
__host__ __device__ inline unsigned match_token(int len, int d, int *nb) {
  int xb, extra;
  const int sym = length_symbol(len, &xb, &extra);
  int cb;
  unsigned code;
  if (sym < 280) {
    cb = 7, code = rev_bits((unsigned)(sym - 256), 7);
  } else {
    cb = 8, code = rev_bits(0xC0u + (unsigned)(sym - 280), 8);
  }
  const unsigned dist = d == 1 ? 0u : 8u;  // distance code 0 (d = 1) or 2 (d = 3), 5 bits, reversed
  *nb = cb + xb + 5;
  return code | (unsigned)extra << cb | dist << (cb + xb);
}

// ---- where a token's bits come from --------------------------------------------------------------------------------------------
struct FixedCoder {  // RFC 1951 3.2.6
  __host__ __device__ unsigned literal(unsigned v, int *nb) const { return literal_token(v, nb); }
  __host__ __device__ unsigned match(int len, int d, int *nb) const { return match_token(len, d, nb); }
};
struct SymbolCoder {  // no bits: the literal / length symbol itself, for the histogram
  __host__ __device__ unsigned literal(unsigned v, int *nb) const {
    *nb = 0;
    return v;
  }
  __host__ __device__ unsigned match(int len, int, int *nb) const {
    int xb, extra;
    *nb = 0;
    return (unsigned)length_symbol(len, &xb, &extra);
  }
};
// an image's own code: tab[symbol] = the canonical code, bit-reversed, | its length << 16.  The one distance code in use has
// length 1 and the code 0, whatever the distance.
struct TableCoder {
  const unsigned *tab;
  __host__ __device__ unsigned literal(unsigned v, int *nb) const {
    const unsigned e = tab[v];
    *nb = (int)(e >> 16);
    return e & 0xffffu;
  }
  __host__ __device__ unsigned match(int len, int, int *nb) const {
    int xb, extra;
    const unsigned e = tab[length_symbol(len, &xb, &extra)];
    const int cb = (int)(e >> 16);
    *nb = cb + xb + 1;
    return (e & 0xffffu) | (unsigned)extra << cb;
  }
};

struct Record {
  unsigned bytes, a, b, offset;  // fixed: the segment's size, its Adler sums from (1, 0), its place behind the stream's 78 01
};                               // dynamic: `bytes` holds the row's BITS, `offset` is unused (the places are 64-bit, beside)

// ---- K28's per-image code table, as the code kernel leaves it in the workspace ------------------------------------------------
constexpr int kSymbols = 286, kTableSymbols = 288;
// 78 01 (16 bits), BFINAL + BTYPE (3), HLIT + HDIST + HCLEN (14), 19 code-length lengths (57), and at most 7 bits per entry of
// the length sequence of at most 286 + 3 entries (a symbol of <= 7 bits per entry, or 7 + 3 bits for >= 3, or 7 + 7 for >= 11)
constexpr int kHeaderBitsMax = 16 + 3 + 14 + 57 + 7 * 289;
constexpr int kHeaderWords = 72;  // ceil(2113 / 32) = 67, and words a funnel shift may read beyond them
struct Table {
  unsigned sym[kTableSymbols];           // the literal / length code (TableCoder)
  unsigned hdr_bits, eob, eob_bits, pad;  // the header's bits (78 01 included); the end-of-block code, LSB-first, and its length
  unsigned hdr[kHeaderWords];            // the header, packed LSB-first from bit 0 of hdr[0]
};

// ---- workgroup scans over 256 values: shuffles inside a wave, four wave totals through LDS ---------------------------------
struct OpAdd {
  __device__ static unsigned id() { return 0u; }
  __device__ static unsigned f(unsigned a, unsigned b) { return a + b; }
};
struct OpMax {
  __device__ static unsigned id() { return 0u; }
  __device__ static unsigned f(unsigned a, unsigned b) { return a > b ? a : b; }
};
struct OpMin {
  __device__ static unsigned id() { return 0xffffffffu; }
  __device__ static unsigned f(unsigned a, unsigned b) { return a < b ? a : b; }
};

// The EXCLUSIVE scan of v in thread order (REV: in reverse thread order, thread 255 first); *total: the reduction over all 256.
// sh: 4 words, free to be reused after the call (it ends in a barrier).
template <class Op, bool REV>
__device__ __forceinline__ unsigned block_scan_excl(unsigned v, unsigned *sh, unsigned *total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int pos = REV ? 63 - lane : lane;  // the lane's place in scan order
  unsigned inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned u = REV ? __shfl_down(inc, o) : __shfl_up(inc, o);
    if (pos >= o) inc = Op::f(u, inc);
  }
  unsigned exc = REV ? __shfl_down(inc, 1) : __shfl_up(inc, 1);
  if (pos == 0) exc = Op::id();
  if (pos == 63) sh[wave] = inc;
  __syncthreads();
  unsigned before = Op::id(), all = Op::id();
#pragma unroll
  for (int w = 0; w < kThreads / kWave; ++w) {
    const unsigned t = sh[w];
    all = Op::f(all, t);
    if (REV ? w > wave : w < wave) before = Op::f(before, t);
  }
  __syncthreads();
  if (total) *total = all;
  return Op::f(before, exc);
}

// a thread's chunk of a segment of n bytes: K bytes, K a multiple of 4 with K / 4 odd, 256 K >= n
__host__ __device__ inline int chunk_bytes(int n) {
  int k4 = ceil_div(ceil_div(n, kThreads), 4);
  k4 |= 1;
  return 4 * k4;
}

// ---- where the images of a call lie: the two sources the kernels are templated over (as ra_ragged.h's, with this encoder's
// plane list and per-image segment sizes) ----------------------------------------------------------------------------------------
//   Uniform   src holds M images of ONE size back to back; image i of the call is source image plane[i] (or i).  h, w, the
//             segment's bytes n and a thread's chunk K are kernel arguments.
//   Ragged    src holds M planes of `total` elements, all laid out by one table of B images; stream i = k * B + b is image b of
//             plane plane[k] (or k).  tab is indexed by blockIdx alone: ONE scalar load per workgroup; n and K are derived from
//             the image's w.  Records, slots and bit places keep a uniform stride of Hmax (Hmax + 1) rows per stream.
// A plane index outside the source is clamped: wrong pixels, never an access outside src.
struct Image {
  size_t first;  // the image's first element in src
  int h, w, n, K;
};

struct Uniform {
  static constexpr bool kRagged = false;
  int M, H, W, n, K;
  __device__ __forceinline__ int rows() const { return H; }  // the stride of a stream's records
  __device__ __forceinline__ Image dims(int) const { return Image{0, H, W, n, K}; }
  __device__ __forceinline__ Image at(int i, const int *plane) const {
    int m = plane ? plane[i] : i;
    m = m < 0 ? 0 : (m >= M ? M - 1 : m);
    return Image{(size_t)m * H * W, H, W, n, K};
  }
};

struct Ragged {
  static constexpr bool kRagged = true;
  const ra_image_geo *tab;
  int B, M, Hmax, bpp;
  size_t total;
  __device__ __forceinline__ int rows() const { return Hmax; }
  __device__ __forceinline__ Image dims(int i) const {
    const ra_image_geo g = tab[i % B];  // i = a blockIdx: a scalar load
    const int n = 1 + g.w * bpp;
    return Image{0, g.h, g.w, n, chunk_bytes(n)};
  }
  __device__ __forceinline__ Image at(int i, const int *plane) const {
    const int k = i / B;
    const ra_image_geo g = tab[i - k * B];
    int m = plane ? plane[k] : k;
    m = m < 0 ? 0 : (m >= M ? M - 1 : m);
    const int n = 1 + g.w * bpp;
    return Image{(size_t)m * total + (size_t)g.offset, g.h, g.w, n, chunk_bytes(n)};
  }
};

// ---- staging a row: file byte j of the row -> sh[j] (sh 16-byte aligned) ----------------------------------------------------
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned quantise(float v) { return (unsigned)(int)(v * 255.0f) & 255u; }  // (uint8)(v * 255.0f)

template <int KIND, bool VEC>
__device__ __forceinline__ void stage_row(const void *row, int W, unsigned char *sh) {
  const int tid = threadIdx.x;
  if (KIND == RA_PNG_GRAY8) {
    const unsigned char *s = static_cast<const unsigned char *>(row);
    if (VEC) {  // W % 16 == 0, the row 16-byte aligned
      for (int v = tid; v < W / 16; v += kThreads)
        reinterpret_cast<u32x4 *>(sh)[v] = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(s) + v);
    } else {
      for (int j = tid; j < W; j += kThreads) sh[j] = s[j];
    }
  } else if (KIND == RA_PNG_BGR8) {
    const unsigned char *s = static_cast<const unsigned char *>(row);
    if (VEC) {  // W % 16 == 0: 16 pixels = 48 bytes = three 16-byte loads per lane, swapped in registers
      for (int g = tid; g < W / 16; g += kThreads) {
        union {
          u32x4 v[3];
          unsigned char c[48];
        } in, out;
#pragma unroll
        for (int k = 0; k < 3; ++k) in.v[k] = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(s) + 3 * g + k);
#pragma unroll
        for (int p = 0; p < 16; ++p) {
          out.c[3 * p] = in.c[3 * p + 2];
          out.c[3 * p + 1] = in.c[3 * p + 1];
          out.c[3 * p + 2] = in.c[3 * p];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) reinterpret_cast<u32x4 *>(sh)[3 * g + k] = out.v[k];
      }
    } else {
      for (int j = tid; j < 3 * W; j += kThreads) {
        const int p = j / 3, c = j - 3 * p;
        sh[j] = s[3 * p + 2 - c];
      }
    }
  } else {
    const float *s = static_cast<const float *>(row);
    if (VEC) {  // W % 4 == 0, the row 16-byte aligned: four pixels per load, one dword to LDS
      for (int q = tid; q < W / 4; q += kThreads) {
        const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(s) + q);
        reinterpret_cast<unsigned *>(sh)[q] = quantise(v[0]) | quantise(v[1]) << 8 | quantise(v[2]) << 16 | quantise(v[3]) << 24;
      }
    } else {
      for (int j = tid; j < W; j += kThreads) sh[j] = (unsigned char)quantise(s[j]);
    }
  }
}

// Row r of image im, staged behind its filter-type byte: sh_raw[kRowPad - 1 ..) holds the segment.  No barrier.  RAGGED: the
// wide loads are this workgroup's decision, from the image's real address and width (its first byte 16-byte aligned and whole
// 16-byte groups per row, so every row is aligned); VEC is the launch's decision otherwise.
template <int KIND, bool VEC, bool RAGGED>
__device__ __forceinline__ void stage_segment(const void *src, const Image &im, int r, unsigned char *sh_raw) {
  constexpr size_t px = KIND == RA_PNG_F32 ? 4 : (KIND == RA_PNG_BGR8 ? 3 : 1);  // source bytes per pixel
  const unsigned char *first = static_cast<const unsigned char *>(src) + im.first * px;
  const unsigned char *row = first + (size_t)r * (size_t)im.w * px;
  if (threadIdx.x == 0) sh_raw[kRowPad - 1] = 0;  // the filter-type byte
  if (RAGGED) {
    if ((reinterpret_cast<uintptr_t>(first) & 15) == 0 && (size_t)im.w * px % 16 == 0)
      stage_row<KIND, true>(row, im.w, sh_raw + kRowPad);
    else
      stage_row<KIND, false>(row, im.w, sh_raw + kRowPad);
  } else {
    stage_row<KIND, VEC>(row, im.w, sh_raw + kRowPad);
  }
}

// Walk 1 over a thread's chunk [lo, hi) of the segment b[0 .. n) and the two scans behind it: *s_in = the start of the stretch
// that enters the chunk, *e_in = the end of the stretch that leaves it (what walk() takes); *s1, *s2: the chunk's Adler sums,
// s2 weighted with the number of bytes from each byte to the segment's end.  sh_scan: 4 words.
__device__ __forceinline__ void chunk_stretches(const unsigned char *b, int lo, int hi, int d, int n, unsigned *sh_scan, int *s_in,
                                                int *e_in, unsigned *s1, unsigned *s2) {
  // 1 + the last / the first position of the chunk whose byte differs from the one d before it
  unsigned last1 = 0u, first = 0xffffffffu, a1 = 0u, a2 = 0u;
  for (int i = lo; i < hi; ++i) {
    const unsigned v = b[i];
    a1 += v;
    a2 += (unsigned)(n - i) * v;  // < 2^15 * 2^8 * K: a chunk is far below 2^9 bytes
    if (i < d || v != b[i - d]) {
      last1 = (unsigned)i + 1u;
      if (first == 0xffffffffu) first = (unsigned)i;
    }
  }
  *s_in = (int)block_scan_excl<OpMax, false>(last1, sh_scan, nullptr);
  const unsigned e_scan = block_scan_excl<OpMin, true>(first, sh_scan, nullptr);
  *e_in = e_scan < (unsigned)n ? (int)e_scan : n;
  *s1 = a1, *s2 = a2;
}

// ---- the token walk over the chunk [lo, hi) of a segment b[0 .. n): s = the start of the stretch that enters the chunk (the
// position behind the last one before lo with b[i] != b[i-d]; positions below d count as such), e_in = the first position
// >= hi with b[i] != b[i-d], or n.  tok(value, bits) receives, in order, every token that STARTS in the chunk.
template <class Coder, class Tok>
__host__ __device__ __forceinline__ void walk(const Coder &code, const unsigned char *b, int lo, int hi, int d, int s, int e_in,
                                              Tok &&tok) {
  int i = lo, nb;
  while (i < hi) {
    if (i < d || b[i] != b[i - d]) {
      const unsigned t = code.literal(b[i], &nb);
      tok(t, nb);
      s = ++i;
      continue;
    }
    int j = i + 1;
    while (j < hi && b[j] == b[j - d]) ++j;
    const int e = j < hi ? j : e_in;
    const int R = e - s, full = R / 258 * 258, r = R - full;
    for (int p = i; p < j; ++p) {
      const int off = p - s;
      if (off < full) {
        if (off % 258 == 0) {
          const unsigned t = code.match(258, d, &nb);
          tok(t, nb);
        }
      } else if (r >= 3) {
        if (off == full) {
          const unsigned t = code.match(r, d, &nb);
          tok(t, nb);
        }
      } else {
        const unsigned t = code.literal(b[p], &nb);
        tok(t, nb);
      }
    }
    i = j;  // j < hi: b[j] differs from b[j-d] and starts a new stretch behind it
  }
}

// Walk 3: the tokens of the chunk OR-ed into the LDS bit buffer sh_out (cleared before) from bit `at` on, 64 bits gathered per
// thread and OR-ed in a dword at a time.  A token has at most 32 bits.
template <class Coder>
__device__ __forceinline__ void emit_chunk(const Coder &code, const unsigned char *b, int lo, int hi, int d, int s_in, int e_in,
                                           unsigned at, unsigned *sh_out) {
  unsigned w = at >> 5;
  int fill = (int)(at & 31u);
  unsigned long long acc = 0ull;
  walk(code, b, lo, hi, d, s_in, e_in, [&](unsigned t, int nb) {
    acc |= (unsigned long long)t << fill;
    fill += nb;
    if (fill >= 32) {
      atomicOr(&sh_out[w++], (unsigned)acc);
      acc >>= 32;
      fill -= 32;
    }
  });
  if (fill > 0 && acc) atomicOr(&sh_out[w], (unsigned)acc);
}

// Workgroup = image: every row's place in its stream, the stream's size and Adler-32.  Fixed format: byte places behind 78 01
// into rec[].offset.  DYN: rec[].bytes are BITS; 64-bit bit places from the stream's first byte on, behind the header's
// tab[img].hdr_bits, into start[img * (S + 1) + r], the end-of-block code's place into start[img * (S + 1) + H]; S = the
// stride of a stream's records (H; ragged: the tallest image's), H and n the image's own.
template <bool DYN, class GEO>
__global__ __launch_bounds__(kThreads) void scan_kernel(Record *rec, GEO geom, int *sizes, unsigned *adler, const Table *tab,
                                                         unsigned long long *start) {
  __shared__ unsigned sh_scan[4];
  const int tid = threadIdx.x, img = blockIdx.x;
  const Image im = geom.dims(img);
  const int H = im.h, n = im.n, S = geom.rows();
  Record *q = rec + (size_t)img * S;
  unsigned long long *st = DYN ? start + (size_t)img * (S + 1) : nullptr;
  // bytes (bits) before this trip: a trip adds below 2^8 * 2^19; the sum of (A_k - 1) mod 65521 before it; this thread's part of B
  unsigned long long at = DYN ? tab[img].hdr_bits : 0ull;
  unsigned apre = 0u, bsum = 0u;
  for (int r0 = 0; r0 < H; r0 += kThreads) {
    const int r = r0 + tid;
    const bool live = r < H;
    const unsigned nb = live ? q[r].bytes : 0u, a1 = live ? q[r].a + kAdler - 1u : 0u, bk = live ? q[r].b : 0u;
    unsigned tb, ta;
    const unsigned pb = block_scan_excl<OpAdd, false>(nb, sh_scan, &tb);
    const unsigned pa = block_scan_excl<OpAdd, false>(a1 % kAdler, sh_scan, &ta);
    if (live) {
      if (DYN)
        st[r] = at + pb;
      else
        q[r].offset = (unsigned)at + pb;
      bsum = (bsum + bk + (unsigned)n % kAdler * ((apre + pa) % kAdler) % kAdler) % kAdler;
    }
    at += tb;
    apre = (apre + ta) % kAdler;
  }
  unsigned B;
  block_scan_excl<OpAdd, false>(bsum, sh_scan, &B);
  if (tid == 0) {
    if (DYN) {
      st[H] = at;
      sizes[img] = (int)((at + tab[img].eob_bits + 7ull) / 8ull + 4ull);
    } else {
      sizes[img] = (int)(2u + (unsigned)at + 2u + 4u);
    }
    adler[img] = (B % kAdler) << 16 | (apre + 1u) % kAdler;
  }
}

// The place of stream img in `out`: the sizes of the images before it (each below 2^31: low and high halves are summed apart).
// sh_scan: 4 words, sh_hi: one 64-bit word.  Contains barriers.
__device__ __forceinline__ unsigned long long stream_base(const int *sizes, int img, unsigned *sh_scan, unsigned long long *sh_hi) {
  unsigned lo32 = 0u, hi32 = 0u;
  for (int j = threadIdx.x; j < img; j += kThreads) {
    const unsigned v = (unsigned)sizes[j];
    lo32 += v & 0xffffu;
    hi32 += v >> 16;
  }
  unsigned tl, th;
  block_scan_excl<OpAdd, false>(lo32, sh_scan, &tl);
  block_scan_excl<OpAdd, false>(hi32, sh_scan, &th);
  if (threadIdx.x == 0) *sh_hi = ((unsigned long long)th << 16) + tl;
  __syncthreads();
  return *sh_hi;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
__host__ __device__ inline size_t segment_bound(size_t n) { return (9 * n + 7) / 8 + 7; }
// K28: 15 bits per scanline byte (a literal <= 15; a match of L >= 3 bytes <= 15 + 5 + 1 <= 15 L), the header, an end-of-block
// code of <= 15 bits, the byte padding, the Adler-32: ceil((2113 + 15 n H + 15) / 8) + 4 <= 270 + ceil(15 n H / 8)
inline size_t dynamic_stream_bound(size_t n, size_t H) { return 270 + (15 * n * H + 7) / 8; }

struct Geometry {
  int d, bpp;        // match distance = file bytes per pixel
  size_t n, stream;  // segment bytes, the bound of a stream
};

// every check that does not depend on where the data lives; 0 or the refusal
inline int check(const char *who, bool dynamic, const void *src, int kind, int M, int N, int H, int W, const void *out,
                 size_t out_bytes, const void *sizes, const void *offsets, const void *adler, Geometry *g) {
  if (!src || !out || !sizes || !offsets || !adler) return fail(RA_E_INVALID, "%s: src, out, sizes, offsets or adler is NULL", who);
  if (kind != RA_PNG_GRAY8 && kind != RA_PNG_BGR8 && kind != RA_PNG_F32)
    return fail(RA_E_INVALID, "%s: kind %d (RA_PNG_GRAY8, RA_PNG_BGR8 or RA_PNG_F32)", who, kind);
  if (N < 1 || N > RA_PNG_MAX_IMAGES) return fail(RA_E_SHAPE, "%s: N=%d (1 <= N <= %d)", who, N, RA_PNG_MAX_IMAGES);
  if (M < 1) return fail(RA_E_SHAPE, "%s: M=%d (the source holds at least one image)", who, M);
  if (H < 1) return fail(RA_E_SHAPE, "%s: H=%d (H >= 1)", who, H);
  if (W < 1) return fail(RA_E_SHAPE, "%s: W=%d (W >= 1)", who, W);
  g->bpp = g->d = kind == RA_PNG_BGR8 ? 3 : 1;
  g->n = 1 + (size_t)W * g->bpp;
  if (g->n > RA_PNG_MAX_ROW_BYTES)
    return fail(RA_E_SHAPE, "%s: W=%d gives scanlines of %zu bytes (at most %d)", who, W, g->n, RA_PNG_MAX_ROW_BYTES);
  g->stream = dynamic ? dynamic_stream_bound(g->n, H) : 8 + (size_t)H * segment_bound(g->n);
  const size_t px = kind == RA_PNG_F32 ? 4 : g->bpp;
  if (g->stream >= (1ull << 31) || (size_t)H * W * px >= (1ull << 31))
    return fail(RA_E_SHAPE, "%s: H=%d W=%d: an image of %zu source bytes, a stream of up to %zu (both below 2^31)", who, H, W,
                (size_t)H * W * px, g->stream);
  if (out_bytes < (size_t)N * g->stream)
    return fail(RA_E_WORKSPACE, "%s: out_bytes=%zu, %d streams of up to %zu bytes need %zu", who, out_bytes, N, g->stream,
                (size_t)N * g->stream);
  return 0;
}

// the checks of the bound queries; 0 (and *n = the scanline's bytes) or the refusal
inline int check_bound(const char *who, int N, int H, int W, int bpp, const void *stream_bytes, const void *workspace_bytes,
                       size_t *n) {
  if (!stream_bytes || !workspace_bytes) return fail(RA_E_INVALID, "%s: stream_bytes or workspace_bytes is NULL", who);
  if (bpp != 1 && bpp != 3) return fail(RA_E_SHAPE, "%s: bpp=%d (1 = grey, 3 = RGB)", who, bpp);
  if (N < 1 || N > RA_PNG_MAX_IMAGES) return fail(RA_E_SHAPE, "%s: N=%d (1 <= N <= %d)", who, N, RA_PNG_MAX_IMAGES);
  if (H < 1) return fail(RA_E_SHAPE, "%s: H=%d (H >= 1)", who, H);
  if (W < 1) return fail(RA_E_SHAPE, "%s: W=%d (W >= 1)", who, W);
  *n = 1 + (size_t)W * bpp;
  if (*n > RA_PNG_MAX_ROW_BYTES)
    return fail(RA_E_SHAPE, "%s: W=%d gives scanlines of %zu bytes (at most %d)", who, W, *n, RA_PNG_MAX_ROW_BYTES);
  return 0;
}

// ---- a ragged call (ra_png_deflate*_ragged_*): what the table gives the host side --------------------------------------------
struct RaggedShape {
  int N, Hmax;   // streams of the call; the tallest image's rows: the row stride of every stream's records, slots and places
  size_t n_max;  // the widest image's scanline bytes: what slots and LDS are sized by
  size_t out;    // Np * the sum of the images' stream bounds
};

// The per-image limits of the uniform entries, image by image; 0 (and *s filled) or RA_E_SHAPE with a message that names the
// image or the count.  px: source bytes per pixel (the bound queries know only bpp).
inline int ragged_shape(const char *who, bool dynamic, const ra_image_geo *geo, int B, int Np, int bpp, size_t px, RaggedShape *s) {
  if (B < 1 || Np < 1 || (long long)B * Np > RA_PNG_MAX_IMAGES)
    return fail(RA_E_SHAPE, "%s: B=%d images times Np=%d planes (1 <= N = Np * B <= %d)", who, B, Np, RA_PNG_MAX_IMAGES);
  s->N = B * Np, s->Hmax = 0, s->n_max = 0;
  size_t sum = 0;
  for (int b = 0; b < B; ++b) {
    const int h = geo[b].h, w = geo[b].w;
    if (h < 1 || w < 1) return fail(RA_E_SHAPE, "%s: image %d is %d x %d (h, w >= 1)", who, b, h, w);
    const size_t n = 1 + (size_t)w * bpp;
    if (n > RA_PNG_MAX_ROW_BYTES)
      return fail(RA_E_SHAPE, "%s: image %d: w=%d gives scanlines of %zu bytes (at most %d)", who, b, w, n, RA_PNG_MAX_ROW_BYTES);
    const size_t stream = dynamic ? dynamic_stream_bound(n, h) : 8 + (size_t)h * segment_bound(n);
    if (stream >= (1ull << 31) || (size_t)h * w * px >= (1ull << 31))
      return fail(RA_E_SHAPE, "%s: image %d is %d x %d: %zu source bytes, a stream of up to %zu (both below 2^31)", who, b, h, w,
                  (size_t)h * w * px, stream);
    s->Hmax = h > s->Hmax ? h : s->Hmax;
    s->n_max = n > s->n_max ? n : s->n_max;
    sum += stream;
  }
  s->out = (size_t)Np * sum;
  return 0;
}

// every check of a ragged entry that does not depend on where the data lives, in the order the header states; 0 or the refusal
inline int check_ragged(const char *who, bool dynamic, const void *src, int kind, int M, size_t total, const ra_image_geo *geo, int B,
                        const int *plane, int Np, const void *out, size_t out_bytes, const void *sizes, const void *offsets,
                        const void *adler, RaggedShape *s) {
  if (!src || !geo || !out || !sizes || !offsets || !adler)
    return fail(RA_E_INVALID, "%s: src, geo, out, sizes, offsets or adler is NULL", who);
  if (kind != RA_PNG_GRAY8 && kind != RA_PNG_BGR8 && kind != RA_PNG_F32)
    return fail(RA_E_INVALID, "%s: kind %d (RA_PNG_GRAY8, RA_PNG_BGR8 or RA_PNG_F32)", who, kind);
  if (M < 1) return fail(RA_E_SHAPE, "%s: M=%d (the source holds at least one plane)", who, M);
  const int bpp = kind == RA_PNG_BGR8 ? 3 : 1;
  if (B < 1 || Np < 1 || (long long)B * Np > RA_PNG_MAX_IMAGES)
    return fail(RA_E_SHAPE, "%s: B=%d images times Np=%d planes (1 <= N = Np * B <= %d)", who, B, Np, RA_PNG_MAX_IMAGES);
  if (!plane && Np > M) return fail(RA_E_SHAPE, "%s: Np=%d planes of a source of M=%d without a plane list", who, Np, M);
  if (const int rc = geo::check(who, geo, B, total, (1ll << 31) - 1, "h * w < 2^31")) return rc;
  if (const int rc = ragged_shape(who, dynamic, geo, B, Np, bpp, kind == RA_PNG_F32 ? 4 : bpp, s)) return rc;
  if (out_bytes < s->out)
    return fail(RA_E_WORKSPACE, "%s: out_bytes=%zu, %d streams need up to %zu (Np * the sum of the images' bounds)", who, out_bytes,
                s->N, s->out);
  return 0;
}

inline size_t records_bytes(int N, int H) { return ((size_t)N * H * sizeof(Record) + 15) / 16 * 16; }

// 16-byte loads: the source 16-byte aligned and whole 16-byte groups per row
inline bool vector_rows(const void *src, int kind, int W) {
  return (reinterpret_cast<uintptr_t>(src) & 15) == 0 && (kind == RA_PNG_F32 ? W % 4 == 0 : W % 16 == 0);
}

// scanline r of the image of width W whose first element is `base`, as the file holds it: the filter-type byte 0 and the row
// (host entries)
inline void host_scanline(const void *src, int kind, size_t base, int W, int r, unsigned char *seg) {
  seg[0] = 0;
  const size_t first = base + (size_t)r * (size_t)W;
  if (kind == RA_PNG_GRAY8) {
    memcpy(&seg[1], static_cast<const unsigned char *>(src) + first, W);
  } else if (kind == RA_PNG_BGR8) {
    const unsigned char *s = static_cast<const unsigned char *>(src) + 3 * first;
    for (int p = 0; p < W; ++p) seg[1 + 3 * p] = s[3 * p + 2], seg[2 + 3 * p] = s[3 * p + 1], seg[3 + 3 * p] = s[3 * p];
  } else {
    const float *s = static_cast<const float *>(src) + first;
    for (int p = 0; p < W; ++p) seg[1 + p] = (unsigned char)((unsigned)(int)(s[p] * 255.0f) & 255u);
  }
}

// the sequential bit writer of the host encoders
struct BitWriter {
  unsigned char *p;
  size_t bit = 0;
  void put(unsigned v, int nb) {
    for (int k = 0; k < nb; ++k, ++bit) {
      if ((bit & 7) == 0) p[bit >> 3] = 0;
      p[bit >> 3] |= (unsigned char)((v >> k & 1u) << (bit & 7));
    }
  }
  void align() {
    if (bit & 7) bit = (bit | 7) + 1;
  }
  void byte(unsigned v) {
    p[bit >> 3] = (unsigned char)v;
    bit += 8;
  }
};

}  // namespace png
}  // namespace ra
