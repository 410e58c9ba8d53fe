// K27 — PNG output on the device: the deflate stage of utils/png's writers, for a batch of images that are already in device
// memory.  The stream format is fixed in include/recattend.h (ra_png_deflate_*): one SEGMENT per scanline (a filter byte 0 and
// the row's bytes, n = 1 + W * bpp), every segment a fixed-Huffman block of the greedy run code at distance d = bpp followed
// by an empty stored block, so that segments end on byte boundaries, are produced independently and are concatenated.
//
//   encode    one workgroup of 256 threads per (row, image).  The row is staged into LDS with coalesced loads (16-byte loads
//             where the source allows, the colour swap B,G,R -> R,G,B and the float quantisation done in the load).  Thread t
//             then owns the K consecutive bytes [tK, tK + K) of the segment, K a multiple of 4 with K / 4 odd (the lanes of a
//             half-wave fall on 32 different LDS banks).  A token of the run code is decided by the maximal stretch of
//             positions with b[i] == b[i-d] it lies in: per stretch of R positions R / 258 matches of 258, then one match of
//             R % 258 if that is >= 3, else R % 258 literals (the closed form of the greedy rule).  So
//               walk 1   the first and last position of the chunk where b[i] != b[i-d], and the chunk's Adler sums;
//               2 scans  a forward max and a backward min over the threads give every chunk the start of the stretch that
//                        enters it and the end of the stretch that leaves it;
//               walk 2   the bits of the tokens that START in the chunk (a closed form per position), 1 scan -> bit offsets;
//               walk 3   the same walk, the bits OR-ed into an LDS buffer (cleared first), 64-bit accumulator per thread;
//             and the finished segment leaves with 16-byte stores into its worst-case slot of the workspace, with a record
//             (bytes, Adler A, Adler B) beside it.
//   scan      one workgroup per image: the exclusive prefix of the segment sizes (-> each segment's place in the stream), the
//             stream's size and its Adler-32 from the per-segment (A, B, n) — B = sum_k B_k + n * sum_k (Apre_k - 1), the
//             prefix of (A_k - 1) being a second scan of the same shape.
//   compact   one wave per segment copies it from its slot to its final place (dword stores to the aligned middle, a funnel
//             shift from the 16-byte-aligned slot); the workgroup of an image's first rows also writes 78 01, the final block
//             03 00, the Adler-32 and offsets[image] = the sum of the sizes of the images before it.
// Three plain launches on the caller's stream; no workgroup waits for another, every loop is bounded by n, H or N.
//
// Size bound.  A literal takes 8 or 9 bits, so at most 9 per byte.  A match of L >= 3 bytes takes at most 8 (length code) + 5
// (extra) + 5 (distance code, d = 1 and d = 3 have no extra bits) = 18 <= 9 L bits.  So the tokens of n bytes take <= 9 n bits,
// the block header 3, end-of-block 7, the stored block's header 3: 3 + 9n + 7 + 3 bits, padded to a byte, + 4 bytes LEN/NLEN
//   <= ceil((9n + 13) / 8) + 4 <= ceil(9n / 8) + 2 + 4 < ceil(9n / 8) + 7 bytes.  A stream: 2 + H segments + 2 + 4.
#include <cstdint>
#include <cstring>
#include <vector>

#include "ra_common.h"

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

// a match of length len (3 .. 258) at distance d (1 or 3): length code, its extra bits, the 5-bit distance code (0 or 2)
__host__ __device__ inline unsigned match_token(int len, int d, int *nb) {
  int sym, extra = 0, xb = 0;
  if (len <= 10) {
    sym = 257 + (len - 3);
  } else if (len == 258) {
    sym = 285;
  } else {
    const int l = len - 3;                   // 8 .. 254
    xb = 29 - __builtin_clz((unsigned)l);    // floor(log2 l) - 2: 1 .. 5 extra bits
    sym = 261 + 4 * xb + ((l >> xb) & 3);
    extra = l & ((1 << xb) - 1);
  }
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

__host__ __device__ inline size_t segment_bound(size_t n) { return (9 * n + 7) / 8 + 7; }
// a segment's slot in the workspace: the bound, 4 bytes the compaction's funnel shift may read beyond it, whole 16-byte stores
inline size_t slot_bytes(size_t n) { return (segment_bound(n) + 4 + 15) / 16 * 16; }

struct Record {
  unsigned bytes, a, b, offset;  // the segment's size, its Adler sums from (1, 0), its place behind the stream's 78 01
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

// ---- the token walk over the chunk [lo, hi) of a segment b[0 .. n): s = the start of the stretch that enters the chunk (the
// position behind the last one before lo with b[i] != b[i-d]; positions below d count as such), e_in = the first position
// >= hi with b[i] != b[i-d], or n.  tok(value, bits) receives, in order, every token that STARTS in the chunk.
template <class Tok>
__host__ __device__ __forceinline__ void walk(const unsigned char *b, int lo, int hi, int d, int s, int e_in, Tok &&tok) {
  int i = lo, nb;
  while (i < hi) {
    if (i < d || b[i] != b[i - d]) {
      const unsigned t = literal_token(b[i], &nb);
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
          const unsigned t = match_token(258, d, &nb);
          tok(t, nb);
        }
      } else if (r >= 3) {
        if (off == full) {
          const unsigned t = match_token(r, d, &nb);
          tok(t, nb);
        }
      } else {
        const unsigned t = literal_token(b[p], &nb);
        tok(t, nb);
      }
    }
    i = j;  // j < hi: b[j] differs from b[j-d] and starts a new stretch behind it
  }
}

// Workgroup (row, image).  Dynamic LDS: [0, row_bytes) the staged segment, then out_words dwords of bits, then 4 scan words.
template <int KIND, bool VEC>
__global__ __launch_bounds__(kThreads) void encode_kernel(const void *src, int M, int H, int W, const int *plane, int n, int K,
                                                           unsigned row_bytes, unsigned out_words, unsigned char *slots,
                                                           size_t slot, Record *rec) {
  extern __shared__ u32x4 dyn[];
  unsigned char *sh_raw = reinterpret_cast<unsigned char *>(dyn);
  unsigned *sh_out = reinterpret_cast<unsigned *>(sh_raw + row_bytes);
  unsigned *sh_scan = sh_out + out_words;
  const int tid = threadIdx.x, r = blockIdx.x, img = blockIdx.y;
  constexpr int d = KIND == RA_PNG_BGR8 ? 3 : 1;
  constexpr size_t px = KIND == RA_PNG_F32 ? 4 : (KIND == RA_PNG_BGR8 ? 3 : 1);  // source bytes per pixel

  int m = plane ? plane[img] : img;
  m = m < 0 ? 0 : (m >= M ? M - 1 : m);  // an index outside the source gives wrong pixels, never an access outside it
  const unsigned char *row = static_cast<const unsigned char *>(src) + ((size_t)m * H + r) * (size_t)W * px;
  if (tid == 0) sh_raw[kRowPad - 1] = 0;  // the filter-type byte
  stage_row<KIND, VEC>(row, W, sh_raw + kRowPad);
  for (unsigned w = tid; w < out_words; w += kThreads) sh_out[w] = 0u;  // bits are OR-ed in: LDS holds anything at entry
  __syncthreads();

  const unsigned char *b = sh_raw + (kRowPad - 1);
  const int lo = tid * K < n ? tid * K : n, hi = lo + K < n ? lo + K : n;
  // walk 1: 1 + the last / the first position of the chunk whose byte differs from the one d before it, and the Adler sums
  unsigned last1 = 0u, first = 0xffffffffu, s1 = 0u, s2 = 0u;
  for (int i = lo; i < hi; ++i) {
    const unsigned v = b[i];
    s1 += v;
    s2 += (unsigned)(n - i) * v;  // < 2^15 * 2^8 * K: a chunk is far below 2^9 bytes
    if (i < d || v != b[i - d]) {
      last1 = (unsigned)i + 1u;
      if (first == 0xffffffffu) first = (unsigned)i;
    }
  }
  const int s_in = (int)block_scan_excl<OpMax, false>(last1, sh_scan, nullptr);
  const unsigned e_scan = block_scan_excl<OpMin, true>(first, sh_scan, nullptr);
  const int e_in = e_scan < (unsigned)n ? (int)e_scan : n;
  unsigned sum1, sum2;
  block_scan_excl<OpAdd, false>(s1 % kAdler, sh_scan, &sum1);
  block_scan_excl<OpAdd, false>(s2 % kAdler, sh_scan, &sum2);

  // walk 2: the bits of the chunk's tokens
  unsigned bits = 0u;
  walk(b, lo, hi, d, s_in, e_in, [&](unsigned, int nb) { bits += (unsigned)nb; });
  unsigned tok_bits;
  const unsigned at = 3u + block_scan_excl<OpAdd, false>(bits, sh_scan, &tok_bits);  // behind BFINAL = 0, BTYPE = 01

  // walk 3: the tokens themselves, 64 bits gathered per thread and OR-ed in a dword at a time
  {
    unsigned w = at >> 5;
    int fill = (int)(at & 31u);
    unsigned long long acc = 0ull;
    walk(b, lo, hi, d, s_in, e_in, [&](unsigned t, int nb) {
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
  if (tid == 0) atomicOr(&sh_out[0], 2u);  // BFINAL = 0, BTYPE = 01 (bits 0, 1, 0)
  __syncthreads();
  // end-of-block (7 zero bits), the stored block's header (3 zero bits), zero bits to the byte boundary, 00 00 FF FF
  const unsigned body = (3u + tok_bits + 10u + 7u) >> 3, bytes = body + 4u;
  if (tid == 0) {
    unsigned char *o = reinterpret_cast<unsigned char *>(sh_out);
    o[body + 2] = 0xff;
    o[body + 3] = 0xff;
    Record q;
    q.bytes = bytes, q.a = (1u + sum1) % kAdler, q.b = ((unsigned)n + sum2) % kAdler, q.offset = 0u;
    rec[(size_t)img * H + r] = q;
  }
  __syncthreads();
  u32x4 *dst = reinterpret_cast<u32x4 *>(slots + ((size_t)img * H + r) * slot);
  for (unsigned v = tid; v < (bytes + 15u) / 16u; v += kThreads) dst[v] = reinterpret_cast<const u32x4 *>(sh_out)[v];
}

// Workgroup = image: every segment's place in its stream, the stream's size and Adler-32.
__global__ __launch_bounds__(kThreads) void scan_kernel(Record *rec, int H, int n, int *sizes, unsigned *adler) {
  __shared__ unsigned sh_scan[4];
  const int tid = threadIdx.x, img = blockIdx.x;
  Record *q = rec + (size_t)img * H;
  unsigned at = 0u, apre = 0u, bsum = 0u;  // bytes and sum of (A_k - 1) mod 65521 before this trip; this thread's part of B
  for (int r0 = 0; r0 < H; r0 += kThreads) {
    const int r = r0 + tid;
    const bool live = r < H;
    const unsigned nb = live ? q[r].bytes : 0u, a1 = live ? q[r].a + kAdler - 1u : 0u, bk = live ? q[r].b : 0u;
    unsigned tb, ta;
    const unsigned pb = block_scan_excl<OpAdd, false>(nb, sh_scan, &tb);
    const unsigned pa = block_scan_excl<OpAdd, false>(a1 % kAdler, sh_scan, &ta);
    if (live) {
      q[r].offset = at + pb;
      bsum = (bsum + bk + (unsigned)n % kAdler * ((apre + pa) % kAdler) % kAdler) % kAdler;
    }
    at += tb;
    apre = (apre + ta) % kAdler;
  }
  unsigned B;
  block_scan_excl<OpAdd, false>(bsum, sh_scan, &B);
  if (tid == 0) {
    sizes[img] = (int)(2u + at + 2u + 4u);
    adler[img] = (B % kAdler) << 16 | (apre + 1u) % kAdler;
  }
}

// Workgroup (group of kCompactRows rows, image); a wave copies one segment at a time.
__global__ __launch_bounds__(kThreads) void compact_kernel(const unsigned char *slots, size_t slot, const Record *rec, int H,
                                                            const int *sizes, const unsigned *adler, unsigned char *out,
                                                            unsigned long long *offsets) {
  __shared__ unsigned sh_scan[4];
  __shared__ unsigned long long sh_hi;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, img = blockIdx.y;
  // the stream's place: the sizes of the images before it (each below 2^31: low and high halves are summed apart)
  unsigned lo32 = 0u, hi32 = 0u;
  for (int j = tid; j < img; j += kThreads) {
    const unsigned v = (unsigned)sizes[j];
    lo32 += v & 0xffffu;
    hi32 += v >> 16;
  }
  unsigned tl, th;
  block_scan_excl<OpAdd, false>(lo32, sh_scan, &tl);
  block_scan_excl<OpAdd, false>(hi32, sh_scan, &th);
  if (tid == 0) sh_hi = ((unsigned long long)th << 16) + tl;
  __syncthreads();
  const unsigned long long base = sh_hi;
  unsigned char *o = out + base;
  if (blockIdx.x == 0 && tid == 0) {
    const unsigned size = (unsigned)sizes[img], ad = adler[img];
    offsets[img] = base;
    o[0] = 0x78, o[1] = 0x01;
    unsigned char *t = o + size - 6;
    t[0] = 0x03, t[1] = 0x00;  // BFINAL = 1, BTYPE = 01, end-of-block
    t[2] = (unsigned char)(ad >> 24), t[3] = (unsigned char)(ad >> 16), t[4] = (unsigned char)(ad >> 8), t[5] = (unsigned char)ad;
  }
  for (int k = 0; k < kRowsPerWave; ++k) {
    const int r = blockIdx.x * kCompactRows + wave * kRowsPerWave + k;
    if (r >= H) break;
    const Record q = rec[(size_t)img * H + r];
    const unsigned char *s = slots + ((size_t)img * H + r) * slot;
    unsigned char *dst = o + 2 + q.offset;
    unsigned head = (unsigned)(4u - (unsigned)(reinterpret_cast<uintptr_t>(dst) & 3u)) & 3u;
    head = head < q.bytes ? head : q.bytes;
    if ((unsigned)lane < head) dst[lane] = s[lane];
    const unsigned nd = (q.bytes - head) / 4u;
    const unsigned *s4 = reinterpret_cast<const unsigned *>(s);
    unsigned *d4 = reinterpret_cast<unsigned *>(dst + head);
    for (unsigned w = lane; w < nd; w += 64u) {  // s4[w + 1] lies inside the slot: it is 4 bytes longer than the bound
      const unsigned long long two = (unsigned long long)s4[w + 1] << 32 | s4[w];
      d4[w] = (unsigned)(two >> (8u * head));
    }
    const unsigned done = head + 4u * nd, tail = q.bytes - done;
    if ((unsigned)lane < tail) dst[done + lane] = s[done + lane];
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
struct Geometry {
  int d, bpp;        // match distance = file bytes per pixel
  size_t n, stream;  // segment bytes, the bound of a stream
};

// every check that does not depend on where the data lives; 0 or the refusal
int check(const char *who, const void *src, int kind, int M, int N, int H, int W, const void *out, size_t out_bytes,
          const void *sizes, const void *offsets, const void *adler, Geometry *g) {
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
  g->stream = 8 + (size_t)H * segment_bound(g->n);
  const size_t px = kind == RA_PNG_F32 ? 4 : g->bpp;
  if (g->stream >= (1ull << 31) || (size_t)H * W * px >= (1ull << 31))
    return fail(RA_E_SHAPE, "%s: H=%d W=%d: an image of %zu source bytes, a stream of up to %zu (both below 2^31)", who, H, W,
                (size_t)H * W * px, g->stream);
  if (out_bytes < (size_t)N * g->stream)
    return fail(RA_E_WORKSPACE, "%s: out_bytes=%zu, %d streams of up to %zu bytes need %zu", who, out_bytes, N, g->stream,
                (size_t)N * g->stream);
  return 0;
}

inline size_t records_bytes(int N, int H) { return ((size_t)N * H * sizeof(Record) + 15) / 16 * 16; }

template <int KIND>
void launch_encode(bool vec, dim3 grid, size_t lds, hipStream_t st, const void *src, int M, int H, int W, const int *plane, int n,
                   int K, unsigned row_bytes, unsigned out_words, unsigned char *slots, size_t slot, Record *rec) {
  if (vec)
    hipLaunchKernelGGL((encode_kernel<KIND, true>), grid, dim3(kThreads), lds, st, src, M, H, W, plane, n, K, row_bytes, out_words,
                       slots, slot, rec);
  else
    hipLaunchKernelGGL((encode_kernel<KIND, false>), grid, dim3(kThreads), lds, st, src, M, H, W, plane, n, K, row_bytes, out_words,
                       slots, slot, rec);
}

// the sequential bit writer of the host encoder
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

using namespace ra;

extern "C" int ra_png_deflate_bound(int N, int H, int W, int bpp, unsigned long long *stream_bytes,
                                    unsigned long long *workspace_bytes) {
  if (!stream_bytes || !workspace_bytes) return fail(RA_E_INVALID, "ra_png_deflate_bound: stream_bytes or workspace_bytes is NULL");
  if (bpp != 1 && bpp != 3) return fail(RA_E_SHAPE, "ra_png_deflate_bound: bpp=%d (1 = grey, 3 = RGB)", bpp);
  if (N < 1 || N > RA_PNG_MAX_IMAGES) return fail(RA_E_SHAPE, "ra_png_deflate_bound: N=%d (1 <= N <= %d)", N, RA_PNG_MAX_IMAGES);
  if (H < 1) return fail(RA_E_SHAPE, "ra_png_deflate_bound: H=%d (H >= 1)", H);
  if (W < 1) return fail(RA_E_SHAPE, "ra_png_deflate_bound: W=%d (W >= 1)", W);
  const size_t n = 1 + (size_t)W * bpp;
  if (n > RA_PNG_MAX_ROW_BYTES)
    return fail(RA_E_SHAPE, "ra_png_deflate_bound: W=%d gives scanlines of %zu bytes (at most %d)", W, n, RA_PNG_MAX_ROW_BYTES);
  const size_t stream = 8 + (size_t)H * png::segment_bound(n);
  if (stream >= (1ull << 31))
    return fail(RA_E_SHAPE, "ra_png_deflate_bound: H=%d W=%d: a stream of up to %zu bytes (below 2^31)", H, W, stream);
  *stream_bytes = stream;
  *workspace_bytes = png::records_bytes(N, H) + (size_t)N * H * png::slot_bytes(n);
  return 0;
}

extern "C" int ra_png_deflate_u8(const void *src, int kind, int M, int N, int H, int W, const int *plane, unsigned char *out,
                                 size_t out_bytes, int *sizes, unsigned long long *offsets, unsigned int *adler, void *ws,
                                 size_t ws_bytes, void *stream) {
  png::Geometry g;
  if (const int rc = png::check("ra_png_deflate_u8", src, kind, M, N, H, W, out, out_bytes, sizes, offsets, adler, &g)) return rc;
  if (!plane && N > M) return fail(RA_E_SHAPE, "ra_png_deflate_u8: N=%d images of a source of M=%d without a plane list", N, M);
  const size_t slot = png::slot_bytes(g.n), need = png::records_bytes(N, H) + (size_t)N * H * slot;
  if (!ws || ws_bytes < need || (reinterpret_cast<uintptr_t>(ws) & 15))
    return fail(RA_E_WORKSPACE, "ra_png_deflate_u8: ws=%p ws_bytes=%zu, %zu bytes at a 16-byte boundary are needed", ws, ws_bytes, need);
  png::Record *rec = static_cast<png::Record *>(ws);
  unsigned char *slots = static_cast<unsigned char *>(ws) + png::records_bytes(N, H);
  // a thread's chunk: K bytes, K / 4 odd, 256 K >= n
  const int n = (int)g.n;
  int k4 = ceil_div(ceil_div(n, png::kThreads), 4);
  k4 |= 1;
  const int K = 4 * k4;
  const unsigned row_bytes = (unsigned)round_up(png::kRowPad + n, 16);
  const unsigned out_words = (unsigned)(slot / 4) + 4u;
  const size_t lds = row_bytes + (size_t)out_words * 4 + 16;  // at most 16 + 24576 + 27680 + 16 + 16 bytes: below 64 KiB
  const uintptr_t a = reinterpret_cast<uintptr_t>(src);
  const bool vec = (a & 15) == 0 && (kind == RA_PNG_F32 ? W % 4 == 0 : W % 16 == 0);
  const dim3 grid(H, N);
  hipStream_t st = as_stream(stream);
  if (kind == RA_PNG_GRAY8)
    png::launch_encode<RA_PNG_GRAY8>(vec, grid, lds, st, src, M, H, W, plane, n, K, row_bytes, out_words, slots, slot, rec);
  else if (kind == RA_PNG_BGR8)
    png::launch_encode<RA_PNG_BGR8>(vec, grid, lds, st, src, M, H, W, plane, n, K, row_bytes, out_words, slots, slot, rec);
  else
    png::launch_encode<RA_PNG_F32>(vec, grid, lds, st, src, M, H, W, plane, n, K, row_bytes, out_words, slots, slot, rec);
  if (const int rc = launch_status("ra_png_deflate_u8 (encode)")) return rc;
  hipLaunchKernelGGL(png::scan_kernel, dim3(N), dim3(png::kThreads), 0, st, rec, H, n, sizes, adler);
  if (const int rc = launch_status("ra_png_deflate_u8 (scan)")) return rc;
  hipLaunchKernelGGL(png::compact_kernel, dim3(ceil_div(H, png::kCompactRows), N), dim3(png::kThreads), 0, st, slots, slot, rec, H,
                     sizes, adler, out, offsets);
  return launch_status("ra_png_deflate_u8 (compact)");
}

// HOST code, no GPU call: the rule as it is stated, one byte after the other.
extern "C" int ra_png_deflate_host(const void *src, int kind, int M, int N, int H, int W, const int *plane, unsigned char *out,
                                   size_t out_bytes, int *sizes, unsigned long long *offsets, unsigned int *adler, void *ws,
                                   size_t ws_bytes) {
  (void)ws, (void)ws_bytes;  // the sequential form needs none
  png::Geometry g;
  if (const int rc = png::check("ra_png_deflate_host", src, kind, M, N, H, W, out, out_bytes, sizes, offsets, adler, &g)) return rc;
  if (!plane && N > M) return fail(RA_E_SHAPE, "ra_png_deflate_host: N=%d images of a source of M=%d without a plane list", N, M);
  for (int i = 0; plane && i < N; ++i)
    if (plane[i] < 0 || plane[i] >= M) return fail(RA_E_SHAPE, "ra_png_deflate_host: plane[%d]=%d (0 <= index < M=%d)", i, plane[i], M);
  const int n = (int)g.n, d = g.d;
  std::vector<unsigned char> seg(g.n);
  size_t at = 0;
  for (int i = 0; i < N; ++i) {
    const size_t m = plane ? plane[i] : i;
    png::BitWriter bw{out + at};
    bw.byte(0x78), bw.byte(0x01);
    unsigned A = 1u, B = 0u;
    for (int r = 0; r < H; ++r) {
      seg[0] = 0;
      const size_t first = (m * H + r) * (size_t)W;
      if (kind == RA_PNG_GRAY8) {
        memcpy(&seg[1], static_cast<const unsigned char *>(src) + first, W);
      } else if (kind == RA_PNG_BGR8) {
        const unsigned char *s = static_cast<const unsigned char *>(src) + 3 * first;
        for (int p = 0; p < W; ++p) seg[1 + 3 * p] = s[3 * p + 2], seg[2 + 3 * p] = s[3 * p + 1], seg[3 + 3 * p] = s[3 * p];
      } else {
        const float *s = static_cast<const float *>(src) + first;
        for (int p = 0; p < W; ++p) seg[1 + p] = (unsigned char)((unsigned)(int)(s[p] * 255.0f) & 255u);
      }
      for (int k = 0; k < n; ++k) {  // a segment is below zlib's 5552 bytes only by luck: reduce every byte
        A = (A + seg[k]) % png::kAdler;
        B = (B + A) % png::kAdler;
      }
      bw.put(2u, 3);  // BFINAL = 0, BTYPE = 01
      int nb;
      for (int k = 0; k < n;) {
        int L = 0;
        if (k >= d)
          while (L < 258 && k + L < n && seg[k + L] == seg[k + L - d]) ++L;
        if (L >= 3) {
          const unsigned t = png::match_token(L, d, &nb);
          bw.put(t, nb);
          k += L;
        } else {
          const unsigned t = png::literal_token(seg[k], &nb);
          bw.put(t, nb);
          ++k;
        }
      }
      bw.put(0u, 7);  // end-of-block
      bw.put(0u, 3);  // an empty stored block: BFINAL = 0, BTYPE = 00
      bw.align();
      bw.byte(0x00), bw.byte(0x00), bw.byte(0xff), bw.byte(0xff);
    }
    bw.byte(0x03), bw.byte(0x00);
    bw.byte(B >> 8), bw.byte(B & 255u), bw.byte(A >> 8), bw.byte(A & 255u);
    const size_t bytes = bw.bit >> 3;
    sizes[i] = (int)bytes;
    offsets[i] = at;
    adler[i] = B << 16 | A;
    at += bytes;
  }
  return 0;
}
