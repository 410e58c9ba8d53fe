// K27 — PNG output on the device: the deflate stage of utils/png's writers, for a batch of images that are already in device
// memory.  The stream format is fixed in include/recattend.h (ra_png_deflate_*): one SEGMENT per scanline (a filter byte 0 and
// the row's bytes, n = 1 + W * bpp), every segment a fixed-Huffman block of the greedy run code at distance d = bpp followed
// by an empty stored block, so that segments end on byte boundaries, are produced independently and are concatenated.
// (The second format, one dynamic-Huffman block per image, is K28 in ra_png_dyn.hip; the parts both use are in ra_png_parts.h.)
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
// The kernels are templates over where the images lie (ra_png_parts.h: Uniform, one size per call, or Ragged, a batch of mixed
// sizes behind one ra_image_geo table — ra_png_deflate_ragged_u8): a ragged launch keeps a uniform stride of the tallest
// image's rows per stream, a workgroup beyond its own image's rows leaves before its first barrier, and n, K and the load width
// are the image's own.  The streams do not depend on the form.
//
// Size bound.  A literal takes 8 or 9 bits, so at most 9 per byte.  A match of L >= 3 bytes takes at most 8 (length code) + 5
// (extra) + 5 (distance code, d = 1 and d = 3 have no extra bits) = 18 <= 9 L bits.  So the tokens of n bytes take <= 9 n bits,
// the block header 3, end-of-block 7, the stored block's header 3: 3 + 9n + 7 + 3 bits, padded to a byte, + 4 bytes LEN/NLEN
//   <= ceil((9n + 13) / 8) + 4 <= ceil(9n / 8) + 2 + 4 < ceil(9n / 8) + 7 bytes.  A stream: 2 + H segments + 2 + 4.
#include <vector>

#include "ra_png_parts.h"

namespace ra {
namespace png {

// a segment's slot in the workspace: the bound, 4 bytes the compaction's funnel shift may read beyond it, whole 16-byte stores
inline size_t slot_bytes(size_t n) { return (segment_bound(n) + 4 + 15) / 16 * 16; }

// Workgroup (row, stream).  Dynamic LDS: [0, row_bytes) the staged segment, then out_words dwords of bits, then 4 scan words.
// GEO: Uniform or Ragged (ra_png_parts.h).  Ragged: the grid's x extent is the tallest image's rows and a workgroup beyond its
// own image's leaves before the first barrier; n and K are the image's own, the LDS offsets the launch's (the widest image's).
template <int KIND, bool VEC, class GEO>
__global__ __launch_bounds__(kThreads) void encode_kernel(const void *src, GEO geom, const int *plane, unsigned row_bytes,
                                                           unsigned out_words, unsigned char *slots, size_t slot, Record *rec) {
  extern __shared__ u32x4 dyn[];
  unsigned char *sh_raw = reinterpret_cast<unsigned char *>(dyn);
  unsigned *sh_out = reinterpret_cast<unsigned *>(sh_raw + row_bytes);
  unsigned *sh_scan = sh_out + out_words;
  const int tid = threadIdx.x, r = blockIdx.x, img = blockIdx.y;
  constexpr int d = KIND == RA_PNG_BGR8 ? 3 : 1;
  const Image im = geom.at(img, plane);
  if (GEO::kRagged && r >= im.h) return;
  const int n = im.n, K = im.K;

  stage_segment<KIND, VEC, GEO::kRagged>(src, im, r, sh_raw);
  for (unsigned w = tid; w < out_words; w += kThreads) sh_out[w] = 0u;  // bits are OR-ed in: LDS holds anything at entry
  __syncthreads();

  const unsigned char *b = sh_raw + (kRowPad - 1);
  const int lo = tid * K < n ? tid * K : n, hi = lo + K < n ? lo + K : n;
  // walk 1 and its two scans: the stretches that enter and leave the chunk, and the Adler sums
  int s_in, e_in;
  unsigned s1, s2;
  chunk_stretches(b, lo, hi, d, n, sh_scan, &s_in, &e_in, &s1, &s2);
  unsigned sum1, sum2;
  block_scan_excl<OpAdd, false>(s1 % kAdler, sh_scan, &sum1);
  block_scan_excl<OpAdd, false>(s2 % kAdler, sh_scan, &sum2);

  // walk 2: the bits of the chunk's tokens
  const FixedCoder code{};
  unsigned bits = 0u;
  walk(code, b, lo, hi, d, s_in, e_in, [&](unsigned, int nb) { bits += (unsigned)nb; });
  unsigned tok_bits;
  const unsigned at = 3u + block_scan_excl<OpAdd, false>(bits, sh_scan, &tok_bits);  // behind BFINAL = 0, BTYPE = 01

  // walk 3: the tokens themselves
  emit_chunk(code, b, lo, hi, d, s_in, e_in, at, sh_out);
  if (tid == 0) atomicOr(&sh_out[0], 2u);  // BFINAL = 0, BTYPE = 01 (bits 0, 1, 0)
  __syncthreads();
  // end-of-block (7 zero bits), the stored block's header (3 zero bits), zero bits to the byte boundary, 00 00 FF FF
  const unsigned body = (3u + tok_bits + 10u + 7u) >> 3, bytes = body + 4u;
  const size_t at_rec = (size_t)img * geom.rows() + r;
  if (tid == 0) {
    unsigned char *o = reinterpret_cast<unsigned char *>(sh_out);
    o[body + 2] = 0xff;
    o[body + 3] = 0xff;
    Record q;
    q.bytes = bytes, q.a = (1u + sum1) % kAdler, q.b = ((unsigned)n + sum2) % kAdler, q.offset = 0u;
    rec[at_rec] = q;
  }
  __syncthreads();
  u32x4 *dst = reinterpret_cast<u32x4 *>(slots + at_rec * slot);
  for (unsigned v = tid; v < (bytes + 15u) / 16u; v += kThreads) dst[v] = reinterpret_cast<const u32x4 *>(sh_out)[v];
}

// Workgroup (group of kCompactRows rows, stream); a wave copies one segment at a time.
template <class GEO>
__global__ __launch_bounds__(kThreads) void compact_kernel(const unsigned char *slots, size_t slot, const Record *rec, GEO geom,
                                                            const int *sizes, const unsigned *adler, unsigned char *out,
                                                            unsigned long long *offsets) {
  __shared__ unsigned sh_scan[4];
  __shared__ unsigned long long sh_hi;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, img = blockIdx.y;
  const int H = geom.dims(img).h, S = geom.rows();
  if (GEO::kRagged && blockIdx.x * kCompactRows >= H) return;  // nothing of this image here: before the first barrier
  const unsigned long long base = stream_base(sizes, img, sh_scan, &sh_hi);
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
    const Record q = rec[(size_t)img * S + r];
    const unsigned char *s = slots + ((size_t)img * S + r) * slot;
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

// The three launches of a call of N streams: `rows` scanlines per stream in the grid, segments of up to n_max bytes.
template <int KIND, class GEO>
int launch_chain(const char *who, bool vec, hipStream_t st, const void *src, const GEO &geom, int N, int rows, size_t n_max,
                 const int *plane, unsigned char *ws, unsigned char *out, int *sizes, unsigned long long *offsets, unsigned *adler) {
  const size_t slot = slot_bytes(n_max);
  Record *rec = reinterpret_cast<Record *>(ws);
  unsigned char *slots = ws + records_bytes(N, rows);
  const unsigned row_bytes = (unsigned)round_up(kRowPad + (int)n_max, 16);
  const unsigned out_words = (unsigned)(slot / 4) + 4u;
  const size_t lds = row_bytes + (size_t)out_words * 4 + 16;  // at most 16 + 24576 + 27680 + 16 + 16 bytes: below 64 KiB
  constexpr bool kWide = !GEO::kRagged;  // a ragged workgroup decides the load width itself: one instantiation
  const dim3 grid(rows, N), block(kThreads);
  if (vec)
    hipLaunchKernelGGL((encode_kernel<KIND, kWide, GEO>), grid, block, lds, st, src, geom, plane, row_bytes, out_words, slots, slot, rec);
  else
    hipLaunchKernelGGL((encode_kernel<KIND, false, GEO>), grid, block, lds, st, src, geom, plane, row_bytes, out_words, slots, slot, rec);
  if (const int rc = launch_status(who)) return rc;
  hipLaunchKernelGGL((scan_kernel<false, GEO>), dim3(N), block, 0, st, rec, geom, sizes, adler, static_cast<const Table *>(nullptr),
                     static_cast<unsigned long long *>(nullptr));
  if (const int rc = launch_status(who)) return rc;
  hipLaunchKernelGGL(compact_kernel<GEO>, dim3(ceil_div(rows, kCompactRows), N), block, 0, st, slots, slot, rec, geom, sizes, adler,
                     out, offsets);
  return launch_status(who);
}

template <class GEO>
int launch_kind(const char *who, int kind, bool vec, hipStream_t st, const void *src, const GEO &geom, int N, int rows, size_t n_max,
                const int *plane, unsigned char *ws, unsigned char *out, int *sizes, unsigned long long *offsets, unsigned *adler) {
  if (kind == RA_PNG_GRAY8)
    return launch_chain<RA_PNG_GRAY8>(who, vec, st, src, geom, N, rows, n_max, plane, ws, out, sizes, offsets, adler);
  if (kind == RA_PNG_BGR8)
    return launch_chain<RA_PNG_BGR8>(who, vec, st, src, geom, N, rows, n_max, plane, ws, out, sizes, offsets, adler);
  return launch_chain<RA_PNG_F32>(who, vec, st, src, geom, N, rows, n_max, plane, ws, out, sizes, offsets, adler);
}

// HOST code: the stream of the image of H x W whose first element is `base`, written at o; its bytes, *adler = its Adler-32
inline size_t host_stream(const void *src, int kind, size_t base, int H, int W, int d, unsigned char *seg, unsigned char *o,
                          unsigned *adler) {
  const int n = 1 + W * d;
  BitWriter bw{o};
  bw.byte(0x78), bw.byte(0x01);
  unsigned A = 1u, B = 0u;
  for (int r = 0; r < H; ++r) {
    host_scanline(src, kind, base, W, r, seg);
    for (int k = 0; k < n; ++k) {  // a segment is below zlib's 5552 bytes only by luck: reduce every byte
      A = (A + seg[k]) % kAdler;
      B = (B + A) % kAdler;
    }
    bw.put(2u, 3);  // BFINAL = 0, BTYPE = 01
    int nb;
    for (int k = 0; k < n;) {
      int L = 0;
      if (k >= d)
        while (L < 258 && k + L < n && seg[k + L] == seg[k + L - d]) ++L;
      if (L >= 3) {
        const unsigned t = match_token(L, d, &nb);
        bw.put(t, nb);
        k += L;
      } else {
        const unsigned t = literal_token(seg[k], &nb);
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
  *adler = B << 16 | A;
  return bw.bit >> 3;
}

}  // namespace png
}  // namespace ra

using namespace ra;

extern "C" int ra_png_deflate_bound(int N, int H, int W, int bpp, unsigned long long *stream_bytes,
                                    unsigned long long *workspace_bytes) {
  size_t n;
  if (const int rc = png::check_bound("ra_png_deflate_bound", N, H, W, bpp, stream_bytes, workspace_bytes, &n)) return rc;
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
  if (const int rc = png::check("ra_png_deflate_u8", false, src, kind, M, N, H, W, out, out_bytes, sizes, offsets, adler, &g)) return rc;
  if (!plane && N > M) return fail(RA_E_SHAPE, "ra_png_deflate_u8: N=%d images of a source of M=%d without a plane list", N, M);
  const size_t need = png::records_bytes(N, H) + (size_t)N * H * png::slot_bytes(g.n);
  if (!ws || ws_bytes < need || (reinterpret_cast<uintptr_t>(ws) & 15))
    return fail(RA_E_WORKSPACE, "ra_png_deflate_u8: ws=%p ws_bytes=%zu, %zu bytes at a 16-byte boundary are needed", ws, ws_bytes, need);
  const int n = (int)g.n;
  return png::launch_kind("ra_png_deflate_u8", kind, png::vector_rows(src, kind, W), as_stream(stream), src,
                          png::Uniform{M, H, W, n, png::chunk_bytes(n)}, N, H, g.n, plane, static_cast<unsigned char *>(ws), out, sizes,
                          offsets, adler);
}

extern "C" int ra_png_deflate_ragged_bound(const ra_image_geo *geo, int B, int Np, int bpp, unsigned long long *out_bytes,
                                           unsigned long long *workspace_bytes) {
  const char *who = "ra_png_deflate_ragged_bound";
  if (!geo || !out_bytes || !workspace_bytes) return fail(RA_E_INVALID, "%s: geo, out_bytes or workspace_bytes is NULL", who);
  if (bpp != 1 && bpp != 3) return fail(RA_E_SHAPE, "%s: bpp=%d (1 = grey, 3 = RGB)", who, bpp);
  png::RaggedShape s;
  if (const int rc = png::ragged_shape(who, false, geo, B, Np, bpp, bpp, &s)) return rc;
  *out_bytes = s.out;
  *workspace_bytes = png::records_bytes(s.N, s.Hmax) + (size_t)s.N * s.Hmax * png::slot_bytes(s.n_max);
  return 0;
}

extern "C" int ra_png_deflate_ragged_u8(const void *src, int kind, int M, size_t total, const ra_image_geo *geo,
                                        ra_image_geo *geo_dev, int B, const int *plane, int Np, unsigned char *out, size_t out_bytes,
                                        int *sizes, unsigned long long *offsets, unsigned int *adler, void *ws, size_t ws_bytes,
                                        void *stream) {
  const char *who = "ra_png_deflate_ragged_u8";
  if (!geo_dev) return fail(RA_E_INVALID, "%s: geo_dev is NULL", who);
  png::RaggedShape s;
  if (const int rc = png::check_ragged(who, false, src, kind, M, total, geo, B, plane, Np, out, out_bytes, sizes, offsets, adler, &s))
    return rc;
  const size_t need = png::records_bytes(s.N, s.Hmax) + (size_t)s.N * s.Hmax * png::slot_bytes(s.n_max);
  if (!ws || ws_bytes < need || (reinterpret_cast<uintptr_t>(ws) & 15))
    return fail(RA_E_WORKSPACE, "%s: ws=%p ws_bytes=%zu, %zu bytes at a 16-byte boundary are needed", who, ws, ws_bytes, need);
  hipStream_t st = as_stream(stream);
  if (const int rc = geo::upload(who, geo, geo_dev, B, st)) return rc;
  return png::launch_kind(who, kind, false, st, src, png::Ragged{geo_dev, B, M, s.Hmax, kind == RA_PNG_BGR8 ? 3 : 1, total}, s.N, s.Hmax,
                          s.n_max, plane, static_cast<unsigned char *>(ws), out, sizes, offsets, adler);
}

// HOST code, no GPU call: the rule as it is stated, one byte after the other.
extern "C" int ra_png_deflate_host(const void *src, int kind, int M, int N, int H, int W, const int *plane, unsigned char *out,
                                   size_t out_bytes, int *sizes, unsigned long long *offsets, unsigned int *adler, void *ws,
                                   size_t ws_bytes) {
  (void)ws, (void)ws_bytes;  // the sequential form needs none
  png::Geometry g;
  if (const int rc = png::check("ra_png_deflate_host", false, src, kind, M, N, H, W, out, out_bytes, sizes, offsets, adler, &g)) return rc;
  if (!plane && N > M) return fail(RA_E_SHAPE, "ra_png_deflate_host: N=%d images of a source of M=%d without a plane list", N, M);
  for (int i = 0; plane && i < N; ++i)
    if (plane[i] < 0 || plane[i] >= M) return fail(RA_E_SHAPE, "ra_png_deflate_host: plane[%d]=%d (0 <= index < M=%d)", i, plane[i], M);
  std::vector<unsigned char> seg(g.n);
  size_t at = 0;
  for (int i = 0; i < N; ++i) {
    const size_t m = plane ? plane[i] : i;
    sizes[i] = (int)png::host_stream(src, kind, m * H * W, H, W, g.d, seg.data(), out + at, &adler[i]);
    offsets[i] = at;
    at += (size_t)sizes[i];
  }
  return 0;
}

// HOST code, no GPU call: the sequential rule per image of the table
extern "C" int ra_png_deflate_ragged_host(const void *src, int kind, int M, size_t total, const ra_image_geo *geo, int B,
                                          const int *plane, int Np, unsigned char *out, size_t out_bytes, int *sizes,
                                          unsigned long long *offsets, unsigned int *adler, void *ws, size_t ws_bytes) {
  (void)ws, (void)ws_bytes;  // the sequential form needs none
  const char *who = "ra_png_deflate_ragged_host";
  png::RaggedShape s;
  if (const int rc = png::check_ragged(who, false, src, kind, M, total, geo, B, plane, Np, out, out_bytes, sizes, offsets, adler, &s))
    return rc;
  for (int k = 0; plane && k < Np; ++k)
    if (plane[k] < 0 || plane[k] >= M) return fail(RA_E_SHAPE, "%s: plane[%d]=%d (0 <= index < M=%d)", who, k, plane[k], M);
  std::vector<unsigned char> seg(s.n_max);
  size_t at = 0;
  for (int i = 0; i < s.N; ++i) {
    const int k = i / B, b = i - k * B;
    const size_t m = plane ? plane[k] : k;
    sizes[i] = (int)png::host_stream(src, kind, m * total + (size_t)geo[b].offset, geo[b].h, geo[b].w, kind == RA_PNG_BGR8 ? 3 : 1,
                                     seg.data(), out + at, &adler[i]);
    offsets[i] = at;
    at += (size_t)sizes[i];
  }
  return 0;
}
