// K28 — the device PNG encoder's second stream format: ONE dynamic-Huffman block per image, the rows bit-contiguous.  The same
// scanlines, the same tokens (the greedy run code at distance d = bpp within a row) and the same Adler-32 as K27 (ra_png.hip);
// the literal / length code is built on the device from the image's own histogram.  The format and its rules are stated in full in
// include/recattend.h (ra_png_deflate_dyn_*).  The staging, the stretch analysis, the token walk and the row scan are K27's
// (ra_png_parts.h).
//
//   histogram  workgroup (row, image): the row staged as in K27's encode, walk 1 and its two scans, then the token walk with the
//              SYMBOL of every token counted in an LDS histogram (cleared first; a thread adds a run of equal symbols at once) and
//              the non-zero bins flushed with 32-bit integer atomic adds into the image's histogram in the workspace, which the
//              chain zeroes before (a stream-ordered memset).  Integer adds: the counts do not depend on the order.
//   code       one wave per image, lane 0 at work: the limited code lengths (huffman_lengths below, the function behind
//              ra_png_huffman_lengths), the canonical codes bit-reversed for LSB-first packing, and the finished header bits
//              (78 01 included) -> the image's Table in the workspace.  Sequential and small: a sort of <= 286 keys, <= 285
//              merges per round of the limiter, a header of <= 2113 bits.
//   encode     workgroup (row, image): K27's three walks with the token bits from the image's table, held in LDS.  The row's bits
//              start at bit 0 of its worst-case slot (15 bits per byte); a record (bits, Adler A, Adler B) beside it.
//   scan       workgroup = image (ra_png_parts.h, scan_kernel<true>): the 64-bit exclusive prefix of the rows' bits behind the
//              header, the stream's size, the combined Adler-32.
//   place      a wave per PIECE (piece 0 = the header, 1 .. H = the rows, H + 1 = the end-of-block code): OWNER COMPUTES per
//              destination dword.  A dword of `out` belongs to the piece that holds its first bit; the owner takes its own bits
//              with a funnel shift and, for the one dword its end falls into, gathers the starts of the pieces behind it (at most
//              32, each has a bit).  No atomics and nothing cleared: every byte of a stream is written exactly once, the bytes
//              around it never (the first and last dword of a stream are stored by bytes where they reach outside it).  The
//              zero padding falls out of the gather; the image's first workgroup adds the Adler-32 and offsets[image].
// One memset and five plain launches on the caller's stream; no workgroup waits for another; every loop is bounded by n, H, N,
// 286 or the limiter's rounds (<= 32: the counts halve).
#include <vector>

#include "ra_png_parts.h"

namespace ra {
namespace png {

// ---- the code: lengths, canonical codes, header ----------------------------------------------------------------------------------
struct HuffScratch {                        // LDS in the code kernel, the stack on the host: nothing here is a local array
  unsigned long long w[2 * kSymbols];      // weights: the sorted leaves, then the internal nodes in the order they are made
  unsigned short parent[2 * kSymbols], depth[2 * kSymbols], order[kSymbols];
  unsigned cnt[kSymbols];                  // the limiter's working counts
  unsigned hist[kTableSymbols];            // the image's histogram, end-of-block counted
  unsigned char len[kTableSymbols + 4];    // the literal / length lengths, then the distance lengths: the length sequence
  unsigned bl[16], next[16];               // canonical codes: lengths in use, next code per length
  unsigned clh[19], clc[19];               // the code-length code: histogram, codes
  unsigned char cll[19];
};

// The rule (include/recattend.h): Huffman by two queues over the used symbols sorted by (count, symbol) — a leaf before an
// internal node on a tie, internal nodes first made first —; while the deepest leaf exceeds `limit`, every count becomes
// (c + 1) >> 1 and the tree is rebuilt.  Unused symbols get 0; one used symbol gets 1.  Sequential.
__host__ __device__ inline void huffman_lengths(const unsigned *counts, int n, int limit, unsigned char *lengths, HuffScratch *s) {
  int m = 0;
  for (int i = 0; i < n; ++i) {
    s->cnt[i] = counts[i];
    lengths[i] = 0;
    m += counts[i] != 0u;
  }
  if (m == 0) return;
  if (m == 1) {
    for (int i = 0; i < n; ++i) lengths[i] = s->cnt[i] ? 1 : 0;
    return;
  }
  for (;;) {
    int k = 0;
    for (int i = 0; i < n; ++i) {  // insertion sort; symbols arrive in index order and pass only strictly larger counts
      const unsigned c = s->cnt[i];
      if (!c) continue;
      int j = k++;
      while (j > 0 && s->cnt[s->order[j - 1]] > c) {
        s->order[j] = s->order[j - 1];
        --j;
      }
      s->order[j] = (unsigned short)i;
    }
    for (int j = 0; j < m; ++j) s->w[j] = s->cnt[s->order[j]];
    int leaf = 0, inner = m, made = m;
    while (made < 2 * m - 1) {
      // the smaller head of the two queues, twice; written out, so that the queue heads stay in registers
      const int first = (leaf < m && (inner >= made || s->w[leaf] <= s->w[inner])) ? leaf++ : inner++;
      const int second = (leaf < m && (inner >= made || s->w[leaf] <= s->w[inner])) ? leaf++ : inner++;
      s->w[made] = s->w[first] + s->w[second];
      s->parent[first] = s->parent[second] = (unsigned short)made;
      ++made;
    }
    s->depth[2 * m - 2] = 0;
    for (int q = 2 * m - 3; q >= 0; --q) s->depth[q] = (unsigned short)(s->depth[s->parent[q]] + 1);  // a parent is made later
    int deepest = 0;
    for (int j = 0; j < m; ++j) deepest = s->depth[j] > deepest ? s->depth[j] : deepest;
    if (deepest <= limit) {
      for (int j = 0; j < m; ++j) lengths[s->order[j]] = (unsigned char)s->depth[j];
      return;
    }
    for (int i = 0; i < n; ++i)
      if (s->cnt[i]) s->cnt[i] = (s->cnt[i] + 1u) >> 1;
  }
}

// RFC 1951 3.2.2: code[i] = the canonical code of length len[i], bit-reversed, | len[i] << 16 (0 for an unused symbol)
__host__ __device__ inline void canonical_codes(const unsigned char *len, int n, unsigned *code, HuffScratch *s) {
  for (int b = 0; b < 16; ++b) s->bl[b] = 0u;
  for (int i = 0; i < n; ++i) ++s->bl[len[i]];
  s->bl[0] = 0u;
  unsigned c = 0u;
  for (int b = 1; b < 16; ++b) {
    c = (c + s->bl[b - 1]) << 1;
    s->next[b] = c;
  }
  for (int i = 0; i < n; ++i) code[i] = len[i] ? rev_bits(s->next[len[i]]++, len[i]) | (unsigned)len[i] << 16 : 0u;
}

// The run-length rule of the length sequence seq[0 .. total): a zero run is cut greedily into symbols 18 (11 .. 138 zeros), then
// one 17 (3 .. 10), then single zeros; every non-zero length is sent on its own (symbol 16 is not used).  emit(symbol, the value
// of its extra bits, their number).
template <class Emit>
__host__ __device__ __forceinline__ void length_runs(const unsigned char *seq, int total, Emit &&emit) {
  for (int i = 0; i < total;) {
    if (seq[i]) {
      emit(seq[i], 0, 0);
      ++i;
      continue;
    }
    int run = 1;
    while (i + run < total && !seq[i + run]) ++run;
    i += run;
    while (run >= 11) {
      const int take = run < 138 ? run : 138;
      emit(18, take - 11, 7);
      run -= take;
    }
    if (run >= 3) {
      emit(17, run - 3, 3);
      run = 0;
    }
    for (; run > 0; --run) emit(0, 0, 0);
  }
}

// nb <= 16 bits of v, LSB-first, into the zeroed 32-bit words w[] at bit *bit
__host__ __device__ __forceinline__ void put_bits(unsigned *w, unsigned *bit, unsigned v, int nb) {
  const unsigned i = *bit >> 5, sh = *bit & 31u;
  w[i] |= v << sh;
  if (sh + (unsigned)nb > 32u) w[i + 1] |= v >> (32u - sh);
  *bit += (unsigned)nb;
}

// s->hist (end-of-block counted) and the match distance d -> the image's table: codes, header bits, end-of-block code
__host__ __device__ inline void build_table(int d, Table *t, HuffScratch *s) {
  huffman_lengths(s->hist, kSymbols, 15, s->len, s);
  canonical_codes(s->len, kSymbols, t->sym, s);
  t->sym[286] = t->sym[287] = 0u;
  int nl = kSymbols;
  while (nl > 257 && !s->len[nl - 1]) --nl;  // HLIT: symbol 256 is always in use
  // the distance lengths follow the literal / length lengths in one sequence: code 0 (d = 1) or code 2 (d = 3), length 1
  const int nd = d == 1 ? 1 : 3;
  for (int k = 0; k < nd; ++k) s->len[nl + k] = k == nd - 1 ? 1 : 0;
  const int total = nl + nd;
  for (int k = 0; k < 19; ++k) s->clh[k] = 0u;
  length_runs(s->len, total, [&](int sym, int, int) { ++s->clh[sym]; });
  huffman_lengths(s->clh, 19, 7, s->cll, s);
  canonical_codes(s->cll, 19, s->clc, s);
  constexpr unsigned char kOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  int hclen = 19;
  while (hclen > 4 && !s->cll[kOrder[hclen - 1]]) --hclen;
  for (int k = 0; k < kHeaderWords; ++k) t->hdr[k] = 0u;
  unsigned *bit = &t->hdr_bits;  // the writer's place lives in the table: no object on a stack
  *bit = 0u;
  put_bits(t->hdr, bit, 0x78u, 8), put_bits(t->hdr, bit, 0x01u, 8);
  put_bits(t->hdr, bit, 5u, 3);  // BFINAL = 1, BTYPE = 10
  put_bits(t->hdr, bit, (unsigned)(nl - 257), 5), put_bits(t->hdr, bit, (unsigned)(nd - 1), 5), put_bits(t->hdr, bit, (unsigned)(hclen - 4), 4);
  for (int k = 0; k < hclen; ++k) put_bits(t->hdr, bit, s->cll[kOrder[k]], 3);
  length_runs(s->len, total, [&](int sym, int extra, int xb) {
    put_bits(t->hdr, bit, s->clc[sym] & 0xffffu, (int)(s->clc[sym] >> 16));
    if (xb) put_bits(t->hdr, bit, (unsigned)extra, xb);
  });
  t->eob = t->sym[256] & 0xffffu, t->eob_bits = t->sym[256] >> 16, t->pad = 0u;
}

// ---- the kernels -----------------------------------------------------------------------------------------------------------------
// Workgroup (row, stream).  Dynamic LDS: [0, row_bytes) the staged segment, then kTableSymbols histogram words, then 4 scan words.
// GEO: Uniform or Ragged (ra_png_parts.h); a ragged workgroup beyond its image's rows leaves before the first barrier.
template <int KIND, bool VEC, class GEO>
__global__ __launch_bounds__(kThreads) void histogram_kernel(const void *src, GEO geom, const int *plane, unsigned row_bytes,
                                                              unsigned *hist) {
  extern __shared__ u32x4 dyn[];
  unsigned char *sh_raw = reinterpret_cast<unsigned char *>(dyn);
  unsigned *sh_hist = reinterpret_cast<unsigned *>(sh_raw + row_bytes);
  unsigned *sh_scan = sh_hist + kTableSymbols;
  const int tid = threadIdx.x, r = blockIdx.x, img = blockIdx.y;
  constexpr int d = KIND == RA_PNG_BGR8 ? 3 : 1;
  const Image im = geom.at(img, plane);
  if (GEO::kRagged && r >= im.h) return;
  const int n = im.n, K = im.K;

  stage_segment<KIND, VEC, GEO::kRagged>(src, im, r, sh_raw);
  for (int k = tid; k < kTableSymbols; k += kThreads) sh_hist[k] = 0u;  // LDS holds anything at entry
  __syncthreads();

  const unsigned char *b = sh_raw + (kRowPad - 1);
  const int lo = tid * K < n ? tid * K : n, hi = lo + K < n ? lo + K : n;
  int s_in, e_in;
  unsigned s1, s2;
  chunk_stretches(b, lo, hi, d, n, sh_scan, &s_in, &e_in, &s1, &s2);
  unsigned cur = 0u, run = 0u;  // a run of equal symbols is added at once
  walk(SymbolCoder(), b, lo, hi, d, s_in, e_in, [&](unsigned sym, int) {
    if (run && sym != cur) {
      atomicAdd(&sh_hist[cur], run);
      run = 0u;
    }
    cur = sym;
    ++run;
  });
  if (run) atomicAdd(&sh_hist[cur], run);
  __syncthreads();
  unsigned *g = hist + (size_t)img * kTableSymbols;
  for (int k = tid; k < kSymbols; k += kThreads) {
    const unsigned c = sh_hist[k];
    if (c) atomicAdd(&g[k], c);
  }
}

// One wave per image; lane 0 builds the table.
__global__ __launch_bounds__(kWave) void code_kernel(const unsigned *hist, int d, Table *tab) {
  __shared__ HuffScratch s;
  const int img = blockIdx.x;
  for (int k = threadIdx.x; k < kTableSymbols; k += kWave) s.hist[k] = k < kSymbols ? hist[(size_t)img * kTableSymbols + k] : 0u;
  __syncthreads();
  if (threadIdx.x == 0) {
    s.hist[256] += 1u;  // end-of-block
    build_table(d, tab + img, &s);
  }
}

// a row's slot in the workspace: 15 bits per byte, 4 bytes the placement's funnel shift may read beyond them, whole 16-byte stores
constexpr size_t dynamic_slot_bytes(size_t n) { return ((15 * n + 7) / 8 + 4 + 15) / 16 * 16; }

// Workgroup (row, stream).  Dynamic LDS: [0, row_bytes) the staged segment, out_words dwords of bits, kTableSymbols code words, 4
// scan words.  GEO as in the histogram kernel; the LDS offsets are the launch's (ragged: the widest image's).
template <int KIND, bool VEC, class GEO>
__global__ __launch_bounds__(kThreads) void encode_dynamic_kernel(const void *src, GEO geom, const int *plane, unsigned row_bytes,
                                                                   unsigned out_words, const Table *tab, unsigned char *slots,
                                                                   size_t slot, Record *rec) {
  extern __shared__ u32x4 dyn[];
  unsigned char *sh_raw = reinterpret_cast<unsigned char *>(dyn);
  unsigned *sh_out = reinterpret_cast<unsigned *>(sh_raw + row_bytes);
  unsigned *sh_tab = sh_out + out_words;
  unsigned *sh_scan = sh_tab + kTableSymbols;
  const int tid = threadIdx.x, r = blockIdx.x, img = blockIdx.y;
  constexpr int d = KIND == RA_PNG_BGR8 ? 3 : 1;
  const Image im = geom.at(img, plane);
  if (GEO::kRagged && r >= im.h) return;
  const int n = im.n, K = im.K;

  stage_segment<KIND, VEC, GEO::kRagged>(src, im, r, sh_raw);
  for (unsigned w = tid; w < out_words; w += kThreads) sh_out[w] = 0u;  // bits are OR-ed in: LDS holds anything at entry
  for (int k = tid; k < kTableSymbols; k += kThreads) sh_tab[k] = tab[img].sym[k];
  __syncthreads();

  const unsigned char *b = sh_raw + (kRowPad - 1);
  const int lo = tid * K < n ? tid * K : n, hi = lo + K < n ? lo + K : n;
  int s_in, e_in;
  unsigned s1, s2;
  chunk_stretches(b, lo, hi, d, n, sh_scan, &s_in, &e_in, &s1, &s2);
  unsigned sum1, sum2;
  block_scan_excl<OpAdd, false>(s1 % kAdler, sh_scan, &sum1);
  block_scan_excl<OpAdd, false>(s2 % kAdler, sh_scan, &sum2);

  const TableCoder code{sh_tab};
  unsigned bits = 0u;  // at most 15 * 2^15 per row
  walk(code, b, lo, hi, d, s_in, e_in, [&](unsigned, int nb) { bits += (unsigned)nb; });
  unsigned row_bits;
  const unsigned at = block_scan_excl<OpAdd, false>(bits, sh_scan, &row_bits);
  emit_chunk(code, b, lo, hi, d, s_in, e_in, at, sh_out);
  __syncthreads();
  const size_t at_rec = (size_t)img * geom.rows() + r;
  if (tid == 0) {
    Record q;
    q.bytes = row_bits, q.a = (1u + sum1) % kAdler, q.b = ((unsigned)n + sum2) % kAdler, q.offset = 0u;
    rec[at_rec] = q;
  }
  u32x4 *dst = reinterpret_cast<u32x4 *>(slots + at_rec * slot);
  for (unsigned v = tid; v < (row_bits + 127u) / 128u; v += kThreads) dst[v] = reinterpret_cast<const u32x4 *>(sh_out)[v];
}

// 32 bits of a piece of nbits bits packed from bit 0 of w[]: bit i of the result = the piece's bit off + i, 0 outside the piece.
// -32 < off < nbits; w[(off >> 5) + 1] is readable.
__device__ __forceinline__ unsigned piece_bits(const unsigned *w, unsigned nbits, long long off) {
  if (off < 0) {
    unsigned v = w[0];
    if (nbits < 32u) v &= (1u << nbits) - 1u;
    return v << (unsigned)(-off);
  }
  const unsigned i = (unsigned)(off >> 5), sh = (unsigned)off & 31u;
  unsigned v = (unsigned)(((unsigned long long)w[i + 1] << 32 | w[i]) >> sh);
  const unsigned long long valid = nbits - (unsigned long long)off;
  if (valid < 32ull) v &= (1u << (unsigned)valid) - 1u;
  return v;
}

// Workgroup (group of kCompactRows pieces, stream); a wave places one piece at a time.  Bit places are counted from the dword
// boundary at or before the stream's first byte (`lead` bits before it), so that a dword index is an aligned address.  H is the
// image's own, S the stride of a stream's records (GEO: ra_png_parts.h).
template <class GEO>
__global__ __launch_bounds__(kThreads) void place_kernel(const unsigned char *slots, size_t slot, const Record *rec,
                                                          const unsigned long long *start, const Table *tab, GEO geom, const int *sizes,
                                                          const unsigned *adler, unsigned char *out, unsigned long long *offsets) {
  __shared__ unsigned sh_scan[4];
  __shared__ unsigned long long sh_hi;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, img = blockIdx.y;
  const int H = geom.dims(img).h, S = geom.rows();
  if (GEO::kRagged && blockIdx.x * kCompactRows > H + 1) return;  // no piece of this image here: before the first barrier
  const unsigned long long base = stream_base(sizes, img, sh_scan, &sh_hi);
  unsigned char *o = out + base;
  const unsigned size = (unsigned)sizes[img];
  if (blockIdx.x == 0 && tid == 0) {
    const unsigned ad = adler[img];
    offsets[img] = base;
    unsigned char *t = o + size - 4;
    t[0] = (unsigned char)(ad >> 24), t[1] = (unsigned char)(ad >> 16), t[2] = (unsigned char)(ad >> 8), t[3] = (unsigned char)ad;
  }
  const Table *t = tab + img;
  const unsigned long long *st = start + (size_t)img * (S + 1);
  const Record *q = rec + (size_t)img * S;
  const unsigned lead = 8u * (unsigned)(reinterpret_cast<uintptr_t>(o) & 3u);
  unsigned char *o4 = o - lead / 8u;                                     // 4-byte aligned; bytes before o are never touched
  const unsigned long long end = lead + 8ull * (size - 4u);              // the Adler-32 starts here
  // piece p: its words, its first bit (from the aligned dword on) and its bits
  auto piece = [&](int p, const unsigned **w, unsigned long long *s, unsigned *nbits) {
    if (p == 0) {
      *w = t->hdr, *s = lead, *nbits = t->hdr_bits;
    } else if (p <= H) {
      *w = reinterpret_cast<const unsigned *>(slots + ((size_t)img * S + (p - 1)) * slot), *s = lead + st[p - 1], *nbits = q[p - 1].bytes;
    } else {
      *w = &t->eob, *s = lead + st[H], *nbits = t->eob_bits;
    }
  };
  for (int k = 0; k < kRowsPerWave; ++k) {
    const int p = blockIdx.x * kCompactRows + wave * kRowsPerWave + k;
    if (p > H + 1) break;
    const unsigned *w;
    unsigned long long s;
    unsigned nbits;
    piece(p, &w, &s, &nbits);
    const unsigned long long e = s + nbits;
    // the dwords j whose first bit 32 j lies in [s, e); the header also owns the dword the stream starts in
    const unsigned long long j0 = p == 0 ? 0ull : (s + 31ull) >> 5, j1 = (e + 31ull) >> 5;
    for (unsigned long long j = j0 + lane; j < j1; j += 64ull) {
      const unsigned long long first = 32ull * j;
      unsigned v = piece_bits(w, nbits, (long long)first - (long long)s);
      if (first + 32ull > e) {  // the dword the piece ends in: the pieces behind it that start in it, each at least a bit long
        for (int g = p + 1; g <= H + 1; ++g) {
          const unsigned *wg;
          unsigned long long sg;
          unsigned ng;
          piece(g, &wg, &sg, &ng);
          if (sg >= first + 32ull) break;
          v |= piece_bits(wg, ng, (long long)first - (long long)sg);
        }
      }
      if (first >= lead && first + 32ull <= end) {
        reinterpret_cast<unsigned *>(o4)[j] = v;
      } else {  // the stream's first or last dword: only the bytes inside [lead, end)
        for (unsigned c = 0; c < 4u; ++c)
          if (first + 8ull * c >= lead && first + 8ull * c < end) o4[4ull * j + c] = (unsigned char)(v >> (8u * c));
      }
    }
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
struct Workspace {  // the device entry's workspace, every part at a 16-byte boundary
  size_t hist, tab, rec, start, slots, total, slot;
  Workspace(int N, int H, size_t n) {
    auto r16 = [](size_t v) { return (v + 15) / 16 * 16; };
    slot = dynamic_slot_bytes(n);
    hist = 0;
    tab = hist + r16((size_t)N * kTableSymbols * sizeof(unsigned));
    rec = tab + r16((size_t)N * sizeof(Table));
    start = rec + records_bytes(N, H);
    slots = start + r16((size_t)N * (H + 1) * sizeof(unsigned long long));
    total = slots + (size_t)N * H * slot;
  }
};

// the encode kernel's dynamic LDS for scanlines of n bytes: the staged row, the bit buffer (the slot and 4 words), the table, the scan
constexpr size_t encode_lds(size_t n) {
  return (kRowPad + n + 15) / 16 * 16 + (dynamic_slot_bytes(n) + 16) + (size_t)kTableSymbols * 4 + 16;
}

// The clear and the five launches of a call of N streams: `rows` scanlines per stream in the grid (wsp is laid out for them),
// segments of up to n_max bytes.
template <int KIND, class GEO>
int launch_chain(const char *who, bool vec, hipStream_t st, const void *src, const GEO &geom, int N, int rows, size_t n_max,
                 const int *plane, const Workspace &wsp, unsigned char *ws, unsigned char *out, int *sizes, unsigned long long *offsets,
                 unsigned *adler) {
  constexpr int d = KIND == RA_PNG_BGR8 ? 3 : 1;
  unsigned *hist = reinterpret_cast<unsigned *>(ws + wsp.hist);
  Table *tab = reinterpret_cast<Table *>(ws + wsp.tab);
  Record *rec = reinterpret_cast<Record *>(ws + wsp.rec);
  unsigned long long *start = reinterpret_cast<unsigned long long *>(ws + wsp.start);
  unsigned char *slots = ws + wsp.slots;
  const unsigned row_bytes = (unsigned)round_up(kRowPad + (int)n_max, 16);
  const unsigned out_words = (unsigned)(wsp.slot / 4) + 4u;
  const size_t lds_hist = row_bytes + (size_t)kTableSymbols * 4 + 16;
  const size_t lds_enc = encode_lds(n_max);
  // the longest row takes 24592 + 46112 + 1152 + 16 bytes of LDS: above the default limit of 64 KiB, below the CU's 160 KiB
  constexpr size_t kMaxEnc = encode_lds(RA_PNG_MAX_ROW_BYTES);
  constexpr bool kWide = !GEO::kRagged;  // a ragged workgroup decides the load width itself: one instantiation
  const dim3 grid(rows, N), block(kThreads);
  if (const hipError_t e = hipMemsetAsync(hist, 0, (size_t)N * kTableSymbols * sizeof(unsigned), st))
    return fail((int)e, "%s (clearing the histograms): %s", who, hipGetErrorString(e));
  if (vec) {
    hipLaunchKernelGGL((histogram_kernel<KIND, kWide, GEO>), grid, block, lds_hist, st, src, geom, plane, row_bytes, hist);
  } else {
    hipLaunchKernelGGL((histogram_kernel<KIND, false, GEO>), grid, block, lds_hist, st, src, geom, plane, row_bytes, hist);
  }
  if (const int rc = launch_status(who)) return rc;
  hipLaunchKernelGGL(code_kernel, dim3(N), dim3(kWave), 0, st, hist, d, tab);
  if (const int rc = launch_status(who)) return rc;
  if (vec) {
    static MaxDynamicLds once(encode_dynamic_kernel<KIND, kWide, GEO>, kMaxEnc);
    hipLaunchKernelGGL((encode_dynamic_kernel<KIND, kWide, GEO>), grid, block, lds_enc, st, src, geom, plane, row_bytes, out_words, tab,
                       slots, wsp.slot, rec);
  } else {
    static MaxDynamicLds once(encode_dynamic_kernel<KIND, false, GEO>, kMaxEnc);
    hipLaunchKernelGGL((encode_dynamic_kernel<KIND, false, GEO>), grid, block, lds_enc, st, src, geom, plane, row_bytes, out_words, tab,
                       slots, wsp.slot, rec);
  }
  if (const int rc = launch_status(who)) return rc;
  hipLaunchKernelGGL((scan_kernel<true, GEO>), dim3(N), block, 0, st, rec, geom, sizes, adler, tab, start);
  if (const int rc = launch_status(who)) return rc;
  hipLaunchKernelGGL(place_kernel<GEO>, dim3(ceil_div(rows + 2, kCompactRows), N), block, 0, st, slots, wsp.slot, rec, start, tab, geom,
                     sizes, adler, out, offsets);
  return launch_status(who);
}

template <class GEO>
int launch_kind(const char *who, int kind, bool vec, hipStream_t st, const void *src, const GEO &geom, int N, int rows, size_t n_max,
                const int *plane, const Workspace &wsp, unsigned char *ws, unsigned char *out, int *sizes, unsigned long long *offsets,
                unsigned *adler) {
  if (kind == RA_PNG_GRAY8)
    return launch_chain<RA_PNG_GRAY8>(who, vec, st, src, geom, N, rows, n_max, plane, wsp, ws, out, sizes, offsets, adler);
  if (kind == RA_PNG_BGR8)
    return launch_chain<RA_PNG_BGR8>(who, vec, st, src, geom, N, rows, n_max, plane, wsp, ws, out, sizes, offsets, adler);
  return launch_chain<RA_PNG_F32>(who, vec, st, src, geom, N, rows, n_max, plane, wsp, ws, out, sizes, offsets, adler);
}

// HOST code: the stream of the image of H x W whose first element is `base`, written at o — the histogram of the greedy tokens,
// the table (the function the code kernel runs), then the tokens again, one bit after the other; its bytes, *adler = its Adler-32
inline size_t host_stream(const void *src, int kind, size_t base, int H, int W, int d, unsigned char *seg, HuffScratch *s, Table *t,
                          unsigned char *o, unsigned *adler) {
  const int n = 1 + W * d;
  // the greedy tokens of the scanline in seg: tok(literal / length symbol, extra value, extra bits, is a match)
  auto tokens = [&](auto &&tok) {
    for (int k = 0; k < n;) {
      int L = 0;
      if (k >= d)
        while (L < 258 && k + L < n && seg[k + L] == seg[k + L - d]) ++L;
      if (L >= 3) {
        int xb, extra;
        const int sym = length_symbol(L, &xb, &extra);
        tok(sym, extra, xb, true);
        k += L;
      } else {
        tok((int)seg[k], 0, 0, false);
        ++k;
      }
    }
  };
  for (int k = 0; k < kTableSymbols; ++k) s->hist[k] = 0u;
  unsigned A = 1u, B = 0u;
  for (int r = 0; r < H; ++r) {
    host_scanline(src, kind, base, W, r, seg);
    for (int k = 0; k < n; ++k) {
      A = (A + seg[k]) % kAdler;
      B = (B + A) % kAdler;
    }
    tokens([&](int sym, int, int, bool) { ++s->hist[sym]; });
  }
  s->hist[256] += 1u;  // end-of-block
  build_table(d, t, s);
  BitWriter bw{o};
  for (unsigned k = 0; k < t->hdr_bits; k += 16u) bw.put(t->hdr[k >> 5] >> (k & 31u), (int)(t->hdr_bits - k < 16u ? t->hdr_bits - k : 16u));
  for (int r = 0; r < H; ++r) {
    host_scanline(src, kind, base, W, r, seg);
    tokens([&](int sym, int extra, int xb, bool is_match) {
      bw.put(t->sym[sym] & 0xffffu, (int)(t->sym[sym] >> 16));
      if (xb) bw.put((unsigned)extra, xb);
      if (is_match) bw.put(0u, 1);  // the one distance code
    });
  }
  bw.put(t->eob, (int)t->eob_bits);
  bw.align();
  bw.byte(B >> 8), bw.byte(B & 255u), bw.byte(A >> 8), bw.byte(A & 255u);
  *adler = B << 16 | A;
  return bw.bit >> 3;
}

}  // namespace png
}  // namespace ra

using namespace ra;

extern "C" int ra_png_huffman_lengths(const unsigned int *counts, int n, int limit, unsigned char *lengths) {
  if (!counts || !lengths) return fail(RA_E_INVALID, "ra_png_huffman_lengths: counts or lengths is NULL");
  if (limit != 7 && limit != 15) return fail(RA_E_INVALID, "ra_png_huffman_lengths: limit=%d (7 or 15)", limit);
  if (n < 1 || n > png::kSymbols || n > (1 << limit))
    return fail(RA_E_SHAPE, "ra_png_huffman_lengths: n=%d (1 <= n <= %d and n <= 2^limit)", n, png::kSymbols);
  png::HuffScratch s;
  png::huffman_lengths(counts, n, limit, lengths, &s);
  return 0;
}

extern "C" int ra_png_deflate_dyn_bound(int N, int H, int W, int bpp, unsigned long long *stream_bytes,
                                        unsigned long long *workspace_bytes) {
  size_t n;
  if (const int rc = png::check_bound("ra_png_deflate_dyn_bound", N, H, W, bpp, stream_bytes, workspace_bytes, &n)) return rc;
  const size_t stream = png::dynamic_stream_bound(n, H);
  if (stream >= (1ull << 31))
    return fail(RA_E_SHAPE, "ra_png_deflate_dyn_bound: H=%d W=%d: a stream of up to %zu bytes (below 2^31)", H, W, stream);
  *stream_bytes = stream;
  *workspace_bytes = png::Workspace(N, H, n).total;
  return 0;
}

extern "C" int ra_png_deflate_dyn_u8(const void *src, int kind, int M, int N, int H, int W, const int *plane, unsigned char *out,
                                     size_t out_bytes, int *sizes, unsigned long long *offsets, unsigned int *adler, void *ws,
                                     size_t ws_bytes, void *stream) {
  png::Geometry g;
  if (const int rc = png::check("ra_png_deflate_dyn_u8", true, src, kind, M, N, H, W, out, out_bytes, sizes, offsets, adler, &g)) return rc;
  if (!plane && N > M) return fail(RA_E_SHAPE, "ra_png_deflate_dyn_u8: N=%d images of a source of M=%d without a plane list", N, M);
  const png::Workspace wsp(N, H, g.n);
  if (!ws || ws_bytes < wsp.total || (reinterpret_cast<uintptr_t>(ws) & 15))
    return fail(RA_E_WORKSPACE, "ra_png_deflate_dyn_u8: ws=%p ws_bytes=%zu, %zu bytes at a 16-byte boundary are needed", ws, ws_bytes,
                wsp.total);
  return png::launch_kind("ra_png_deflate_dyn_u8", kind, png::vector_rows(src, kind, W), as_stream(stream), src,
                          png::Uniform{M, H, W, (int)g.n, png::chunk_bytes((int)g.n)}, N, H, g.n, plane, wsp,
                          static_cast<unsigned char *>(ws), out, sizes, offsets, adler);
}

extern "C" int ra_png_deflate_dyn_ragged_bound(const ra_image_geo *geo, int B, int Np, int bpp, unsigned long long *out_bytes,
                                               unsigned long long *workspace_bytes) {
  const char *who = "ra_png_deflate_dyn_ragged_bound";
  if (!geo || !out_bytes || !workspace_bytes) return fail(RA_E_INVALID, "%s: geo, out_bytes or workspace_bytes is NULL", who);
  if (bpp != 1 && bpp != 3) return fail(RA_E_SHAPE, "%s: bpp=%d (1 = grey, 3 = RGB)", who, bpp);
  png::RaggedShape s;
  if (const int rc = png::ragged_shape(who, true, geo, B, Np, bpp, bpp, &s)) return rc;
  *out_bytes = s.out;
  *workspace_bytes = png::Workspace(s.N, s.Hmax, s.n_max).total;
  return 0;
}

extern "C" int ra_png_deflate_dyn_ragged_u8(const void *src, int kind, int M, size_t total, const ra_image_geo *geo,
                                            ra_image_geo *geo_dev, int B, const int *plane, int Np, unsigned char *out,
                                            size_t out_bytes, int *sizes, unsigned long long *offsets, unsigned int *adler, void *ws,
                                            size_t ws_bytes, void *stream) {
  const char *who = "ra_png_deflate_dyn_ragged_u8";
  if (!geo_dev) return fail(RA_E_INVALID, "%s: geo_dev is NULL", who);
  png::RaggedShape s;
  if (const int rc = png::check_ragged(who, true, src, kind, M, total, geo, B, plane, Np, out, out_bytes, sizes, offsets, adler, &s))
    return rc;
  const png::Workspace wsp(s.N, s.Hmax, s.n_max);
  if (!ws || ws_bytes < wsp.total || (reinterpret_cast<uintptr_t>(ws) & 15))
    return fail(RA_E_WORKSPACE, "%s: ws=%p ws_bytes=%zu, %zu bytes at a 16-byte boundary are needed", who, ws, ws_bytes, wsp.total);
  hipStream_t st = as_stream(stream);
  if (const int rc = geo::upload(who, geo, geo_dev, B, st)) return rc;
  return png::launch_kind(who, kind, false, st, src, png::Ragged{geo_dev, B, M, s.Hmax, kind == RA_PNG_BGR8 ? 3 : 1, total}, s.N, s.Hmax,
                          s.n_max, plane, wsp, static_cast<unsigned char *>(ws), out, sizes, offsets, adler);
}

// HOST code, no GPU call: the rule as it is stated, one image after the other: the histogram of the greedy tokens, the table
// (the function the code kernel runs), then the tokens again, one bit after the other.
extern "C" int ra_png_deflate_dyn_host(const void *src, int kind, int M, int N, int H, int W, const int *plane, unsigned char *out,
                                       size_t out_bytes, int *sizes, unsigned long long *offsets, unsigned int *adler, void *ws,
                                       size_t ws_bytes) {
  (void)ws, (void)ws_bytes;  // the sequential form needs none
  png::Geometry g;
  if (const int rc = png::check("ra_png_deflate_dyn_host", true, src, kind, M, N, H, W, out, out_bytes, sizes, offsets, adler, &g)) return rc;
  if (!plane && N > M) return fail(RA_E_SHAPE, "ra_png_deflate_dyn_host: N=%d images of a source of M=%d without a plane list", N, M);
  for (int i = 0; plane && i < N; ++i)
    if (plane[i] < 0 || plane[i] >= M) return fail(RA_E_SHAPE, "ra_png_deflate_dyn_host: plane[%d]=%d (0 <= index < M=%d)", i, plane[i], M);
  std::vector<unsigned char> seg(g.n);
  std::vector<png::HuffScratch> scratch(1);
  std::vector<png::Table> table(1);
  size_t at = 0;
  for (int i = 0; i < N; ++i) {
    const size_t m = plane ? plane[i] : i;
    sizes[i] = (int)png::host_stream(src, kind, m * H * W, H, W, g.d, seg.data(), scratch.data(), table.data(), out + at, &adler[i]);
    offsets[i] = at;
    at += (size_t)sizes[i];
  }
  return 0;
}

// HOST code, no GPU call: the sequential rule per image of the table
extern "C" int ra_png_deflate_dyn_ragged_host(const void *src, int kind, int M, size_t total, const ra_image_geo *geo, int B,
                                              const int *plane, int Np, unsigned char *out, size_t out_bytes, int *sizes,
                                              unsigned long long *offsets, unsigned int *adler, void *ws, size_t ws_bytes) {
  (void)ws, (void)ws_bytes;  // the sequential form needs none
  const char *who = "ra_png_deflate_dyn_ragged_host";
  png::RaggedShape s;
  if (const int rc = png::check_ragged(who, true, src, kind, M, total, geo, B, plane, Np, out, out_bytes, sizes, offsets, adler, &s))
    return rc;
  for (int k = 0; plane && k < Np; ++k)
    if (plane[k] < 0 || plane[k] >= M) return fail(RA_E_SHAPE, "%s: plane[%d]=%d (0 <= index < M=%d)", who, k, plane[k], M);
  std::vector<unsigned char> seg(s.n_max);
  std::vector<png::HuffScratch> scratch(1);
  std::vector<png::Table> table(1);
  size_t at = 0;
  for (int i = 0; i < s.N; ++i) {
    const int k = i / B, b = i - k * B;
    const size_t m = plane ? plane[k] : k;
    sizes[i] = (int)png::host_stream(src, kind, m * total + (size_t)geo[b].offset, geo[b].h, geo[b].w, kind == RA_PNG_BGR8 ? 3 : 1,
                                     seg.data(), scratch.data(), table.data(), out + at, &adler[i]);
    offsets[i] = at;
    at += (size_t)sizes[i];
  }
  return 0;
}
