// A stand-alone run of the image stage's HOST code under the host sanitizers: ra_png_unfilter_u8 and ra_resize_cubic_tables of
// csrc/ra_image.hip on seeded inputs, the degenerate sizes included, with buffers of exactly the documented size so that a byte
// read or written past them is reported.  CPU only; it makes no GPU call.  Build and run (from the repository root):
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -ffp-contract=off -Iinclude \
//         -Irec-attend-public_amd/csrc tools/image_host_check.cpp rec-attend-public_amd/csrc/ra_image.hip -o tools/bin/image_host_check
//   tools/bin/image_host_check
// It prints one line per group and exits 0 when every check held.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "recattend.h"

namespace ra {
void set_error(const char *, ...) {}  // ra_core.hip's, which this program does not link
}

static uint32_t rng_state = 12345;
static uint32_t rnd() {  // xorshift32
  rng_state ^= rng_state << 13, rng_state ^= rng_state >> 17, rng_state ^= rng_state << 5;
  return rng_state;
}

static int failures = 0;
#define CHECK(cond)                                                 \
  do {                                                              \
    if (!(cond)) {                                                  \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      ++failures;                                                   \
    }                                                               \
  } while (0)

// PNG specification 9.2, written apart from the library's loop: one byte at a time with explicit neighbours
static void unfilter_ref(const std::vector<unsigned char> &raw, int H, int stride, int bpp, std::vector<unsigned char> &out) {
  for (int r = 0; r < H; ++r)
    for (int i = 0; i < stride; ++i) {
      const int a = i >= bpp ? out[(size_t)r * stride + i - bpp] : 0, b = r ? out[(size_t)(r - 1) * stride + i] : 0;
      const int c = (r && i >= bpp) ? out[(size_t)(r - 1) * stride + i - bpp] : 0;
      const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
      const int ft = raw[(size_t)r * (stride + 1)];
      const int pred = ft == 0 ? 0 : ft == 1 ? a : ft == 2 ? b : ft == 3 ? (a + b) / 2 : ((pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c));
      out[(size_t)r * stride + i] = (unsigned char)(raw[(size_t)r * (stride + 1) + 1 + i] + pred);
    }
}

static void check_unfilter() {
  const int bpps[] = {1, 2, 3, 4, 6, 8}, widths[] = {1, 2, 5, 33, 257}, heights[] = {1, 2, 7, 40};
  int n = 0;
  for (int bpp : bpps)
    for (int w : widths)
      for (int H : heights)
        for (int first = 0; first < 5; ++first) {
          const int stride = w * bpp;
          std::vector<unsigned char> raw((size_t)H * (stride + 1)), out((size_t)H * stride), ref((size_t)H * stride);
          for (auto &v : raw) v = (unsigned char)rnd();
          for (int r = 0; r < H; ++r) raw[(size_t)r * (stride + 1)] = (unsigned char)(r == 0 ? first : rnd() % 5);
          CHECK(ra_png_unfilter_u8(raw.data(), H, stride, bpp, out.data()) == 0);
          unfilter_ref(raw, H, stride, bpp, ref);
          CHECK(out == ref);
          ++n;
        }
  std::vector<unsigned char> raw(3 * 7, 0), out(3 * 6);
  raw[7] = 5;
  CHECK(ra_png_unfilter_u8(raw.data(), 3, 6, 3, out.data()) == RA_E_SHAPE);
  CHECK(ra_png_unfilter_u8(raw.data(), 0, 6, 3, out.data()) == RA_E_SHAPE);
  CHECK(ra_png_unfilter_u8(raw.data(), 3, 0, 3, out.data()) == RA_E_SHAPE);
  CHECK(ra_png_unfilter_u8(raw.data(), 3, 6, 4, out.data()) == RA_E_SHAPE);
  CHECK(ra_png_unfilter_u8(raw.data(), 3, 6, 0, out.data()) == RA_E_SHAPE);
  CHECK(ra_png_unfilter_u8(nullptr, 3, 6, 3, out.data()) == RA_E_SHAPE);
  CHECK(ra_png_unfilter_u8(raw.data(), 3, 6, 3, nullptr) == RA_E_SHAPE);
  printf("unfilter: %d seeded images against the byte-wise definition, 7 refusals\n", n);
}

static void check_tables() {
  const int pairs[][2] = {{1, 1}, {1, 7}, {7, 1}, {2, 3}, {3, 2}, {5, 4}, {8, 8}, {2048, 512}, {1024, 256}, {1242, 448}, {375, 128},
                          {530, 224}, {500, 224}, {1, 4096}, {1 << 20, 3}, {3, 1 << 16}};
  int n = 0;
  for (const auto &p : pairs) {
    const int S = p[0], D = p[1];
    std::vector<int> ofs(D);
    std::vector<short> coef((size_t)D * 4);
    CHECK(ra_resize_cubic_tables(S, D, ofs.data(), coef.data()) == 0);
    for (int d = 0; d < D; ++d) {
      const int sum = coef[4 * d] + coef[4 * d + 1] + coef[4 * d + 2] + coef[4 * d + 3];
      CHECK(sum >= 2047 && sum <= 2049);
      CHECK(ofs[d] >= -1 && ofs[d] <= S - 1);       // f lies in [-0.5, S - 0.5)
      CHECK(d == 0 || ofs[d] >= ofs[d - 1]);        // non-decreasing
      if (S == D) CHECK(ofs[d] == d && coef[4 * d + 1] == 2048 && sum == 2048);
    }
    ++n;
  }
  int one = 0;
  short four[4];
  CHECK(ra_resize_cubic_tables(0, 1, &one, four) == RA_E_SHAPE);
  CHECK(ra_resize_cubic_tables(1, 0, &one, four) == RA_E_SHAPE);
  CHECK(ra_resize_cubic_tables(-3, 1, &one, four) == RA_E_SHAPE);
  CHECK(ra_resize_cubic_tables(1, 1, nullptr, four) == RA_E_SHAPE);
  CHECK(ra_resize_cubic_tables(1, 1, &one, nullptr) == RA_E_SHAPE);
  CHECK(ra_resize_cubic_u8(nullptr, 1, 8, 8, 3, 4, 4, &one, four, &one, four, nullptr, nullptr, nullptr) == RA_E_SHAPE);  // before any GPU call
  printf("tables: %d (S, D) pairs, 6 refusals\n", n);
}

int main() {
  check_unfilter();
  check_tables();
  printf(failures ? "image_host_check: %d check(s) FAILED\n" : "image_host_check: all checks held\n", failures);
  return failures ? 1 : 0;
}
