// AddressSanitizer / UBSan harness for the depth-map loader (rtxn_load_png_gray16, rtx_nerf_amd/csrc/loader.cpp).  Built by
// tests/test_depth_loader_sanitized.py with
//   g++ -fsanitize=address,undefined -fno-sanitize-recover=undefined  loader.cpp depth_png_fuzz.cpp -lz
// It writes valid gray PNGs of 16 and 8 bits, plain and Adam7-interlaced, with every row filter, checks that they load to the
// values written, then loads `iters` damaged copies: bits flipped, bytes overwritten, files truncated, header fields (size, bit
// depth, colour type, interlace) set to other values.  Every load must return -- RTXN_OK or an error code -- without a sanitizer
// report; a load that succeeds must hand back width * height values (they are read end to end), one that fails no buffer.
//   depth_png_fuzz <dir> <iters> <seed>
#include <zlib.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rtxn.h"

// librtxn's error sink lives in common.hip beside a kernel; the harness links its own
namespace rtxn {
static char g_err[512];
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
}  // namespace rtxn

namespace {
uint64_t g_state;
uint64_t rnd() {   // xorshift64*
  g_state ^= g_state >> 12;
  g_state ^= g_state << 25;
  g_state ^= g_state >> 27;
  return g_state * 2685821657736338717ull;
}
void spit(const std::string& p, const std::vector<unsigned char>& v) {
  FILE* f = fopen(p.c_str(), "wb");
  if (!f) { perror(p.c_str()); exit(2); }
  if (!v.empty()) fwrite(v.data(), 1, v.size(), f);
  fclose(f);
}
void put32(std::vector<unsigned char>& v, uint32_t x) { for (int b = 3; b >= 0; --b) v.push_back((unsigned char)(x >> (8 * b))); }
void chunk(std::vector<unsigned char>& png, const char* type, const std::vector<unsigned char>& body) {
  put32(png, (uint32_t)body.size());
  const size_t at = png.size();
  png.insert(png.end(), type, type + 4);
  png.insert(png.end(), body.begin(), body.end());
  put32(png, (uint32_t)crc32(0, png.data() + at, (uInt)(png.size() - at)));
}
int paeth(int a, int b, int c) {
  const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
  return (pa <= pb && pa <= pc) ? a : pb <= pc ? b : c;
}
// one pass of a gray image as filtered scanlines; filter: 0 .. 4, or -1 for a random one per row
void add_pass(std::vector<unsigned char>& raw, const std::vector<uint16_t>& v, int w, int depth, int x0, int y0, int dx, int dy, int pw,
              int ph, int filter) {
  if (pw <= 0 || ph <= 0) return;
  const size_t bpp = depth / 8, stride = (size_t)pw * bpp;
  std::vector<unsigned char> prev(stride, 0), row(stride);
  for (int y = 0; y < ph; ++y) {
    for (int x = 0; x < pw; ++x) {
      const uint16_t s = v[(size_t)(y0 + y * dy) * w + (x0 + x * dx)];
      if (depth == 16) { row[2 * x] = (unsigned char)(s >> 8); row[2 * x + 1] = (unsigned char)s; }
      else row[x] = (unsigned char)s;
    }
    const int ft = filter < 0 ? (int)(rnd() % 5) : filter;
    raw.push_back((unsigned char)ft);
    for (size_t i = 0; i < stride; ++i) {
      const int a = i >= bpp ? row[i - bpp] : 0, b = prev[i], c = i >= bpp ? prev[i - bpp] : 0;
      const int pred = ft == 0 ? 0 : ft == 1 ? a : ft == 2 ? b : ft == 3 ? (a + b) >> 1 : paeth(a, b, c);
      raw.push_back((unsigned char)(row[i] - pred));
    }
    prev = row;
  }
}
std::vector<unsigned char> gray_png(const std::vector<uint16_t>& v, int w, int h, int depth, bool interlace, int filter, int ctype = 0) {
  std::vector<unsigned char> png = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'}, ihdr, raw;
  put32(ihdr, (uint32_t)w);
  put32(ihdr, (uint32_t)h);
  ihdr.push_back((unsigned char)depth);
  ihdr.push_back((unsigned char)ctype);
  ihdr.push_back(0);
  ihdr.push_back(0);
  ihdr.push_back(interlace ? 1 : 0);
  chunk(png, "IHDR", ihdr);
  if (interlace) {
    static const int x0[] = {0, 4, 0, 2, 0, 1, 0}, y0[] = {0, 0, 4, 0, 2, 0, 1}, dx[] = {8, 8, 4, 4, 2, 2, 1}, dy[] = {8, 8, 8, 4, 4, 2, 2};
    for (int p = 0; p < 7; ++p)
      add_pass(raw, v, w, depth, x0[p], y0[p], dx[p], dy[p], (w - x0[p] + dx[p] - 1) / dx[p], (h - y0[p] + dy[p] - 1) / dy[p], filter);
  } else add_pass(raw, v, w, depth, 0, 0, 1, 1, w, h, filter);
  uLongf zn = compressBound((uLong)raw.size());
  std::vector<unsigned char> z(zn);
  compress(z.data(), &zn, raw.data(), (uLong)raw.size());
  z.resize(zn);
  chunk(png, "IDAT", z);
  chunk(png, "IEND", {});
  return png;
}
void mutate(std::vector<unsigned char>& v) {
  if (v.empty()) return;
  switch ((int)(rnd() % 6)) {
    case 0: for (int k = 0, n = 1 + (int)(rnd() % 4); k < n; ++k) v[rnd() % v.size()] ^= (unsigned char)(1u << (rnd() % 8)); break;
    case 1: for (int k = 0, n = 1 + (int)(rnd() % 8); k < n; ++k) v[rnd() % v.size()] = (unsigned char)rnd(); break;
    case 2: v.resize(rnd() % v.size()); break;                                                    // truncated
    case 3: if (v.size() > 29) v[16 + rnd() % 13] = (unsigned char)rnd(); break;                  // a byte of IHDR's body
    case 4: { static const unsigned char dep[] = {1, 2, 4, 8, 16, 3, 0}, ct[] = {0, 2, 3, 4, 6, 1, 7};   // another depth / colour type
              if (v.size() > 26) { if (rnd() & 1) v[24] = dep[rnd() % 7]; else v[25] = ct[rnd() % 7]; } } break;
    default: for (int k = 0, n = (int)(rnd() % 64); k < n; ++k) v.push_back((unsigned char)rnd()); break;   // trailing bytes
  }
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 4) { fprintf(stderr, "usage: depth_png_fuzz <dir> <iters> <seed>\n"); return 2; }
  const std::string path = std::string(argv[1]) + "/depth.png";
  const int iters = atoi(argv[2]);
  g_state = 0x9E3779B97F4A7C15ull ^ (uint64_t)atoll(argv[3]);
  // ---- valid files: every (depth, interlace, filter) loads to the values written
  std::vector<std::vector<unsigned char>> valid;
  for (int depth : {16, 8})
    for (int interlace = 0; interlace < 2; ++interlace)
      for (int filter = -1; filter < 5; ++filter) {
        const int w = 1 + (int)(rnd() % 19), h = 1 + (int)(rnd() % 13);
        std::vector<uint16_t> v((size_t)w * h);
        for (auto& s : v) s = (uint16_t)(depth == 16 ? rnd() : rnd() & 255);
        valid.push_back(gray_png(v, w, h, depth, interlace != 0, filter));
        spit(path, valid.back());
        int gw = 0, gh = 0;
        uint16_t* got = nullptr;
        if (rtxn_load_png_gray16(path.c_str(), &gw, &gh, &got) != RTXN_OK || gw != w || gh != h || memcmp(got, v.data(), v.size() * 2)) {
          fprintf(stderr, "a valid %d-bit depth map (interlace %d, filter %d) does not load to its values: %s\n", depth, interlace, filter, rtxn::g_err);
          return 2;
        }
        rtxn_free_png_gray16(got);
      }
  // ---- damaged copies
  int ok = 0, rejected = 0;
  double sink = 0;
  for (int it = 0; it < iters; ++it) {
    std::vector<unsigned char> bad = valid[rnd() % valid.size()];
    for (int k = 0, n = 1 + (int)(rnd() % 3); k < n; ++k) mutate(bad);
    spit(path, bad);
    int w = -1, h = -1;
    uint16_t* got = nullptr;
    const int rc = rtxn_load_png_gray16(path.c_str(), &w, &h, &got);
    if (rc == RTXN_OK) {
      if (!got || w < 1 || h < 1) { fprintf(stderr, "iteration %d: an accepted load without values\n", it); return 1; }
      for (size_t i = 0; i < (size_t)w * h; ++i) sink += got[i];
      ++ok;
      rtxn_free_png_gray16(got);
    } else {
      ++rejected;
      if (got || w != 0 || h != 0) { fprintf(stderr, "iteration %d: a failed load left a buffer or a size behind\n", it); return 1; }
    }
  }
  printf("depth_png_fuzz: %d corrupted loads, %d accepted, %d rejected, no sanitizer report (checksum %g)\n", iters, ok, rejected, sink);
  return 0;
}
