// host_fuzz_main.cpp — a stand-alone program over the host-only sources (csrc/host_io.cpp, host_scene.cpp, host_debug.cpp,
// blas_builder.cpp; normals_plan.cpp and morph_plan.cpp to link) for the host sanitizer builds of tests/test_host_sanitized.py.
//
//   host_fuzz_main <section> <seed> [hashes]       sections: hdr png pfm resize scene blas debug threads
//
// Every input is generated from the seed (splitmix64): no corpus, no clock.  Every output buffer is a heap allocation of exactly the
// stated capacity, pre-filled with a sentinel, so that an overrun is the sanitizer's to see and "written completely" / "not touched" are
// the program's.  Every check is a property with a ground truth computed here.  Files are written into the current directory.
// Prints "<section>: ok <cases>" and returns 0; a broken property prints the section, the case number and the seed and returns 1.
// With a third argument the blas section also prints one line "blas hash <case> <fnv64 of the BlasResult>" per successful build.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <string>
#include <thread>
#include <vector>

#include "../include/urt.h"
#include "../include/urt_math.h"
#include "../unityraytracer_amd/csrc/blas_builder.h"

namespace {

const char* g_section = "?";
uint64_t g_seed = 0;
int g_case = 0;
std::atomic<int> g_failures{0};
bool g_hashes = false;

#define EXPECT(cond)                                                                                                                   \
  do {                                                                                                                                 \
    if (!(cond)) {                                                                                                                     \
      if (g_failures.fetch_add(1) < 20) std::printf("FAILED %s case %d seed %llu: %s (line %d)\n", g_section, g_case, (unsigned long long)g_seed, #cond, __LINE__); \
    }                                                                                                                                  \
  } while (0)

struct Rng {
  uint64_t s;
  explicit Rng(uint64_t seed) : s(seed) {}
  uint64_t next() {                                    // splitmix64
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
  }
  int below(int n) { return (int)(next() % (uint64_t)n); }
  float unit() { return (float)(next() >> 40) * (1.0f / 16777216.0f); }          // [0, 1)
  float range(float a, float b) { return a + (b - a) * unit(); }
  float grid(int half, float step) { return (float)(below(2 * half + 1) - half) * step; }
};

inline uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
inline float from_bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
const uint32_t kSentinel = 0xffc0ffeeu;                 // a NaN no function here produces
const float kInf = std::numeric_limits<float>::infinity();
const float kNaN = std::numeric_limits<float>::quiet_NaN();

// an exact-size heap array of floats filled with the sentinel
struct FloatBuf {
  float* p; size_t n;
  explicit FloatBuf(size_t n_) : p(n_ ? new float[n_] : nullptr), n(n_) { for (size_t i = 0; i < n; i++) p[i] = from_bits(kSentinel); }
  ~FloatBuf() { delete[] p; }
  FloatBuf(const FloatBuf&) = delete; FloatBuf& operator=(const FloatBuf&) = delete;
  bool untouched(size_t from = 0) const { for (size_t i = from; i < n; i++) if (bits(p[i]) != kSentinel) return false; return true; }
  bool all_written(size_t upto) const { for (size_t i = 0; i < upto; i++) if (bits(p[i]) == kSentinel) return false; return true; }
};
// the same for node records: every byte 0xA5
struct NodeBuf {
  urt_BVHNode* p; size_t n;
  explicit NodeBuf(size_t n_) : p(n_ ? new urt_BVHNode[n_] : nullptr), n(n_) { if (n) std::memset(p, 0xA5, n * sizeof(urt_BVHNode)); }
  ~NodeBuf() { delete[] p; }
  NodeBuf(const NodeBuf&) = delete; NodeBuf& operator=(const NodeBuf&) = delete;
  bool untouched(size_t from = 0) const {
    const unsigned char* b = (const unsigned char*)p;
    for (size_t i = from * sizeof(urt_BVHNode); i < n * sizeof(urt_BVHNode); i++) if (b[i] != 0xA5) return false;
    return true;
  }
};

bool write_file(const std::string& path, const std::vector<unsigned char>& data) {
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  bool ok = data.empty() || std::fwrite(data.data(), 1, data.size(), f) == data.size();
  std::fclose(f);
  return ok;
}
bool read_file(const std::string& path, std::vector<unsigned char>& data) {
  data.clear();
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) return false;
  unsigned char buf[65536];
  size_t n;
  while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) data.insert(data.end(), buf, buf + n);
  std::fclose(f);
  return true;
}
void append(std::vector<unsigned char>& v, const std::string& s) { v.insert(v.end(), s.begin(), s.end()); }

inline bool never(const char*) { return false; }      // EXPECT(never("what went wrong"))

// ======================================================================================================================= hdr ====
struct HdrFile {
  std::vector<unsigned char> bytes;
  size_t header_end = 0, first_scan_end = 0;
  int w = 0, h = 0;
  std::vector<float> expect;                           // w * h * 4, row 0 = bottom
};

unsigned char pick_exponent(Rng& r) {
  static const unsigned char k[4] = {0, 1, 128, 255};
  return r.below(3) ? k[r.below(4)] : (unsigned char)r.below(256);
}

// expected pixel: mantissa * 2^(e - 136) in double (exact; every such value is a float), alpha 1; e == 0 is black
void rgbe_expect(const unsigned char* p, float* out) {
  for (int c = 0; c < 3; c++) out[c] = p[3] == 0 ? 0.0f : (float)std::ldexp((double)p[c], (int)p[3] - 136);
  out[3] = 1.0f;
}

HdrFile make_hdr(Rng& r, int w, int h, bool minus_y, bool rle, const std::string& extra_header = "") {
  HdrFile f; f.w = w; f.h = h;
  append(f.bytes, "#?RADIANCE\n" + extra_header + "FORMAT=32-bit_rle_rgbe\n\n" + (minus_y ? "-Y " : "+Y ") + std::to_string(h) + " +X " + std::to_string(w) + "\n");
  f.header_end = f.bytes.size();
  f.expect.assign((size_t)w * h * 4, 0.0f);
  std::vector<unsigned char> px((size_t)w * 4);
  static const int kLens[3] = {1, 127, 128};
  for (int y = 0; y < h; y++) {
    if (rle) {                                         // new-style RLE, 8 <= w <= 32767: the encoding decides the pixels
      f.bytes.push_back(2); f.bytes.push_back(2); f.bytes.push_back((unsigned char)(w >> 8)); f.bytes.push_back((unsigned char)(w & 255));
      for (int ch = 0; ch < 4; ch++) {
        int x = 0;
        while (x < w) {
          const bool run = r.below(2) == 0;
          int n = r.below(4) ? kLens[r.below(3)] : 1 + r.below(128);
          if (run && n > 127) n = 127;
          n = std::min(n, w - x);
          if (run) {
            unsigned char v = ch == 3 ? pick_exponent(r) : (unsigned char)r.below(256);
            f.bytes.push_back((unsigned char)(128 + n)); f.bytes.push_back(v);
            for (int k = 0; k < n; k++) px[(size_t)(x++) * 4 + ch] = v;
          } else {
            f.bytes.push_back((unsigned char)n);
            for (int k = 0; k < n; k++) {
              unsigned char v = ch == 3 ? pick_exponent(r) : (unsigned char)r.below(256);
              f.bytes.push_back(v); px[(size_t)(x++) * 4 + ch] = v;
            }
          }
        }
      }
    } else {
      for (int x = 0; x < w; x++) { for (int c = 0; c < 3; c++) px[(size_t)x * 4 + c] = (unsigned char)r.below(256); px[(size_t)x * 4 + 3] = pick_exponent(r); }
      // a flat row that begins like an RLE header IS one where RLE applies; outside 8..32767 the same bytes are a pixel
      if (w < 8 || w > 32767) { px[0] = 2; px[1] = 2; px[2] = (unsigned char)(w >> 8); px[3] = (unsigned char)(w & 255); }
      else if (px[0] == 2 && px[1] == 2) px[0] = 3;
      f.bytes.insert(f.bytes.end(), px.begin(), px.end());
    }
    if (y == 0) f.first_scan_end = f.bytes.size();
    const int row = minus_y ? h - 1 - y : y;
    for (int x = 0; x < w; x++) rgbe_expect(&px[(size_t)x * 4], &f.expect[((size_t)row * w + x) * 4]);
  }
  return f;
}

// The contract of one file, whatever is in it.  expect: NULL (hostile: the contract alone), or the pixels a valid file must give.
// must_fail: the file cannot be a complete image (a strict prefix of one, a named malformation).  Returns the status of the full load.
int check_hdr(const char* path, const HdrFile* expect, bool must_fail) {
  int w = -7, h = -7;
  const int q = urt_host_load_hdr(path, &w, &h, nullptr, 0);
  EXPECT(q == URT_OK || q == URT_ERR_INVALID_ARGUMENT || q == URT_ERR_LAYOUT);
  if (q != URT_OK) {
    EXPECT(urt_host_io_last_error()[0] != 0);
    EXPECT(!expect);
    FloatBuf small(16);
    int w2 = 0, h2 = 0;
    EXPECT(urt_host_load_hdr(path, &w2, &h2, small.p, small.n) == q);           // the same verdict with a buffer, which stays untouched
    EXPECT(small.untouched());
    return q;
  }
  EXPECT(w >= 1 && h >= 1 && w <= 65536 && h <= 65536);
  if (expect) EXPECT(w == expect->w && h == expect->h);
  const size_t need = (size_t)w * (size_t)h * 4;
  {                                                                             // capacity one float short: refused, untouched
    FloatBuf shorter(need - 1 <= ((size_t)1 << 22) ? need - 1 : 64);            // (a header that promises more than this program allocates: far short)
    int w2 = 0, h2 = 0;
    const int rc = urt_host_load_hdr(path, &w2, &h2, shorter.p, shorter.n);
    EXPECT(rc == URT_ERR_INVALID_ARGUMENT && shorter.untouched() && urt_host_io_last_error()[0] != 0);
  }
  if (need > ((size_t)1 << 22)) return URT_ERR_INVALID_ARGUMENT;               // a header that promises more than this program allocates
  FloatBuf out(need);
  int w2 = 0, h2 = 0;
  const int rc = urt_host_load_hdr(path, &w2, &h2, out.p, need);
  EXPECT(rc == URT_OK || rc == URT_ERR_LAYOUT);
  EXPECT(w2 == w && h2 == h);
  if (must_fail) EXPECT(rc != URT_OK);
  if (rc == URT_OK) {
    EXPECT(out.all_written(need));
    for (size_t i = 3; i < need; i += 4) if (bits(out.p[i]) != 0x3f800000u) { EXPECT(never("alpha is 1")); break; }
    if (expect) EXPECT(std::memcmp(out.p, expect->expect.data(), need * sizeof(float)) == 0);
  } else {
    EXPECT(urt_host_io_last_error()[0] != 0);
    EXPECT(!expect);
  }
  return rc;
}

int check_hdr_bytes(const std::vector<unsigned char>& bytes, const HdrFile* expect, bool must_fail) {
  EXPECT(write_file("fuzz.hdr", bytes));
  return check_hdr("fuzz.hdr", expect, must_fail);
}

void section_hdr(Rng& r) {
  static const int kWidths[9] = {1, 7, 8, 9, 127, 128, 129, 32767, 32768};
  for (int wi = 0; wi < 9; wi++)
    for (int h = 1; h <= 3; h++)
      for (int style = 0; style < 2; style++) {
        const int w = kWidths[wi];
        const bool rle = style == 1;
        if (rle && (w < 8 || w > 32767)) continue;
        if (w >= 32767 && h == 2) continue;                                    // the big rows: heights 1 and 3
        g_case++;
        HdrFile f = make_hdr(r, w, h, r.below(2) == 0, rle);
        EXPECT(check_hdr_bytes(f.bytes, &f, false) == URT_OK);
      }
  // a header line of 4096 bytes is read, one of 4097 is not
  for (int len = 4096; len <= 4097; len++) {
    g_case++;
    HdrFile f = make_hdr(r, 9, 2, true, true, "#" + std::string((size_t)len - 1, 'a') + "\n");
    if (len == 4096) EXPECT(check_hdr_bytes(f.bytes, &f, false) == URT_OK);
    else EXPECT(check_hdr_bytes(f.bytes, nullptr, true) == URT_ERR_LAYOUT);
  }
  // hostile variants of small files
  for (int round = 0; round < 16; round++) {
    HdrFile f = make_hdr(r, round % 4 < 2 ? 9 : 3, 2, round % 2 == 0, round % 4 < 2);
    EXPECT(f.bytes.size() <= 256);
    for (size_t cut = 0; cut < f.bytes.size(); cut++) {                         // every strict prefix
      g_case++;
      std::vector<unsigned char> t(f.bytes.begin(), f.bytes.begin() + (long)cut);
      check_hdr_bytes(t, nullptr, true);
    }
    for (size_t at = 0; at < f.first_scan_end; at++) {                          // every single-byte change up to the end of scanline 0
      g_case++;
      std::vector<unsigned char> t = f.bytes;
      t[at] ^= (unsigned char)(1 + r.below(255));
      check_hdr_bytes(t, nullptr, false);
    }
  }
  {
    auto with_resolution = [&](const std::string& line, const std::vector<unsigned char>& body) {
      std::vector<unsigned char> b;
      append(b, "#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n" + line + "\n");
      b.insert(b.end(), body.begin(), body.end());
      return b;
    };
    const std::vector<unsigned char> one = {11, 20, 30, 128};
    static const char* kBad[] = {"-Y 0 +X 1", "-Y 1 +X 0", "-Y -1 +X 1", "-Y 1 +X -1", "-Y 1 +X 65537", "-Y 65537 +X 1", "-Y 1 +X 99999999999",
                                 "-Y 99999999999 +X 1", "+Y 1 -X 1", "-Y 1 -X 1", "-X 1 +Y 1", "", "-Y 1", "Y 1 X 1"};
    for (const char* line : kBad) { g_case++; EXPECT(check_hdr_bytes(with_resolution(line, one), nullptr, true) == URT_ERR_LAYOUT); }
    g_case++;                                                                   // 65536 is the largest size: the header is taken, the pixels are missing
    EXPECT(check_hdr_bytes(with_resolution("-Y 1 +X 65536", one), nullptr, true) == URT_ERR_LAYOUT);
    g_case++;
    EXPECT(check_hdr_bytes(with_resolution("-Y 65536 +X 65536", one), nullptr, true) == URT_ERR_INVALID_ARGUMENT);
    g_case++;                                                                   // a resolution line that ends the file without a newline
    {
      std::vector<unsigned char> b; append(b, "#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y 1 +X 1");
      check_hdr_bytes(b, nullptr, true);
      b.insert(b.end(), one.begin(), one.end());                                // ... and "1" followed by pixel bytes is no line at all or a truncated image
      check_hdr_bytes(b, nullptr, true);
    }
    g_case++;
    { std::vector<unsigned char> b; append(b, "#?RADIANCE"); EXPECT(check_hdr_bytes(b, nullptr, true) == URT_ERR_LAYOUT); }
    g_case++;
    { std::vector<unsigned char> b; append(b, "#?RADIANCE\n\n-Y 1 +X 1\n"); b.insert(b.end(), one.begin(), one.end()); EXPECT(check_hdr_bytes(b, nullptr, true) == URT_ERR_LAYOUT); }   // no FORMAT line
    g_case++;
    { std::vector<unsigned char> b; append(b, "RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y 1 +X 1\n"); b.insert(b.end(), one.begin(), one.end()); EXPECT(check_hdr_bytes(b, nullptr, true) == URT_ERR_LAYOUT); }
    g_case++;
    EXPECT(check_hdr_bytes(std::vector<unsigned char>(), nullptr, true) == URT_ERR_LAYOUT);                      // an empty file
    g_case++;
    { const int rc = check_hdr(".", nullptr, true); EXPECT(rc == URT_ERR_LAYOUT || rc == URT_ERR_INVALID_ARGUMENT); }   // a directory
    g_case++;
    { const int rc = check_hdr("no/such/file.hdr", nullptr, true); EXPECT(rc == URT_ERR_INVALID_ARGUMENT); }
    g_case++;
    { int w = 0, h = 0; EXPECT(urt_host_load_hdr(nullptr, &w, &h, nullptr, 0) == URT_ERR_INVALID_ARGUMENT); EXPECT(urt_host_load_hdr("fuzz.hdr", nullptr, &h, nullptr, 0) == URT_ERR_INVALID_ARGUMENT); }
    // runs and literals that overrun the width by one, and a literal of count 0
    const int w = 9;
    auto rle_row = [&](const std::vector<unsigned char>& first_channel) {
      std::vector<unsigned char> b = {2, 2, 0, (unsigned char)w};
      b.insert(b.end(), first_channel.begin(), first_channel.end());
      for (int ch = 1; ch < 4; ch++) { b.push_back((unsigned char)(128 + w)); b.push_back(77); }
      return b;
    };
    const std::string res = "-Y 1 +X 9";
    g_case++;
    EXPECT(check_hdr_bytes(with_resolution(res, rle_row({(unsigned char)(128 + w), 5})), nullptr, false) == URT_OK);                    // exact: fine
    g_case++;
    EXPECT(check_hdr_bytes(with_resolution(res, rle_row({(unsigned char)(128 + w + 1), 5})), nullptr, true) == URT_ERR_LAYOUT);         // run of w + 1
    g_case++;
    EXPECT(check_hdr_bytes(with_resolution(res, rle_row({(unsigned char)(128 + w - 1), 5, (unsigned char)(128 + 2), 5})), nullptr, true) == URT_ERR_LAYOUT);
    g_case++;
    { std::vector<unsigned char> lit = {(unsigned char)(w + 1)}; for (int k = 0; k < w + 1; k++) lit.push_back((unsigned char)k);
      EXPECT(check_hdr_bytes(with_resolution(res, rle_row(lit)), nullptr, true) == URT_ERR_LAYOUT); }                                 // literal of w + 1
    g_case++;
    EXPECT(check_hdr_bytes(with_resolution(res, rle_row({0, (unsigned char)(128 + w), 5})), nullptr, true) == URT_ERR_LAYOUT);          // literal count 0
  }
}

// ================================================================================================================ png / pfm ====
uint32_t crc32_bitwise(const unsigned char* p, size_t n) {
  uint32_t c = 0xffffffffu;
  for (size_t i = 0; i < n; i++) { c ^= p[i]; for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u))); }
  return ~c;
}
uint32_t be32(const unsigned char* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

// specials, both sides of every sRGB step, random values
std::vector<float> special_image(Rng& r, int w, int h) {
  float steps[256];
  EXPECT(urt_host_srgb8_first_floats(steps) == 0);
  std::vector<float> pool = {kNaN, -kNaN, kInf, -kInf, 0.0f, -0.0f, from_bits(1), from_bits(0x007fffff), from_bits(0x80000001u), -1.0f, -3e38f, 3e38f, 1.0f, from_bits(0x3f7fffff), from_bits(0x3f800001)};
  for (int k = 1; k < 256; k++) { pool.push_back(steps[k]); pool.push_back(from_bits(bits(steps[k]) - 1)); }
  std::vector<float> img((size_t)w * h * 4);
  size_t at = (size_t)r.below((int)pool.size());
  for (size_t i = 0; i < img.size(); i++) img[i] = r.below(3) ? pool[(at++) % pool.size()] : r.range(-0.25f, 1.25f);
  return img;
}

void check_step_table() {
  float steps[256];
  EXPECT(urt_host_srgb8_first_floats(steps) == 0);
  EXPECT(steps[0] == -kInf);
  for (int k = 1; k < 256; k++) {
    const float px[8] = {steps[k], from_bits(bits(steps[k]) - 1), 0, 0.5f, 0, 0, 0, 0};
    unsigned char out[8] = {0};
    EXPECT(urt_host_encode_srgb8(px, 2, out) == 0);
    EXPECT(out[0] == k && out[1] == k - 1 && out[3] == 128);
    if (k > 1) EXPECT(steps[k] > steps[k - 1]);
  }
}

void section_png(Rng& r) {
  check_step_table();
  static const int kSizes[6][2] = {{1456, 15}, {1456, 30}, {1456, 16}, {1, 1}, {1, 65536}, {21845, 1}};
  for (int s = 0; s < 6; s++) {
    g_case++;
    const int w = kSizes[s][0], h = kSizes[s][1];
    std::vector<float> img = special_image(r, w, h);
    EXPECT(urt_host_write_png("fuzz.png", img.data(), w, h) == URT_OK);
    std::vector<unsigned char> f;
    EXPECT(read_file("fuzz.png", f));
    static const unsigned char kSig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    if (f.size() < 8 + 25 + 12 + 12 || std::memcmp(f.data(), kSig, 8) != 0) { EXPECT(never("signature")); continue; }
    size_t at = 8;
    std::vector<unsigned char> z;
    int n_chunks = 0; bool ended = false, bad = false;
    while (at + 12 <= f.size() && !ended) {
      const uint32_t len = be32(&f[at]);
      if (at + 12 + (size_t)len > f.size()) { bad = true; break; }
      const std::string tag((const char*)&f[at + 4], 4);
      EXPECT(be32(&f[at + 8 + len]) == crc32_bitwise(&f[at + 4], 4 + (size_t)len));
      if (n_chunks == 0) {
        EXPECT(tag == "IHDR" && len == 13);
        if (len == 13) { EXPECT(be32(&f[at + 8]) == (uint32_t)w && be32(&f[at + 12]) == (uint32_t)h); EXPECT(f[at + 16] == 8 && f[at + 17] == 2 && f[at + 18] == 0 && f[at + 19] == 0 && f[at + 20] == 0); }
      } else if (tag == "IDAT") z.insert(z.end(), f.begin() + (long)(at + 8), f.begin() + (long)(at + 8 + len));
      else if (tag == "IEND") { EXPECT(len == 0); ended = true; }
      else EXPECT(never("an unexpected chunk"));
      at += 12 + (size_t)len; n_chunks++;
    }
    EXPECT(!bad && ended && at == f.size());
    // zlib: stored blocks only
    const size_t raw_size = (size_t)h * (1 + 3 * (size_t)w);
    std::vector<unsigned char> raw;
    if (z.size() < 6) { EXPECT(never("zlib stream")); continue; }
    EXPECT(z[0] == 0x78 && ((z[0] << 8) | z[1]) % 31 == 0);
    size_t p = 2; bool final_seen = false;
    while (!final_seen && p + 5 <= z.size()) {
      const unsigned hdr = z[p], len = z[p + 1] | (z[p + 2] << 8), nlen = z[p + 3] | (z[p + 4] << 8);
      EXPECT((hdr & ~1u) == 0 && len == (~nlen & 0xffffu));
      if (p + 5 + len > z.size()) { bad = true; break; }
      raw.insert(raw.end(), z.begin() + (long)(p + 5), z.begin() + (long)(p + 5 + len));
      p += 5 + len;
      final_seen = (hdr & 1) != 0;
      if (!final_seen) EXPECT(len == 65535);                                    // every block but the last is full
      EXPECT(final_seen == (raw.size() == raw_size));                           // the final flag on the last block only
    }
    EXPECT(!bad && final_seen && raw.size() == raw_size && p + 4 == z.size());
    if (raw.size() != raw_size || p + 4 != z.size()) continue;
    uint32_t a = 1, b = 0;
    for (unsigned char c : raw) { a = (a + c) % 65521u; b = (b + a) % 65521u; }
    EXPECT(be32(&z[p]) == ((b << 16) | a));
    std::vector<unsigned char> codes((size_t)w * h * 4);
    EXPECT(urt_host_encode_srgb8(img.data(), (size_t)w * h, codes.data()) == 0);
    bool same = true;
    for (int y = 0; y < h && same; y++) {                                       // PNG row y is the image's row h - 1 - y
      const unsigned char* row = &raw[(size_t)y * (1 + 3 * (size_t)w)];
      if (row[0] != 0) same = false;
      for (int x = 0; x < w && same; x++) for (int c = 0; c < 3; c++) if (row[1 + 3 * x + c] != codes[((size_t)(h - 1 - y) * w + x) * 4 + c]) same = false;
    }
    EXPECT(same);
  }
  g_case++;
  const float one[4] = {0, 0, 0, 1};
  EXPECT(urt_host_write_png(nullptr, one, 1, 1) == URT_ERR_INVALID_ARGUMENT && urt_host_io_last_error()[0]);
  EXPECT(urt_host_write_png("fuzz.png", nullptr, 1, 1) == URT_ERR_INVALID_ARGUMENT);
  EXPECT(urt_host_write_png("fuzz.png", one, 0, 1) == URT_ERR_INVALID_ARGUMENT && urt_host_write_png("fuzz.png", one, 1, -1) == URT_ERR_INVALID_ARGUMENT);
  EXPECT(urt_host_write_png("no/such/dir/fuzz.png", one, 1, 1) == URT_ERR_INVALID_ARGUMENT && urt_host_io_last_error()[0]);
}

void section_pfm(Rng& r) {
  static const int kSizes[5][2] = {{1, 1}, {7, 5}, {1456, 3}, {1, 4099}, {21845, 1}};
  for (int s = 0; s < 5; s++) {
    g_case++;
    const int w = kSizes[s][0], h = kSizes[s][1];
    std::vector<float> img = special_image(r, w, h);
    EXPECT(urt_host_write_pfm("fuzz.pfm", img.data(), w, h) == URT_OK);
    std::vector<unsigned char> f;
    EXPECT(read_file("fuzz.pfm", f));
    const std::string head = "PF\n" + std::to_string(w) + " " + std::to_string(h) + "\n-1.0\n";
    EXPECT(f.size() == head.size() + (size_t)w * h * 12);
    if (f.size() != head.size() + (size_t)w * h * 12) continue;
    EXPECT(std::memcmp(f.data(), head.data(), head.size()) == 0);
    bool same = true;
    for (size_t px = 0; px < (size_t)w * h && same; px++)                       // bottom row first = the image's own order; little-endian floats
      for (int c = 0; c < 3; c++) {
        const unsigned char* q = &f[head.size() + (px * 3 + c) * 4];
        const uint32_t u = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
        if (u != bits(img[px * 4 + c])) same = false;
      }
    EXPECT(same);
  }
  g_case++;
  const float one[4] = {0, 0, 0, 1};
  EXPECT(urt_host_write_pfm(nullptr, one, 1, 1) == URT_ERR_INVALID_ARGUMENT && urt_host_io_last_error()[0]);
  EXPECT(urt_host_write_pfm("fuzz.pfm", nullptr, 1, 1) == URT_ERR_INVALID_ARGUMENT && urt_host_write_pfm("fuzz.pfm", one, 1, 0) == URT_ERR_INVALID_ARGUMENT);
  EXPECT(urt_host_write_pfm("no/such/dir/fuzz.pfm", one, 1, 1) == URT_ERR_INVALID_ARGUMENT && urt_host_io_last_error()[0]);
}

// ==================================================================================================================== resize ====
long double mitchell_ld(long double x) {
  x = std::fabs(x);
  const long double B = 1.0L / 3.0L, C = 1.0L / 3.0L;
  if (x < 1.0L) return ((12 - 9 * B - 6 * C) * x * x * x + (-18 + 12 * B + 6 * C) * x * x + (6 - 2 * B)) / 6.0L;
  if (x < 2.0L) return ((-B - 6 * C) * x * x * x + (6 * B + 30 * C) * x * x + (-12 * B - 48 * C) * x + (8 * B + 24 * C)) / 6.0L;
  return 0.0L;
}
// taps of output d along one axis: the header's definition (Mitchell B = C = 1/3, support widened by the scale, edges clamped,
// weights normalised) over the window floor(centre - support) .. ceil(centre + support)
struct Taps { int lo, hi; std::vector<long double> w; };
Taps taps_of(int n_src, int n_dst, int d) {
  const long double scale = (long double)n_src / (long double)n_dst, wide = std::max(1.0L, scale), support = 2.0L * wide;
  const long double centre = ((long double)d + 0.5L) * scale - 0.5L;
  Taps t; t.lo = (int)std::floor(centre - support); t.hi = (int)std::ceil(centre + support);
  long double sum = 0;
  for (int k = t.lo; k <= t.hi; k++) { t.w.push_back(mitchell_ld(((long double)k - centre) / wide)); sum += t.w.back(); }
  for (long double& v : t.w) v /= sum;
  return t;
}

double g_resize_worst = 0;      // largest error / tolerance seen on finite windows

void resize_case(Rng& r, int w, int h, int nw, int nh, bool specials) {
  g_case++;
  std::vector<float> src((size_t)w * h * 4);
  for (float& v : src) v = r.below(8) ? r.range(-4.0f, 4.0f) : r.range(-1000.0f, 1000.0f);
  if (specials) {
    static const float kSp[6] = {kNaN, kInf, -kInf, 3e38f, -3e38f, 0.0f};
    const int n = 1 + (int)(src.size() / 64);
    for (int k = 0; k < n; k++) src[(size_t)r.below((int)src.size())] = kSp[r.below(6)];
    src[(size_t)r.below((int)src.size())] = from_bits(1);                      // a denormal
  }
  FloatBuf dst((size_t)nw * nh * 4);
  EXPECT(urt_host_resize_rgba(src.data(), w, h, dst.p, nw, nh) == URT_OK);
  EXPECT(dst.all_written(dst.n));
  std::vector<Taps> tx, ty;
  for (int d = 0; d < nw; d++) tx.push_back(taps_of(w, nw, d));
  for (int d = 0; d < nh; d++) ty.push_back(taps_of(h, nh, d));
  auto clampi = [](int v, int n) { return std::min(std::max(v, 0), n - 1); };
  // pass 1 in long double: [h][nw][4]
  std::vector<long double> tmp((size_t)h * nw * 4, 0.0L);
  std::vector<char> tmp_finite((size_t)h * nw, 1);
  std::vector<long double> tmp_mag((size_t)h * nw, 0.0L);
  for (int y = 0; y < h; y++)
    for (int d = 0; d < nw; d++) {
      const Taps& t = tx[(size_t)d];
      for (int k = t.lo - 1; k <= t.hi + 1; k++) {                               // (a window one tap wider for the specials: a float centre may round outwards)
        const float* p = &src[((size_t)y * w + clampi(k, w)) * 4];
        for (int c = 0; c < 4; c++) {
          if (!std::isfinite(p[c]) || std::fabs(p[c]) > 1e30f) tmp_finite[(size_t)y * nw + d] = 0;
          else if (k >= t.lo && k <= t.hi) { tmp[((size_t)y * nw + d) * 4 + c] += t.w[(size_t)(k - t.lo)] * (long double)p[c]; tmp_mag[(size_t)y * nw + d] = std::max(tmp_mag[(size_t)y * nw + d], (long double)std::fabs(p[c])); }
        }
      }
    }
  for (int e = 0; e < nh; e++)
    for (int d = 0; d < nw; d++) {
      const Taps& t = ty[(size_t)e];
      long double acc[4] = {0, 0, 0, 0}, mag = 0;
      bool finite = true;
      for (int k = t.lo - 1; k <= t.hi + 1; k++) {
        const size_t at = (size_t)clampi(k, h) * nw + d;
        if (!tmp_finite[at]) finite = false;
        if (k < t.lo || k > t.hi) continue;
        mag = std::max(mag, tmp_mag[at]);
        for (int c = 0; c < 4; c++) acc[c] += t.w[(size_t)(k - t.lo)] * tmp[at * 4 + c];
      }
      if (!finite) continue;                                                   // a special in the window: written (above), no value claimed
      // one rounding per multiply-add of a normalised sum, in each of the two passes: (taps_x + taps_y) * 2^-23 * largest |tap value|
      const long double tol = (long double)(tx[(size_t)d].w.size() + t.w.size()) * 0x1p-23L * mag;
      for (int c = 0; c < 4; c++) {
        const long double err = std::fabs((long double)dst.p[((size_t)e * nw + d) * 4 + c] - acc[c]);
        if (!(err <= tol)) { EXPECT(never("resize: beyond (taps) * 2^-23 * max |tap|")); std::printf("  %dx%d -> %dx%d texel (%d, %d) c %d: got %.9g want %.9Lg err %.3Lg tol %.3Lg\n", w, h, nw, nh, d, e, c, (double)dst.p[((size_t)e * nw + d) * 4 + c], acc[c], err, tol); return; }
        if (tol > 0) g_resize_worst = std::max(g_resize_worst, (double)(err / tol));
      }
    }
}

void section_resize(Rng& r) {
  static const int kShapes[][4] = {{1, 1, 1, 1}, {1, 1, 4096, 1}, {1, 1, 1, 4096}, {4096, 1, 1, 1}, {1, 4096, 1, 1}, {3, 3, 2, 2}, {2, 2, 3, 3}, {7, 5, 5, 7},
                                   {5, 7, 7, 5}, {4096, 2, 2048, 1}, {2, 4096, 1, 2048}, {2048, 3, 2048, 2}, {2049, 1, 2048, 1}, {4097, 2, 2048, 1}, {1, 3000, 1, 2048}};
  for (const auto& s : kShapes)
    for (int specials = 0; specials < 2; specials++) resize_case(r, s[0], s[1], s[2], s[3], specials != 0);
  for (int k = 0; k < 120; k++) resize_case(r, 1 + r.below(40), 1 + r.below(40), 1 + r.below(40), 1 + r.below(40), k % 2 != 0);
  g_case++;
  const float one[4] = {1, 2, 3, 4};
  FloatBuf d(4);
  EXPECT(urt_host_resize_rgba(nullptr, 1, 1, d.p, 1, 1) == URT_ERR_INVALID_ARGUMENT && urt_host_io_last_error()[0]);
  EXPECT(urt_host_resize_rgba(one, 1, 1, nullptr, 1, 1) == URT_ERR_INVALID_ARGUMENT);
  EXPECT(urt_host_resize_rgba(one, 0, 1, d.p, 1, 1) == URT_ERR_INVALID_ARGUMENT && urt_host_resize_rgba(one, 1, -1, d.p, 1, 1) == URT_ERR_INVALID_ARGUMENT);
  EXPECT(urt_host_resize_rgba(one, 1, 1, d.p, 0, 1) == URT_ERR_INVALID_ARGUMENT && urt_host_resize_rgba(one, 1, 1, d.p, 1, 0) == URT_ERR_INVALID_ARGUMENT);
  EXPECT(d.untouched());
  std::printf("resize: largest error / tolerance = %.4f\n", g_resize_worst);
}

// ===================================================================================================================== scene ====
struct Scene {
  std::vector<urt_MeshObject> mo;
  std::vector<float> v;
  std::vector<int32_t> idx;
  int nv() const { return (int)v.size() / 3; }
};

void random_matrix(Rng& r, float* m) {
  for (int k = 0; k < 16; k++) m[k] = 0;
  for (int c = 0; c < 3; c++) for (int row = 0; row < 3; row++) m[c * 4 + row] = (c == row ? 1.0f : 0.0f) + r.grid(4, 0.125f);
  for (int row = 0; row < 3; row++) m[12 + row] = r.grid(20, 0.25f);
  m[15] = 1;
}

// meshes over consecutive ranges of whole triangles; `overlap`: ranges anywhere, empty ones included
Scene random_scene(Rng& r, int n_meshes, int tris_each_max, bool overlap) {
  Scene s;
  const int nv = 3 + r.below(40);
  for (int i = 0; i < nv * 3; i++) s.v.push_back(r.grid(8, 0.5f));
  std::vector<int> tris((size_t)n_meshes);
  int total = 0;
  for (int& t : tris) { t = r.below(tris_each_max + 1); total += t; }
  if (total == 0) { tris[0] = 1; total = 1; }
  for (int i = 0; i < total * 3; i++) s.idx.push_back(r.below(nv));
  int at = 0;
  for (int m = 0; m < n_meshes; m++) {
    urt_MeshObject o; std::memset(&o, 0, sizeof o);
    random_matrix(r, o.localToWorldMatrix);
    if (overlap) { const int t0 = r.below(total + 1), tn = r.below(total - t0 + 1); o.indices_offset = 3 * t0; o.indices_count = 3 * tn; }
    else { o.indices_offset = 3 * at; o.indices_count = 3 * tris[(size_t)m]; at += tris[(size_t)m]; }
    s.mo.push_back(o);
  }
  return s;
}

void point3x4(const float* m, const float* p, float* out) {                     // MultiplyPoint3x4: rows left to right, mul then add
  for (int row = 0; row < 3; row++) out[row] = m[row] * p[0] + m[4 + row] * p[1] + m[8 + row] * p[2] + m[12 + row];
}

// SetupBVHLeaves(List<MeshObject>) restated: a plain min / max loop, std::min(lo, t) / std::max(hi, t) in that argument order
bool leaf_bounds_ref(const Scene& s, int literal, std::vector<urt_BVHNode>& out) {
  out.assign(s.mo.size(), urt_BVHNode());
  for (size_t m = 0; m < s.mo.size(); m++) {
    const urt_MeshObject& o = s.mo[m];
    const long off = o.indices_offset, cnt = o.indices_count;
    urt_BVHNode& n = out[m];
    n.index = (int32_t)m;
    long first = off;
    if (literal) first = 0;                                                     // seeded from _indices[0] through this mesh's matrix ...
    else if (cnt == 0) { std::memset(&n, 0, sizeof n); n.index = (int32_t)m; continue; }
    float lo[3], hi[3];
    point3x4(o.localToWorldMatrix, &s.v[3 * (size_t)s.idx[(size_t)first]], lo);
    std::memcpy(hi, lo, sizeof lo);
    for (long i = off + 1; i < off + cnt; i++) {                                // ... and refined from offset + 1 on
      float t[3];
      point3x4(o.localToWorldMatrix, &s.v[3 * (size_t)s.idx[(size_t)i]], t);
      for (int k = 0; k < 3; k++) { lo[k] = std::min(lo[k], t[k]); hi[k] = std::max(hi[k], t[k]); }
    }
    for (int k = 0; k < 3; k++) { n.vmin[k] = lo[k]; n.vmax[k] = hi[k]; }
  }
  return true;
}

long long heap_length_ref(long long n) {
  if (n <= 0) return 0;
  long long depth = 1;
  while ((1ll << (depth - 1)) < n) depth++;
  const long long len = (1ll << depth) - 1;
  return len > 0x7fffffffll ? -1 : len;
}

// the heap contract: fillers all-zero with index -1; a node that names an object is that object's leaf, bit for bit; every other node
// is the union (over both corners: leaves may be inverted) of its two children.  exactly_once: every leaf index exactly once (the
// median builder); the pairing builder also copies a lone tree's root onto an interior position
void check_heap(const urt_BVHNode* leaves, int n, const urt_BVHNode* heap, int len, bool exactly_once, bool finite) {
  std::vector<int> seen((size_t)n, 0);
  urt_BVHNode zero; std::memset(&zero, 0, sizeof zero); zero.index = -1;
  auto filler = [&](int i) { return i >= len || std::memcmp(&heap[i], &zero, sizeof zero) == 0; };
  for (int i = 0; i < len; i++) {
    const urt_BVHNode& nd = heap[i];
    if (nd.index >= 0) {
      EXPECT(nd.index < n);
      if (nd.index < n) { seen[(size_t)nd.index]++; EXPECT(std::memcmp(&nd, &leaves[nd.index], sizeof nd) == 0); }
      continue;
    }
    EXPECT(nd.index == -1);
    if (filler(i)) { EXPECT(filler(2 * i + 1) && filler(2 * i + 2)); continue; }
    if (!exactly_once && !filler(2 * i + 1) && filler(2 * i + 2)) {            // the pairing joins a lone tree with nothing, under a copy of its root
      EXPECT(std::memcmp(nd.vmin, heap[2 * i + 1].vmin, 24) == 0);
      continue;
    }
    EXPECT(!filler(2 * i + 1) && !filler(2 * i + 2));
    if (filler(2 * i + 1) || filler(2 * i + 2) || !finite) continue;
    const urt_BVHNode &a = heap[2 * i + 1], &b = heap[2 * i + 2];
    for (int k = 0; k < 3; k++) {
      EXPECT(nd.vmin[k] == std::min(std::min(a.vmin[k], a.vmax[k]), std::min(b.vmin[k], b.vmax[k])));
      EXPECT(nd.vmax[k] == std::max(std::max(a.vmin[k], a.vmax[k]), std::max(b.vmin[k], b.vmax[k])));
    }
  }
  for (int c : seen) EXPECT(exactly_once ? c == 1 : c >= 1);
}

std::vector<urt_BVHNode> random_leaves(Rng& r, int n) {
  std::vector<urt_BVHNode> lv((size_t)n);
  const bool clustered = r.below(3) == 0;
  for (int i = 0; i < n; i++) {
    for (int k = 0; k < 3; k++) {
      const float c = clustered ? r.grid(2, 1.0f) : r.range(-50.0f, 50.0f), e = r.range(0.01f, 3.0f);
      lv[(size_t)i].vmin[k] = c - e; lv[(size_t)i].vmax[k] = c + e;
    }
    if (r.below(4) == 0) for (int k = 0; k < 3; k++) std::swap(lv[(size_t)i].vmin[k], lv[(size_t)i].vmax[k]);   // an inverted (sphere) box
    lv[(size_t)i].index = i;
  }
  return lv;
}

void heap_case(Rng& r, int n, bool pairing) {
  g_case++;
  auto fn = pairing ? urt_host_build_object_bvh_pairing : urt_host_build_object_bvh;
  std::vector<urt_BVHNode> lv = random_leaves(r, n);
  const int len = urt_host_object_bvh_length(n);
  EXPECT(len == heap_length_ref(n));
  {
    NodeBuf out((size_t)len);
    EXPECT(fn(lv.data(), n, out.p, len) == URT_OK);
    if (n > 0) check_heap(lv.data(), n, out.p, len, !pairing, true);
  }
  if (n == 0) return;
  {                                                                             // capacity one short, NULL arrays, a negative count
    NodeBuf out((size_t)len - 1);
    EXPECT(fn(lv.data(), n, out.p, len - 1) == URT_ERR_INVALID_ARGUMENT && out.untouched() && urt_host_last_error()[0]);
    NodeBuf full((size_t)len);
    EXPECT(fn(nullptr, n, full.p, len) == URT_ERR_INVALID_ARGUMENT && fn(lv.data(), n, nullptr, len) == URT_ERR_INVALID_ARGUMENT);
    EXPECT(fn(lv.data(), -n, full.p, len) == URT_ERR_INVALID_ARGUMENT && fn(lv.data(), n, full.p, -1) == URT_ERR_INVALID_ARGUMENT);
    EXPECT(full.untouched());
  }
  // hostile coordinates
  static const float kSp[6] = {kNaN, kInf, -kInf, 3e38f, -3e38f, 1e-42f};
  bool non_finite = false;
  for (int k = 0, m = 1 + r.below(1 + n / 2); k < m; k++) {
    const float v = kSp[r.below(6)];
    if (!std::isfinite(v)) non_finite = true;
    urt_BVHNode& q = lv[(size_t)r.below(n)];
    (r.below(2) ? q.vmin : q.vmax)[r.below(3)] = v;
  }
  NodeBuf out((size_t)len);
  const int rc = fn(lv.data(), n, out.p, len);
  if (pairing && non_finite) {                                                  // the reference's FindIndex throws on such a box (urt.h)
    EXPECT(rc == URT_ERR_SCENE && out.untouched() && urt_host_last_error()[0]);
  } else {
    EXPECT(rc == URT_OK);
    if (rc == URT_OK) check_heap(lv.data(), n, out.p, len, !pairing, false);
  }
}

// ComputeNormals (RM:340-368) literally, O(V * I): the sum over every index slot whose vertex lies within EPSILON of this one
void normals_ref(const Scene& s, std::vector<float>& out) {
  const int nv = s.nv();
  out.assign((size_t)nv * 3, 0.0f);
  for (int i = 0; i < nv; i++) {
    float acc[3] = {0, 0, 0};
    for (size_t j = 0; j < s.idx.size(); j++) {
      const float* q = &s.v[3 * (size_t)s.idx[j]];
      const float dx = q[0] - s.v[3 * (size_t)i], dy = q[1] - s.v[3 * (size_t)i + 1], dz = q[2] - s.v[3 * (size_t)i + 2];
      if (!(dx * dx + dy * dy + dz * dz <= 4.2e-45f)) continue;
      const size_t t = j - j % 3;
      const float *a = &s.v[3 * (size_t)s.idx[t]], *b = &s.v[3 * (size_t)s.idx[t + 1]], *c = &s.v[3 * (size_t)s.idx[t + 2]];
      const float e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
      acc[0] = acc[0] + (e1[1] * e2[2] - e1[2] * e2[1]); acc[1] = acc[1] + (e1[2] * e2[0] - e1[0] * e2[2]); acc[2] = acc[2] + (e1[0] * e2[1] - e1[1] * e2[0]);
    }
    const float mag = std::sqrt(acc[0] * acc[0] + acc[1] * acc[1] + acc[2] * acc[2]);
    if (mag > 1e-5f) for (int k = 0; k < 3; k++) out[3 * (size_t)i + k] = acc[k] / mag;
  }
}

void scene_case(Rng& r) {
  g_case++;
  Scene s = random_scene(r, 1 + r.below(5), 12, r.below(2) == 0);
  const int nm = (int)s.mo.size(), nv = s.nv(), ni = (int)s.idx.size();
  for (int literal = 0; literal < 2; literal++) {
    std::vector<urt_BVHNode> want;
    leaf_bounds_ref(s, literal, want);
    NodeBuf out((size_t)nm);
    EXPECT(urt_host_mesh_leaf_bounds(s.mo.data(), nm, s.v.data(), nv, s.idx.data(), ni, literal, out.p) == URT_OK);
    EXPECT(std::memcmp(out.p, want.data(), (size_t)nm * sizeof(urt_BVHNode)) == 0);
  }
  {
    std::vector<float> want;
    normals_ref(s, want);
    FloatBuf out((size_t)nv * 3);
    EXPECT(urt_host_compute_normals(s.v.data(), nv, s.idx.data(), ni, out.p) == URT_OK);
    EXPECT(std::memcmp(out.p, want.data(), want.size() * sizeof(float)) == 0);
  }
  // ---- hostile records: each must give a documented error, a message, and leave what lies beyond the records before it untouched
  auto leaf_fails = [&](const Scene& h, int n_vertices, int n_indices, const float* vp, const int32_t* ip, int want_rc) {
    for (int literal = 0; literal < 2; literal++) {
      NodeBuf out(h.mo.size());
      const int rc = urt_host_mesh_leaf_bounds(h.mo.data(), (int)h.mo.size(), vp, n_vertices, ip, n_indices, literal, out.p);
      EXPECT(rc == want_rc && urt_host_last_error()[0]);
      EXPECT(out.untouched(h.mo.size() - 1));                                   // the hostile record is the last one: its own leaf is never written
    }
  };
  static const int kBadRange[][2] = {{-1, 3}, {0, -3}, {0x7fffffff, 3}, {0, 0x7fffffff}, {0x7fffffff, 0x7fffffff}, {-0x7fffffff - 1, 3}, {3, -0x7fffffff - 1}};
  for (const auto& br : kBadRange) { Scene h = s; h.mo.back().indices_offset = br[0]; h.mo.back().indices_count = br[1]; leaf_fails(h, nv, ni, h.v.data(), h.idx.data(), URT_ERR_SCENE); }
  { Scene h = s; h.mo.back().indices_offset = ni - 2; h.mo.back().indices_count = 3; leaf_fails(h, nv, ni, h.v.data(), h.idx.data(), URT_ERR_SCENE); }   // one past the end
  { Scene h = s; h.mo.back().indices_offset = ni; h.mo.back().indices_count = 1; leaf_fails(h, nv, ni, h.v.data(), h.idx.data(), URT_ERR_SCENE); }
  for (int bad : {-1, nv, 0x7fffffff, -0x7fffffff - 1}) {                       // an index outside the vertices, in the last mesh's range (and slot 0 for literal)
    Scene h = s;
    h.mo.back().indices_offset = 0; h.mo.back().indices_count = ni;
    h.idx[(size_t)r.below(ni)] = bad; h.idx[0] = bad;
    leaf_fails(h, nv, ni, h.v.data(), h.idx.data(), URT_ERR_SCENE);
    FloatBuf nrm((size_t)nv * 3);
    EXPECT(urt_host_compute_normals(h.v.data(), nv, h.idx.data(), ni, nrm.p) == URT_ERR_SCENE && urt_host_last_error()[0]);
  }
  { Scene h = s; h.mo.back().indices_offset = 0; h.mo.back().indices_count = 3; leaf_fails(h, nv, ni, nullptr, h.idx.data(), URT_ERR_INVALID_ARGUMENT); leaf_fails(h, nv, ni, h.v.data(), nullptr, URT_ERR_INVALID_ARGUMENT); }
  {
    NodeBuf out((size_t)nm);
    EXPECT(urt_host_mesh_leaf_bounds(nullptr, nm, s.v.data(), nv, s.idx.data(), ni, 0, out.p) == URT_ERR_INVALID_ARGUMENT);
    EXPECT(urt_host_mesh_leaf_bounds(s.mo.data(), nm, s.v.data(), nv, s.idx.data(), ni, 0, nullptr) == URT_ERR_INVALID_ARGUMENT);
    EXPECT(urt_host_mesh_leaf_bounds(s.mo.data(), -1, s.v.data(), nv, s.idx.data(), ni, 0, out.p) == URT_ERR_INVALID_ARGUMENT);
    EXPECT(out.untouched());
    FloatBuf nrm((size_t)nv * 3);
    EXPECT(urt_host_compute_normals(s.v.data(), nv, s.idx.data(), ni - 1, nrm.p) == URT_ERR_INVALID_ARGUMENT && urt_host_last_error()[0]);   // not a multiple of 3
    EXPECT(urt_host_compute_normals(s.v.data(), nv, s.idx.data(), ni + 1, nrm.p) == URT_ERR_INVALID_ARGUMENT);
    EXPECT(urt_host_compute_normals(nullptr, nv, s.idx.data(), ni, nrm.p) == URT_ERR_INVALID_ARGUMENT && urt_host_compute_normals(s.v.data(), nv, nullptr, ni, nrm.p) == URT_ERR_INVALID_ARGUMENT);
    EXPECT(urt_host_compute_normals(s.v.data(), nv, s.idx.data(), ni, nullptr) == URT_ERR_INVALID_ARGUMENT && urt_host_compute_normals(s.v.data(), -1, s.idx.data(), ni, nrm.p) == URT_ERR_INVALID_ARGUMENT);
    EXPECT(urt_host_compute_normals(s.v.data(), nv, s.idx.data(), -3, nrm.p) == URT_ERR_INVALID_ARGUMENT);
    EXPECT(nrm.untouched());
  }
  // hostile coordinates are data, not errors: the boxes still follow the min / max loop bit for bit, the normals are all written
  {
    Scene h = s;
    static const float kSp[7] = {kNaN, kInf, -kInf, 3e38f, -3e38f, 1e-42f, -1e-42f};
    for (int k = 0, m = 1 + r.below(6); k < m; k++) h.v[(size_t)r.below((int)h.v.size())] = kSp[r.below(7)];
    for (int literal = 0; literal < 2; literal++) {
      std::vector<urt_BVHNode> want;
      leaf_bounds_ref(h, literal, want);
      NodeBuf out((size_t)nm);
      EXPECT(urt_host_mesh_leaf_bounds(h.mo.data(), nm, h.v.data(), nv, h.idx.data(), ni, literal, out.p) == URT_OK);
      for (int m = 0; m < nm; m++) {                                            // bit for bit, but a NaN is a NaN: which of two NaN operands an
        EXPECT(out.p[m].index == want[(size_t)m].index);                        // add passes on (and so its sign and payload) is the compiler's choice
        for (int k = 0; k < 3; k++) {
          const float g[2] = {out.p[m].vmin[k], out.p[m].vmax[k]}, w[2] = {want[(size_t)m].vmin[k], want[(size_t)m].vmax[k]};
          for (int e = 0; e < 2; e++) EXPECT(bits(g[e]) == bits(w[e]) || (g[e] != g[e] && w[e] != w[e]));
        }
      }
    }
    FloatBuf nrm((size_t)nv * 3);
    EXPECT(urt_host_compute_normals(h.v.data(), nv, h.idx.data(), ni, nrm.p) == URT_OK && nrm.all_written(nrm.n));
  }
}

void sphere_case(Rng& r) {
  g_case++;
  const int n = r.below(9);
  std::vector<urt_Sphere> sp((size_t)n), prev;
  static const float kSp[7] = {kNaN, kInf, -kInf, 3e38f, -3e38f, 1e-42f, 0.0f};
  for (urt_Sphere& s : sp) {
    std::memset(&s, 0, sizeof s);
    for (int k = 0; k < 3; k++) s.position[k] = r.below(8) ? r.range(-20.0f, 20.0f) : kSp[r.below(7)];
    s.radius = r.below(8) ? r.range(0.1f, 5.0f) : kSp[r.below(7)];
  }
  for (int literal = 0; literal < 2; literal++) {
    NodeBuf out((size_t)n);
    EXPECT(urt_host_sphere_leaf_bounds(sp.data(), n, literal, out.p) == URT_OK);
    for (int i = 0; i < n; i++) {
      urt_BVHNode want; want.index = i;
      for (int k = 0; k < 3; k++) {
        const float a = sp[(size_t)i].position[k] - (-sp[(size_t)i].radius), b = sp[(size_t)i].position[k] - sp[(size_t)i].radius;
        want.vmin[k] = literal ? a : std::min(a, b); want.vmax[k] = literal ? b : std::max(a, b);
      }
      EXPECT(std::memcmp(&out.p[i], &want, sizeof want) == 0);
    }
  }
  if (n) {
    NodeBuf out((size_t)n);
    EXPECT(urt_host_sphere_leaf_bounds(nullptr, n, 0, out.p) == URT_ERR_INVALID_ARGUMENT && urt_host_last_error()[0]);
    EXPECT(urt_host_sphere_leaf_bounds(sp.data(), n, 0, nullptr) == URT_ERR_INVALID_ARGUMENT && urt_host_sphere_leaf_bounds(sp.data(), -n, 0, out.p) == URT_ERR_INVALID_ARGUMENT);
    EXPECT(out.untouched());
  }
  // sphere motion: identity bits where nothing moved, all-NaN without a positive current radius, else s = r_prev / r_cur in double
  prev = sp;
  for (urt_Sphere& s : prev) if (r.below(3)) { s.position[r.below(3)] += 1.5f; if (r.below(2)) s.radius = r.range(0.1f, 5.0f); }
  FloatBuf out((size_t)n * 12);
  EXPECT(urt_host_sphere_motion(prev.data(), sp.data(), n, (urt_ObjectMotion*)out.p) == URT_OK);
  static const float kId[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
  for (int i = 0; i < n; i++) {
    const float* a = out.p + 12 * (size_t)i;
    if (std::memcmp(&prev[(size_t)i], &sp[(size_t)i], 16) == 0) { EXPECT(std::memcmp(a, kId, sizeof kId) == 0); continue; }
    if (!(sp[(size_t)i].radius > 0.0f)) { for (int k = 0; k < 12; k++) EXPECT(a[k] != a[k] && bits(a[k]) != kSentinel); continue; }
    const double sc = (double)prev[(size_t)i].radius / (double)sp[(size_t)i].radius;
    float want[12] = {(float)sc, 0, 0, 0, (float)sc, 0, 0, 0, (float)sc, 0, 0, 0};
    for (int k = 0; k < 3; k++) want[9 + k] = (float)((double)prev[(size_t)i].position[k] - sc * (double)sp[(size_t)i].position[k]);
    for (int k = 0; k < 12; k++) EXPECT(bits(a[k]) == bits(want[k]) || (a[k] != a[k] && want[k] != want[k]));
  }
  if (n) {
    FloatBuf o2((size_t)n * 12);
    EXPECT(urt_host_sphere_motion(nullptr, sp.data(), n, (urt_ObjectMotion*)o2.p) == URT_ERR_INVALID_ARGUMENT && urt_host_last_error()[0]);
    EXPECT(urt_host_sphere_motion(prev.data(), nullptr, n, (urt_ObjectMotion*)o2.p) == URT_ERR_INVALID_ARGUMENT && urt_host_sphere_motion(prev.data(), sp.data(), n, nullptr) == URT_ERR_INVALID_ARGUMENT);
    EXPECT(urt_host_sphere_motion(prev.data(), sp.data(), -1, (urt_ObjectMotion*)o2.p) == URT_ERR_INVALID_ARGUMENT && o2.untouched());
  }
}

void mesh_motion_case(Rng& r) {
  g_case++;
  const int n = 1 + r.below(6);
  std::vector<urt_MeshObject> cur((size_t)n), prev;
  for (urt_MeshObject& o : cur) { std::memset(&o, 0, sizeof o); random_matrix(r, o.localToWorldMatrix); }
  prev = cur;
  std::vector<int> kind((size_t)n);                                             // 0 not moved, 1 moved, 2 singular current, 3 NaN current
  for (int i = 0; i < n; i++) {
    kind[(size_t)i] = r.below(5) == 0 ? 2 + r.below(2) : r.below(3) ? 1 : 0;
    if (kind[(size_t)i]) random_matrix(r, prev[(size_t)i].localToWorldMatrix);
    if (kind[(size_t)i] == 2) for (int row = 0; row < 3; row++) cur[(size_t)i].localToWorldMatrix[4 + row] = cur[(size_t)i].localToWorldMatrix[row] * 2.0f;   // column 1 = 2 * column 0
    if (kind[(size_t)i] == 3) cur[(size_t)i].localToWorldMatrix[r.below(3) * 4 + r.below(3)] = r.below(2) ? kNaN : kInf;
    if (std::memcmp(prev[(size_t)i].localToWorldMatrix, cur[(size_t)i].localToWorldMatrix, 64) == 0) kind[(size_t)i] = 0;
  }
  FloatBuf out((size_t)n * 12);
  EXPECT(urt_host_mesh_motion(prev.data(), cur.data(), n, (urt_ObjectMotion*)out.p) == URT_OK);
  EXPECT(out.all_written(out.n));
  static const float kId[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
  for (int i = 0; i < n; i++) {
    const float* a = out.p + 12 * (size_t)i;
    if (kind[(size_t)i] == 0) { EXPECT(std::memcmp(a, kId, sizeof kId) == 0); continue; }
    if (kind[(size_t)i] >= 2) { for (int k = 0; k < 12; k++) EXPECT(a[k] != a[k]); continue; }
    // the definition: the motion takes curL * p to prevL * p for every object-space p (long double, relative to the sizes involved).
    // random_matrix keeps |det| away from 0 only by chance: a badly conditioned curL is given a tolerance by its condition
    const float *C = cur[(size_t)i].localToWorldMatrix, *P = prev[(size_t)i].localToWorldMatrix;
    long double det = (long double)C[0] * ((long double)C[5] * C[10] - (long double)C[9] * C[6]) - (long double)C[4] * ((long double)C[1] * C[10] - (long double)C[9] * C[2]) +
                      (long double)C[8] * ((long double)C[1] * C[6] - (long double)C[5] * C[2]);
    if (det == 0) { for (int k = 0; k < 12; k++) EXPECT(a[k] != a[k]); continue; }
    long double amag = 0;
    for (int k = 0; k < 12; k++) amag = std::max(amag, (long double)std::fabs(a[k]));
    for (int t = 0; t < 4; t++) {
      const long double p[3] = {t == 1 ? 1.0L : 0.0L, t == 2 ? 1.0L : 0.0L, t == 3 ? 1.0L : 0.0L};
      long double wc[3], wp[3];
      for (int row = 0; row < 3; row++) {
        wc[row] = (long double)C[row] * p[0] + (long double)C[4 + row] * p[1] + (long double)C[8 + row] * p[2] + (long double)C[12 + row];
        wp[row] = (long double)P[row] * p[0] + (long double)P[4 + row] * p[1] + (long double)P[8 + row] * p[2] + (long double)P[12 + row];
      }
      for (int row = 0; row < 3; row++) {
        const long double got = (long double)a[row] * wc[0] + (long double)a[3 + row] * wc[1] + (long double)a[6 + row] * wc[2] + (long double)a[9 + row];
        // twelve entries rounded once to float32 (2^-24 relative each) against coordinates of at most 40 in size
        const long double tol = 4.0L * 0x1p-24L * amag * 41.0L + 0x1p-24L * 41.0L;
        EXPECT(std::fabs(got - wp[row]) <= tol);
      }
    }
  }
  FloatBuf o2((size_t)n * 12);
  EXPECT(urt_host_mesh_motion(nullptr, cur.data(), n, (urt_ObjectMotion*)o2.p) == URT_ERR_INVALID_ARGUMENT && urt_host_last_error()[0]);
  EXPECT(urt_host_mesh_motion(prev.data(), nullptr, n, (urt_ObjectMotion*)o2.p) == URT_ERR_INVALID_ARGUMENT && urt_host_mesh_motion(prev.data(), cur.data(), n, nullptr) == URT_ERR_INVALID_ARGUMENT);
  EXPECT(urt_host_mesh_motion(prev.data(), cur.data(), -1, (urt_ObjectMotion*)o2.p) == URT_ERR_INVALID_ARGUMENT && o2.untouched());
}

void section_scene(Rng& r) {
  g_case++;
  std::vector<long long> ns = {-0x7fffffffll - 1, -0x7fffffffll, -65536, -2, -1, 0, 1, 2, 3, 0x7fffffffll, 0x7ffffffell};
  for (int k = 2; k <= 30; k++) { ns.push_back((1ll << k) - 1); ns.push_back(1ll << k); ns.push_back((1ll << k) + 1); }
  for (long long n : ns) EXPECT((long long)urt_host_object_bvh_length((int)n) == heap_length_ref(n));
  {                                                                             // a count whose heap has no int length is refused by both builders
    urt_BVHNode one; std::memset(&one, 0, sizeof one);
    NodeBuf out(1);
    EXPECT(urt_host_build_object_bvh(&one, (1 << 30) + 1, out.p, 0x7fffffff) == URT_ERR_INVALID_ARGUMENT && urt_host_last_error()[0]);
    EXPECT(urt_host_build_object_bvh_pairing(&one, 0x7fffffff, out.p, 0x7fffffff) == URT_ERR_INVALID_ARGUMENT && out.untouched());
  }
  for (int n : {0, 1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 31, 33, 64, 65, 100, 257}) heap_case(r, n, false);
  for (int k = 0; k < 200; k++) heap_case(r, 1 + r.below(300), false);
  for (int n : {0, 1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 33, 40}) heap_case(r, n, true);
  for (int k = 0; k < 40; k++) heap_case(r, 1 + r.below(40), true);
  for (int k = 0; k < 4000; k++) scene_case(r);
  for (int k = 0; k < 1000; k++) { sphere_case(r); mesh_motion_case(r); }
}

// ====================================================================================================================== blas ====
using urtd::BlasResult;

uint64_t fnv(uint64_t h, const void* p, size_t n) { const unsigned char* b = (const unsigned char*)p; for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 0x100000001b3ull; return h; }
uint64_t hash_result(const BlasResult& b) {
  uint64_t h = 0xcbf29ce484222325ull;
  h = fnv(h, b.nodes.data(), b.nodes.size() * 4); h = fnv(h, b.tri_slot.data(), b.tri_slot.size() * 4); h = fnv(h, b.tri_mesh.data(), b.tri_mesh.size() * 4);
  h = fnv(h, b.tri_verts.data(), b.tri_verts.size() * 4); h = fnv(h, b.tri_norms.data(), b.tri_norms.size() * 4);
  h = fnv(h, b.mesh_root.data(), b.mesh_root.size() * 4); h = fnv(h, b.mesh_first_tri.data(), b.mesh_first_tri.size() * 4);
  return fnv(h, &b.max_depth, sizeof b.max_depth);
}
bool same_result(const BlasResult& a, const BlasResult& b) {
  auto eq = [](const auto& x, const auto& y) { return x.size() == y.size() && (x.empty() || std::memcmp(x.data(), y.data(), x.size() * sizeof(x[0])) == 0); };
  return eq(a.nodes, b.nodes) && eq(a.tri_slot, b.tri_slot) && eq(a.tri_mesh, b.tri_mesh) && eq(a.tri_verts, b.tri_verts) && eq(a.tri_norms, b.tri_norms) &&
         eq(a.mesh_root, b.mesh_root) && eq(a.mesh_first_tri, b.mesh_first_tri) && a.max_depth == b.max_depth;
}

bool build(const Scene& s, const std::vector<float>* normals, BlasResult& out, std::string& err, urtd::BlasCache* cache = nullptr) {
  return urtd::build_blas((const uint8_t*)s.mo.data(), (int)s.mo.size(), s.v.data(), s.nv(), s.idx.data(), (int)s.idx.size(), normals ? normals->data() : nullptr,
                          normals ? (int)normals->size() / 3 : 0, out, err, cache);
}

struct Walk {
  const Scene& s; const BlasResult& b; int leaf_max;
  std::vector<char> tri_seen, node_seen;
  int deepest = 0;
  Walk(const Scene& s_, const BlasResult& b_, int lm) : s(s_), b(b_), leaf_max(lm), tri_seen(b_.tri_slot.size(), 0), node_seen(b_.nodes.size() / 16, 0) {}
  // world-space corners of leaf-order triangle k, as the builder computes them
  void corners(size_t k, float w[3][3]) const {
    const urt_MeshObject& o = s.mo[(size_t)b.tri_mesh[k]];
    for (int j = 0; j < 3; j++) {
      const float* v = &s.v[3 * (size_t)s.idx[(size_t)b.tri_slot[k] + (size_t)j]];
      urt::v3 p = urt::mul_m4(o.localToWorldMatrix, v[0], v[1], v[2], 1.0f);
      w[j][0] = p.x; w[j][1] = p.y; w[j][2] = p.z;
    }
  }
  // visits the subtree under `code`; returns the box of the finite coordinates below it and the first / last leaf-order slot
  void visit(int32_t code, int mesh, int depth, float lo[3], float hi[3], long& first, long& last) {
    deepest = std::max(deepest, depth);
    for (int k = 0; k < 3; k++) { lo[k] = kInf; hi[k] = -kInf; }
    if (code < 0) {
      const uint32_t u = ~(uint32_t)code;
      const size_t t0 = u >> 3, cnt = (u & 7u) + 1;
      EXPECT(t0 + cnt <= b.tri_slot.size());
      if (t0 + cnt > b.tri_slot.size()) return;
      first = (long)t0; last = (long)(t0 + cnt - 1);
      float clo[3] = {kInf, kInf, kInf}, chi[3] = {-kInf, -kInf, -kInf};
      for (size_t k = t0; k < t0 + cnt; k++) {
        EXPECT(!tri_seen[k] && b.tri_mesh[k] == mesh);
        tri_seen[k] = 1;
        float w[3][3];
        corners(k, w);
        float plo[3] = {kInf, kInf, kInf}, phi[3] = {-kInf, -kInf, -kInf};
        for (int j = 0; j < 3; j++) for (int c = 0; c < 3; c++) {
          plo[c] = std::min(plo[c], w[j][c]); phi[c] = std::max(phi[c], w[j][c]);
          if (std::isfinite(w[j][c])) { lo[c] = std::min(lo[c], w[j][c]); hi[c] = std::max(hi[c], w[j][c]); }
        }
        for (int c = 0; c < 3; c++) { const float ctr = 0.5f * plo[c] + 0.5f * phi[c]; clo[c] = std::min(clo[c], ctr); chi[c] = std::max(chi[c], ctr); }
      }
      // more than leaf_max triangles (and then at most 8) only on the degenerate path, where binning cannot separate the centroids:
      // on every axis their extent is not positive (coincident, or NaN), or not finite, or so small that kBins / extent is not
      // finite — or the surface area of the triangles' box, which every split's cost carries, overflows
      bool degenerate = true;
      for (int c = 0; c < 3; c++) { const float ext = chi[c] - clo[c]; if (ext > 0 && std::isfinite(ext) && std::isfinite(32.0f / ext)) degenerate = false; }
      float all_lo[3] = {kInf, kInf, kInf}, all_hi[3] = {-kInf, -kInf, -kInf};
      for (size_t k = t0; k < t0 + cnt; k++) { float w[3][3]; corners(k, w); for (int j = 0; j < 3; j++) for (int c = 0; c < 3; c++) { all_lo[c] = std::min(all_lo[c], w[j][c]); all_hi[c] = std::max(all_hi[c], w[j][c]); } }
      const float dx = all_hi[0] - all_lo[0], dy = all_hi[1] - all_lo[1], dz = all_hi[2] - all_lo[2];
      if (!std::isfinite(dx * dy + dy * dz + dz * dx)) degenerate = true;
      EXPECT((int)cnt <= leaf_max || (degenerate && cnt <= 8));
      return;
    }
    EXPECT((size_t)code < node_seen.size());
    if ((size_t)code >= node_seen.size()) return;
    EXPECT(!node_seen[(size_t)code]);
    if (node_seen[(size_t)code]) return;
    node_seen[(size_t)code] = 1;
    const float* nd = &b.nodes[(size_t)code * 16];
    first = 0x7fffffffl; last = -1;
    for (int c = 0; c < 2; c++) {
      float l[3], h[3]; long f = 0x7fffffffl, e = -1;
      visit((int32_t)bits(nd[12 + c]), mesh, depth + 1, l, h, f, e);
      for (int k = 0; k < 3; k++) {
        if (l[k] <= h[k]) EXPECT(nd[6 * c + k] <= l[k] && nd[6 * c + 3 + k] >= h[k]);     // the child's (padded) box holds every finite coordinate below it
        lo[k] = std::min(lo[k], l[k]); hi[k] = std::max(hi[k], h[k]);
      }
      if (c == 1) EXPECT(f == last + 1);                                        // leaf order: the second child's triangles follow the first's
      first = std::min(first, f); last = std::max(last, e);
    }
  }
};

void check_blas(const Scene& s, const std::vector<float>* normals, const BlasResult& b, int leaf_max) {
  const size_t nm = s.mo.size();
  size_t total = 0;
  for (const urt_MeshObject& o : s.mo) total += (size_t)(o.indices_count / 3);
  EXPECT(b.mesh_root.size() == nm && b.mesh_first_tri.size() == nm);
  EXPECT(b.tri_slot.size() == total && b.tri_mesh.size() == total && b.tri_verts.size() == total * 12 && b.tri_norms.size() == total * 12 && b.nodes.size() % 16 == 0);
  if (b.mesh_root.size() != nm || b.tri_slot.size() != total || b.tri_mesh.size() != total || b.tri_verts.size() != total * 12) return;
  for (size_t k = 0; k < total; k++) { EXPECT(b.tri_mesh[k] >= 0 && (size_t)b.tri_mesh[k] < nm && b.tri_slot[k] >= 0 && (size_t)b.tri_slot[k] + 2 < s.idx.size()); if (!(b.tri_mesh[k] >= 0 && (size_t)b.tri_mesh[k] < nm && b.tri_slot[k] >= 0 && (size_t)b.tri_slot[k] + 2 < s.idx.size())) return; }
  Walk w(s, b, leaf_max);
  size_t at = 0;
  for (size_t m = 0; m < nm; m++) {
    const size_t cnt = (size_t)(s.mo[m].indices_count / 3);
    EXPECT((size_t)b.mesh_first_tri[m] == at);
    if (cnt == 0) { EXPECT(b.mesh_root[m] == urtd::kEmptyMeshRoot); continue; }
    EXPECT(b.mesh_root[m] != urtd::kEmptyMeshRoot);
    float lo[3], hi[3]; long first = 0, last = -1;
    w.visit(b.mesh_root[m], (int)m, 1, lo, hi, first, last);
    EXPECT(first == (long)at && last == (long)(at + cnt - 1));                  // the mesh's triangles are one run of leaf order
    std::vector<int32_t> slots(b.tri_slot.begin() + (long)at, b.tri_slot.begin() + (long)(at + cnt));
    std::sort(slots.begin(), slots.end());
    for (size_t k = 0; k < cnt; k++) EXPECT(slots[k] == s.mo[m].indices_offset + 3 * (int32_t)k);   // every index slot exactly once
    at += cnt;
  }
  for (char c : w.tri_seen) EXPECT(c);
  for (char c : w.node_seen) EXPECT(c);
  EXPECT(b.max_depth == w.deepest);
  // the first min(256, n) node indices are the breadth-first top of the forest
  {
    std::vector<int32_t> queue;
    for (size_t m = 0; m < nm; m++) if (b.mesh_root[m] >= 0 && b.mesh_root[m] != urtd::kEmptyMeshRoot) queue.push_back(b.mesh_root[m]);
    const size_t nn = b.nodes.size() / 16;
    for (size_t head = 0; head < queue.size() && head < (size_t)urtd::kTopOrderNodes; head++) {
      EXPECT(queue[head] == (int32_t)head);
      if ((size_t)queue[head] >= nn) break;
      for (int c = 0; c < 2; c++) { const int32_t ch = (int32_t)bits(b.nodes[(size_t)queue[head] * 16 + 12 + c]); if (ch >= 0) queue.push_back(ch); }
    }
  }
  for (size_t k = 0; k < total; k++) {
    float c[3][3];
    w.corners(k, c);
    urt::v3 w0 = urt::mk3(c[0][0], c[0][1], c[0][2]), e1 = urt::mk3(c[1][0], c[1][1], c[1][2]) - w0, e2 = urt::mk3(c[2][0], c[2][1], c[2][2]) - w0;
    const float want[12] = {w0.x, w0.y, w0.z, from_bits((uint32_t)b.tri_slot[k]), e1.x, e1.y, e1.z, from_bits((uint32_t)b.tri_mesh[k]), e2.x, e2.y, e2.z, 0.0f};
    EXPECT(std::memcmp(&b.tri_verts[12 * k], want, sizeof want) == 0);
    float wn[12] = {0};
    if (normals) for (int j = 0; j < 3; j++) for (int q = 0; q < 3; q++) wn[4 * j + q] = (*normals)[3 * (size_t)s.idx[(size_t)b.tri_slot[k] + (size_t)j] + (size_t)q];
    EXPECT(std::memcmp(&b.tri_norms[12 * k], wn, sizeof wn) == 0);
  }
}

int g_blas_builds = 0;
void blas_ok(const Scene& s, int leaf_max, bool with_normals) {
  g_case++;
  urtd::set_blas_leaf_max(leaf_max);
  std::vector<float> normals;
  if (with_normals) { Rng q(g_seed + (uint64_t)g_case); for (size_t i = 0; i < s.v.size(); i++) normals.push_back(q.range(-1.0f, 1.0f)); }
  BlasResult b; std::string err;
  const bool ok = build(s, with_normals ? &normals : nullptr, b, err);
  EXPECT(ok && err.empty());
  if (!ok) return;
  check_blas(s, with_normals ? &normals : nullptr, b, leaf_max);
  if (g_hashes) std::printf("blas hash %d %016llx\n", g_blas_builds, (unsigned long long)hash_result(b));
  g_blas_builds++;
}

Scene one_mesh(const std::vector<float>& v, const std::vector<int32_t>& idx) {
  Scene s; s.v = v; s.idx = idx;
  urt_MeshObject o; std::memset(&o, 0, sizeof o);
  o.localToWorldMatrix[0] = o.localToWorldMatrix[5] = o.localToWorldMatrix[10] = o.localToWorldMatrix[15] = 1.0f;
  o.indices_offset = 0; o.indices_count = (int32_t)idx.size();
  s.mo.push_back(o);
  return s;
}
// n triangles with their own vertices; place(i, corner, axis) gives the coordinates
Scene soup(int n, const std::function<float(int, int, int)>& place) {
  std::vector<float> v; std::vector<int32_t> idx;
  for (int i = 0; i < n; i++) for (int j = 0; j < 3; j++) { for (int k = 0; k < 3; k++) v.push_back(place(i, j, k)); idx.push_back(3 * i + j); }
  if (v.empty()) v = {0, 0, 0};
  return one_mesh(v, idx);
}

Scene big_scene(Rng& r) {                                 // one mesh of 16,384 triangles (a subtree fork happens), one of 2,000
  const int side = 129;                                   // 128 x 128 x 2 triangles
  Scene s;
  for (int y = 0; y < side; y++) for (int x = 0; x < side; x++) { s.v.push_back((float)x * 0.37f + r.range(-0.1f, 0.1f)); s.v.push_back(r.range(-1.0f, 1.0f)); s.v.push_back((float)y * 0.41f + r.range(-0.1f, 0.1f)); }
  for (int y = 0; y + 1 < side; y++) for (int x = 0; x + 1 < side; x++) {
    const int a = y * side + x;
    for (int q : {a, a + 1, a + side, a + 1, a + side + 1, a + side}) s.idx.push_back(q);
  }
  const int big = (int)s.idx.size();
  for (int i = 0; i < 6000; i++) s.idx.push_back(r.below(side * side));
  urt_MeshObject o; std::memset(&o, 0, sizeof o);
  random_matrix(r, o.localToWorldMatrix);
  o.indices_offset = 0; o.indices_count = big; s.mo.push_back(o);
  random_matrix(r, o.localToWorldMatrix);
  o.indices_offset = big; o.indices_count = 6000; s.mo.push_back(o);
  return s;
}

void set_threads(int n) { setenv("URT_BLAS_THREADS", std::to_string(n).c_str(), 1); }

void section_blas(Rng& r) {
  set_threads(1);
  static const float kBad[4] = {kNaN, kInf, -kInf, kNaN};
  for (int leaf_max : {1, 2, 8}) {
    for (int n : {0, 1, leaf_max - 1, leaf_max, leaf_max + 1, 9, 33})
      blas_ok(soup(std::max(n, 0), [&](int i, int j, int k) { return (float)(i * (k + 1)) * 0.5f + (j == k ? 1.0f : 0.0f); }), leaf_max, n % 2 == 1);
    for (int n : {leaf_max + 1, 9, 40}) {
      blas_ok(soup(n, [&](int, int j, int k) { return j == k ? 1.0f : 0.0f; }), leaf_max, false);                                   // copies: all centroids coincide
      blas_ok(soup(n, [&](int i, int j, int k) { return (j == k ? 1.0f : -0.5f) * (float)(1 + i % 3); }), leaf_max, false);          // concentric: coincident centroids, different boxes
      blas_ok(soup(n, [&](int i, int j, int k) { return (float)i * (k == 0 ? 1.0f : 0.0f) + (j == k ? 0.25f : 0.0f); }), leaf_max, true);   // collinear centroids
      blas_ok(soup(n, [&](int i, int j, int k) { return (i * 7 + j * 3 + k) % 11 == 0 ? kBad[(i + j + k) % 4] : (float)((i * 5 + j + k) % 13); }), leaf_max, false);   // mixed non-finite
      for (int which = 0; which < 3; which++)                                   // one kind of non-finite value only
        blas_ok(soup(n, [&](int i, int j, int k) { return (i % 4 == 1 && j == 1 && k == which) ? kBad[which] : (float)((i * 5 + j * 2 + k) % 13); }), leaf_max, false);
      blas_ok(soup(n, [&](int i, int j, int k) { return i % 3 == 0 ? kBad[(i / 3) % 3] : (float)(i + j + k); }), leaf_max, false);    // whole triangles non-finite
      blas_ok(soup(n, [&](int i, int j, int k) { return (i % 2 ? 3e38f : -3e38f) * (k == 0 ? 1.0f : 0.5f) + (float)j; }), leaf_max, false);   // hi - lo overflows
      blas_ok(soup(n, [&](int i, int j, int k) { return from_bits((uint32_t)(1 + i * 3 + (j == k ? 2 : 0))); }), leaf_max, false);     // denormal extents
      blas_ok(soup(n, [&](int i, int j, int k) { return 1.0f + from_bits((uint32_t)(1 + i)) + (j == k ? 1e-38f : 0.0f); }), leaf_max, false);
    }
    blas_ok(soup(1000, [&](int, int j, int k) { return j == k ? 2.0f : -1.0f; }), leaf_max, false);                                  // 1,000 copies: the median fallback past depth 56
    for (int k = 0; k < 400; k++) blas_ok(random_scene(r, 1 + r.below(6), 40, k % 2 == 0), leaf_max, k % 3 == 0);                   // several MeshObjects, overlapping and empty ranges
    for (int k = 0; k < 400; k++) {                                             // random scenes with hostile coordinates
      Scene s = random_scene(r, 1 + r.below(4), 60, k % 2 == 0);
      static const float kSp[7] = {kNaN, kInf, -kInf, 3e38f, -3e38f, 1e-42f, -1e-42f};
      for (int q = 0, m = 1 + r.below(5); q < m; q++) s.v[(size_t)r.below((int)s.v.size())] = kSp[r.below(7)];
      blas_ok(s, leaf_max, false);
    }
  }
  // bad ranges and bad indices: false, and err names the MeshObject or the slot
  urtd::set_blas_leaf_max(2);
  for (int k = 0; k < 24; k++) {
    g_case++;
    Scene s = random_scene(r, 1 + r.below(4), 10, false);
    const int ni = (int)s.idx.size(), m = r.below((int)s.mo.size());
    std::string want;
    static const int kBadRange[][2] = {{-1, 3}, {0, -3}, {0x7fffffff, 3}, {0, 0x7fffffff}, {0x7fffffff, 0x7fffffff}, {-0x7fffffff - 1, 3}};
    if (k % 3 == 0) { s.mo[(size_t)m].indices_offset = kBadRange[(k / 3) % 6][0]; s.mo[(size_t)m].indices_count = kBadRange[(k / 3) % 6][1]; want = "MeshObject " + std::to_string(m); }
    else if (k % 3 == 1) { s.mo[(size_t)m].indices_offset = ni - 2; s.mo[(size_t)m].indices_count = 3; want = "MeshObject " + std::to_string(m); }
    else {
      const int slot = r.below(ni);
      s.mo[0].indices_offset = 0; s.mo[0].indices_count = ni;                   // mesh 0 covers every slot, so the first error is this slot's
      static const int kBadIndex[4] = {-1, 0, 0x7fffffff, -0x7fffffff - 1};
      s.idx[(size_t)slot] = kBadIndex[k / 3 % 4] ? kBadIndex[k / 3 % 4] : s.nv();
      want = "_Indices[" + std::to_string(slot) + "]";
    }
    BlasResult b; std::string err;
    EXPECT(!build(s, nullptr, b, err));
    EXPECT(err.find(want) != std::string::npos);
  }
  { g_case++; Scene s = random_scene(r, 2, 10, false); std::vector<float> nrm((size_t)(s.nv() - 1) * 3, 0.0f); s.idx[0] = s.nv() - 1; BlasResult b; std::string err;
    EXPECT(!build(s, &nrm, b, err) && err.find("_Indices[0]") != std::string::npos); }                                           // an index beyond the normals
  // determinism across thread counts, with and without a cache, and on a cache hit
  g_case++;
  urtd::set_blas_leaf_max(2);
  Scene big = big_scene(r);
  EXPECT(big.idx.size() >= 30000 && big.mo[0].indices_count / 3 >= 16384);
  BlasResult ref; std::string err;
  set_threads(1);
  EXPECT(build(big, nullptr, ref, err));
  check_blas(big, nullptr, ref, 2);
  if (g_hashes) std::printf("blas hash %d %016llx\n", g_blas_builds, (unsigned long long)hash_result(ref));
  g_blas_builds++;
  for (int threads : {1, 2, 8}) {
    set_threads(threads);
    BlasResult b, c1, c2;
    urtd::BlasCache cache;
    EXPECT(build(big, nullptr, b, err) && same_result(b, ref));
    EXPECT(build(big, nullptr, c1, err, &cache) && same_result(c1, ref) && cache.builds == 2 && cache.hits == 0);
    EXPECT(build(big, nullptr, c2, err, &cache) && same_result(c2, ref) && cache.builds == 2 && cache.hits == 2);
  }
  set_threads(1);
}

// ===================================================================================================================== debug ====
int count_lines(const std::string& path) {
  std::vector<unsigned char> f;
  if (!read_file(path, f)) return -1;
  return (int)std::count(f.begin(), f.end(), (unsigned char)'\n');
}
int walk_count(int n_nodes, int depth, int index) { return depth <= 0 || index >= n_nodes ? 0 : 1 + walk_count(n_nodes, depth - 1, 2 * index + 1) + walk_count(n_nodes, depth - 1, 2 * index + 2); }

void section_debug(Rng& r) {
  for (int n : {0, 1, 2, 7})
    for (int depth : {0, 1, 2, 40})
      for (int ray = 0; ray < 2; ray++) {
        g_case++;
        std::vector<urt_BVHNode> nodes = random_leaves(r, std::max(n, 1));
        if (n >= 2) nodes[1].vmin[0] = kNaN;
        const float a[3] = {-100, 0.5f, 0.25f}, b[3] = {100, 0.5f, 0.25f};
        int lines = -5;
        EXPECT(urt_host_dump_bvh("fuzz_bvh.txt", nodes.data(), n, depth, ray ? a : nullptr, ray ? b : nullptr, &lines) == URT_OK);
        EXPECT(lines == walk_count(n, depth, 0) && lines == count_lines("fuzz_bvh.txt"));
        // the labels in pre-order: "(position, object index)"
        std::vector<unsigned char> f; read_file("fuzz_bvh.txt", f);
        std::vector<int> order;
        std::function<void(int, int)> pre = [&](int d, int i) { if (d <= 0 || i >= n) return; order.push_back(i); pre(d - 1, 2 * i + 1); pre(d - 1, 2 * i + 2); };
        pre(depth, 0);
        size_t at = 0;
        for (int i : order) {
          while (at < f.size() && f[at] == ' ') at++;
          const std::string want = "(" + std::to_string(i) + ", " + std::to_string(nodes[(size_t)i].index) + ") min (";
          EXPECT(at + want.size() <= f.size() && std::memcmp(&f[at], want.data(), want.size()) == 0);
          while (at < f.size() && f[at] != '\n') at++;
          at++;
        }
        lines = -5;                                                             // one end of the segment missing
        EXPECT(urt_host_dump_bvh("fuzz_bvh2.txt", nodes.data(), n, depth, a, nullptr, &lines) == URT_ERR_INVALID_ARGUMENT && lines == 0 && urt_host_debug_last_error()[0]);
        EXPECT(urt_host_dump_bvh("fuzz_bvh2.txt", nodes.data(), n, depth, nullptr, b, &lines) == URT_ERR_INVALID_ARGUMENT && count_lines("fuzz_bvh2.txt") == -1);
      }
  g_case++;
  {
    urt_BVHNode one; std::memset(&one, 0, sizeof one); int lines = 3;
    EXPECT(urt_host_dump_bvh(nullptr, &one, 1, 1, nullptr, nullptr, &lines) == URT_ERR_INVALID_ARGUMENT && lines == 0);
    EXPECT(urt_host_dump_bvh("fuzz_bvh2.txt", nullptr, 1, 1, nullptr, nullptr, &lines) == URT_ERR_INVALID_ARGUMENT && urt_host_dump_bvh("fuzz_bvh2.txt", &one, -1, 1, nullptr, nullptr, &lines) == URT_ERR_INVALID_ARGUMENT);
    EXPECT(urt_host_dump_bvh("fuzz_bvh2.txt", &one, 1, -1, nullptr, nullptr, &lines) == URT_ERR_INVALID_ARGUMENT && urt_host_dump_bvh("no/such/dir/x.txt", &one, 1, 1, nullptr, nullptr, &lines) == URT_ERR_INVALID_ARGUMENT);
    EXPECT(urt_host_debug_last_error()[0] && count_lines("fuzz_bvh2.txt") == -1);
  }
  for (int k = 0; k < 160; k++) {
    g_case++;
    Scene s = random_scene(r, 1 + r.below(4), 8, k % 2 == 0);
    const int nm = (int)s.mo.size(), nv = s.nv(), ni = (int)s.idx.size();
    std::vector<float> nrm(s.v.size(), 0.5f);
    int lines = -1, total = 0;
    for (const urt_MeshObject& o : s.mo) total += o.indices_count;
    EXPECT(urt_host_dump_normals("fuzz_nrm.txt", s.mo.data(), nm, s.v.data(), nv, s.idx.data(), ni, nrm.data(), nv, &lines) == URT_OK);
    EXPECT(lines == total && count_lines("fuzz_nrm.txt") == total);
    static const int kBadRange[][2] = {{-1, 3}, {-3, 3}, {0x7fffffff, 3}, {0x7fffffff, 0x7fffffff}, {-0x7fffffff - 1, 3}};
    Scene h = s;
    const int which = k % 8;
    if (which < 5) { h.mo.back().indices_offset = kBadRange[which][0]; h.mo.back().indices_count = kBadRange[which][1]; }
    else if (which == 5) { h.mo.back().indices_offset = ni - 2; h.mo.back().indices_count = 3; }
    else { h.mo.back().indices_offset = 0; h.mo.back().indices_count = ni; h.idx[(size_t)r.below(ni)] = which == 6 ? -1 : nv; }
    lines = -1;
    EXPECT(urt_host_dump_normals("fuzz_nrm.txt", h.mo.data(), nm, h.v.data(), nv, h.idx.data(), ni, nrm.data(), nv, &lines) == URT_ERR_SCENE && lines == 0 && urt_host_debug_last_error()[0]);
    EXPECT(urt_host_dump_normals("fuzz_nrm.txt", nullptr, nm, s.v.data(), nv, s.idx.data(), ni, nrm.data(), nv, &lines) == URT_ERR_INVALID_ARGUMENT && lines == 0);
    EXPECT(urt_host_dump_normals("fuzz_nrm.txt", s.mo.data(), nm, nullptr, nv, s.idx.data(), ni, nrm.data(), nv, &lines) == URT_ERR_INVALID_ARGUMENT);
    EXPECT(urt_host_dump_normals("fuzz_nrm.txt", s.mo.data(), nm, s.v.data(), nv, nullptr, ni, nrm.data(), nv, &lines) == URT_ERR_INVALID_ARGUMENT);
    EXPECT(urt_host_dump_normals("fuzz_nrm.txt", s.mo.data(), nm, s.v.data(), nv, s.idx.data(), ni, nullptr, nv, &lines) == URT_ERR_INVALID_ARGUMENT);
    EXPECT(urt_host_dump_normals(nullptr, s.mo.data(), nm, s.v.data(), nv, s.idx.data(), ni, nrm.data(), nv, &lines) == URT_ERR_INVALID_ARGUMENT && urt_host_dump_normals("fuzz_nrm.txt", s.mo.data(), -1, s.v.data(), nv, s.idx.data(), ni, nrm.data(), nv, &lines) == URT_ERR_INVALID_ARGUMENT);
  }
  // the log: written when level <= debug_level (text + newline, appended), else 1 and nothing written
  std::remove("fuzz_log.txt");
  std::string want;
  for (int k = 0; k < 40; k++) {
    g_case++;
    const int debug_level = r.below(5) - 1, level = debug_level + r.below(3) - 1;
    std::string text = "line " + std::to_string(k) + std::string((size_t)r.below(50), 'x');
    const int rc = urt_host_log("fuzz_log.txt", debug_level, level, text.c_str());
    if (level <= debug_level) { EXPECT(rc == URT_OK); want += text + "\n"; } else EXPECT(rc == 1);
    std::vector<unsigned char> f;
    read_file("fuzz_log.txt", f);
    EXPECT(std::string(f.begin(), f.end()) == want);
  }
  g_case++;
  EXPECT(urt_host_log(nullptr, 1, 1, "x") == URT_ERR_INVALID_ARGUMENT && urt_host_log("fuzz_log.txt", 1, 1, nullptr) == URT_ERR_INVALID_ARGUMENT && urt_host_debug_last_error()[0]);
  EXPECT(urt_host_log("no/such/dir/log.txt", 1, 1, "x") == URT_ERR_INVALID_ARGUMENT && urt_host_log("no/such/dir/log.txt", 1, 2, "x") == 1);
  std::remove("fuzz_log2.txt");
  EXPECT(urt_host_log_scene_counts("fuzz_log2.txt", 2, 1, 2, 3, 4, 5) == URT_OK && count_lines("fuzz_log2.txt") == 5);
  EXPECT(urt_host_log_scene_counts("fuzz_log2.txt", 1, 1, 2, 3, 4, 5) == 1 && count_lines("fuzz_log2.txt") == 5);
  EXPECT(urt_host_log_tree_report("fuzz_log2.txt", 2, 3, 3, 7, 0, 0, 0) == URT_OK && count_lines("fuzz_log2.txt") == 15);
}

// =================================================================================================================== threads ====
void section_threads(Rng& r) {
  // first thing after start: two threads write a PNG each (the CRC table is filled on first use)
  {
    g_case++;
    const float px[8] = {0.1f, 0.5f, 0.9f, 1, 0.2f, 0.4f, 0.6f, 1};
    auto job = [&](const char* path) { EXPECT(urt_host_write_png(path, px, 2, 1) == URT_OK); };
    std::thread t1(job, "fuzz_t1.png"), t2(job, "fuzz_t2.png");
    t1.join(); t2.join();
    std::vector<unsigned char> a, b;
    EXPECT(read_file("fuzz_t1.png", a) && read_file("fuzz_t2.png", b) && a == b && a.size() > 57);
    if (a.size() > 57) EXPECT(be32(&a[29]) == crc32_bitwise(&a[12], 17));        // IHDR's CRC
  }
  // two threads that fail in a loop and read their own message back: each thread's message is its own
  {
    g_case++;
    auto job = [&](int id) {
      const std::string missing = "no/such/dir/thread" + std::to_string(id) + ".hdr";
      urt_BVHNode one; std::memset(&one, 0, sizeof one);
      const float a[3] = {0, 0, 0};
      for (int k = 0; k < 300; k++) {
        int w = 0, h = 0, lines = 0;
        EXPECT(urt_host_load_hdr(missing.c_str(), &w, &h, nullptr, 0) == URT_ERR_INVALID_ARGUMENT);
        EXPECT(std::string(urt_host_io_last_error()).find(missing) != std::string::npos);
        if (id == 0) { EXPECT(urt_host_sphere_leaf_bounds(nullptr, 1, 0, nullptr) == URT_ERR_INVALID_ARGUMENT); EXPECT(std::string(urt_host_last_error()).find("SetupBVHLeaves") == 0); }
        else { EXPECT(urt_host_mesh_motion(nullptr, nullptr, 1, nullptr) == URT_ERR_INVALID_ARGUMENT); EXPECT(std::string(urt_host_last_error()).find("mesh_motion") == 0); }
        if (id == 0) { EXPECT(urt_host_dump_bvh("fuzz_t.txt", &one, 1, 1, a, nullptr, &lines) == URT_ERR_INVALID_ARGUMENT); EXPECT(std::string(urt_host_debug_last_error()).find("both ends") != std::string::npos); }
        else { EXPECT(urt_host_dump_bvh(missing.c_str(), &one, 1, 1, nullptr, nullptr, &lines) == URT_ERR_INVALID_ARGUMENT); EXPECT(std::string(urt_host_debug_last_error()).find(missing) != std::string::npos); }
      }
    };
    std::thread t1(job, 0), t2(job, 1);
    t1.join(); t2.join();
  }
  // the determinism scene on two host threads at once, each with its own cache, eight builder threads each
  {
    g_case++;
    urtd::set_blas_leaf_max(2);
    Scene big = big_scene(r);
    set_threads(1);
    BlasResult ref; std::string err;
    EXPECT(build(big, nullptr, ref, err));
    set_threads(8);
    BlasResult out[2][2]; bool ok[2] = {true, true};
    auto job = [&](int id) {
      urtd::BlasCache cache; std::string e;
      for (int k = 0; k < 2; k++) ok[id] = build(big, nullptr, out[id][k], e, &cache) && ok[id];
      ok[id] = ok[id] && cache.builds == 2 && cache.hits == 2;
    };
    std::thread t1(job, 0), t2(job, 1);
    t1.join(); t2.join();
    set_threads(1);
    EXPECT(ok[0] && ok[1]);
    for (int id = 0; id < 2; id++) for (int k = 0; k < 2; k++) EXPECT(same_result(out[id][k], ref));
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) { std::printf("usage: host_fuzz_main <hdr|png|pfm|resize|scene|blas|debug|threads> <seed> [hashes]\n"); return 2; }
  g_section = argv[1];
  g_seed = std::strtoull(argv[2], nullptr, 10);
  g_hashes = argc > 3;
  const std::string s = argv[1];
  uint64_t salt = 0;
  for (char c : s) salt = salt * 131 + (unsigned char)c;
  Rng r(g_seed * 0x9e3779b97f4a7c15ull + salt);
  if (s == "hdr") section_hdr(r);
  else if (s == "png") section_png(r);
  else if (s == "pfm") section_pfm(r);
  else if (s == "resize") section_resize(r);
  else if (s == "scene") section_scene(r);
  else if (s == "blas") section_blas(r);
  else if (s == "debug") section_debug(r);
  else if (s == "threads") section_threads(r);
  else { std::printf("unknown section %s\n", argv[1]); return 2; }
  if (g_failures.load()) { std::printf("%s: FAILED %d checks, seed %llu\n", g_section, g_failures.load(), (unsigned long long)g_seed); return 1; }
  std::printf("%s: ok %d\n", g_section, g_case);
  return 0;
}
