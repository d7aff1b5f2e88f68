// check_icc_host.cpp — drives the host side of the colour profiles (ist_icc.cpp: profile -> tables; the profile walks of ist_jpeg.cpp,
// ist_png_decode.cpp and ist_webp.cpp) over seeded random and adversarial inputs, under ASan + UBSan, on the CPU:
// tools/run_fuzz.sh icc ITERS [SEED].
// Every input is a heap block of exactly its stated size, so that a byte read beyond one is caught.  Checked per input: the kind is
// one of the four; UNSUPPORTED and NONE leave zeroed tables; CONVERT / IDENTITY tables carry every code through the per-pixel rule
// without a trap, IDENTITY maps every code to itself; the container walks return a profile only as large as the file could hold.
#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "ist_icc.h"
#include "ist_internal.h"

using namespace ist;

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "iteration %d: %s:%d: %s\n", g_iter, __FILE__, __LINE__, #c); std::exit(1); } } while (0)
static int g_iter = 0;
static std::mt19937_64 rng;

static uint32_t rnd(uint32_t n) { return n ? static_cast<uint32_t>(rng() % n) : 0; }
static void be32(std::vector<uint8_t>* v, uint32_t x) { for (int s = 24; s >= 0; s -= 8) v->push_back(static_cast<uint8_t>(x >> s)); }
static void be16(std::vector<uint8_t>* v, uint32_t x) { v->push_back(static_cast<uint8_t>(x >> 8)); v->push_back(static_cast<uint8_t>(x)); }
static void put32(std::vector<uint8_t>* v, size_t at, uint32_t x) { for (int k = 0; k < 4; ++k) (*v)[at + k] = static_cast<uint8_t>(x >> (24 - 8 * k)); }
static void tag4(std::vector<uint8_t>* v, const char* s) { v->insert(v->end(), s, s + 4); }

// A calm iteration draws a profile the contract takes unless one of the few remaining dice says otherwise; the others are hostile.
static bool g_calm = false;
static bool ok(uint32_t k) { return g_calm ? rnd(4 * k) != 0 : rnd(k) != 0; }

// the s15.16 values an adversary would pick, or a plausible one
static uint32_t fixed() {
  if (g_calm) return 4096u + rnd(98304);                  // 0.06 .. 1.56
  static const uint32_t k[] = {0u, 1u, 0xFFFFFFFFu, 0x80000000u, 0x7FFFFFFFu, 65536u, 0xFFFF0000u, 32768u, 157286u, 62119u, 3417u};
  return rnd(3) ? k[rnd(sizeof k / sizeof *k)] : static_cast<uint32_t>(rng());
}

static std::vector<uint8_t> curve() {
  std::vector<uint8_t> t;
  if (rnd(2)) {
    tag4(&t, "curv"); be32(&t, 0);
    const uint32_t shape = g_calm ? rnd(4) : rnd(5);
    const uint32_t n = shape == 0 ? 0 : shape == 1 ? 1 : shape == 2 ? 2 + rnd(6) : shape == 3 ? 256 + rnd(4096) : rnd(3) ? 0xFFFFFFFFu - rnd(4) : 0x80000000u;
    be32(&t, n);
    const uint32_t have = n > 8192 ? rnd(64) : ok(8) ? n : rnd(n + 1);      // (sometimes fewer entries than the count says)
    for (uint32_t i = 0; i < have; ++i) be16(&t, rnd(4) ? (i * 65535u) / (have > 1 ? have - 1 : 1) : rnd(65536));
  } else {
    static const int kParams[5] = {1, 3, 4, 5, 7};
    const uint32_t type = ok(12) ? rnd(5) : rnd(65536);
    tag4(&t, "para"); be32(&t, 0); be16(&t, type); be16(&t, 0);
    const int n = type < 5 ? kParams[type] : 7;
    const int have = ok(8) ? n : static_cast<int>(rnd(static_cast<uint32_t>(n) + 1));
    for (int i = 0; i < have; ++i) be32(&t, fixed());
  }
  return t;
}

static std::vector<uint8_t> make_profile() {
  std::vector<uint8_t> p(128, 0);
  std::memcpy(p.data() + 12, "mntr", 4);
  std::memcpy(p.data() + 16, ok(16) ? "RGB " : rnd(2) ? "GRAY" : "CMYK", 4);
  std::memcpy(p.data() + 20, ok(16) ? "XYZ " : "Lab ", 4);
  std::memcpy(p.data() + 36, ok(16) ? "acsp" : "acsq", 4);
  static const char* const kNames[8] = {"rXYZ", "gXYZ", "bXYZ", "rTRC", "gTRC", "bTRC", "A2B0", "wtpt"};
  std::vector<int> order;
  for (int q = 0; q < 8; ++q) if (q >= 6 ? rnd(2) != 0 : ok(24)) order.push_back(q);
  if (!ok(8) && !order.empty()) order.push_back(order[rnd(static_cast<uint32_t>(order.size()))]);      // a signature twice
  for (size_t i = order.size(); i > 1; --i) std::swap(order[i - 1], order[rnd(static_cast<uint32_t>(i))]);
  const size_t n = order.size();
  be32(&p, ok(16) ? static_cast<uint32_t>(n) : rnd(4) ? static_cast<uint32_t>(rng()) : static_cast<uint32_t>(n) + 1);
  p.resize(132 + 12 * n, 0);
  for (size_t k = 0; k < n; ++k) {
    const int q = order[k];
    std::vector<uint8_t> body;
    if (q < 3 || q == 7) { tag4(&body, ok(16) ? "XYZ " : "text"); be32(&body, 0); for (int c = 0; c < (ok(16) ? 3 : 2); ++c) be32(&body, fixed()); }
    else if (q < 6) body = curve();
    else { tag4(&body, "mft2"); body.resize(52, 0); }
    uint32_t off = static_cast<uint32_t>(p.size()), len = static_cast<uint32_t>(body.size());
    p.insert(p.end(), body.begin(), body.end());
    while (p.size() & 3) p.push_back(0);
    if (!ok(12)) off = rnd(2) ? static_cast<uint32_t>(rng()) : off + rnd(64);
    if (!ok(12)) len = rnd(2) ? static_cast<uint32_t>(rng()) : len + rnd(64);
    std::memcpy(p.data() + 132 + 12 * k, kNames[q], 4);
    put32(&p, 132 + 12 * k + 4, off); put32(&p, 132 + 12 * k + 8, len);
  }
  put32(&p, 0, ok(12) ? static_cast<uint32_t>(p.size()) : rnd(2) ? static_cast<uint32_t>(rng()) : rnd(static_cast<uint32_t>(p.size()) + 8));
  if (!ok(6)) for (uint32_t k = 0, m = 1 + rnd(8); k < m; ++k) p[rnd(static_cast<uint32_t>(p.size()))] = static_cast<uint8_t>(rng());
  if (!ok(6)) p.resize(rnd(static_cast<uint32_t>(p.size()) + 1));
  return p;
}

static int g_kinds[4] = {0, 0, 0, 0};

static void check_tables(int kind, const ist_color_tables& t) {
  REQUIRE(kind >= IST_COLOR_NONE && kind <= IST_COLOR_UNSUPPORTED && t.kind == kind);
  ++g_kinds[kind];
  if (kind == IST_COLOR_UNSUPPORTED || kind == IST_COLOR_NONE) {
    static const ist_color_tables zero = {};
    ist_color_tables z = t; z.kind = 0;
    REQUIRE(std::memcmp(&z, &zero, sizeof z) == 0);
    return;
  }
  if (kind == IST_COLOR_IDENTITY && t.mq[0][0] == 0) return;      // (a PNG's sRGB chunk: no tables)
  for (int v = 0; v < 256; ++v) {
    const uint8_t in[3] = {static_cast<uint8_t>(v), static_cast<uint8_t>(255 - v), static_cast<uint8_t>((v * 7) & 255)};
    uint8_t out[3];
    color_convert_pixel(t, in, out);
    if (kind == IST_COLOR_IDENTITY) REQUIRE(out[0] == in[0] && out[1] == in[1] && out[2] == in[2]);
  }
}

// the profile through ist_icc_tables from a heap block of exactly its size
static void check_profile(const std::vector<uint8_t>& p) {
  std::unique_ptr<uint8_t[]> block(new uint8_t[p.size() ? p.size() : 1]);
  if (!p.empty()) std::memcpy(block.get(), p.data(), p.size());
  ist_color_tables t;
  std::memset(&t, 0xEE, sizeof t);
  const int kind = ist_icc_tables(block.get(), static_cast<int64_t>(p.size()), &t);
  if (p.empty()) { REQUIRE(kind == IST_E_INVALID); return; }
  check_tables(kind, t);
}

static void chunk_png(std::vector<uint8_t>* f, const char* type, const std::vector<uint8_t>& d, uint32_t len_field) {
  be32(f, len_field); tag4(f, type); f->insert(f->end(), d.begin(), d.end()); be32(f, static_cast<uint32_t>(rng()));
}

// the profile inside a JPEG, PNG or WebP container (no image data behind it: the walks stop there), with the container damaged now and then
static std::vector<uint8_t> wrap(const std::vector<uint8_t>& icc, int form) {
  std::vector<uint8_t> f;
  if (form == 0) {
    f = {0xFF, 0xD8};
    const uint32_t chunks = 1 + rnd(4), step = static_cast<uint32_t>((icc.size() + chunks - 1) / chunks);
    for (uint32_t s = 1; s <= chunks; ++s) {
      const size_t a = std::min(icc.size(), static_cast<size_t>(step) * (s - 1)), b = std::min(icc.size(), static_cast<size_t>(step) * s);
      if (b - a > 65000 || !rnd(24)) continue;                              // (too long for a segment, or a missing chunk)
      f.push_back(0xFF); f.push_back(rnd(24) ? 0xE2 : 0xE1);
      be16(&f, static_cast<uint32_t>(b - a) + 16);
      f.insert(f.end(), {'I', 'C', 'C', '_', 'P', 'R', 'O', 'F', 'I', 'L', 'E', 0});
      f.push_back(static_cast<uint8_t>(rnd(16) ? s : rnd(256))); f.push_back(static_cast<uint8_t>(rnd(16) ? chunks : rnd(256)));
      f.insert(f.end(), icc.begin() + static_cast<long>(a), icc.begin() + static_cast<long>(b));
    }
    f.insert(f.end(), {0xFF, 0xDA, 0x00, 0x02, 0xFF, 0xD9});
  } else if (form == 1) {
    f = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    chunk_png(&f, "IHDR", std::vector<uint8_t>(13, 1), 13);
    if (!rnd(4)) chunk_png(&f, "sRGB", {0}, 1);
    if (rnd(8)) {
      std::vector<uint8_t> d = {'n', 0, static_cast<uint8_t>(rnd(16) ? 0 : 1)};
      uLongf zn = compressBound(static_cast<uLong>(icc.size()));
      std::vector<uint8_t> z(zn);
      compress(z.data(), &zn, icc.data(), static_cast<uLong>(icc.size()));
      z.resize(rnd(8) ? zn : rnd(static_cast<uint32_t>(zn) + 1));
      if (!rnd(8) && !z.empty()) z[rnd(static_cast<uint32_t>(z.size()))] ^= static_cast<uint8_t>(1 + rnd(255));
      d.insert(d.end(), z.begin(), z.end());
      chunk_png(&f, "iCCP", d, rnd(16) ? static_cast<uint32_t>(d.size()) : static_cast<uint32_t>(rng()));
    }
    chunk_png(&f, "IDAT", {}, 0);
  } else {
    std::vector<uint8_t> body = {'W', 'E', 'B', 'P'};
    auto chunk = [&](const char* tag, const std::vector<uint8_t>& d, uint32_t len_field) {
      tag4(&body, tag);
      for (int k = 0; k < 4; ++k) body.push_back(static_cast<uint8_t>(len_field >> (8 * k)));
      body.insert(body.end(), d.begin(), d.end());
      if (d.size() & 1) body.push_back(0);
    };
    if (rnd(8)) chunk("VP8X", std::vector<uint8_t>(10, 0), 10);
    chunk("ICCP", icc, rnd(16) ? static_cast<uint32_t>(icc.size()) : static_cast<uint32_t>(rng()));
    chunk("VP8L", std::vector<uint8_t>(8, 0), 8);
    f = {'R', 'I', 'F', 'F'};
    const uint32_t n = rnd(16) ? static_cast<uint32_t>(body.size()) : static_cast<uint32_t>(rng());
    for (int k = 0; k < 4; ++k) f.push_back(static_cast<uint8_t>(n >> (8 * k)));
    f.insert(f.end(), body.begin(), body.end());
  }
  if (!rnd(8) && !f.empty()) f.resize(rnd(static_cast<uint32_t>(f.size()) + 1));
  return f;
}

static void check_file(const std::vector<uint8_t>& f) {
  std::unique_ptr<uint8_t[]> block(new uint8_t[f.size() ? f.size() : 1]);
  if (!f.empty()) std::memcpy(block.get(), f.data(), f.size());
  std::vector<uint8_t> icc;
  bool srgb = false;
  if (jpeg_icc_profile(block.get(), static_cast<int64_t>(f.size()), &icc)) REQUIRE(icc.size() <= f.size());
  if (webp_icc_profile(block.get(), static_cast<int64_t>(f.size()), &icc)) REQUIRE(icc.size() <= f.size());
  if (png_icc_profile(block.get(), static_cast<int64_t>(f.size()), &icc, &srgb)) REQUIRE(icc.size() <= kMaxIccBytes && !srgb);
  ist_color_tables t;
  std::memset(&t, 0xEE, sizeof t);
  const int kind = image_color_tables(block.get(), static_cast<int64_t>(f.size()), &t);
  check_tables(kind, t);
  int32_t k2 = -1;
  if (!f.empty()) REQUIRE(ist_image_color(block.get(), static_cast<int64_t>(f.size()), &k2) == IST_OK && k2 == kind);
}

int main(int argc, char** argv) {
  const int iters = argc > 1 ? std::atoi(argv[1]) : 1000;
  rng.seed(argc > 2 ? static_cast<uint64_t>(std::atoll(argv[2])) : 1);
  for (g_iter = 0; g_iter < iters; ++g_iter) {
    g_calm = (g_iter & 1) != 0;
    const std::vector<uint8_t> p = make_profile();
    check_profile(p);
    for (int form = 0; form < 3; ++form) check_file(wrap(p, form));
  }
  // a PNG whose profile inflates past the cap counts as untagged
  {
    std::vector<uint8_t> big(kMaxIccBytes + 4096, 0);
    const std::vector<uint8_t> f = wrap(big, 1);
    ist_color_tables t;
    const int kind = image_color_tables(f.data(), static_cast<int64_t>(f.size()), &t);
    REQUIRE(kind == IST_COLOR_NONE || kind == IST_COLOR_IDENTITY);      // (IDENTITY: the wrapper drew an sRGB chunk and no iCCP)
  }
  std::printf("%d profiles (none %d, identity %d, convert %d, unsupported %d): ok\n", iters, g_kinds[0], g_kinds[1], g_kinds[2], g_kinds[3]);
  return 0;
}
