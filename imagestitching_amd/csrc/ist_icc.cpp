// ist_icc.cpp — an ICC profile -> the integer tables of the colour contract (include/imagestitch.h, "colour profiles"), and the
// colour kind of a file.  Host only, no device: every byte of a profile is untrusted, every read is bounded by the profile's own size
// field, and what the contract does not take is IST_COLOR_UNSUPPORTED - never an error, never a failed decode.
//
// Reference anchor: the Image.src step (utils/canvas.js:27-121) hands the page a bitmap the platform has already colour-managed.
#include "ist_icc.h"

#include <cmath>
#include <cstring>

#include "ist_internal.h"
#include "ist_webp.h"

namespace ist {

namespace {

inline uint32_t be16(const uint8_t* p) { return (uint32_t(p[0]) << 8) | p[1]; }
inline uint32_t be32(const uint8_t* p) { return (uint32_t(p[0]) << 24) | (uint32_t(p[1]) << 16) | (uint32_t(p[2]) << 8) | p[3]; }
inline int32_t s15f16(const uint8_t* p) { return static_cast<int32_t>(be32(p)); }

// the inverse of the sRGB colorants (D50), Q24
constexpr int64_t kInv[3][3] = {{52584397, -27133356, -8233164}, {-16421465, 32147857, 561266}, {1207600, -3841813, 23584544}};

struct Tag { size_t at = 0, len = 0; bool found = false; };

uint16_t quantise(double y) {
  const double q = std::floor(65535.0 * y + 0.5);
  if (!(q > 0.0)) return 0;                   // (a NaN ends here too; the contract's max(., 0) keeps pow away from one)
  return q >= 65535.0 ? 65535 : static_cast<uint16_t>(q);
}

// one TRC tag -> dec[0 .. 255]; false: not a curve the contract takes
bool curve_table(const uint8_t* p, size_t n, uint16_t* dec) {
  if (n < 12) return false;
  if (!std::memcmp(p, "curv", 4)) {
    const uint32_t cnt = be32(p + 8);
    if (cnt > (n - 12) / 2) return false;
    if (cnt == 0) { for (int v = 0; v < 256; ++v) dec[v] = static_cast<uint16_t>(257 * v); return true; }
    if (cnt == 1) {
      const uint32_t g8 = be16(p + 12);
      if (g8 == 0) return false;
      const double g = g8 / 256.0;
      for (int v = 0; v < 256; ++v) dec[v] = quantise(std::pow(v / 255.0, g));
      return true;
    }
    const uint8_t* t = p + 12;
    for (uint64_t v = 0; v < 256; ++v) {
      const uint64_t pos = v * (cnt - 1), i = pos / 255, r = pos % 255, j = i + 1 < cnt ? i + 1 : cnt - 1;
      dec[v] = static_cast<uint16_t>((be16(t + 2 * i) * (255 - r) + be16(t + 2 * j) * r + 127) / 255);
    }
    return true;
  }
  if (!std::memcmp(p, "para", 4)) {
    static const int kParams[5] = {1, 3, 4, 5, 7};
    const uint32_t type = be16(p + 8);
    if (type > 4 || n < 12 + 4 * static_cast<size_t>(kParams[type])) return false;
    double q[7] = {0, 0, 0, 0, 0, 0, 0};      // g a b c d e f
    for (int k = 0; k < kParams[type]; ++k) q[k] = s15f16(p + 12 + 4 * k) / 65536.0;
    const double g = q[0], a = q[1], b = q[2], c = q[3], d = q[4], e = q[5], f = q[6];
    if (!(g > 0.0)) return false;
    if ((type == 1 || type == 2) && a == 0.0) return false;
    for (int v = 0; v < 256; ++v) {
      const double x = v / 255.0;
      const double base = a * x + b > 0.0 ? a * x + b : 0.0;
      double y;
      switch (type) {
        case 0: y = std::pow(x, g); break;
        case 1: y = x >= -b / a ? std::pow(base, g) : 0.0; break;
        case 2: y = x >= -b / a ? std::pow(base, g) + c : c; break;
        case 3: y = x >= d ? std::pow(base, g) : c * x; break;
        default: y = x >= d ? std::pow(base, g) + e : c * x + f; break;
      }
      dec[v] = quantise(y);
    }
    return true;
  }
  return false;
}

int unsupported(ist_color_tables* out) { std::memset(out, 0, sizeof *out); out->kind = IST_COLOR_UNSUPPORTED; return IST_COLOR_UNSUPPORTED; }

}  // namespace

void color_convert_pixel(const ist_color_tables& t, const uint8_t in[3], uint8_t out[3]) {
  const int64_t lin[3] = {t.dec[0][in[0]], t.dec[1][in[1]], t.dec[2][in[2]]};
  for (int i = 0; i < 3; ++i) {
    int64_t o = (t.mq[i][0] * lin[0] + t.mq[i][1] * lin[1] + t.mq[i][2] * lin[2] + 32768) >> 16;
    o = o < 0 ? 0 : o > 65535 ? 65535 : o;
    out[i] = static_cast<uint8_t>(srgb_encode(static_cast<uint32_t>(o)));
  }
}

int icc_tables(const uint8_t* icc, size_t len, ist_color_tables* out) {
  std::memset(out, 0, sizeof *out);
  if (!icc || len < 132) return unsupported(out);
  const size_t size = be32(icc);
  if (size < 132 || size > len) return unsupported(out);
  if (std::memcmp(icc + 36, "acsp", 4) != 0 || std::memcmp(icc + 16, "RGB ", 4) != 0 || std::memcmp(icc + 20, "XYZ ", 4) != 0) return unsupported(out);
  const size_t n_tags = be32(icc + 128);
  if (n_tags > (size - 132) / 12) return unsupported(out);
  static const char* const kNames[6] = {"rXYZ", "gXYZ", "bXYZ", "rTRC", "gTRC", "bTRC"};
  Tag tag[6];
  for (size_t k = 0; k < n_tags; ++k) {
    const uint8_t* e = icc + 132 + 12 * k;
    for (int q = 0; q < 6; ++q) {
      if (tag[q].found || std::memcmp(e, kNames[q], 4) != 0) continue;
      tag[q].found = true; tag[q].at = be32(e + 4); tag[q].len = be32(e + 8);
    }
  }
  for (const Tag& t : tag) if (!t.found || t.at > size || t.len > size - t.at) return unsupported(out);
  int64_t C[3][3];                            // rows X, Y, Z; columns r, g, b
  for (int j = 0; j < 3; ++j) {
    const uint8_t* p = icc + tag[j].at;
    if (tag[j].len < 20 || std::memcmp(p, "XYZ ", 4) != 0) return unsupported(out);
    for (int k = 0; k < 3; ++k) C[k][j] = s15f16(p + 8 + 4 * k);
  }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const int64_t m = (kInv[i][0] * C[0][j] + kInv[i][1] * C[1][j] + kInv[i][2] * C[2][j] + (int64_t(1) << 23)) >> 24;
      if (m < INT32_MIN || m > INT32_MAX) return unsupported(out);
      out->mq[i][j] = static_cast<int32_t>(m);
    }
  for (int c = 0; c < 3; ++c)
    if (!curve_table(icc + tag[3 + c].at, tag[3 + c].len, out->dec[c])) return unsupported(out);
  bool identity = true;
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) identity = identity && out->mq[i][j] == (i == j ? 65536 : 0);
  for (int c = 0; identity && c < 3; ++c) for (int v = 0; identity && v < 256; ++v) identity = srgb_encode(out->dec[c][v]) == v;
  out->kind = identity ? IST_COLOR_IDENTITY : IST_COLOR_CONVERT;
  return out->kind;
}

int image_color_tables(const uint8_t* f, int64_t n, ist_color_tables* out) {
  std::memset(out, 0, sizeof *out);
  out->kind = IST_COLOR_NONE;
  if (!f || n < 12) return IST_COLOR_NONE;
  std::vector<uint8_t> icc;
  bool found = false, srgb = false;
  if (f[0] == 0xFF && f[1] == 0xD8) found = jpeg_icc_profile(f, n, &icc);
  else if (is_webp(f, n)) found = webp_icc_profile(f, n, &icc);
  else if (f[0] == 0x89 && f[1] == 'P' && f[2] == 'N' && f[3] == 'G') found = png_icc_profile(f, n, &icc, &srgb);
  if (srgb) { out->kind = IST_COLOR_IDENTITY; return IST_COLOR_IDENTITY; }      // (no tables: nothing is launched for it)
  if (!found) return IST_COLOR_NONE;
  return icc_tables(icc.data(), icc.size(), out);
}

}  // namespace ist

using namespace ist;

extern "C" {

int ist_image_color(const uint8_t* file, int64_t len, int32_t* kind) {
  if (!file || len <= 0 || !kind) return fail(IST_E_INVALID, "ist_image_color: bad argument");
  ist_color_tables t;
  *kind = image_color_tables(file, len, &t);
  return IST_OK;
}

int ist_icc_tables(const uint8_t* icc, int64_t len, ist_color_tables* out) {
  if (!icc || len <= 0 || !out) return fail(IST_E_INVALID, "ist_icc_tables: bad argument");
  return icc_tables(icc, static_cast<size_t>(len), out);
}

}  // extern "C"
