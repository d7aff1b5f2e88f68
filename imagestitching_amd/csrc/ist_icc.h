// ist_icc.h — colour profiles: the ICC profile a file carries, its integer tables (ist_icc.cpp) and the in-place conversion of a
// decoded bitmap to sRGB (ist_color.hip).  The contract is stated in include/imagestitch.h ("colour profiles") and restated in numpy
// by tests/icc_reference.py.
#ifndef IST_ICC_H_
#define IST_ICC_H_

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/imagestitch.h"

namespace ist {

// the sRGB encode thresholds T[1 .. 255] (T[0] is a placeholder): the output code of a linear value o is the number of c with
// T[c] <= o.  tools/gen_icc_encode_table.py regenerates the literal; tests/test_icc_reference.py holds it against the formula.
constexpr uint16_t kSrgbEncodeT[256] = {
      0,    10,    30,    50,    70,    90,   110,   130,   150,   170,   189,   209,   230,   253,   276,   301,
    327,   354,   382,   412,   443,   475,   509,   544,   580,   618,   657,   698,   740,   783,   828,   875,
    923,   972,  1023,  1075,  1129,  1185,  1242,  1300,  1360,  1422,  1486,  1551,  1617,  1685,  1755,  1827,
   1900,  1975,  2052,  2130,  2210,  2292,  2376,  2461,  2548,  2637,  2727,  2820,  2914,  3010,  3108,  3208,
   3309,  3412,  3518,  3625,  3734,  3844,  3957,  4072,  4188,  4307,  4427,  4550,  4674,  4800,  4928,  5059,
   5191,  5325,  5461,  5599,  5740,  5882,  6026,  6173,  6321,  6471,  6624,  6778,  6935,  7094,  7255,  7418,
   7583,  7750,  7919,  8091,  8265,  8440,  8618,  8798,  8981,  9165,  9352,  9541,  9732,  9925, 10121, 10318,
  10518, 10720, 10925, 11132, 11341, 11552, 11765, 11981, 12199, 12420, 12643, 12868, 13095, 13325, 13557, 13791,
  14028, 14267, 14508, 14752, 14998, 15247, 15498, 15751, 16007, 16265, 16525, 16788, 17054, 17321, 17592, 17864,
  18139, 18417, 18697, 18980, 19264, 19552, 19842, 20134, 20429, 20727, 21027, 21329, 21634, 21942, 22252, 22564,
  22880, 23197, 23518, 23840, 24166, 24494, 24824, 25158, 25493, 25832, 26173, 26516, 26862, 27211, 27563, 27917,
  28273, 28633, 28995, 29359, 29727, 30097, 30469, 30845, 31223, 31603, 31987, 32373, 32762, 33153, 33547, 33944,
  34344, 34747, 35152, 35560, 35970, 36384, 36800, 37219, 37640, 38065, 38492, 38922, 39355, 39790, 40229, 40670,
  41114, 41561, 42011, 42463, 42918, 43377, 43838, 44301, 44768, 45238, 45710, 46185, 46663, 47144, 47628, 48115,
  48605, 49097, 49593, 50091, 50592, 51096, 51604, 52114, 52627, 53142, 53661, 54183, 54708, 55235, 55766, 56300,
  56836, 57376, 57918, 58464, 59012, 59564, 60118, 60675, 61236, 61799, 62366, 62935, 63508, 64083, 64662, 65244,
};

// the number of c in 1 .. 255 with T[c] <= o (o in 0 .. 65535): the sRGB code of a linear value
constexpr int srgb_encode(uint32_t o) {
  int lo = 0, hi = 255;                      // the answer lies in [lo, hi]
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (kSrgbEncodeT[mid] <= o) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// one pixel channel triple through the tables of a CONVERT / IDENTITY profile (the contract's "per pixel" rule), on the host
void color_convert_pixel(const ist_color_tables& t, const uint8_t in[3], uint8_t out[3]);

// an ICC profile -> kind + tables (ist_icc_tables without the argument checks); never fails: what it does not take is UNSUPPORTED
int icc_tables(const uint8_t* icc, size_t len, ist_color_tables* out);

// The profile a file carries, reassembled: true when one was found (icc filled), *srgb set for a PNG whose sRGB chunk stands for it.
// Pure container walks, each in its decoder's file; a damaged container or chunk reads as "no profile", never as an error.
bool jpeg_icc_profile(const uint8_t* file, int64_t len, std::vector<uint8_t>* icc);                 // ist_jpeg.cpp: APP2 ICC_PROFILE chunks
bool png_icc_profile(const uint8_t* file, int64_t len, std::vector<uint8_t>* icc, bool* srgb);      // ist_png_decode.cpp: iCCP, else sRGB
bool webp_icc_profile(const uint8_t* file, int64_t len, std::vector<uint8_t>* icc);                 // ist_webp.cpp: ICCP of a VP8X file
constexpr size_t kMaxIccBytes = 4u << 20;    // a PNG's inflated profile above this counts as absent

// kind + tables of a file by its signature (ist_image_color with the tables); BMP, GIF and anything unknown: IST_COLOR_NONE
int image_color_tables(const uint8_t* file, int64_t len, ist_color_tables* out);

// ist_color.hip: the w x h box of RGBA8 at `px` (4-byte aligned, rows `pitch` bytes apart) through t, in place, on `stream`.
// t.kind must be IST_COLOR_CONVERT; arguments are checked by the caller.
int launch_color_convert(uint8_t* px, size_t pitch, int64_t w, int64_t h, const ist_color_tables& t, void* stream);

}  // namespace ist

#endif  // IST_ICC_H_
