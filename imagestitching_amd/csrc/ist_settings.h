// ist_settings.h — the per-context settings (ist_ctx_set_png_level / _png_color / _png_filter / _png_match / _color_profile / _timing):
// ONE atomic word in the context, ONE snapshot per library call.  An entry point reads the word once, where it checks its arguments,
// and hands the value down; no layer below reads the context's settings again, so a setter that lands in the middle of a call changes
// the NEXT call and nothing of this one.  A setter replaces its own field with a compare-exchange loop: it takes no lock and never
// waits for a running call.  The next setting is one more Field below, one more member of Settings and one more setter - nothing else.
// Plain C++17, nothing of HIP: tools/check_settings_host.cpp compiles it alone (it supplies ist::fail).
#ifndef IST_SETTINGS_H_
#define IST_SETTINGS_H_

#include <atomic>
#include <cstdint>
#include <string>

#include "../../include/imagestitch.h"

struct ist_ctx;

namespace ist {

int fail(int code, const std::string& msg);

// the form of one PNG export
struct PngForm {
  int level = 0;                          // 1: Paeth + run-length + Huffman; 0: stored deflate blocks
  int color = IST_PNG_RGBA;               // colour type 6, or IST_PNG_RGB: colour type 2, alpha not read
  int filter = IST_PNG_FILTER_PAETH;      // type 4 on every row, or IST_PNG_FILTER_ADAPTIVE: a type per row, level 1 only
  int match = IST_PNG_MATCH_RUN;          // runs inside a span, or IST_PNG_MATCH_WINDOW: also matches at a distance, level 1 only
  bool compressed() const { return level > 0; }
  bool adaptive() const { return filter == IST_PNG_FILTER_ADAPTIVE; }
  bool window() const { return match == IST_PNG_MATCH_WINDOW; }
  int bpp() const { return color == IST_PNG_RGB ? 3 : 4; }
  // IST_E_UNSUPPORTED for the forms no encoder serves: the stored form (level 0) in RGB, with adaptive row filters or with window
  // matches.  Every *_png entry point calls it on its snapshot before anything is read or enqueued; nothing below checks again.
  int check() const {
    if (level == 0 && window())
      return fail(IST_E_UNSUPPORTED, "PNG window matches need the compressing encoder (pngLevel 1): the stored form matches nothing");
    if (level == 0 && adaptive())
      return fail(IST_E_UNSUPPORTED, "adaptive PNG row filters need the compressing encoder (pngLevel 1): the stored form filters nothing");
    if (level == 0 && color == IST_PNG_RGB)
      return fail(IST_E_UNSUPPORTED, "RGB PNG export needs the compressing encoder (pngLevel 1): the stored form writes RGBA only");
    return IST_OK;
  }
};

// what one call reads of its context (the default: what a call without a context gets)
struct Settings {
  PngForm png;
  int color_profile = IST_COLOR_PROFILE_IGNORE;   // or IST_COLOR_PROFILE_SRGB: ICC-tagged files are converted to sRGB behind their decode
  bool timing = false;                            // the file pipeline records its phase times (adds a sync per phase)
};

// a setting's place in the word: `count` values, 0 .. count - 1, from bit `shift`; `invalid`: the setter's message for any other value
struct Field { int shift; uint32_t count; const char* invalid; };
constexpr Field kPngLevel{0, 2, "PNG level must be 0 (stored) or 1 (compressed)"};
constexpr Field kPngColor{1, 2, "PNG colour must be IST_PNG_RGBA (0) or IST_PNG_RGB (1)"};
constexpr Field kPngFilter{2, 2, "PNG filter must be IST_PNG_FILTER_PAETH (0) or IST_PNG_FILTER_ADAPTIVE (1)"};
constexpr Field kPngMatch{3, 2, "PNG match must be IST_PNG_MATCH_RUN (0) or IST_PNG_MATCH_WINDOW (1)"};
constexpr Field kColorProfile{4, 2, "colour profile must be IST_COLOR_PROFILE_IGNORE (0) or IST_COLOR_PROFILE_SRGB (1)"};
constexpr Field kTiming{5, 2, "timing must be 0 or 1"};      // (ist_ctx_set_timing hands over on != 0: never said)
static_assert(IST_PNG_RGBA == 0 && IST_PNG_RGB == 1 && IST_PNG_FILTER_PAETH == 0 && IST_PNG_FILTER_ADAPTIVE == 1 && IST_PNG_MATCH_RUN == 0 &&
              IST_PNG_MATCH_WINDOW == 1 && IST_COLOR_PROFILE_IGNORE == 0 && IST_COLOR_PROFILE_SRGB == 1, "a field holds its setting's own value");

constexpr uint32_t field_mask(const Field& f) { uint32_t m = 1; while (m < f.count - 1) m = 2 * m + 1; return m << f.shift; }      // the bits that hold 0 .. count - 1
constexpr int field_of(uint32_t word, const Field& f) { return static_cast<int>((word & field_mask(f)) >> f.shift); }
constexpr uint32_t kDefaultSettings = 1u << kPngLevel.shift;      // a new context: level 1, RGBA, Paeth, runs, profiles ignored, no timing

inline Settings settings_unpack(uint32_t word) {
  Settings s;
  s.png.level = field_of(word, kPngLevel); s.png.color = field_of(word, kPngColor);
  s.png.filter = field_of(word, kPngFilter); s.png.match = field_of(word, kPngMatch);
  s.color_profile = field_of(word, kColorProfile); s.timing = field_of(word, kTiming) != 0;
  return s;
}

// one setter: IST_E_INVALID (and nothing changes) for a value the field does not take; else the field alone is replaced, whatever other
// setters do to theirs meanwhile.  (Relaxed: the word guards no other memory.)
inline int settings_set(std::atomic<uint32_t>* word, const Field& f, int value) {
  if (value < 0 || static_cast<uint32_t>(value) >= f.count) return fail(IST_E_INVALID, f.invalid);
  uint32_t old = word->load(std::memory_order_relaxed);
  while (!word->compare_exchange_weak(old, (old & ~field_mask(f)) | (static_cast<uint32_t>(value) << f.shift), std::memory_order_relaxed)) {}
  return IST_OK;
}

// the call's snapshot: one load (ist_ctx.h).  NULL: Settings{}
Settings settings_of(const ist_ctx* ctx);

}  // namespace ist

#endif  // IST_SETTINGS_H_
