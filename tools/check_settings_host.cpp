// check_settings_host.cpp — the context's settings word (imagestitching_amd/csrc/ist_settings.h) under ThreadSanitizer, CPU only
// (tools/run_fuzz.sh settings ITERS).  Five setter threads, one per field, walk their field through its valid values and try a few
// invalid ones; four reader threads take snapshots meanwhile.  Checked: a valid set returns IST_OK and is what its own thread reads
// back (nobody else writes that field); an invalid set returns IST_E_INVALID and changes nothing; every snapshot holds a value of its
// field in every field and nothing outside the fields; at the end the word is the last valid value of each setter.
#include <atomic>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "ist_settings.h"

namespace ist {
int fail(int code, const std::string&) { return code; }      // (the library's keeps the message for ist_last_error)
}

using namespace ist;

static const Field kFields[5] = {kPngLevel, kPngColor, kPngFilter, kPngMatch, kColorProfile};
static std::atomic<uint32_t> g_word{kDefaultSettings};
static std::atomic<long> g_bad{0};

#define EXPECT(cond, ...) do { if (!(cond)) { if (g_bad.fetch_add(1) < 20) { std::fprintf(stderr, "FAILED %s: ", #cond); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); } } } while (0)

static void setter(int k, long iters, int* last_out) {
  const Field& f = kFields[k];
  const int invalid[] = {-1, static_cast<int>(f.count), 7, 255, INT_MAX, INT_MIN};
  int last = field_of(g_word.load(), f);
  for (long i = 0; i < iters; ++i) {
    const int v = static_cast<int>((i + k) % f.count);
    EXPECT(settings_set(&g_word, f, v) == IST_OK, "field %d, value %d", k, v);
    last = v;
    EXPECT(field_of(g_word.load(), f) == last, "field %d does not hold the %d just set", k, last);
    if (i % 7 == 0) {
      const int bad = invalid[(i / 7) % 6];
      EXPECT(settings_set(&g_word, f, bad) == IST_E_INVALID, "field %d took %d", k, bad);
      EXPECT(field_of(g_word.load(), f) == last, "field %d changed by the refused value %d", k, bad);
    }
  }
  *last_out = last;
}

static void reader(const std::atomic<bool>* stop, long* n_out) {
  uint32_t fields = field_mask(kTiming);
  for (const Field& f : kFields) fields |= field_mask(f);
  long n = 0;
  do {
    const uint32_t w = g_word.load(std::memory_order_relaxed);
    const Settings s = settings_unpack(w);
    EXPECT((w & ~fields) == 0, "bits outside the fields: %08x", w);
    EXPECT((s.png.level == 0 || s.png.level == 1) && (s.png.color == IST_PNG_RGBA || s.png.color == IST_PNG_RGB) &&
           (s.png.filter == IST_PNG_FILTER_PAETH || s.png.filter == IST_PNG_FILTER_ADAPTIVE) &&
           (s.png.match == IST_PNG_MATCH_RUN || s.png.match == IST_PNG_MATCH_WINDOW) &&
           (s.color_profile == IST_COLOR_PROFILE_IGNORE || s.color_profile == IST_COLOR_PROFILE_SRGB) && !s.timing, "snapshot %08x", w);
    for (const Field& f : kFields) EXPECT(static_cast<uint32_t>(field_of(w, f)) < f.count, "a field of %08x holds no value of its own", w);
    ++n;
  } while (!stop->load(std::memory_order_relaxed));
  *n_out = n;
}

int main(int argc, char** argv) {
  const long iters = argc > 1 ? std::atol(argv[1]) : 200000;
  const Settings d = settings_unpack(kDefaultSettings), none = Settings{};
  EXPECT(d.png.level == 1 && d.png.color == IST_PNG_RGBA && d.png.filter == IST_PNG_FILTER_PAETH && d.png.match == IST_PNG_MATCH_RUN &&
         d.color_profile == IST_COLOR_PROFILE_IGNORE && !d.timing && d.png.check() == IST_OK, "the defaults of a new context");
  EXPECT(none.png.level == 0 && none.png.check() == IST_OK, "the settings of a call without a context");
  std::atomic<bool> stop{false};
  int last[5] = {0, 0, 0, 0, 0};
  long seen[4] = {0, 0, 0, 0};
  std::vector<std::thread> readers, setters;
  for (int r = 0; r < 4; ++r) readers.emplace_back(reader, &stop, &seen[r]);
  for (int k = 0; k < 5; ++k) setters.emplace_back(setter, k, iters, &last[k]);
  for (std::thread& t : setters) t.join();
  stop.store(true);
  for (std::thread& t : readers) t.join();
  uint32_t want = 0;
  for (int k = 0; k < 5; ++k) want |= static_cast<uint32_t>(last[k]) << kFields[k].shift;
  EXPECT(g_word.load() == want, "the word is %08x, the setters' last values make %08x", g_word.load(), want);
  // one setter more, alone: timing, and the forms the check refuses
  EXPECT(settings_set(&g_word, kTiming, 1) == IST_OK && settings_unpack(g_word.load()).timing && (g_word.load() & ~field_mask(kTiming)) == want, "timing");
  PngForm f; f.level = 0; f.color = IST_PNG_RGB;
  EXPECT(f.check() == IST_E_UNSUPPORTED, "level 0 in RGB");
  f.color = IST_PNG_RGBA; f.filter = IST_PNG_FILTER_ADAPTIVE;
  EXPECT(f.check() == IST_E_UNSUPPORTED, "level 0 with adaptive filters");
  f.filter = IST_PNG_FILTER_PAETH; f.match = IST_PNG_MATCH_WINDOW;
  EXPECT(f.check() == IST_E_UNSUPPORTED, "level 0 with window matches");
  f.level = 1; f.color = IST_PNG_RGB; f.filter = IST_PNG_FILTER_ADAPTIVE;
  EXPECT(f.check() == IST_OK && f.bpp() == 3 && f.adaptive() && f.window() && f.compressed(), "level 1 takes every form");
  const long snapshots = seen[0] + seen[1] + seen[2] + seen[3];
  if (g_bad.load()) { std::printf("%ld checks failed\n", g_bad.load()); return 1; }
  std::printf("%ld sets per field on 5 threads, %ld snapshots on 4 threads: ok\n", iters, snapshots);
  return 0;
}
