// source_layout.cpp — prints what SourceLayout (ist_sources.cpp) makes of requests' sources, for tests/test_source_layout.py.  Pure CPU,
// no HIP; nothing is copied, the copy items are printed as offsets:
//   g++ -std=c++17 -Iinclude -Iimagestitching_amd/csrc tools/source_layout.cpp imagestitching_amd/csrc/{ist_plan,ist_sources}.cpp
// stdin, any number of cases, whitespace separated:
//   <n_requests>
//   per request:  <n_images> <n_held> <dense>                     dense 1: src_pitch NULL
//                 n_images x (<width> <height> <bmp_width> <bmp_height> <pitch> <null>)   null 1: the source pointer is NULL
//                 n_held x (<image> <y0> <y1>)
//   <n_copies> n_copies x (<image> <r0> <r1>)                    images numbered across the requests
// stdout per case:
//   add <rc> <message>                                            per request, "-" when rc is 0; after a failure only "end" follows
//   bytes <n>
//   place <image> <ptr - base, or -1 for NULL> <pitch>           per image
//   copy <image> <r0> <r1> <dev - base> <host_src - src[image]> <host_pitch> <row> <rows>
//   all <dev - base> <host_src - src[image]> <host_pitch> <row> <rows>     copy_all's items, in order
//   end
#include <cstdio>
#include <vector>

#include "ist_internal.h"

using namespace ist;

int main() {
  int n_req;
  while (std::scanf("%d", &n_req) == 1) {
    struct Req { std::vector<ist_image_desc> d; std::vector<size_t> pitch; std::vector<const uint8_t*> src; std::map<int, RowSpan> held; bool dense; };
    std::vector<Req> reqs(static_cast<size_t>(n_req));
    std::vector<char> null_src;                   // per image across the requests: its source pointer is NULL
    size_t src_bytes = 1;
    for (Req& r : reqs) {
      int n, n_held, dense;
      if (std::scanf("%d %d %d", &n, &n_held, &dense) != 3) return 2;
      r.dense = dense != 0;
      r.d.resize(static_cast<size_t>(n));
      r.pitch.resize(static_cast<size_t>(n));
      r.src.resize(static_cast<size_t>(n));
      for (int i = 0; i < n; ++i) {
        ist_image_desc& d = r.d[static_cast<size_t>(i)];
        d = ist_image_desc{};
        long long pitch;
        int null;
        if (std::scanf("%d %d %d %d %lld %d", &d.width, &d.height, &d.bmp_width, &d.bmp_height, &pitch, &null) != 6) return 2;
        r.pitch[static_cast<size_t>(i)] = static_cast<size_t>(pitch);
        null_src.push_back(static_cast<char>(null != 0));
        if (!null && bitmap_h(d) > 0) src_bytes = std::max(src_bytes, static_cast<size_t>(pitch) * static_cast<size_t>(bitmap_h(d)));
      }
      for (int k = 0; k < n_held; ++k) {
        int i;
        long long y0, y1;
        if (std::scanf("%d %lld %lld", &i, &y0, &y1) != 3) return 2;
        r.held[i] = RowSpan{y0, y1};
      }
    }
    // every source reads one buffer large enough for the largest image: offsets from src[image] are what the test checks
    std::vector<uint8_t> pixels(src_bytes);
    size_t g = 0;
    for (Req& r : reqs)
      for (const uint8_t*& s : r.src) s = null_src[g++] ? nullptr : pixels.data();
    int n_copies;
    if (std::scanf("%d", &n_copies) != 1) return 2;
    std::vector<std::vector<long long>> copies(static_cast<size_t>(n_copies), std::vector<long long>(3));
    for (auto& c : copies) if (std::scanf("%lld %lld %lld", &c[0], &c[1], &c[2]) != 3) return 2;

    SourceLayout lay;
    bool ok = true;
    for (const Req& r : reqs) {
      g_last_error.clear();
      const int rc = lay.add(r.d.data(), static_cast<int>(r.d.size()), r.src.data(), r.dense ? nullptr : r.pitch.data(), r.held);
      std::printf("add %d %s\n", rc, rc ? g_last_error.c_str() : "-");
      if (rc) { ok = false; break; }
    }
    if (ok) {
      std::vector<uint8_t> block(lay.bytes());
      const uintptr_t base = reinterpret_cast<uintptr_t>(block.data());
      std::printf("bytes %zu\n", lay.bytes());
      const SourceLayout::Placed at = lay.place(block.data());
      for (size_t i = 0; i < at.ptr.size(); ++i)
        std::printf("place %zu %lld %zu\n", i, at.ptr[i] ? static_cast<long long>(reinterpret_cast<uintptr_t>(at.ptr[i]) - base) : -1LL, at.pitch[i]);
      auto print = [&](const RowsCopy& c, const uint8_t* src) {
        std::printf("%lld %lld %zu %zu %zu\n", static_cast<long long>(reinterpret_cast<uintptr_t>(c.dev) - base),
                    static_cast<long long>(static_cast<const uint8_t*>(c.host_src) - src), c.host_pitch, c.row, c.rows);
      };
      for (const auto& c : copies) {
        std::printf("copy %lld %lld %lld ", c[0], c[1], c[2]);
        print(lay.copy(static_cast<int>(c[0]), c[1], c[2]), pixels.data());
      }
      std::vector<RowsCopy> items;
      lay.copy_all(&items);
      for (const RowsCopy& c : items) { std::printf("all "); print(c, pixels.data()); }
    }
    std::printf("end\n");
  }
  return 0;
}
