// check_jpeg_join_host.cpp — drives the host side of the lossless JPEG join (ist_jpeg_join_host.cpp: eligibility from the headers,
// the joined geometry, the per-image table) and the block mapping the kernel shares with the host (join_source, ist_jpeg_join.h) over
// seeded random and hostile sets of files, under ASan + UBSan, on the CPU: tools/run_fuzz.sh jpegjoin ITERS [SEED].
// Every file is a heap block of exactly its length, so that a byte read beyond it is caught.  For every eligible set the joined size
// is held against ist_plan_compute's canvas (mode min, gap 0, unlimited caps), and the slab walk - every MCU row of every slab, every
// block of the row, as the kernel's grid covers them - must name a block inside its image's plane, reach every block of every plane
// exactly once, and stay inside the slab.  Sets with one defect must be refused with that defect's reason at that image; files with
// random damage must be refused or accepted without a fault.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "ist_internal.h"
#include "ist_jpeg_enc.h"
#include "ist_jpeg_join.h"

namespace ist { bool tuning_mode() { return false; } }      // (the one thing ist_jpeg_enc_host.cpp takes from the rest of the library)

using namespace ist;

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "iteration %d: %s:%d: %s\n", g_iter, __FILE__, __LINE__, #c); std::exit(1); } } while (0)
static int g_iter = 0;

typedef std::vector<uint8_t> Bytes;

// a file whose headers are the export's (jpeg_enc_header) and whose scan is a few bytes: all the eligibility check reads
static Bytes make_file(int w, int h, int ss, const JpegTables& T, std::mt19937_64& rng) {
  Bytes f = jpeg_enc_header(w, h, ss, T, 1);
  for (int k = 0, n = static_cast<int>(rng() % 24); k < n; ++k) { const uint8_t b = static_cast<uint8_t>(rng()); f.push_back(b); if (b == 0xFF) f.push_back(0); }
  f.push_back(0xFF); f.push_back(0xD9);
  return f;
}
static size_t find_marker(const Bytes& f, uint8_t m) {      // a walk over the segments behind SOI
  size_t k = 2;
  while (k + 4 <= f.size() && f[k] == 0xFF && f[k + 1] != m) k += 2 + ((static_cast<size_t>(f[k + 2]) << 8) | f[k + 3]);
  return k;
}
static void add_orientation(Bytes* f, int o) {
  const uint8_t app1[] = {0xFF, 0xE1, 0, 34, 'E', 'x', 'i', 'f', 0, 0, 'I', 'I', 42, 0, 8, 0, 0, 0, 1, 0, 0x12, 0x01, 3, 0, 1, 0, 0, 0,
                          static_cast<uint8_t>(o), 0, 0, 0, 0, 0, 0, 0};
  f->insert(f->begin() + 2, app1, app1 + sizeof app1);
}

struct Set { std::vector<std::unique_ptr<uint8_t[]>> own; std::vector<const uint8_t*> p; std::vector<int64_t> len; };
static void push(Set* s, const Bytes& f) {
  std::unique_ptr<uint8_t[]> b(new uint8_t[f.size() ? f.size() : 1]);
  if (!f.empty()) std::memcpy(b.get(), f.data(), f.size());
  s->p.push_back(b.get()); s->len.push_back(static_cast<int64_t>(f.size())); s->own.push_back(std::move(b));
}

// the slab walk of an eligible plan: what the kernel's grids cover, slab by slab
static void walk(const JoinPlan& plan, int64_t slab_rows) {
  const bool is420 = jpeg_ss_420(plan.subsampling), horizontal = plan.direction == IST_HORIZONTAL;
  std::vector<JpegCoefPlanes> planes(static_cast<size_t>(plan.n));
  std::vector<std::vector<uint8_t>> seen(static_cast<size_t>(plan.n) * 3);
  for (int i = 0; i < plan.n; ++i)
    for (int c = 0; c < 3; ++c) {
      const int s = is420 && c == 0 ? 2 : 1;
      planes[i].coef[c] = reinterpret_cast<const int16_t*>(uintptr_t(1) << 40);       // (device addresses: never dereferenced)
      planes[i].blocks_x[c] = plan.files[i].mcus_x * s; planes[i].blocks_y[c] = plan.files[i].mcus_y * s;
      seen[static_cast<size_t>(i) * 3 + c].assign(static_cast<size_t>(planes[i].blocks_x[c]) * planes[i].blocks_y[c], 0);
    }
  std::unique_ptr<JoinTable> T(new JoinTable);
  REQUIRE(jpeg_join_table(plan, planes.data(), T.get()) == IST_OK);
  REQUIRE(T->n == plan.n && T->first[0] == 0 && T->first[plan.n] == (horizontal ? plan.mcus_x : plan.mcus_y));
  const JpegGeometry g = jpeg_geometry(plan.width, plan.height, plan.subsampling);
  REQUIRE(g.mcus_x == plan.mcus_x && g.mcus_y == plan.mcus_y);
  int64_t launches = 0;
  for (int64_t r0 = 0; r0 < g.mcus_y; r0 += slab_rows, ++launches) {
    const int64_t rows = std::min(slab_rows, g.mcus_y - r0);
    std::vector<uint8_t> slab(static_cast<size_t>(rows * g.row_blocks), 0);
    const int64_t gx = (g.row_blocks + kJoinBlocksPerWg - 1) / kJoinBlocksPerWg;
    for (int64_t y = 0; y < rows; ++y)
      for (int64_t wg = 0; wg < gx; ++wg)
        for (int slot = 0; slot < kJoinBlocksPerWg; ++slot) {
          const int64_t block = wg * kJoinBlocksPerWg + slot;
          if (block >= g.row_blocks) continue;
          const JoinSource s = join_source(T->first, T->n, horizontal, is420, static_cast<int32_t>(r0 + y), static_cast<int32_t>(block));
          REQUIRE(s.image >= 0 && s.image < plan.n && s.comp >= 0 && s.comp < 3);
          const JoinImage& I = T->img[s.image];
          REQUIRE(s.bx >= 0 && s.bx < I.blocks_x[s.comp] && s.by >= 0 && s.by < I.blocks_y[s.comp]);
          uint8_t& hit = seen[static_cast<size_t>(s.image) * 3 + s.comp][static_cast<size_t>(s.by) * I.blocks_x[s.comp] + s.bx];
          REQUIRE(hit == 0); hit = 1;
          const size_t at = static_cast<size_t>(y * g.row_blocks + block);
          REQUIRE(at < slab.size() && slab[at] == 0); slab[at] = 1;
        }
    for (uint8_t v : slab) REQUIRE(v == 1);
  }
  REQUIRE(launches == (g.mcus_y + slab_rows - 1) / slab_rows);
  for (const std::vector<uint8_t>& p : seen) for (uint8_t v : p) REQUIRE(v == 1);      // every source block is carried
}

int main(int argc, char** argv) {
  const int iters = argc > 1 ? std::atoi(argv[1]) : 2000;
  std::mt19937_64 rng(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 12345);
  auto pick = [&](int64_t lo, int64_t hi) { return lo + static_cast<int64_t>(rng() % static_cast<uint64_t>(hi - lo + 1)); };
  int64_t eligible = 0, refused = 0, blocks = 0;
  for (g_iter = 0; g_iter < iters; ++g_iter) {
    const int ss = static_cast<int>(pick(0, 1)), mcu = ss == IST_JPEG_420 ? 16 : 8;
    const int direction = static_cast<int>(pick(0, 1));
    const int n = pick(0, 9) == 0 ? static_cast<int>(pick(100, 128)) : static_cast<int>(pick(1, 7));
    const int across = static_cast<int>(pick(1, pick(0, 3) ? 70 : 600));
    JpegTables T, T2;
    jpeg_enc_tables(static_cast<int>(pick(1, 100)), &T);
    T2 = T; T2.q[static_cast<int>(pick(0, 1))][pick(0, 63)] ^= 1; if (!T2.q[0][0]) T2.q[0][0] = 2;
    // one defect, or none
    const int defect = pick(0, 2) ? IST_JOIN_OK : static_cast<int>(pick(IST_JOIN_NOT_JPEG, IST_JOIN_LIMIT));
    const int where = static_cast<int>(pick(0, n - 1));
    int want_reason = IST_JOIN_OK, want_image = -1;
    Set set;
    std::vector<ist_image_desc> descs;
    for (int i = 0; i < n; ++i) {
      int along = i == n - 1 ? static_cast<int>(pick(1, 5 * mcu)) : mcu * static_cast<int>(pick(1, n > 20 ? 2 : 5));
      int w = direction == IST_HORIZONTAL ? along : across, h = direction == IST_HORIZONTAL ? across : along;
      const JpegTables* tab = &T;
      bool hit = i == where;
      if (hit && defect == IST_JOIN_SIZE && n > 1 && i > 0) { (direction == IST_HORIZONTAL ? h : w) += 1; }
      else if (hit && defect == IST_JOIN_ALIGN && i < n - 1) { (direction == IST_HORIZONTAL ? w : h) += static_cast<int>(pick(1, mcu - 1)); }
      else if (hit && defect == IST_JOIN_TABLES && i > 0) tab = &T2;
      else if (hit && (defect == IST_JOIN_ORIENT || defect == IST_JOIN_NOT_JPEG || defect == IST_JOIN_LAYOUT || (defect == IST_JOIN_MIXED && i > 0))) {}
      else hit = false;
      Bytes f = make_file(w, h, hit && defect == IST_JOIN_MIXED ? 1 - ss : ss, *tab, rng);
      if (hit && defect == IST_JOIN_ORIENT) add_orientation(&f, static_cast<int>(pick(2, 8)));
      if (hit && defect == IST_JOIN_NOT_JPEG) { if (pick(0, 1)) f[1] = 0xD9; else f.resize(static_cast<size_t>(pick(0, 30))); }
      if (hit && defect == IST_JOIN_LAYOUT) f[find_marker(f, 0xC0) + 11] = 0x21;      // 4:2:2
      if (hit) { want_reason = defect; want_image = i; }
      push(&set, f);
      ist_image_desc d; std::memset(&d, 0, sizeof d); d.width = w; d.height = h; d.orientation = 1; d.opaque = 1;
      descs.push_back(d);
    }
    ist_jpeg_join_info info;
    JoinPlan plan;
    const int rc = jpeg_join_eligible(set.p.data(), set.len.data(), n, direction, &info, &plan);
    REQUIRE(info.reason == want_reason && info.image == want_image);
    REQUIRE((rc == IST_OK) == (want_reason == IST_JOIN_OK));
    if (rc == IST_OK) {
      ++eligible;
      ist_limits lim; ist_limits_unlimited(&lim);
      ist_plan p; std::memset(&p, 0, sizeof p);
      REQUIRE(ist_plan_compute(descs.data(), n, direction, IST_MODE_MIN, 0.0, &lim, &p) == IST_OK);
      REQUIRE(p.canvas_w == plan.width && p.canvas_h == plan.height && info.width == plan.width && info.height == plan.height);
      ist_plan_free(&p);
      const int64_t rows_choice[] = {1, 2, 3, plan.mcus_y, plan.mcus_y + 5};
      walk(plan, rows_choice[pick(0, 4)]);
      blocks += plan.mcus_x * plan.mcus_y;
    } else {
      ++refused;
      REQUIRE(rc == IST_E_UNSUPPORTED && info.width == 0 && info.height == 0 && g_last_error.rfind("image " + std::to_string(want_image) + ": ", 0) == 0);
    }
    // the same set with random damage in one file: any answer, no fault; then more than 128 files
    {
      Set hurt;
      for (int i = 0; i < n; ++i) {
        Bytes f(set.p[i], set.p[i] + set.len[i]);
        if (i == where && !f.empty()) {
          for (int k = 0, m = static_cast<int>(pick(1, 6)); k < m; ++k) f[static_cast<size_t>(pick(0, static_cast<int64_t>(f.size()) - 1))] = static_cast<uint8_t>(rng());
          if (pick(0, 3) == 0) f.resize(static_cast<size_t>(pick(0, static_cast<int64_t>(f.size()))));
        }
        push(&hurt, f);
      }
      ist_jpeg_join_info hi; JoinPlan hp;
      const int hrc = jpeg_join_eligible(hurt.p.data(), hurt.len.data(), n, direction, &hi, &hp);
      REQUIRE(hrc == IST_OK || hrc == IST_E_UNSUPPORTED);
      if (hrc == IST_OK && hp.mcus_x * hp.mcus_y <= 200000) walk(hp, pick(1, 3));      // (a damaged size may be huge)
    }
    if (g_iter % 50 == 0) {
      std::vector<const uint8_t*> many(129, set.p[0]); std::vector<int64_t> lens(129, set.len[0]);
      REQUIRE(jpeg_join_eligible(many.data(), lens.data(), 129, direction, &info, &plan) == IST_E_UNSUPPORTED && info.reason == IST_JOIN_LIMIT && info.image == 128);
      // a joined side above 65535: heights of 8 x 4096 rows each
      Set tall;
      for (int i = 0; i < 3; ++i) push(&tall, make_file(direction == IST_HORIZONTAL ? 32768 : 8, direction == IST_HORIZONTAL ? 8 : 32768, IST_JPEG_444, T, rng));
      REQUIRE(jpeg_join_eligible(tall.p.data(), tall.len.data(), 3, direction, &info, &plan) == IST_E_UNSUPPORTED && info.reason == IST_JOIN_LIMIT && info.image == 1);
    }
  }
  std::printf("check_jpeg_join_host: %d iterations, %lld eligible sets (%lld MCUs walked), %lld refused\n", iters, static_cast<long long>(eligible),
              static_cast<long long>(blocks), static_cast<long long>(refused));
  return 0;
}
