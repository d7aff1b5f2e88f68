// check_jpeg_batch_host.cpp — drives the host side of the batched JPEG export (ist_jpeg_enc_host.cpp: the rounds, the header blob and
// the piece records) over random batches, under ASan + UBSan, on the CPU: tools/run_fuzz.sh jpegbatch ITERS.
// Every buffer is a heap block of exactly the size the plan states, so that a byte written beyond it is caught; the records are
// checked against the plan: every pointer inside its block, pieces that tile the scratch without overlap, prefix sums of the grids.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "ist_internal.h"
#include "ist_jpeg_enc.h"

namespace ist { bool tuning_mode() { return false; } }      // (the one thing ist_jpeg_enc_host.cpp takes from the rest of the library)

using namespace ist;

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "iteration %d: %s:%d: %s\n", g_iter, __FILE__, __LINE__, #c); std::exit(1); } } while (0)
static int g_iter = 0;

// ist_jpeg_bound (the encoder's own translation unit needs the device runtime)
static int64_t bound(int64_t w, int64_t h, int subsampling) {
  const JpegGeometry g = jpeg_geometry(w, h, subsampling);
  return 1024 + g.mcus_y * (g.row_blocks * kJpegBlockBytes + 16);
}

int main(int argc, char** argv) {
  const int iters = argc > 1 ? std::atoi(argv[1]) : 2000;
  std::mt19937_64 rng(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 12345);
  auto pick = [&](int64_t lo, int64_t hi) { return lo + static_cast<int64_t>(rng() % static_cast<uint64_t>(hi - lo + 1)); };
  const uint8_t* const dev = reinterpret_cast<const uint8_t*>(uintptr_t(1) << 40);       // (device addresses: never dereferenced)
  uint8_t* const scratch = reinterpret_cast<uint8_t*>(uintptr_t(1) << 41);
  int64_t total_pieces = 0, total_rounds = 0;
  for (g_iter = 0; g_iter < iters; ++g_iter) {
    const int n = static_cast<int>(pick(1, 12));
    std::vector<JpegBatchFile> files(static_cast<size_t>(n));
    std::vector<int64_t> w(static_cast<size_t>(n)), h(static_cast<size_t>(n));
    std::vector<int> ss(static_cast<size_t>(n));
    int64_t dear = 0;
    for (int k = 0; k < n; ++k) {
      const bool wide = pick(0, 19) == 0;
      w[k] = wide ? pick(1, 65535) : pick(1, 600); h[k] = pick(0, 29) == 0 ? pick(1, 65535) : pick(1, 600); ss[k] = static_cast<int>(pick(0, 1));
      if (wide) h[k] = pick(1, 40);
      files[k] = JpegBatchFile{dev, static_cast<size_t>(w[k]) * 4, w[k], h[k], static_cast<int>(pick(1, 100)), ss[k], scratch, bound(w[k], h[k], ss[k]), 0};
      dear = std::max(dear, jpeg_geometry(w[k], h[k], ss[k]).row_cost());
    }
    const int64_t budgets[] = {1, dear / 2 + 1, dear, dear + 1, 3 * dear, 17 * dear + 5, int64_t(kJpegEncBudget)};
    const int64_t budget = budgets[pick(0, 6)];
    // the C-ABI: the count, and a cap that is too small
    const int64_t count = ist_jpeg_batch_layout(w.data(), h.data(), ss.data(), n, budget, nullptr, 0);
    REQUIRE(count >= n);
    const int64_t cap = pick(0, count);
    std::unique_ptr<ist_jpeg_piece[]> some(new ist_jpeg_piece[static_cast<size_t>(cap)]);
    REQUIRE(ist_jpeg_batch_layout(w.data(), h.data(), ss.data(), n, budget, some.get(), cap) == count);
    const std::vector<ist_jpeg_piece> pieces = jpeg_batch_pieces(files.data(), n, budget);
    REQUIRE(static_cast<int64_t>(pieces.size()) == count);
    for (int64_t p = 0; p < cap; ++p) REQUIRE(std::memcmp(&some[p], &pieces[p], sizeof(ist_jpeg_piece)) == 0);
    // every row once and in order
    {
      int f = 0; int64_t row = 0;
      for (const ist_jpeg_piece& pc : pieces) {
        if (pc.file != f) { REQUIRE(row == jpeg_geometry(w[f], h[f], ss[f]).mcus_y && pc.file == f + 1); f = pc.file; row = 0; }
        REQUIRE(pc.mcu_row0 == row && pc.mcu_rows >= 1);
        row += pc.mcu_rows;
      }
      REQUIRE(f == n - 1 && row == jpeg_geometry(w[f], h[f], ss[f]).mcus_y);
    }
    int round = 0;
    for (int p0 = 0; p0 < static_cast<int>(count);) {
      int p1 = p0 + 1;
      while (p1 < static_cast<int>(count) && pieces[p1].round == pieces[p0].round) ++p1;
      REQUIRE(pieces[p0].round == round);
      const JpegRound R = jpeg_round_plan(files.data(), pieces.data(), p0, p1);
      std::unique_ptr<uint8_t[]> host(new uint8_t[R.table_bytes]);
      jpeg_round_pack(R, files.data(), pieces.data(), host.get(), dev, scratch);
      const JpegPiece* rec = reinterpret_cast<const JpegPiece*>(host.get() + R.at_pieces);
      int64_t wg = 0, iv = 0, rows = 0, cost = 0;
      size_t coef_end = 0, slot_end = R.at_slots;
      for (int p = p0; p < p1; ++p) {
        const JpegPiece& P = rec[p - p0];
        const JpegBatchFile& f = files[pieces[p].file];
        const JpegGeometry g = jpeg_geometry(f.w, f.h, f.subsampling);
        REQUIRE(P.wg0 == wg && P.iv0 == iv && P.gx >= 1 && P.mcu_rows == pieces[p].mcu_rows && P.mcu_row0 == pieces[p].mcu_row0);
        REQUIRE(P.mcus_y == g.mcus_y && P.mcus_x == g.mcus_x && P.row_blocks == g.row_blocks && P.slot == g.slot && P.bpm == g.bpm);
        REQUIRE(P.mcu_row0 + P.mcu_rows <= P.mcus_y && P.w == f.w && P.h == f.h && P.out == f.out && P.out_cap == f.cap);
        wg += static_cast<int64_t>(P.gx) * P.mcu_rows; iv += P.mcu_rows; rows += P.mcu_rows; cost += P.mcu_rows * g.row_cost();
        // its coefficients and slots: behind the piece before it, inside the scratch
        REQUIRE(reinterpret_cast<uint8_t*>(P.coef) == scratch + coef_end && P.slots == scratch + slot_end);
        coef_end += static_cast<size_t>(P.mcu_rows) * static_cast<size_t>(g.row_blocks) * 128;
        slot_end += static_cast<size_t>(P.mcu_rows) * static_cast<size_t>(g.slot);
        REQUIRE((reinterpret_cast<uintptr_t>(P.coef) & 15) == 0 && (reinterpret_cast<uintptr_t>(P.slots) & 15) == 0);
        // its tables and its header: inside the table block, and the right ones
        const size_t tab_at = static_cast<size_t>(reinterpret_cast<const uint8_t*>(P.tab) - dev);
        REQUIRE(tab_at + sizeof(JpegTables) <= R.at_heads && tab_at % sizeof(JpegTables) == 0);
        JpegTables want;
        jpeg_enc_tables(f.quality, &want);
        REQUIRE(std::memcmp(host.get() + tab_at, &want, sizeof want) == 0);
        if (P.mcu_row0 == 0) {
          const size_t at = static_cast<size_t>(P.head - dev);
          REQUIRE(P.head_len == kJpegHeaderBytes && at >= R.at_heads && at + static_cast<size_t>(P.head_len) <= R.at_pieces);
          const std::vector<uint8_t> head = jpeg_enc_header(f.w, f.h, f.subsampling, want, g.mcus_x);
          REQUIRE(static_cast<int>(head.size()) == kJpegHeaderBytes && std::memcmp(host.get() + at, head.data(), head.size()) == 0);
          REQUIRE(P.head_len + 2 <= P.out_cap);
        } else {
          REQUIRE(P.head == nullptr && P.head_len == 0);
        }
      }
      REQUIRE(wg == R.wgs && iv == R.ivs && coef_end <= R.at_slots && slot_end == R.scratch_bytes);
      REQUIRE(cost <= budget || rows == 1);
      REQUIRE(R.scratch_bytes <= static_cast<size_t>(cost) + 256);
      ++round; ++total_rounds; total_pieces += p1 - p0;
      p0 = p1;
    }
  }
  // bad arguments
  {
    int64_t w1 = 16, h1 = 16, big = 65536, zero = 0; int s1 = IST_JPEG_420, sbad = 2;
    REQUIRE(ist_jpeg_batch_layout(&w1, &h1, &s1, 1, 0, nullptr, 0) == 1);
    REQUIRE(ist_jpeg_batch_layout(&w1, &h1, &s1, 0, 0, nullptr, 0) < 0 && ist_jpeg_batch_layout(nullptr, &h1, &s1, 1, 0, nullptr, 0) < 0);
    REQUIRE(ist_jpeg_batch_layout(&big, &h1, &s1, 1, 0, nullptr, 0) < 0 && ist_jpeg_batch_layout(&w1, &zero, &s1, 1, 0, nullptr, 0) < 0);
    REQUIRE(ist_jpeg_batch_layout(&w1, &h1, &sbad, 1, 0, nullptr, 0) < 0 && ist_jpeg_batch_layout(&w1, &h1, &s1, 1, -1, nullptr, 0) < 0);
    REQUIRE(ist_jpeg_batch_layout(&w1, &h1, &s1, 1, 0, nullptr, -1) < 0);
  }
  std::printf("jpeg batch host: %d batches, %lld rounds, %lld pieces: ok\n", iters, static_cast<long long>(total_rounds), static_cast<long long>(total_pieces));
  return 0;
}
