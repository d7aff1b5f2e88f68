// check_jpeg_optimize_host.cpp — drives the host side of the JPEG export's optimised Huffman tables (ist_jpeg_enc_host.cpp: the table
// builder, the codes the kernels read and the header's DHT segments) over seeded random and adversarial count vectors, under ASan +
// UBSan, on the CPU: tools/run_fuzz.sh jpegoptimize ITERS [SEED].
// The outputs are heap blocks of exactly their stated size, so that a byte written beyond one is caught; every table is checked for
// the invariants of include/imagestitch.h: one value per counted symbol, lengths 1..16, a Kraft sum that leaves the reserved point
// free, no code of all ones, HUFFVAL ordered by (length, ...) consistently with the canonical codes, a header of at most 629 bytes
// whose DHT segments hold exactly the tables.
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

// one histogram through jpeg_optimal_table; returns the number of values
static int check_table(const int64_t* freq) {
  std::unique_ptr<int64_t[]> f(new int64_t[256]);
  std::memcpy(f.get(), freq, 256 * sizeof(int64_t));
  std::unique_ptr<uint8_t[]> bits(new uint8_t[16]), vals(new uint8_t[256]);
  std::memset(vals.get(), 0xEE, 256);
  const int n = jpeg_optimal_table(f.get(), bits.get(), vals.get());
  int counted = 0, total = 0;
  for (int s = 0; s < 256; ++s) counted += freq[s] > 0;
  for (int l = 0; l < 16; ++l) total += bits[l];
  REQUIRE(n == counted && total == n);
  bool seen[256] = {false};
  for (int k = 0; k < n; ++k) { REQUIRE(freq[vals[k]] > 0 && !seen[vals[k]]); seen[vals[k]] = true; }
  // canonical codes: the code after the last one of each length stays inside the length (the reserved point, no all-ones code)
  uint32_t code = 0;
  for (int l = 1; l <= 16; ++l) {
    code += bits[l - 1];
    REQUIRE(code < (1u << l) || (n == 0 && code == 0));
    if (bits[l - 1]) REQUIRE(code - 1 < (1u << l) - 1);
    code <<= 1;
  }
  if (n == 0) for (int l = 0; l < 16; ++l) REQUIRE(bits[l] == 0);
  return n;
}

int main(int argc, char** argv) {
  const int iters = argc > 1 ? std::atoi(argv[1]) : 2000;
  std::mt19937_64 rng(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 12345);
  auto pick = [&](int64_t lo, int64_t hi) { return lo + static_cast<int64_t>(rng() % static_cast<uint64_t>(hi - lo + 1)); };
  int64_t tables = 0, deepest_header = 0;
  for (g_iter = 0; g_iter < iters; ++g_iter) {
    // the counts of one file: per slot 16 DC sizes and 256 AC symbols
    std::unique_ptr<int64_t[]> counts(new int64_t[kJpegCounters]);
    std::memset(counts.get(), 0, kJpegCounters * sizeof(int64_t));
    const int kind = static_cast<int>(pick(0, 7));
    for (int s = 0; s < 2; ++s) {
      int64_t* dc = counts.get() + s * (16 + 256); int64_t* ac = dc + 16;
      // what a file can hold: DC sizes 0..11, AC symbols with size 1..10 and run 0..15, ZRL and EOB
      std::vector<int> ac_syms{0x00, 0xF0};
      for (int r = 0; r < 16; ++r) for (int z = 1; z <= 10; ++z) ac_syms.push_back(r * 16 + z);
      const int n_dc = static_cast<int>(pick(1, 12)), n_ac = static_cast<int>(pick(1, 162));
      auto count = [&](int k) -> int64_t {
        switch (kind) {
          case 0: return pick(1, 1000);
          case 1: return pick(1, 3);                                     // ties
          case 2: return int64_t(1) << pick(0, 61);                      // deep trees: the length limit, every depth the arrays allow
          case 3: return pick(1, int64_t(1) << 40);
          case 4: return INT64_MAX - pick(0, 5);                         // sums beyond 64 bits
          case 5: return 1;
          case 6: return int64_t(1) << std::min(61, k / 3);              // a chain
          default: return k % 7 == 0 ? pick(1, 4) : (int64_t(1) << 33) + pick(0, 3);
        }
      };
      for (int k = 0; k < n_dc; ++k) dc[pick(0, 11)] = count(k);
      for (int k = 0; k < n_ac; ++k) ac[ac_syms[static_cast<size_t>(pick(0, static_cast<int64_t>(ac_syms.size()) - 1))]] = count(k);
      if (pick(0, 9) == 0) std::memset(dc, 0, 16 * sizeof(int64_t));   // (an empty histogram: no real file, still no overrun)
      int64_t f[256] = {0};
      std::memcpy(f, dc, 16 * sizeof(int64_t));
      check_table(f);
      check_table(ac);
      tables += 2;
    }
    std::unique_ptr<JpegTables> T(new JpegTables);
    std::unique_ptr<JpegHuffSpec> H(new JpegHuffSpec);
    const int quality = static_cast<int>(pick(1, 100));
    jpeg_enc_tables_optimal(quality, counts.get(), T.get(), H.get());
    JpegTables std_tables;
    jpeg_enc_tables(quality, &std_tables);
    REQUIRE(std::memcmp(T->q, std_tables.q, sizeof T->q) == 0 && std::memcmp(T->zz_of, std_tables.zz_of, sizeof T->zz_of) == 0);
    // every counted symbol has a code of 1..16 bits, no other symbol has one, and the codes are prefix-free
    for (int s = 0; s < 2; ++s) {
      const int64_t* dc = counts.get() + s * (16 + 256); const int64_t* ac = dc + 16;
      std::vector<uint32_t> codes;
      for (int k = 0; k < 16; ++k) { REQUIRE((T->dc[s][k] != 0) == (dc[k] > 0)); if (T->dc[s][k]) codes.push_back(T->dc[s][k]); }
      for (size_t a = 0; a < codes.size(); ++a)
        for (size_t b = 0; b < codes.size(); ++b) {
          const uint32_t la = codes[a] >> 16, lb = codes[b] >> 16;
          REQUIRE(la >= 1 && la <= 16 && (codes[a] & 0xFFFFu) < (1u << la) - 1u);
          if (a != b && la <= lb) REQUIRE(((codes[b] & 0xFFFFu) >> (lb - la)) != (codes[a] & 0xFFFFu));
        }
      codes.clear();
      for (int k = 0; k < 256; ++k) { REQUIRE((T->ac[s][k] != 0) == (ac[k] > 0)); if (T->ac[s][k]) codes.push_back(T->ac[s][k]); }
      for (size_t a = 0; a < codes.size(); ++a) {
        const uint32_t la = codes[a] >> 16;
        REQUIRE(la >= 1 && la <= 16 && (codes[a] & 0xFFFFu) < (1u << la) - 1u);
        for (size_t b = 0; b < codes.size(); ++b) {
          const uint32_t lb = codes[b] >> 16;
          if (a != b && la <= lb) REQUIRE(((codes[b] & 0xFFFFu) >> (lb - la)) != (codes[a] & 0xFFFFu));
        }
      }
    }
    // the header: at most 629 bytes; its four DHT segments, in the order DC0 DC1 AC0 AC1, hold exactly the tables
    const int64_t w = pick(1, 65535), h = pick(1, 65535);
    const int ss = static_cast<int>(pick(0, 1)) | IST_JPEG_OPTIMIZE;
    const JpegGeometry g = jpeg_geometry(w, h, ss);
    REQUIRE(g.block_bytes == kJpegBlockBytesWide && g.slot >= g.row_blocks * 417 + 2 && g.slot % 16 == 0);
    const std::vector<uint8_t> head = jpeg_enc_header(w, h, ss, *T, g.mcus_x, H.get());
    REQUIRE(static_cast<int>(head.size()) <= kJpegHeaderBytes && head[0] == 0xFF && head[1] == 0xD8);
    deepest_header = std::max<int64_t>(deepest_header, static_cast<int64_t>(head.size()));
    const std::vector<uint8_t> plain = jpeg_enc_header(w, h, ss & ~IST_JPEG_OPTIMIZE, std_tables, g.mcus_x);
    REQUIRE(static_cast<int>(plain.size()) == kJpegHeaderBytes);
    size_t at = 2; int dht = 0; std::vector<uint8_t> rest, rest_plain;
    while (at < head.size()) {
      REQUIRE(at + 4 <= head.size() && head[at] == 0xFF);
      const int marker = head[at + 1]; const size_t len = (size_t(head[at + 2]) << 8) | head[at + 3];
      REQUIRE(len >= 2 && at + 2 + len <= head.size());
      if (marker == 0xC4) {
        static const int want_id[4] = {0x00, 0x01, 0x10, 0x11};
        REQUIRE(dht < 4 && head[at + 4] == want_id[dht]);
        int n = 0;
        for (int l = 0; l < 16; ++l) { REQUIRE(head[at + 5 + l] == H->bits[dht][l]); n += H->bits[dht][l]; }
        REQUIRE(n == H->n[dht] && len == size_t(2 + 1 + 16 + n) && std::memcmp(&head[at + 21], H->vals[dht], static_cast<size_t>(n)) == 0);
        ++dht;
      } else {
        rest.insert(rest.end(), head.begin() + static_cast<long>(at), head.begin() + static_cast<long>(at + 2 + len));
      }
      at += 2 + len;
    }
    REQUIRE(at == head.size() && dht == 4);
    for (at = 2; at < plain.size();) {                       // everything but the DHT segments is the standard file's
      const size_t len = (size_t(plain[at + 2]) << 8) | plain[at + 3];
      if (plain[at + 1] != 0xC4) rest_plain.insert(rest_plain.end(), plain.begin() + static_cast<long>(at), plain.begin() + static_cast<long>(at + 2 + len));
      at += 2 + len;
    }
    REQUIRE(rest == rest_plain);
  }
  // the C-ABI's size rules without the flag are what they were
  REQUIRE(jpeg_geometry(100, 100, IST_JPEG_420).block_bytes == kJpegBlockBytes && jpeg_geometry(100, 100, IST_JPEG_420).slot == ((7 * 6 * 415 + 2 + 15) & ~15));
  REQUIRE(!jpeg_ss_known(0x200) && !jpeg_ss_known(0x102) && !jpeg_ss_known(-1) && !jpeg_ss_known(2) && jpeg_ss_known(0x101) && jpeg_ss_known(0x100));
  std::printf("jpeg optimize host: %d files, %lld tables, longest header %lld bytes: ok\n", iters, static_cast<long long>(tables), static_cast<long long>(deepest_header));
  return 0;
}
