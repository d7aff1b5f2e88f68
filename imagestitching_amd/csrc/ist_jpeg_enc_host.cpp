// ist_jpeg_enc_host.cpp — the JPEG export's host side that needs no device: the Annex K tables, the file header, and how a batch
// of canvases is cut into rounds and pieces and described to the batch kernels (ist_jpeg_encode.hip).  Nothing here calls the
// runtime, so all of it runs, and is checked, without a GPU.
//
// Reference anchor: the export seam, safeCanvasToTempFilePath(canvas, prefer) -> wx.canvasToTempFilePath({fileType: prefer})
// (utils/canvas.js:205-221), for N independent requests.  The file is pinned by include/imagestitch.h ("export: baseline JPEG").
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

#include "ist_internal.h"
#include "ist_jpeg_enc.h"

namespace ist {

namespace {

// T.81 Annex K: the example quantisation tables K.1 / K.2 (natural order) and the Huffman tables K.3 - K.6 (BITS, HUFFVAL)
const uint8_t kQLuma[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                            14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                            49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const uint8_t kQChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                              47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                              99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
const uint8_t kZigzag[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13,
                             6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38,
                             31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};       // zig-zag position -> natural index
const uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
const uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
const uint8_t kAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
     0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
     0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
     0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
     0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
     0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
     0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
     0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
     0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
     0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
     0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
     0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
     0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

void huff_codes(const uint8_t* bits, const uint8_t* vals, uint32_t* out) {       // T.81 C.2: canonical codes
  uint32_t code = 0; int k = 0;
  for (int l = 1; l <= 16; ++l) {
    for (int i = 0; i < bits[l - 1]; ++i) out[vals[k++]] = (static_cast<uint32_t>(l) << 16) | code++;
    code <<= 1;
  }
}

void seg(std::vector<uint8_t>* o, int marker, const std::vector<uint8_t>& body) {
  o->push_back(0xFF); o->push_back(static_cast<uint8_t>(marker));
  o->push_back(static_cast<uint8_t>((body.size() + 2) >> 8)); o->push_back(static_cast<uint8_t>((body.size() + 2) & 255));
  o->insert(o->end(), body.begin(), body.end());
}

}  // namespace

void jpeg_quant_tables(int quality, uint8_t luma[64], uint8_t chroma[64]) {
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int i = 0; i < 64; ++i) {
    luma[i] = static_cast<uint8_t>(std::min(255, std::max(1, (kQLuma[i] * scale + 50) / 100)));
    chroma[i] = static_cast<uint8_t>(std::min(255, std::max(1, (kQChroma[i] * scale + 50) / 100)));
  }
}

// T.81 K.2 with the tie rules of include/imagestitch.h ("the table of one histogram").  257 leaves at most, so the quadratic
// search for the two smallest nodes is some 10^5 steps; a tree may be as deep as its leaves are many (no limit but the arrays').
int jpeg_optimal_table(const int64_t freq[256], uint8_t bits[16], uint8_t vals[256]) {
  constexpr int kLeaves = 257;
  typedef unsigned __int128 Weight;               // (257 counts of up to 2^63 - 1)
  Weight weight[kLeaves];
  int id[kLeaves], owner[kLeaves], size[kLeaves];  // a node lives at the index of the leaf that founded it; owner: a leaf's node
  bool alive[kLeaves];
  int nodes = 0;
  for (int s = 0; s < kLeaves; ++s) {
    const int64_t f = s < 256 ? freq[s] : 1;
    alive[s] = f > 0; weight[s] = static_cast<Weight>(f > 0 ? f : 0); id[s] = s; owner[s] = s; size[s] = 0;
    nodes += alive[s];
  }
  std::memset(bits, 0, 16);
  if (nodes == 1) return 0;                        // nothing but the reserved symbol
  for (; nodes > 1; --nodes) {
    int a = -1, b = -1;                            // the smallest and the second smallest by (weight, id)
    for (int k = 0; k < kLeaves; ++k) {
      if (!alive[k]) continue;
      auto less = [&](int x, int y) { return weight[x] < weight[y] || (weight[x] == weight[y] && id[x] < id[y]); };
      if (a < 0 || less(k, a)) { b = a; a = k; }
      else if (b < 0 || less(k, b)) b = k;
    }
    for (int s = 0; s < kLeaves; ++s)
      if (owner[s] == a || owner[s] == b) { ++size[s]; owner[s] = a; }
    weight[a] += weight[b]; id[a] = std::min(id[a], id[b]); alive[b] = false;
  }
  int count[kLeaves + 1] = {0};                    // BITS before the limit: a size is at most 256
  for (int s = 0; s < kLeaves; ++s)
    if (owner[s] == owner[256]) ++count[size[s]];  // (every leaf that took part ends in the one node left)
  int i = kLeaves - 1;
  for (; i > 16; --i)                              // figure K.3
    while (count[i] > 0) {
      int j = i - 2;
      while (j > 0 && count[j] == 0) --j;
      count[i] -= 2; count[i - 1] += 1; count[j + 1] += 2; count[j] -= 1;
    }
  while (count[i] == 0) --i;
  --count[i];                                      // the reserved code point
  for (int l = 1; l <= 16; ++l) bits[l - 1] = static_cast<uint8_t>(count[l]);
  int n = 0;
  for (int l = 1; l < kLeaves; ++l)                // by (size before the limit, symbol)
    for (int s = 0; s < 256; ++s)
      if (freq[s] > 0 && size[s] == l) vals[n++] = static_cast<uint8_t>(s);
  return n;
}

void jpeg_enc_tables_optimal(int quality, const int64_t* counts, JpegTables* T, JpegHuffSpec* H) {
  jpeg_enc_tables(quality, T);
  jpeg_enc_codes_optimal(counts, T, H);
}

void jpeg_enc_codes_optimal(const int64_t* counts, JpegTables* T, JpegHuffSpec* H) {
  std::memset(T->dc, 0, sizeof T->dc); std::memset(T->ac, 0, sizeof T->ac);
  std::memset(H, 0, sizeof *H);
  for (int tc = 0; tc < 2; ++tc)
    for (int s = 0; s < 2; ++s) {
      int64_t freq[256] = {0};
      const int64_t* c = counts + s * (16 + 256) + (tc ? 16 : 0);
      for (int k = 0; k < (tc ? 256 : 16); ++k) freq[k] = c[k];
      const int t = tc * 2 + s;
      H->n[t] = jpeg_optimal_table(freq, H->bits[t], H->vals[t]);
      if (tc) {
        huff_codes(H->bits[t], H->vals[t], T->ac[s]);
      } else {
        uint32_t codes[256] = {0};                 // (counts of sizes above 11 cannot be: the difference is clamped; no code leaves T->dc)
        huff_codes(H->bits[t], H->vals[t], codes);
        std::memcpy(T->dc[s], codes, sizeof T->dc[s]);
      }
    }
}

void jpeg_enc_tables(int quality, JpegTables* T) {
  std::memset(T, 0, sizeof *T);
  for (int s = 0; s < 2; ++s) { huff_codes(kDcBits[s], kDcVals, T->dc[s]); huff_codes(kAcBits[s], kAcVals[s], T->ac[s]); }
  jpeg_quant_tables(quality, T->q[0], T->q[1]);
  for (int k = 0; k < 64; ++k) T->zz_of[kZigzag[k]] = static_cast<uint8_t>(k);
}

void jpeg_enc_tables_of(const uint8_t luma[64], const uint8_t chroma[64], JpegTables* T) {
  jpeg_enc_tables(50, T);
  std::memcpy(T->q[0], luma, 64); std::memcpy(T->q[1], chroma, 64);
}

std::vector<uint8_t> jpeg_enc_header(int64_t w, int64_t h, int subsampling, const JpegTables& T, int64_t restart, const JpegHuffSpec* H) {
  std::vector<uint8_t> o{0xFF, 0xD8};
  seg(&o, 0xE0, {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
  for (int s = 0; s < 2; ++s) {
    std::vector<uint8_t> b{static_cast<uint8_t>(s)};
    for (int k = 0; k < 64; ++k) b.push_back(T.q[s][kZigzag[k]]);
    seg(&o, 0xDB, b);
  }
  for (int tc = 0; tc < 2; ++tc)
    for (int s = 0; s < 2; ++s) {
      std::vector<uint8_t> b{static_cast<uint8_t>(tc * 16 + s)};
      if (H) {
        const int t = tc * 2 + s;
        b.insert(b.end(), H->bits[t], H->bits[t] + 16);
        b.insert(b.end(), H->vals[t], H->vals[t] + H->n[t]);
      } else {
        const uint8_t* bits = tc ? kAcBits[s] : kDcBits[s];
        b.insert(b.end(), bits, bits + 16);
        if (tc) b.insert(b.end(), kAcVals[s], kAcVals[s] + 162); else b.insert(b.end(), kDcVals, kDcVals + 12);
      }
      seg(&o, 0xC4, b);
    }
  seg(&o, 0xDD, {static_cast<uint8_t>(restart >> 8), static_cast<uint8_t>(restart & 255)});
  const uint8_t hv = jpeg_ss_420(subsampling) ? 0x22 : 0x11;
  seg(&o, 0xC0, {8, static_cast<uint8_t>(h >> 8), static_cast<uint8_t>(h & 255), static_cast<uint8_t>(w >> 8), static_cast<uint8_t>(w & 255), 3,
                 1, hv, 0, 2, 0x11, 1, 3, 0x11, 1});
  seg(&o, 0xDA, {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
  return o;
}

// ---- batches -----------------------------------------------------------------------------------------------------------
// Greedy, in file order, MCU row by MCU row: a round closes when the next row would not fit; a row above the budget has a round
// to itself.  A piece is the run of rows of one file that one round holds.
std::vector<ist_jpeg_piece> jpeg_batch_pieces(const JpegBatchFile* files, int n, int64_t budget) {
  std::vector<ist_jpeg_piece> out;
  int32_t round = 0;
  int64_t used = 0;
  for (int f = 0; f < n; ++f) {
    const JpegGeometry g = jpeg_geometry(files[f].w, files[f].h, files[f].subsampling);
    const int64_t cost = g.row_cost();
    for (int64_t r = 0; r < g.mcus_y;) {
      if (used > 0 && used + cost > budget) { ++round; used = 0; }
      const int64_t rows = std::min(std::max<int64_t>(1, (budget - used) / cost), g.mcus_y - r);
      out.push_back(ist_jpeg_piece{f, round, static_cast<int32_t>(r), static_cast<int32_t>(rows)});
      used += rows * cost;
      r += rows;
    }
  }
  return out;
}

JpegRound jpeg_round_plan(const JpegBatchFile* files, const ist_jpeg_piece* pieces, int p0, int p1) {
  JpegRound R;
  R.p0 = p0; R.p1 = p1;
  size_t heads = 0, coef = 0, slots = 0;
  for (int p = p0; p < p1; ++p) {
    const JpegBatchFile& f = files[pieces[p].file];
    const JpegGeometry g = jpeg_geometry(f.w, f.h, f.subsampling);
    if (jpeg_ss_optimize(f.subsampling)) {
      if (R.opt_files.empty() || R.opt_files.back() != pieces[p].file) R.opt_files.push_back(pieces[p].file);
    } else if (std::find(R.quality.begin(), R.quality.end(), f.quality) == R.quality.end()) {
      R.quality.push_back(f.quality);
    }
    if (pieces[p].mcu_row0 == 0) heads += (kJpegHeaderBytes + 15) & ~size_t(15);
    const int64_t gx = jpeg_ss_420(f.subsampling) ? g.mcus_x : (g.mcus_x + 3) / 4;
    R.wgs += gx * pieces[p].mcu_rows;
    R.ivs += pieces[p].mcu_rows;
    coef += static_cast<size_t>(pieces[p].mcu_rows * g.row_blocks) * 128;
    slots += static_cast<size_t>(pieces[p].mcu_rows * g.slot);
  }
  R.at_tables = 0;
  R.at_heads = round256((R.quality.size() + R.opt_files.size()) * sizeof(JpegTables));
  R.at_pieces = round256(R.at_heads + heads);
  R.table_bytes = R.at_pieces + static_cast<size_t>(p1 - p0) * sizeof(JpegPiece);
  R.at_slots = round256(coef);
  R.scratch_bytes = R.at_slots + slots;
  return R;
}

void jpeg_round_pack(const JpegRound& R, const JpegBatchFile* files, const ist_jpeg_piece* pieces, uint8_t* host, const uint8_t* dev,
                     uint8_t* scratch, const JpegOptFile* opt) {
  std::memset(host, 0, R.table_bytes);
  JpegTables* tabs = reinterpret_cast<JpegTables*>(host + R.at_tables);
  for (size_t q = 0; q < R.quality.size(); ++q) jpeg_enc_tables(R.quality[q], &tabs[q]);
  for (size_t k = 0; k < R.opt_files.size(); ++k) {
    const int f = R.opt_files[k];
    if (opt && opt[f].built) tabs[R.quality.size() + k] = opt[f].T; else jpeg_enc_tables(files[f].quality, &tabs[R.quality.size() + k]);
  }
  JpegPiece* rec = reinterpret_cast<JpegPiece*>(host + R.at_pieces);
  size_t head_at = R.at_heads, coef_at = 0, slot_at = R.at_slots;
  int64_t wg = 0, iv = 0;
  for (int p = R.p0; p < R.p1; ++p) {
    const JpegBatchFile& f = files[pieces[p].file];
    const JpegGeometry g = jpeg_geometry(f.w, f.h, f.subsampling);
    const bool optimize = jpeg_ss_optimize(f.subsampling);
    const size_t q = optimize ? R.quality.size() + static_cast<size_t>(std::find(R.opt_files.begin(), R.opt_files.end(), pieces[p].file) - R.opt_files.begin())
                              : static_cast<size_t>(std::find(R.quality.begin(), R.quality.end(), f.quality) - R.quality.begin());
    JpegPiece& P = rec[p - R.p0];
    P.canvas = static_cast<const uint8_t*>(f.canvas); P.pitch = f.pitch;
    P.tab = reinterpret_cast<const JpegTables*>(dev + R.at_tables) + q;
    P.coef = reinterpret_cast<int16_t*>(scratch + coef_at);
    P.slots = scratch + slot_at;
    P.out = f.out; P.out_cap = f.cap;
    P.slot = g.slot;
    P.w = static_cast<int32_t>(f.w); P.h = static_cast<int32_t>(f.h); P.is420 = jpeg_ss_420(f.subsampling);
    P.mcus_x = static_cast<int32_t>(g.mcus_x); P.mcus_y = static_cast<int32_t>(g.mcus_y);
    P.row_blocks = static_cast<int32_t>(g.row_blocks); P.bpm = g.bpm;
    P.mcu_row0 = pieces[p].mcu_row0; P.mcu_rows = pieces[p].mcu_rows;
    P.wg0 = static_cast<int32_t>(wg); P.iv0 = static_cast<int32_t>(iv);
    P.gx = static_cast<int32_t>(P.is420 ? g.mcus_x : (g.mcus_x + 3) / 4);
    P.hist = optimize && opt ? opt[pieces[p].file].hist : -1;
    if (P.mcu_row0 == 0) {
      const bool own = optimize && opt && opt[pieces[p].file].built;
      const std::vector<uint8_t> head = own ? opt[pieces[p].file].head : jpeg_enc_header(f.w, f.h, f.subsampling, tabs[q], g.mcus_x);
      std::memcpy(host + head_at, head.data(), head.size());
      P.head = dev + head_at; P.head_len = static_cast<int32_t>(head.size());
      head_at += (kJpegHeaderBytes + 15) & ~size_t(15);
    }
    wg += static_cast<int64_t>(P.gx) * P.mcu_rows; iv += P.mcu_rows;
    coef_at += static_cast<size_t>(P.mcu_rows * g.row_blocks) * 128;
    slot_at += static_cast<size_t>(P.mcu_rows * g.slot);
  }
}

int64_t jpeg_batch_budget() {
  static const int64_t knob = (tuning_mode() && std::getenv("IST_JPEG_ENC_BUDGET")) ? std::atoll(std::getenv("IST_JPEG_ENC_BUDGET")) : 0;
  return knob > 0 ? knob : static_cast<int64_t>(kJpegEncBudget);
}

}  // namespace ist

using namespace ist;

extern "C" {

int64_t ist_jpeg_batch_layout(const int64_t* w, const int64_t* h, const int* subsampling, int n, int64_t budget_bytes, ist_jpeg_piece* out,
                              int64_t cap) {
  if (n < 1 || !w || !h || !subsampling || budget_bytes < 0 || cap < 0) return -1;
  std::vector<JpegBatchFile> files(static_cast<size_t>(n));
  for (int k = 0; k < n; ++k) {
    if (w[k] < 1 || h[k] < 1 || w[k] > 65535 || h[k] > 65535 || !jpeg_ss_known(subsampling[k])) return -1;
    files[static_cast<size_t>(k)] = JpegBatchFile{nullptr, 0, w[k], h[k], 0, subsampling[k], nullptr, 0, 0};
  }
  const std::vector<ist_jpeg_piece> pieces = jpeg_batch_pieces(files.data(), n, budget_bytes > 0 ? budget_bytes : jpeg_batch_budget());
  if (out)
    for (size_t p = 0; p < pieces.size() && static_cast<int64_t>(p) < cap; ++p) out[p] = pieces[p];
  return static_cast<int64_t>(pieces.size());
}

}  // extern "C"
