// ist_jpeg_join.h — the lossless JPEG join (include/imagestitch.h, "lossless JPEG joins"): what its host side that needs no device
// (ist_jpeg_join_host.cpp: eligibility, geometry, the per-image table) shares with the entry point and the kernel (ist_jpeg_join.hip).
// The block mapping is ONE function for the kernel and the host, so that the host check (tools/check_jpeg_join_host.cpp) walks exactly
// what the kernel walks.
#ifndef IST_JPEG_JOIN_H_
#define IST_JPEG_JOIN_H_

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/imagestitch.h"
#include "ist_jpeg.h"

#if defined(__HIPCC__)
#define IST_JOIN_HD __host__ __device__
#else
#define IST_JOIN_HD
#endif

namespace ist {

constexpr int kJoinMaxImages = 128;
constexpr int kJoinBlocksPerWg = 32;            // 8 lanes per 128-byte block, 256 threads

// what the eligibility check keeps of one file (from its headers alone)
struct JoinFile { int32_t w, h, mcus_x, mcus_y; };
// an eligible set: the joined file's geometry and the tables it carries
struct JoinPlan {
  int n = 0, direction = 0, subsampling = 0;    // IST_JPEG_444 / IST_JPEG_420: image 0's layout, and so every image's
  int64_t width = 0, height = 0;
  int64_t mcus_x = 0, mcus_y = 0;               // of the joined file
  uint8_t q[2][64];                             // image 0's luma and chroma tables, natural order
  std::vector<JoinFile> files;
};

// The rule of include/imagestitch.h over the files' headers (jpeg_parse_tables: the decoder's own parser).  IST_OK and *plan filled, or
// IST_E_UNSUPPORTED with info->reason / image and the message set.  The arguments have been checked.  info is never NULL.
int jpeg_join_eligible(const uint8_t* const* files, const int64_t* lens, int n, int direction, ist_jpeg_join_info* info, JoinPlan* plan);
const char* jpeg_join_reason_text(int reason);

// ---- what the kernel reads beside the coefficient planes: plain data, one host-to-device copy ----
// first[i]: the joined file's first MCU row (vertical) or MCU column (horizontal) of image i; first[n] = the total.  Unused entries
// repeat the total, so that a search over the whole array is a search over [0, n].
struct JoinImage { const int16_t* coef[3]; int32_t blocks_x[3]; int32_t blocks_y[3]; };
struct JoinTable {
  int32_t first[kJoinMaxImages + 1];
  int32_t n, pad_[2];
  JoinImage img[kJoinMaxImages];
};
static_assert(sizeof(JoinImage) == 48 && sizeof(JoinTable) % 16 == 0, "join table");

// the table of a plan and its files' planes; IST_E_DECODE when a file's planes are not what its header promised
int jpeg_join_table(const JoinPlan& plan, const JpegCoefPlanes* planes, JoinTable* out);

// the largest i in [0, n) with first[i] <= key, for 0 <= key < first[n]
IST_JOIN_HD inline int join_find(const int32_t* first, int n, int32_t key) {
  int lo = 0, hi = n;                            // first[lo] <= key < first[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (first[mid] <= key) lo = mid; else hi = mid;
  }
  return lo;
}

// Block `block` (coding order: MCU by MCU; 4:2:0 Y00 Y01 Y10 Y11 Cb Cr, 4:4:4 Y Cb Cr) of MCU row `mcu_row` of the joined file:
// its source image, its component and its place (bx, by) in that image's plane.
struct JoinSource { int32_t image, comp, bx, by; };
IST_JOIN_HD inline JoinSource join_source(const int32_t* first, int n, int horizontal, int is420, int32_t mcu_row, int32_t block) {
  const int bpm = is420 ? 6 : 3;
  const int32_t m = block / bpm;
  const int k = block - m * bpm;
  const int32_t key = horizontal ? m : mcu_row;
  JoinSource s;
  s.image = join_find(first, n, key);
  const int32_t local = key - first[s.image];
  const int32_t lm = horizontal ? local : m, lr = horizontal ? mcu_row : local;
  if (is420 && k < 4) { s.comp = 0; s.bx = 2 * lm + (k & 1); s.by = 2 * lr + (k >> 1); }
  else { s.comp = is420 ? k - 3 : k; s.bx = lm; s.by = lr; }
  return s;
}

// ---- the kernel's launch (ist_jpeg_join.hip) ----
struct JoinArgs {
  const JoinTable* __restrict__ table;          // device
  int16_t* __restrict__ coef;                   // the slab: MCU rows [mcu_row0, mcu_row0 + rows) of the joined file, coding order, zig-zag order
  uint32_t* flag;                               // set to 1 when a coefficient is outside the range the entropy coder codes without a clamp
  int32_t horizontal, is420, row_blocks, mcu_row0;
};
// fills rows MCU rows of the slab on `stream`; counted by ist_debug_jpeg_join_launches
int jpeg_join_launch(const JoinArgs& args, int64_t rows, void* stream);

}  // namespace ist

#endif  // IST_JPEG_JOIN_H_
