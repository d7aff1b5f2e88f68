// ist_jpeg_enc.h — the JPEG export's host side that needs no device (ist_jpeg_enc_host.cpp): tables, the file header, the geometry
// of a canvas, and how a batch of canvases is cut into rounds and pieces; plus what the batch entry points share.
// The kernels and the two encoders are in ist_jpeg_encode.hip.
#ifndef IST_JPEG_ENC_H_
#define IST_JPEG_ENC_H_

#include <cstddef>
#include <cstdint>
#include <functional>
#include <vector>

#include "../../include/imagestitch.h"

struct ist_ctx;

namespace ist {

constexpr size_t kJpegEncBudget = 256u << 20;     // coefficient scratch + interval slots of one slab (one round of a batch)
constexpr int kJpegBlockBits = 22 + 63 * 26;      // most bits of one block: DC code 11 + 11 magnitude bits, 63 x (AC code 16 + 10)
constexpr int kJpegBlockBytes = 2 * kJpegBlockBits / 8;      // ... as bytes when every byte is 0xFF and stuffed: 415
static_assert(kJpegBlockBits == 1660 && kJpegBlockBytes * 8 == 2 * kJpegBlockBits, "slot bound");
constexpr int kJpegHeaderBytes = 629;             // SOI ... SOS of every file with the Annex K tables; the most with optimised ones
// IST_JPEG_OPTIMIZE: a DC code may be 16 bits long: 27 + 63 x 26 bits, 417 bytes
constexpr int kJpegBlockBitsWide = 27 + 63 * 26;
constexpr int kJpegBlockBytesWide = (2 * kJpegBlockBitsWide + 7) / 8;
static_assert(kJpegBlockBitsWide == 1665 && kJpegBlockBytesWide == 417, "slot bound of optimised files");
constexpr int kJpegCounters = 2 * (16 + 256);     // symbol counts of one file: per slot, 16 DC sizes then 256 AC symbols (int64 each)

inline bool jpeg_ss_known(int subsampling) { const int b = subsampling & ~IST_JPEG_OPTIMIZE; return b == IST_JPEG_444 || b == IST_JPEG_420; }
inline bool jpeg_ss_420(int subsampling) { return (subsampling & ~IST_JPEG_OPTIMIZE) == IST_JPEG_420; }
inline bool jpeg_ss_optimize(int subsampling) { return (subsampling & IST_JPEG_OPTIMIZE) != 0; }

// what the kernels read beside the canvas: one block per quality
struct JpegTables {
  uint32_t dc[2][16];        // Huffman code of a DC size: length << 16 | code (slot 0 luma, 1 chroma)
  uint32_t ac[2][256];       // ... of an AC run/size symbol (0: the symbol has no code)
  uint8_t q[2][64];          // quantisation tables, natural order
  uint8_t zz_of[64];         // natural index -> zig-zag position
};

struct JpegGeometry {
  int mcu_w, mcu_h, bpm;         // MCU size in pixels, blocks per MCU
  int64_t mcus_x, mcus_y, row_blocks;
  int64_t slot;                  // bytes of one interval's slot (a multiple of 16)
  int block_bytes;               // most bytes of one block: 415, or 417 with optimised tables
  int64_t row_cost() const { return row_blocks * 128 + slot; }      // scratch of one MCU row: its coefficients and its slot
};
inline JpegGeometry jpeg_geometry(int64_t w, int64_t h, int subsampling) {
  JpegGeometry g;
  g.mcu_w = g.mcu_h = jpeg_ss_420(subsampling) ? 16 : 8;
  g.bpm = jpeg_ss_420(subsampling) ? 6 : 3;
  g.mcus_x = (w + g.mcu_w - 1) / g.mcu_w; g.mcus_y = (h + g.mcu_h - 1) / g.mcu_h;
  g.row_blocks = g.mcus_x * g.bpm;
  g.block_bytes = jpeg_ss_optimize(subsampling) ? kJpegBlockBytesWide : kJpegBlockBytes;
  g.slot = (g.row_blocks * g.block_bytes + 2 + 15) & ~15ll;      // + the byte the pad can add, and one so that no real length reaches it
  return g;
}

void jpeg_quant_tables(int quality, uint8_t luma[64], uint8_t chroma[64]);       // libjpeg: jpeg_quality_scaling, jpeg_add_quant_table
void jpeg_enc_tables(int quality, JpegTables* T);                                // everything the kernels read for one quality
// BITS / HUFFVAL of the four tables of a file, in DHT order: DC0, DC1, AC0, AC1
struct JpegHuffSpec { uint8_t bits[4][16]; uint8_t vals[4][256]; int n[4]; };
// the optimal table of 256 counts (>= 0), the rule of include/imagestitch.h; returns the number of values
int jpeg_optimal_table(const int64_t freq[256], uint8_t bits[16], uint8_t vals[256]);
// an optimised file's tables from its counts (kJpegCounters of them): the codes into T->dc / T->ac (0: no code), the specs into H
void jpeg_enc_tables_optimal(int quality, const int64_t* counts, JpegTables* T, JpegHuffSpec* H);
// ... the codes alone: T keeps its quantisation tables (whatever they came from)
void jpeg_enc_codes_optimal(const int64_t* counts, JpegTables* T, JpegHuffSpec* H);
// the Annex K codes beside quantisation tables that are given as data (natural order): what a lossless join writes back
void jpeg_enc_tables_of(const uint8_t luma[64], const uint8_t chroma[64], JpegTables* T);
// SOI, APP0, DQT x 2, DHT x 4 (H, or Annex K when NULL), DRI, SOF0, SOS
std::vector<uint8_t> jpeg_enc_header(int64_t w, int64_t h, int subsampling, const JpegTables& T, int64_t restart, const JpegHuffSpec* H = nullptr);

// ---- batches (ist_jpeg_encode_batch_device, ist_stitch_jpeg_batch) ----
// one file of a batch: a canvas in device memory -> its JPEG in a 16-byte aligned device buffer of `cap` >= ist_jpeg_bound bytes
struct JpegBatchFile { const void* canvas; size_t pitch; int64_t w, h; int quality, subsampling; uint8_t* out; int64_t cap; int64_t len; };

// What a workgroup of a batch kernel reads about its piece (a run of MCU rows of one file, encoded in one round).  Read through
// scalar loads: plain data, 128 bytes.
struct JpegPiece {
  const uint8_t* canvas; size_t pitch;
  const JpegTables* tab;         // the tables of the file's quality
  int16_t* coef;                 // the piece's blocks in the round's scratch
  uint8_t* slots;                // ... and its intervals' slots
  uint8_t* out; int64_t out_cap; // the file
  const uint8_t* head;           // the file's header (in the round's table block), written by the file's interval 0
  int64_t slot;                  // bytes of one slot
  int32_t w, h, is420, mcus_x, mcus_y, row_blocks, bpm, head_len;
  int32_t mcu_row0, mcu_rows;    // the piece's MCU rows (= restart intervals) of the file
  int32_t wg0, iv0;              // its first workgroup of the transform grid, its first interval of the entropy and gather grids
  int32_t gx;                    // transform workgroups per MCU row
  int32_t hist;                  // IST_JPEG_OPTIMIZE: the file's block of counters (kJpegCounters each); -1: Annex K tables, not counted
};
static_assert(sizeof(JpegPiece) == 128, "piece record");

// the pieces of a batch in encoding order (the rule of ist_jpeg_batch_layout); budget > 0
std::vector<ist_jpeg_piece> jpeg_batch_pieces(const JpegBatchFile* files, int n, int64_t budget);

// One round of a batch: pieces [p0, p1) of the list.  Where everything sits in the round's table block (one host-to-device copy)
// and in the scratch, and the sizes of the three grids.
struct JpegRound {
  int p0 = 0, p1 = 0;
  std::vector<int> quality;                      // the distinct qualities of the round's files, in order of first use
  std::vector<int> opt_files;                    // the round's files with IST_JPEG_OPTIMIZE, in order: their own tables follow the qualities'
  size_t at_tables = 0, at_heads = 0, at_pieces = 0, table_bytes = 0;
  size_t at_slots = 0, scratch_bytes = 0;        // the scratch: every piece's coefficients, then every piece's slots
  int64_t wgs = 0, ivs = 0;
};
JpegRound jpeg_round_plan(const JpegBatchFile* files, const ist_jpeg_piece* pieces, int p0, int p1);
// the host image of the round's table block.  dev / scratch: where the block and the scratch are on the device (never read here)
// An optimised file as a batch sees it: its block of counters and, once they are counted, its tables and its header.
struct JpegOptFile { int hist = -1; bool built = false; JpegTables T; std::vector<uint8_t> head; };
// opt: per file of the batch (NULL: no file is optimised).  A file whose tables are not built yet gets the Annex K codes beside its
// quantisers (what the transform reads) and a header of the most bytes.
void jpeg_round_pack(const JpegRound& R, const JpegBatchFile* files, const ist_jpeg_piece* pieces, uint8_t* host, const uint8_t* dev,
                     uint8_t* scratch, const JpegOptFile* opt = nullptr);

// ---- one file, slab by slab (ist_jpeg_encode.hip) ----
// The single-file encoder's loop with "fill the slab's scratch" left to the caller: fill(r0, rows, coef, tab, stream) enqueues on
// `stream` whatever leaves MCU rows [r0, r0 + rows) of the w x h file in `coef` (blocks in coding order, 64 int16 each in zig-zag
// order); tab: the file's tables on the device.  A canvas fills it with the transform kernel, a join with its own.  With
// IST_JPEG_OPTIMIZE and more than one slab every slab is filled twice.  synced (optional) is called behind every synchronisation of
// `stream` that follows a fill; what it returns other than IST_OK ends the call.
struct JpegSlabSource {
  std::function<int(int64_t r0, int64_t rows, int16_t* coef, const JpegTables* tab, void* stream)> fill;
  std::function<int()> synced;
};
// T: the file's quantisation tables with the Annex K codes (jpeg_enc_tables / jpeg_enc_tables_of).  `out`: device, 16-byte aligned,
// cap >= ist_jpeg_bound.  Synchronises `stream`.
int jpeg_encode_slabs(ist_ctx* ctx, int64_t w, int64_t h, int subsampling, const JpegTables& T, void* out, int64_t cap, int64_t* out_len,
                      void* stream, const JpegSlabSource& src);
int64_t jpeg_slab_rows(const JpegGeometry& g);   // MCU rows per slab: what kJpegEncBudget holds, or IST_TUNING=1 IST_JPEG_ENC_ROWS=<rows>

int64_t jpeg_batch_budget();                     // kJpegEncBudget, or IST_TUNING=1 IST_JPEG_ENC_BUDGET=<bytes> (read once)
int jpeg_batch_check(const JpegBatchFile& f, const char* what, int k);      // the rules of ist_jpeg_encode_device for file k (message: "<what> k: ...")
void count_jpeg_batch_launch();
// every file in one transform, one entropy and one gather launch per round on `stream`, which is idle when the call returns; file k is
// byte for byte what ist_jpeg_encode_device writes.  The arguments have passed jpeg_batch_check.  A message about file k names it
// "<what> ids[k]" (ids NULL: k itself).  (ist_jpeg_encode.hip)
int jpeg_encode_batch(ist_ctx* ctx, std::vector<JpegBatchFile>& files, void* stream, const char* what = "file", const int* ids = nullptr);

}  // namespace ist

#endif  // IST_JPEG_ENC_H_
