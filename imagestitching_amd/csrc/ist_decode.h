// ist_decode.h — files -> bitmaps in HBM (ist_decode.cpp), as far as the file pipeline (ist_files.cpp) and the resident bitmaps
// (ist_bitmap.cpp) need it.
#ifndef IST_DECODE_H_
#define IST_DECODE_H_

#include <chrono>
#include <functional>
#include <string>
#include <vector>

#include "ist_ctx.h"
#include "ist_icc.h"

namespace ist {

// what is known of one file: after FileDecoder::headers() the size and orientation, after its worker the decoded form
struct Dec { int rc = 0; std::string err; bool jpeg = false; JpegImage J; JpegGpuScan G; int w = 0, h = 0, orient = 0; std::vector<uint8_t> px;
             ist_color_tables color = {}; };      // color: the file's profile, read by its worker when the call converts to sRGB (kind NONE otherwise)

// phase clock: stderr lines under IST_TIMING=1, numbers for ist_ctx_last_timing when the context asked for them.  Phases
// end with a stream synchronisation only while one of the two is on.  record: the call's timing setting (its snapshot, ist_settings.h).
struct Phases {
  ist_ctx* ctx; bool record, print, on;
  std::chrono::steady_clock::time_point t_prev;
  Phases(ist_ctx* c, bool timing);
  void lap(int phase, const char* what, hipStream_t st);
};

// where one image's JPEG stages live on the device: offsets into TWO arenas - `main` (coefficient planes, quantisation
// tables, sample planes: sized from the frame header alone, so it can be laid out before any file is entropy-decoded) and
// `ent` (the sparse entries of a host-decoded sequential file: sized by the decode)
struct JpegDevLayout { size_t coef[3], q[3], plane[3], ent[3], start[3], cnt[3]; };

// One call's decode work.  Lifetime: construct -> headers() -> (caller lays out its arena) -> start() -> take(i) for every
// image the caller consumes, in any order -> finish().  The destructor joins whatever still runs.
class FileDecoder {
 public:
  // denom (optional): the decode denominator of each file, 1, 2, 4 or 8 (checked by the caller: check_denoms); NULL = all 1.  It
  // applies to JPEG files; every other type decodes at 1 / 1.  color_profile: the call's setting (its snapshot), for every image alike.
  FileDecoder(ist_ctx* ctx, const uint8_t* const* files, const int64_t* lens, int n, Phases* ph, int color_profile, const int32_t* denom = nullptr);
  ~FileDecoder();
  // 1. frame headers only (microseconds per file): sizes, sampling, EXIF orientation - what the planner and the arena need
  int headers();
  const Dec& dec(int i) const { return dec_[static_cast<size_t>(i)]; }
  // what the planner needs of each file (orientation from the file, like getImageInfo -> index.js:734): width / height = the natural
  // size; bmp_width / bmp_height = the scaled size of a JPEG decoded at 1 / 2, 1 / 4 or 1 / 8 (0, "as natural", for every other file)
  std::vector<ist_image_desc> descs(const int64_t* lens) const;
  // device bytes of the JPEG stages (coefficient planes, tables, sample planes), carved from *off of the caller's arena
  void layout(size_t* off);
  // 2. the workers.  arena: what layout() was sized for; img[i] / pitch[i]: where bitmap i goes (device memory)
  int start(uint8_t* arena, uint8_t* const* img, const size_t* pitch);
  // 3. bitmap i is needed by work that will be submitted to `consumer` next.  The first call waits for every image's HOST
  // side and runs the Huffman batch on `consumer`; then image i is reconstructed (or, a file the GPU path did not take,
  // uploaded / reconstructed from host coefficients) on `consumer`.  Idempotent per image; one consumer stream per call.
  int take(int i, hipStream_t consumer);
  int finish(hipStream_t consumer);       // take() for every image not taken yet
  int gpu_decoded() const;                // images the GPU entropy decoder took
  // Stopping at the coefficients (the lossless join): layout_coefficients() in place of layout() carves the dense coefficient planes
  // and nothing else (no table, no sample plane); start() then takes NULL img / pitch; coefficients() in place of take() / finish()
  // does what the first take() does (waits for the host side, runs the Huffman batch on `consumer`) and then, per file, what place()
  // does up to the planes: nothing for a file the GPU decoder took, the sparse entries uploaded and scattered into the zeroed plane
  // for a host-decoded sequential file, the dense upload for a progressive one.  No reconstruction launch, no bitmap.  Every file
  // must be a JPEG.  out[i]: the planes of file i, complete on `consumer`.
  void layout_coefficients(size_t* off);
  int coefficients(hipStream_t consumer, std::vector<JpegCoefPlanes>* out);

 private:
  int host_coefficients(int i, hipStream_t consumer, JpegDevLayout* out);
  bool coef_only_ = false;
  hipStream_t stream_of(int i) const;
  int denom_of(int i) const;
  void join_all();
  int first_error();
  int huffman_all(hipStream_t consumer);
  int chroma_all(hipStream_t consumer);
  void worker(int i);
  int place(int i, hipStream_t consumer);      // take() without the colour conversion: bitmap i lands at img_[i] on `consumer`

  ist_ctx* ctx_; const uint8_t* const* files_; const int64_t* lens_; int n_; Phases* ph_; const bool to_srgb_; const int32_t* denom_;
  std::vector<Dec> dec_;
  bool running_ = false;                                       // the context's worker pool is on this call's files
  std::vector<char> on_gpu_, taken_, uploaded_, started_, chroma_done_;      // started_: the image's stream carries uploads of this call; chroma_done_: its chroma planes were made behind the Huffman batch
  std::vector<JpegDevLayout> jo_;
  uint8_t* arena_ = nullptr; uint8_t* const* img_ = nullptr; const size_t* pitch_ = nullptr;
  bool gpu_huffman_ = true, huff_done_ = false, chroma_batch_done_ = false;
};

// files -> bitmaps in device memory: the decode of ist_decode_files_device and ist_bitmaps_decode.  Once every frame header is
// read, place(descs, img, pitch) is told what each file holds (descs[i]: size, EXIF orientation, opaque, file_size) and fills
// img[i] / pitch[i] with where bitmap i goes, or fails the call before anything is decoded.  Caller holds ctx->mu; returns with
// ctx->stream idle.  denom: as FileDecoder's (NULL = all 1); img[i] / pitch[i] then hold bitmap_w x bitmap_h of descs[i].
int check_denoms(const char* who, const int32_t* denom, int n);      // IST_E_INVALID, the message names the image: before anything is enqueued
int decode_files_locked(ist_ctx* ctx, const uint8_t* const* files, const int64_t* lens, int n, const int32_t* denom,
                        const std::function<int(const std::vector<ist_image_desc>&, uint8_t**, size_t*)>& place);

}  // namespace ist

#endif  // IST_DECODE_H_
