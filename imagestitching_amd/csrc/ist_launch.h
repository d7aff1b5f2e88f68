// ist_launch.h — kernel argument block + launch entry shared by ist_kernels.hip and ist_runtime.cpp
#ifndef IST_LAUNCH_H_
#define IST_LAUNCH_H_

#include "ist_internal.h"

namespace ist {

// Source pointers travel BY VALUE in the kernarg segment (2 KiB for 128 images): a stitch can be re-launched on
// new buffers with no table upload and no host synchronisation.  The reference UI caps a stitch at 9 images
// (pages/index/index.js:311); BASELINE config 5 uses 64.
constexpr int kMaxImages = 128;

struct LaunchArgs {
  uint8_t* dst;
  size_t dst_pitch;
  const DevOp* ops;
  const DevCell* cells;
  const DevBand* bands;
  const int32_t* stacks;
  const DevTile* tiles;     // per-tile table, or NULL (then the band / cell prefixes are searched)
  int32_t n_cells;
  int32_t filter;
  int32_t lds_words;        // dynamic LDS the SAMPLE_LDS cells need (32-bit words); 0 when the job has none
  int32_t n_bands;
  int32_t lds_half;         // SAMPLE_LDS footprint buffer (32-bit words)
  int32_t pad_;
  const uint8_t* src[kMaxImages];
  size_t pitch[kMaxImages];
};

// The kernel form a job needs (Compiled::kernel_kind, set by ist_compile.cpp): the instantiation with just the paths of the job's
// cells is launched - the fewer paths, the fewer registers.  THE list: ist_kernels.hip maps each kind to its paths once
// (kind_paths), ist_batch.cpp groups a batch by kind.  The values are part of ist_debug_cells' output: they stay.
enum KernelKind : int32_t {
  KIND_COPY = 0,            // FILL / COPY cells only
  KIND_SAMPLE = 1,          // + axis-aligned resampling (SAMPLE, SAMPLE_LDS, SAMPLE_STREAM)
  KIND_GENERAL = 2,         // + quarter turns (SWAP_LDS) and per-pixel paint stacks (GENERAL), no box filter
  KIND_AREA = 3,            // KIND_SAMPLE + the streamed box filter (AREA_STREAM)
  KIND_FULL = 4,            // KIND_GENERAL + AREA_STREAM: every path but the cubic one
  KIND_CUBIC = 5,           // IST_FILTER_CUBIC jobs that resample: FILL / COPY / AREA_STREAM / CUBIC_STREAM
  KIND_CUBIC_GENERAL = 6    // + the per-pixel paint stack under the cubic rule (no such job holds a bilinear cell)
};
constexpr int kKernelKinds = 7;
int launch_stitch(const LaunchArgs& args, int64_t n_tiles, int kind, void* stream);

// Several jobs of one kind in ONE launch (ist_jobs_launch).  Three device tables, uploaded per launch:
//   jobs[n_jobs]            each job's LaunchArgs, as ist_job_launch would pass them by value
//   tile_begin[n_jobs + 1]  first tile of every job (tiles are numbered job-major); tile_begin[n_jobs] = n_tiles
//   chunk_job[n_chunks + 1] the job holding tile c << kBatchChunkLg (the last entry: n_jobs - 1)
constexpr int kBatchChunkLg = 6;             // chunks of 64 tiles
constexpr int kMaxBatchJobs = 4096;
struct BatchArgs {
  const LaunchArgs* jobs;
  const int64_t* tile_begin;
  const int32_t* chunk_job;
  int64_t n_tiles;
};
int launch_stitch_batch(const BatchArgs& args, int kind, unsigned dyn_lds_bytes, void* stream);

// The preview shrink (ist_preview.hip): a w x h RGBA8 source -> pw x ph, both axes shrinking.  Stage 1 runs groups * chunks * ph
// workgroups, each over <= chunk_rows source rows of one output row's box and the x footprint of per_group neighbouring output
// pixels (passes x 256 columns), and leaves one float4 per (output row, chunk, output pixel) in `partial`; stage 2 adds the chunks.
struct PreviewArgs {
  const uint8_t* src;
  size_t src_pitch;
  uint8_t* dst;
  size_t dst_pitch;
  float* partial;           // ph * chunks * pw entries of 4 floats, 16-byte aligned
  double kx, ky;            // w / pw, h / ph
  int32_t w, h, pw, ph;
  int32_t per_group;        // output pixels per workgroup along x
  int32_t groups;           // ceil(pw / per_group)
  int32_t passes;           // 256-column passes over a group's footprint (> 1 only with per_group == 1)
  int32_t sub;              // lanes per output pixel in the column sum: a power of two, 1 .. 64
  int32_t chunk_rows;       // source rows per workgroup, a multiple of 4
  int32_t chunks;           // ceil(tallest box / chunk_rows)
  int32_t turn;             // batch launches only (kTurn* below): where stage 2 stores pixel (X, Y); the single-image kernels store it at (X, Y)
  int32_t pad_;
};
// the geometry above for a shape (pure CPU); false when an axis does not shrink or the source is too large for the kernel's ints
bool preview_geometry(int64_t w, int64_t h, int32_t pw, int32_t ph, PreviewArgs* out);
int launch_preview(const PreviewArgs& args, bool opaque, void* stream);

// Many reduces of one form (opaque or not) in ONE launch per stage (ist_thumbs_device).  Three device tables, uploaded per launch:
//   items[n]          each reduce's PreviewArgs, as launch_preview would pass them by value; `partial` is the item's own range of the
//                     scratch, `dst` / `dst_pitch` those of the TURNED image ((turn & kTurnTranspose) ? ph x pw : pw x ph)
//   wg_begin[n + 1]   first stage-1 workgroup of every item (groups * chunks * ph each); wg_begin[n] = the grid
//   px_begin[n + 1]   first stage-2 thread of every item: pw * ph rounded up to whole workgroups of 256 each, so that a workgroup
//                     never straddles two items and the lookup stays wave-uniform
// The turn: reduced pixel (X, Y) is mirrored inside the reduced image (kTurnFlipX: X -> pw - 1 - X, kTurnFlipY likewise), then
// kTurnTranspose swaps the two coordinates.
enum : int32_t { kTurnFlipX = 1, kTurnFlipY = 2, kTurnTranspose = 4 };
struct PreviewBatchArgs {
  const PreviewArgs* items;
  const int64_t* wg_begin;
  const int64_t* px_begin;
  int32_t n;
  int32_t pad_;
};
int launch_preview_batch(const PreviewBatchArgs& args, int64_t n_wgs, int64_t n_px, bool opaque, void* stream);

}  // namespace ist

#endif  // IST_LAUNCH_H_
