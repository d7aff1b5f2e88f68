// ist_ctx.h — the two opaque handles of the C-ABI and the helpers every translation unit that works on a context shares
// (device scratch, streams, job tables, readback).  Reference anchors: a context stands for the canvas node obtained at pages/index/index.js:1196-1204; a
// job for the offscreen canvas + the draws recorded on it (utils/canvas.js:131-150, index.js:1391-1428, 1532-1551).
#ifndef IST_CTX_H_
#define IST_CTX_H_

#include <hip/hip_runtime_api.h>

#include <atomic>
#include <memory>
#include <mutex>
#include <vector>

#include "ist_jpeg.h"

#include "ist_device.h"
#include "ist_host.h"
#include "ist_internal.h"
#include "ist_launch.h"

struct ist_ctx {
  int device = 0;
  ist::DevBuf scratch_src;
  ist::DevBuf scratch_dst;
  ist::DevBuf scratch_dec;          // JPEG coefficient / sample planes of ist_decode_files_device
  ist::DevBuf scratch_huff;         // GPU Huffman decoder: scans, tables, per-subsequence state
  ist::DevBuf scratch_png;          // compressing PNG encoder: one slot per 16 KiB chunk + its tables
  ist::DevBuf scratch_file;         // device image of a PNG or JPEG file on its way to the host
  ist::DevBuf scratch_jpg;          // JPEG encoder: tables, one slab of coefficients, one slot per restart interval
  ist::DevBuf scratch_jpg_counts;   // ... IST_JPEG_OPTIMIZE: 544 64-bit symbol counters per optimised file of a call
  ist::DevBuf scratch_arena;        // file pipeline: bitmaps + JPEG planes + canvas + PNG of one call
  ist::DevBuf scratch_ent;          // sparse coefficient entries of host-decoded JPEGs (progressive, restart intervals)
  // file pipeline (ist_stitch_files_png / ist_decode_files_device): one stream (img_stream, below) + event + Huffman scratch per image,
  // so that the images' decode chains (upload -> Huffman passes -> reconstruction) overlap each other and the export of the bands
  // that are already final; grow-only, made on first use
  std::vector<ist::Event> img_event;
  std::vector<ist::DevBuf> img_huff;
  std::unique_ptr<ist::WorkerPool> workers;   // parked host threads for the per-file work of a call (made on first use)
  std::vector<ist::ScanBuf> scan_bufs;        // de-stuffed scans of the last call: their memory is reused (a fresh 1.8 MB block per image and call is 450 page faults on its parse thread)
  std::vector<ist::ScanBuf> file_bufs;        // ist_stitch_paths_png: the files' bytes, read (not mapped) into blocks kept from call to call
  ist::Event render_done;
  // device blocks of destroyed jobs' tables, re-used by the next job of this context instead of a hipMalloc + hipFree pair
  // per job (a free also synchronises the device); at most kTablePool blocks are kept (the file pipeline compiles one job per image + one)
  static constexpr int kTablePool = 32;
  std::vector<ist::DevBuf> table_pool;
  std::mutex table_mu;
  std::mutex mu;                         // one host-path stitch in flight per context (index.js:772 isStitching)
  std::atomic<uint32_t> settings{ist::kDefaultSettings};   // every ist_ctx_set_* setting, packed (ist_settings.h); a call reads it ONCE: settings_of below
  std::unique_ptr<ist::Stager> stager;   // pinned staging ring, built on first use
  double last_ms[IST_PHASE_COUNT] = {0, 0, 0, 0, 0, 0, 0, 0};
  // An event that is recorded on CALLERS' streams behind the last reader of a block of the context: no wait for the context's own
  // streams covers it, so it is waited for itself before it goes - and it is declared BEHIND the blocks it guards, so that it goes first.
  struct LastUse : ist::Event { ~LastUse() { if (e) (void)hipEventSynchronize(e); } };
  // ist_jobs_launch: the per-launch job table goes up through a small ring of (pinned block, device block, event).  The event is
  // recorded behind the kernels that read the slot's device block; the slot is filled again only after it has completed.
  static constexpr int kBatchRing = 4;
  struct BatchSlot { ist::PinnedBuf host; ist::DevBuf dev; bool pending = false; LastUse done; };
  BatchSlot batch_ring[kBatchRing];
  int batch_next = 0;
  std::mutex batch_mu;
  // ist_stitch_rgba8_batch: two halves of device scratch (op tables, sources, canvases of one sub-batch each), so that one sub-batch's
  // sources go up while the previous one's canvases come down; grow-only, each bounded by the sub-batch budget (ist_batch.cpp)
  struct BatchHalf {
    ist::DevBuf tab, src, dst;
    ist::DevBuf file;                    // ist_stitch_png_batch: the sub-batch's PNG files (ist_png_bound each)
    ist::Event kernel_done;              // behind the launch that reads tab / src
    ist::Event read_done;                // behind the downloads that read dst (or file)
  };
  BatchHalf batch_half[2];
  // previews (ist_preview_host.cpp): the partial sums of the reduce, grow-only; one reduce owns them at a time - a call on another stream
  // is ordered behind the event of the one before it
  ist::DevBuf scratch_prev;
  LastUse prev_done; bool prev_pending = false; hipStream_t prev_last = nullptr;
  ist_job* prev_job = nullptr;           // the job path's last one-draw job, kept for the next preview of its shape
  int64_t prev_job_key[5] = {0, 0, 0, 0, 0};
  std::mutex prev_mu;
  // ... of the *_png_preview calls and ist_bitmap_preview: the preview's pixels on their way to the host, and the event that orders
  // the reduce behind the last render
  ist::DevBuf prev_out;
  ist::Event prev_ready;
  // overlap search (ist_overlap_host.cpp): tables, signatures, edge sums, costs and flags of one call, and the pinned block its tables go up
  // from and its results come down to; grow-only.  ovl_rows signature rows of the last call start ovl_sig_at bytes into scratch_ovl.
  ist::DevBuf scratch_ovl;
  ist::PinnedBuf ovl_host;
  int64_t ovl_rows = 0;
  size_t ovl_sig_at = 0;
  // The streams come LAST: members go in reverse order of declaration, so every stream is waited for and destroyed (Stream's
  // destructor) before the first block above is freed.  A stream added here is picked up by streams() below, which is all that
  // ist_ctx_sync and ist_ctx_destroy know about them.
  ist::Stream stream;                    // host-buffer entry points run here; the device path takes the caller's stream
  ist::Stream aux;                       // second stream of the host-path entry points (PNG slabs travel on it while later ones compress)
  ist::Stream render;                    // file pipeline: Huffman batch + per-image reconstruction + band launches, beside the PNG encoder on `stream`
  ist::Stream png2;                      // the compressing PNG encoder alternates its slabs between `stream` and this one
  ist::Stream prev_stream;               // the reduce of a *_png_preview call runs here, beside the encoder
  std::vector<ist::Stream> img_stream;   // file pipeline: the images' decode chains
  // every stream the context has made so far
  std::vector<hipStream_t> streams() const {
    std::vector<hipStream_t> v;
    for (const ist::Stream* s : {&stream, &aux, &render, &png2, &prev_stream}) if (*s) v.push_back(*s);
    for (const ist::Stream& s : img_stream) v.push_back(s);
    return v;
  }
};

namespace ist {
inline Settings settings_of(const ist_ctx* ctx) { return ctx ? settings_unpack(ctx->settings.load(std::memory_order_relaxed)) : Settings{}; }
// where a compiled job's five tables sit in the job's device block
struct DevTables {
  DevOp* ops = nullptr;
  DevCell* cells = nullptr;
  DevBand* bands = nullptr;
  int32_t* stacks = nullptr;
  DevTile* tiles = nullptr;
};
}  // namespace ist

struct ist_job {
  ist_ctx* ctx = nullptr;
  ist::Compiled host;
  std::unique_ptr<ist::FlatTwin> flat;   // or none: the job is not made of whole dense rows (ist_internal.h)
  ist::DevTables flat_dt;
  ist::DevBuf d_tables;                  // ONE device allocation holding the five tables below (from, and back to, ctx->table_pool)
  // the streams the job was launched on since it was created (ist_job_destroy waits for THOSE before it hands the tables to
  // the next job - not for the whole device: other streams of a shared device keep running); more than kStreams distinct
  // ones fall back to a device-wide wait
  static constexpr int kStreams = 4;
  hipStream_t launched_on[kStreams] = {nullptr, nullptr, nullptr, nullptr};
  int n_launched_on = 0;
  bool launched = false, launched_many = false;
  std::mutex launch_mu;
  ist::DevTables dt;
  int max_image = -1;
};

// return IST_E_HIP from the calling function when a HIP call fails
#define IST_HIP(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) return ist::fail(IST_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)
// the same with a fixed message (the runtime's error state is cleared)
#define IST_HIP_OR(expr, msg) do { if ((expr) != hipSuccess) { (void)hipGetLastError(); return ist::fail(IST_E_HIP, msg); } } while (0)

namespace ist {

// carve `bytes` from an arena that is being laid out: the section's offset; *off moves on to the next 256-byte boundary
inline size_t arena_take(size_t* off, size_t bytes) { const size_t at = *off; *off += round256(bytes); return at; }

// ---- pieces of ist_job_create / ist_job_launch shared with the batch entry points (ist_batch.cpp) ----
// compile an op list into a job whose tables are NOT uploaded yet (d_tables stays NULL: ist_job_destroy then frees no table block)
ist_job* job_compile(ist_ctx* ctx, int64_t canvas_w, int64_t canvas_h, const uint8_t clear_rgba[4], const ist_op* ops, int n_ops,
                     const ist_image_desc* images, int n_images, int filter, const ist_region* clip);
// where the job's tables (and its flat twin's) sit in one block: 256-byte aligned sections, `total` bytes
struct TableLayout { size_t bytes[2][5] = {}; size_t at[2][5] = {}; const void* from[2][5] = {}; size_t total = 0; };
TableLayout table_layout(const ist_job& job);
void pack_tables(const TableLayout& L, uint8_t* blob);             // host image of the block
void point_tables(ist_job* job, const TableLayout& L, uint8_t* base);   // the job's table pointers into a device block at base
// every rule of one launch and the kernel arguments it would pass (the flat form when the caller's rows are dense); no side effects
int job_launch_args(const ist_job* job, const void* const* src, const size_t* src_pitch, int n_images, void* dst, size_t dst_pitch,
                    LaunchArgs* out, const Compiled** out_run, bool* out_flat);
// the job was launched on `stream` (ist_job_destroy waits for it)
void note_launch_stream(ist_job* job, void* stream);
void count_flat_launches(int64_t n);

// a slot of ctx->batch_ring large enough for `bytes` whose last readers have completed (ctx->batch_mu held by the caller, who records
// slot->done behind the kernels that read the slot's device block and sets slot->pending)
int batch_take_slot(ist_ctx* ctx, size_t bytes, ist_ctx::BatchSlot** out);

// ---- the context's helpers of the host-buffer entry points (each stream, ring or pool is made on first use) ----
inline Stager& stager_of(ist_ctx* ctx) { if (!ctx->stager) ctx->stager.reset(new Stager(ctx->device)); return *ctx->stager; }
inline WorkerPool& workers_of(ist_ctx* ctx) { if (!ctx->workers) ctx->workers.reset(new WorkerPool()); return *ctx->workers; }
int ensure_aux(ist_ctx* ctx);             // the context's second stream
int ensure_render(ist_ctx* ctx);          // the context's render stream
int read_back_pooled(const void* dev, size_t bytes, hipStream_t stream, uint8_t** out);   // device bytes -> a pooled pinned block
// the PNG file of a canvas in device memory -> a pooled pinned block (need_rows / slab_rows_hint: as png_encode_device_deflate)
// preview (optional): + the preview of the canvas, one reduce queued behind the last render (PreviewTail below)
// form: the call's snapshot, checked by the entry point (PngForm::check)
int png_to_host(ist_ctx* ctx, const PngForm& form, const void* canvas, size_t pitch, int64_t w, int64_t h, void* dfile, uint8_t** out_png, int64_t* out_len,
                const std::function<int(int64_t, void*)>& need_rows = nullptr, int64_t slab_rows_hint = 0, ist_preview* preview = nullptr);

// ---- JPEG export (ist_jpeg_encode.hip) ----
// the baseline JFIF file of a canvas in device memory -> a pooled pinned block of its real length.  Caller holds ctx->mu; the canvas is
// complete on ctx->stream, which is synchronised.  The arguments have passed jpeg_check_export.
int jpeg_to_host(ist_ctx* ctx, const void* canvas, size_t pitch, int64_t w, int64_t h, int quality, int subsampling, uint8_t** out_jpeg,
                 int64_t* out_len);
int jpeg_check_options(const char* who, int quality, int subsampling);                       // IST_E_INVALID: quality outside 1..100, unknown subsampling
int jpeg_check_export(const char* who, int64_t w, int64_t h, int quality, int subsampling);  // + IST_E_UNSUPPORTED: a side above 65535

// ---- previews (ist_preview_host.cpp) ----
// the checks of an *_png_preview entry point on its ist_preview (NULL: fine, no preview); clears the outputs
int preview_check(ist_preview* pv);
// the outputs of an ist_preview cleared (NULL: nothing): the first thing an *_png_preview entry point does, so that `pixels` is NULL on
// EVERY failure, the ones that are found before preview_check included
inline void preview_clear(ist_preview* pv) { if (pv) { pv->width = pv->height = 0; pv->pixels = nullptr; } }
// one preview enqueued on `stream`: the reduce when both axes shrink, a one-draw IST_FILTER_AREA job otherwise.  Arguments checked by the caller.
int preview_enqueue(ist_ctx* ctx, const void* src, size_t src_pitch, int64_t w, int64_t h, bool opaque, void* dst, size_t dst_pitch,
                    int32_t pw, int32_t ph, hipStream_t stream);
// what a call that has retained a bitmap reads of it (ist_bitmap.cpp): its device, row 0, the row pitch and the desc
void bitmap_view(const ist_bitmap* b, int* device, const uint8_t** row0, size_t* pitch, ist_image_desc* desc);
// ---- overlap search (ist_overlap_host.cpp) ----
// the pairs of n >= 2 images in device memory on the context's device -> out[n - 1]; takes ctx->mu; the arguments have been checked
int overlap_run(ist_ctx* ctx, const void* const* src, const size_t* pitch, const ist_image_desc* descs, int n, const ist_overlap_opts* opts,
                ist_overlap* out);
int overlap_check_desc(const ist_image_desc& d, int i);     // IST_E_UNSUPPORTED "image i: ..." for EXIF orientation > 1 or a reduced-scale decode
// The preview of a canvas that an export is reading.  prepare() before the encoder; queue(reader) once every render of the canvas has
// been ordered in front of `reader`: the reduce and its small copy to pinned memory run on ctx->prev_stream behind that point;
// finish() after the encoder waits for that stream alone and hands the pixels over.  Whatever happens, nothing is in flight and
// nothing is leaked when the object goes.
struct PreviewTail {
  ist_ctx* ctx; const void* canvas; size_t pitch; int64_t w, h; ist_preview* pv;
  int32_t pw = 0, ph = 0;
  uint8_t* host = nullptr;
  bool queued = false;
  PreviewTail(ist_ctx* c, const void* cv, size_t p, int64_t w_, int64_t h_, ist_preview* v) : ctx(c), canvas(cv), pitch(p), w(w_), h(h_), pv(v) {}
  ~PreviewTail();
  int prepare();
  int queue(hipStream_t reader);
  int finish();
};

}  // namespace ist

#endif  // IST_CTX_H_
