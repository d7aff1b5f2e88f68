// ist_bitmap.cpp — bitmaps the library keeps in HBM between stitches, and the stitch entry points that read them where they are.
// Reference anchor: the page's bitmap cache (pages/index/index.js:534-627, _getBitmapFromCache / _storeBitmapInCache, used at :1442 and
// :1515-1517): a user who reorders the photos, changes the gap or the direction and stitches again decodes nothing again.  Here a
// bitmap is one device block laid out like a staged source (dense rows + kSourceTail, ist_sources.cpp), so a restitch is the fused
// launch of the host path (ist_host_stitch.cpp, render_to_scratch) with no upload in front of it, plus the readback or the GPU PNG export.
#include <atomic>
#include <cstring>
#include <mutex>
#include <vector>

#include "ist_ctx.h"
#include "ist_decode.h"

using namespace ist;

struct ist_bitmap {
  std::atomic<int> refs{1};
  int device = 0;
  DevBuf block;                          // row 0 first; rows are 4 * bitmap_w(desc) bytes apart, kSourceTail readable bytes behind the last
  ist_image_desc desc{};
  ist_bitmap* parent = nullptr;          // a row view (ist_bitmap_rows): no block of its own, one reference on the bitmap that has it
  uint8_t* row0 = nullptr;               // ... and its first row inside that block
  uint8_t* px() const { return parent ? row0 : static_cast<uint8_t*>(block.p); }
};

namespace {

std::atomic<int64_t> g_bitmap_bytes{0};

size_t row_of(const ist_image_desc& d) { return static_cast<size_t>(bitmap_w(d)) * 4; }

// a new bitmap with one reference: the block on `device` (the caller has made it current), pixels not yet written
ist_bitmap* bitmap_alloc(int device, const ist_image_desc& d) {
  const size_t bytes = round256(row_of(d) * static_cast<size_t>(bitmap_h(d)) + kSourceTail);
  std::unique_ptr<ist_bitmap> b(new ist_bitmap);
  if (b->block.grow(bytes)) {
    fail(IST_E_NOMEM, "out of device memory for a bitmap (" + std::to_string(bytes >> 20) + " MiB)");
    return nullptr;
  }
  b->device = device; b->desc = d;
  g_bitmap_bytes.fetch_add(static_cast<int64_t>(bytes), std::memory_order_relaxed);
  return b.release();
}

// the references one call holds on its bitmaps: taken before anything else, dropped when the call returns
struct Held {
  std::vector<ist_bitmap*> b;
  ~Held() { for (ist_bitmap* x : b) ist_bitmap_release(x); }
};

// the checks of a stitch call, in this order; on success every bitmap is retained in *held
int take_bitmaps(const ist_ctx* ctx, ist_bitmap* const* bitmaps, int n, Held* held) {
  if (!bitmaps) return fail(IST_E_INVALID, "ist_stitch_bitmaps: NULL bitmap table");
  if (n > kMaxImages) return fail(IST_E_UNSUPPORTED, "more than 128 images in one launch");
  for (int i = 0; i < n; ++i) {
    if (!bitmaps[i]) return fail(IST_E_DECODE, "图片" + std::to_string(i) + "解码异常");
    if (bitmaps[i]->device != ctx->device)
      return fail(IST_E_INVALID, "bitmap " + std::to_string(i) + " lives on device " + std::to_string(bitmaps[i]->device) + ", the context on device " +
                                     std::to_string(ctx->device));
  }
  held->b.reserve(static_cast<size_t>(n));
  for (int i = 0; i < n; ++i) { ist_bitmap_retain(bitmaps[i]); held->b.push_back(bitmaps[i]); }
  return IST_OK;
}

// plan + one fused launch from the bitmaps into ctx->scratch_dst (dense canvas rows), then the canvas (want_png = false), its PNG file or
// (jpeg = {quality, subsampling}) its JPEG file into a pooled pinned block.  The launch is the one render_to_scratch makes for the same op list: the sources differ only in where
// they are, so the pixels are the host path's byte for byte.
int stitch_bitmaps(ist_ctx* ctx, ist_bitmap* const* bitmaps, int n, int direction, int mode, double gap, const ist_limits* limits, int filter,
                   bool want_png, ist_plan* out_plan, uint8_t** out, int64_t* out_len, ist_preview* preview = nullptr, const int* jpeg = nullptr) {
  Held held;
  int rc = take_bitmaps(ctx, bitmaps, n, &held);
  if (rc) return rc;
  std::vector<ist_image_desc> descs(static_cast<size_t>(n));
  std::vector<const void*> src(static_cast<size_t>(n));
  std::vector<size_t> pitch(static_cast<size_t>(n));
  for (int i = 0; i < n; ++i) {
    descs[static_cast<size_t>(i)] = bitmaps[i]->desc;
    src[static_cast<size_t>(i)] = bitmaps[i]->px();
    pitch[static_cast<size_t>(i)] = row_of(bitmaps[i]->desc);
  }
  std::vector<ist_op> ops;
  rc = plan_with_ops(descs.data(), n, direction, mode, gap, limits, out_plan, &ops);
  if (rc != IST_OK) return rc;
  PlanGuard pg{out_plan};
  const int64_t cw = out_plan->canvas_w, ch = out_plan->canvas_h;
  if (jpeg) { rc = jpeg_check_export("ist_stitch_bitmaps_jpeg", cw, ch, jpeg[0], jpeg[1]); if (rc) return rc; }
  const PngForm form = settings_of(ctx).png;      // the call's form: read once
  if (want_png) { rc = form.check(); if (rc) return rc; }      // (level 0 in RGB: refused before anything is enqueued)
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(IST_E_NO_DEVICE, "hipSetDevice failed");
  const JobPtr job(ist_job_create(ctx, cw, ch, kTransparent, ops.data(), static_cast<int>(ops.size()), descs.data(), n, filter, nullptr));
  if (!job) return g_last_code ? g_last_code : IST_E_INVALID;
  const size_t row = static_cast<size_t>(cw) * 4;
  rc = ctx->scratch_dst.grow(row * static_cast<size_t>(ch));
  if (rc) return rc;
  rc = ist_job_launch(job.get(), src.data(), pitch.data(), n, ctx->scratch_dst.p, row, ctx->stream);
  if (rc) return rc;
  IST_HIP(hipStreamSynchronize(ctx->stream));      // the canvas is complete; the job's tables may go back to the pool
  if (jpeg) rc = jpeg_to_host(ctx, ctx->scratch_dst.p, row, cw, ch, jpeg[0], jpeg[1], out, out_len);
  else if (want_png) rc = png_to_host(ctx, form, ctx->scratch_dst.p, row, cw, ch, nullptr, out, out_len, nullptr, 0, preview);
  else rc = read_back_pooled(ctx->scratch_dst.p, row * static_cast<size_t>(ch), ctx->stream, out);    // the export as ONE DMA (index.js:1577-1579)
  pg.keep = rc == IST_OK;
  return rc;
}

}  // namespace

namespace ist {
void bitmap_view(const ist_bitmap* b, int* device, const uint8_t** row0, size_t* pitch, ist_image_desc* desc) {
  *device = b->device; *row0 = b->px(); *pitch = row_of(b->desc); *desc = b->desc;
}
}  // namespace ist

extern "C" {

int64_t ist_debug_bitmap_bytes(void) { return g_bitmap_bytes.load(std::memory_order_relaxed); }

ist_bitmap* ist_bitmap_upload(ist_ctx* ctx, const ist_image_desc* desc, const uint8_t* src, size_t src_pitch) {
  if (!ctx) { fail(IST_E_NO_CONTEXT, "无法获取绘图上下文"); return nullptr; }
  if (!desc) { fail(IST_E_INVALID, "ist_bitmap_upload: NULL desc"); return nullptr; }
  // the rules of a staged source (SourceLayout::add)
  if (!src || bitmap_w(*desc) < 1 || bitmap_h(*desc) < 1) { fail(IST_E_DECODE, "图片0解码异常"); return nullptr; }
  const size_t row = row_of(*desc);
  if (src_pitch == 0) src_pitch = row;
  if (src_pitch < row) { fail(IST_E_INVALID, "src_pitch too small"); return nullptr; }
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceGuard g(ctx->device);
  if (!g.ok) { fail(IST_E_NO_DEVICE, "hipSetDevice failed"); return nullptr; }
  ist_bitmap* b = bitmap_alloc(ctx->device, *desc);
  if (!b) return nullptr;
  const std::vector<RowsCopy> up{RowsCopy{b->px(), src, nullptr, src_pitch, row, static_cast<size_t>(bitmap_h(*desc))}};
  int rc = stager_of(ctx).upload(up, ctx->stream);
  if (rc == IST_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) { (void)hipGetLastError(); rc = fail(IST_E_HIP, "bitmap upload failed"); }
  if (rc) { ist_bitmap_release(b); return nullptr; }
  return b;
}

int ist_bitmaps_decode(ist_ctx* ctx, const uint8_t* const* files, const int64_t* lens, int n, ist_bitmap** out) {
  return ist_bitmaps_decode_scaled(ctx, files, lens, n, nullptr, out);
}

int ist_bitmaps_decode_scaled(ist_ctx* ctx, const uint8_t* const* files, const int64_t* lens, int n, const int32_t* denom, ist_bitmap** out) {
  if (!ctx) return fail(IST_E_NO_CONTEXT, "无法获取绘图上下文");
  if (n <= 0) return IST_NOTHING_TO_DO;
  if (!files || !lens || !out) return fail(IST_E_INVALID, "ist_bitmaps_decode: NULL argument");
  if (n > kMaxImages) return fail(IST_E_UNSUPPORTED, "more than 128 images in one call");
  for (int i = 0; i < n; ++i) out[i] = nullptr;
  const int drc = check_denoms("ist_bitmaps_decode_scaled", denom, n);
  if (drc) return drc;
  std::vector<ist_bitmap*> made;
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceGuard g(ctx->device);
  const int rc = decode_files_locked(ctx, files, lens, n, denom, [&](const std::vector<ist_image_desc>& descs, uint8_t** img, size_t* pitch) -> int {
    for (int i = 0; i < n; ++i) {
      ist_bitmap* b = bitmap_alloc(ctx->device, descs[static_cast<size_t>(i)]);
      if (!b) return g_last_code;
      made.push_back(b);
      img[i] = b->px();
      pitch[i] = row_of(b->desc);
    }
    return IST_OK;
  });
  if (rc) {                                        // all or nothing (ctx->stream is idle: nothing writes the blocks any more)
    KeepLastError keep;
    for (ist_bitmap* b : made) ist_bitmap_release(b);
    return rc;
  }
  for (int i = 0; i < n; ++i) out[i] = made[static_cast<size_t>(i)];
  return IST_OK;
}

int ist_bitmap_desc(const ist_bitmap* b, ist_image_desc* out) {
  if (!b || !out) return fail(IST_E_INVALID, "ist_bitmap_desc: NULL argument");
  *out = b->desc;
  return IST_OK;
}

int ist_bitmap_download(ist_bitmap* b, uint8_t* dst, size_t dst_pitch, int64_t dst_rows) {
  if (!b || !dst) return fail(IST_E_INVALID, "ist_bitmap_download: NULL argument");
  const size_t row = row_of(b->desc);
  const int64_t rows = bitmap_h(b->desc);
  if (dst_pitch < row || dst_rows < rows) return fail(IST_E_INVALID, "ist_bitmap_download: the buffer is too small for the bitmap");
  ist_bitmap_retain(b);
  Held held{{b}};
  DeviceGuard g(b->device);
  if (!g.ok) return fail(IST_E_NO_DEVICE, "hipSetDevice failed");
  // (no context here: one synchronous copy on the null stream; every call that writes a bitmap has finished before it returned)
  IST_HIP(hipMemcpy2D(dst, dst_pitch, b->px(), row, row, static_cast<size_t>(rows), hipMemcpyDeviceToHost));
  return IST_OK;
}

void ist_bitmap_retain(ist_bitmap* b) {
  if (b) b->refs.fetch_add(1, std::memory_order_relaxed);
}

void ist_bitmap_release(ist_bitmap* b) {
  if (!b || b->refs.fetch_sub(1, std::memory_order_acq_rel) != 1) return;
  g_bitmap_bytes.fetch_sub(static_cast<int64_t>(b->block.bytes), std::memory_order_relaxed);
  ist_bitmap* parent = b->parent;
  delete b;
  ist_bitmap_release(parent);            // (a view's parent is never a view: one step)
}

ist_bitmap* ist_bitmap_rows(ist_bitmap* b, int32_t y0, int32_t rows) {
  if (!b) { fail(IST_E_INVALID, "ist_bitmap_rows: NULL bitmap"); return nullptr; }
  const ist_image_desc& d = b->desc;
  if (d.orientation > 1) { fail(IST_E_UNSUPPORTED, "ist_bitmap_rows: the bitmap has EXIF orientation " + std::to_string(d.orientation) + " (rows of the stored pixels are not rows of the image)"); return nullptr; }
  if (bitmap_w(d) != d.width || bitmap_h(d) != d.height) { fail(IST_E_UNSUPPORTED, "ist_bitmap_rows: the bitmap was decoded at a reduced scale"); return nullptr; }
  if (y0 < 0 || rows < 1 || static_cast<int64_t>(y0) + rows > bitmap_h(d)) {
    fail(IST_E_INVALID, "ist_bitmap_rows: rows [" + std::to_string(y0) + ", " + std::to_string(static_cast<int64_t>(y0) + rows) + ") are not inside the bitmap's " + std::to_string(bitmap_h(d)));
    return nullptr;
  }
  ist_bitmap* v = new ist_bitmap;
  v->device = b->device;
  v->desc = d;
  v->desc.height = rows; v->desc.bmp_height = d.bmp_height > 0 ? rows : 0; v->desc.file_size = 0;
  v->parent = b->parent ? b->parent : b;     // a view of a view holds the bitmap that owns the block
  v->row0 = b->px() + static_cast<size_t>(y0) * row_of(d);
  ist_bitmap_retain(v->parent);
  return v;
}

int ist_stitch_bitmaps_rgba8(ist_ctx* ctx, ist_bitmap* const* bitmaps, int n, int direction, int mode, double gap, const ist_limits* limits,
                             int filter, ist_plan* out_plan, uint8_t** out_pixels) {
  if (!ctx) return fail(IST_E_NO_CONTEXT, "无法获取绘图上下文");
  if (!out_plan || !out_pixels) return fail(IST_E_INVALID, "ist_stitch_bitmaps_rgba8: NULL output");
  *out_pixels = nullptr;
  std::memset(out_plan, 0, sizeof(*out_plan));
  if (n <= 0) return IST_NOTHING_TO_DO;
  return stitch_bitmaps(ctx, bitmaps, n, direction, mode, gap, limits, filter, false, out_plan, out_pixels, nullptr);
}

int ist_stitch_bitmaps_png_preview(ist_ctx* ctx, ist_bitmap* const* bitmaps, int n, int direction, int mode, double gap, const ist_limits* limits,
                                   int filter, ist_plan* out_plan, uint8_t** out_png, int64_t* out_len, ist_preview* preview) {
  preview_clear(preview);
  if (!ctx) return fail(IST_E_NO_CONTEXT, "无法获取绘图上下文");
  if (!out_plan || !out_png || !out_len) return fail(IST_E_INVALID, "ist_stitch_bitmaps_png: NULL output");
  *out_png = nullptr; *out_len = 0;
  std::memset(out_plan, 0, sizeof(*out_plan));
  const int rc = preview_check(preview);
  if (rc) return rc;
  if (n <= 0) return IST_NOTHING_TO_DO;
  return stitch_bitmaps(ctx, bitmaps, n, direction, mode, gap, limits, filter, true, out_plan, out_png, out_len, preview);
}

int ist_stitch_bitmaps_png(ist_ctx* ctx, ist_bitmap* const* bitmaps, int n, int direction, int mode, double gap, const ist_limits* limits,
                           int filter, ist_plan* out_plan, uint8_t** out_png, int64_t* out_len) {
  return ist_stitch_bitmaps_png_preview(ctx, bitmaps, n, direction, mode, gap, limits, filter, out_plan, out_png, out_len, nullptr);
}

int ist_stitch_bitmaps_jpeg(ist_ctx* ctx, ist_bitmap* const* bitmaps, int n, int direction, int mode, double gap, const ist_limits* limits,
                            int filter, int quality, int subsampling, ist_plan* out_plan, uint8_t** out_jpeg, int64_t* out_len) {
  if (!ctx) return fail(IST_E_NO_CONTEXT, "无法获取绘图上下文");
  if (!out_plan || !out_jpeg || !out_len) return fail(IST_E_INVALID, "ist_stitch_bitmaps_jpeg: NULL output");
  *out_jpeg = nullptr; *out_len = 0;
  std::memset(out_plan, 0, sizeof(*out_plan));
  const int rc = jpeg_check_options("ist_stitch_bitmaps_jpeg", quality, subsampling);
  if (rc) return rc;
  if (n <= 0) return IST_NOTHING_TO_DO;
  const int jpeg[2] = {quality, subsampling};
  return stitch_bitmaps(ctx, bitmaps, n, direction, mode, gap, limits, filter, false, out_plan, out_jpeg, out_len, nullptr, jpeg);
}

int ist_bitmaps_overlap(ist_ctx* ctx, ist_bitmap* const* bitmaps, int n, const ist_overlap_opts* opts, ist_overlap* out) {
  if (!ctx) return fail(IST_E_NO_CONTEXT, "无法获取绘图上下文");
  if (n < 2) return fail(IST_E_INVALID, "ist_bitmaps_overlap: an overlap needs at least two bitmaps");
  if (!bitmaps || !out) return fail(IST_E_INVALID, "ist_bitmaps_overlap: NULL argument");
  if (opts && (opts->tolerance < 0 || opts->min_rows < 0 || opts->min_informative < 0)) return fail(IST_E_INVALID, "ist_bitmaps_overlap: negative option");
  Held held;
  int rc = take_bitmaps(ctx, bitmaps, n, &held);
  if (rc) return rc;
  std::vector<ist_image_desc> descs(static_cast<size_t>(n));
  std::vector<const void*> src(static_cast<size_t>(n));
  std::vector<size_t> pitch(static_cast<size_t>(n));
  for (int i = 0; i < n; ++i) {
    rc = overlap_check_desc(bitmaps[i]->desc, i);
    if (rc) return rc;
    descs[static_cast<size_t>(i)] = bitmaps[i]->desc;
    src[static_cast<size_t>(i)] = bitmaps[i]->px();
    pitch[static_cast<size_t>(i)] = row_of(bitmaps[i]->desc);
  }
  return overlap_run(ctx, src.data(), pitch.data(), descs.data(), n, opts, out);
}

int ist_bitmap_preview(ist_ctx* ctx, ist_bitmap* b, int32_t pw, int32_t ph, uint8_t* dst, size_t dst_pitch) {
  if (!ctx) return fail(IST_E_NO_CONTEXT, "无法获取绘图上下文");
  if (!b || !dst) return fail(IST_E_INVALID, "ist_bitmap_preview: NULL argument");
  if (pw < 1 || ph < 1) return fail(IST_E_INVALID, "ist_bitmap_preview: the preview must be at least 1 x 1");
  const size_t row = static_cast<size_t>(pw) * 4;
  if (dst_pitch < row) return fail(IST_E_INVALID, "dst_pitch too small");
  if (b->device != ctx->device)
    return fail(IST_E_INVALID, "the bitmap lives on device " + std::to_string(b->device) + ", the context on device " + std::to_string(ctx->device));
  ist_bitmap_retain(b);
  Held held{{b}};
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(IST_E_NO_DEVICE, "hipSetDevice failed");
  int rc = ctx->prev_out.grow(row * static_cast<size_t>(ph));
  if (rc) return rc;
  // the stored pixels, as ist_bitmap_download's: EXIF orientation is the planner's business
  rc = preview_enqueue(ctx, b->px(), row_of(b->desc), bitmap_w(b->desc), bitmap_h(b->desc), b->desc.opaque != 0, ctx->prev_out.p, row, pw, ph, ctx->stream);
  if (rc) return rc;
  const std::vector<RowsCopy> down{RowsCopy{ctx->prev_out.p, nullptr, dst, dst_pitch, row, static_cast<size_t>(ph)}};
  return stager_of(ctx).download(down, ctx->stream);
}

}  // extern "C"
