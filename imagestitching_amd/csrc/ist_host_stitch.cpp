// ist_host_stitch.cpp — the host-buffer entry points of the C-ABI: caller pixels -> staged uploads -> fused launch -> the canvas or its
// PNG file in host memory; one shot for small canvases, row bands with both directions of PCIe busy for large ones.  Reference anchor:
// Page.onStitch stages 2-5 (pages/index/index.js:1251-1581) on bitmaps the platform has decoded (utils/canvas.js:27-121).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <vector>

#include "ist_ctx.h"

using namespace ist;

namespace {

std::atomic<int64_t> g_duplex_stitches{0};

// host sources -> device scratch -> fused launch into ctx->scratch_dst (left on the device, stream NOT synchronised).
// The scratch holds exactly the rendered region, rows contiguous (the launch addresses it as if it were the canvas: dst is
// biased by the region's origin), so every readback is one linear copy.  Caller holds ctx->mu.
int render_to_scratch(ist_ctx* ctx, int64_t canvas_w, int64_t canvas_h, const uint8_t clear_rgba[4],
                      const ist_op* ops, int n_ops, const ist_image_desc* images, const uint8_t* const* src,
                      const size_t* src_pitch, int n_images, int filter, const ist_region* region,
                      int64_t* out_w, int64_t* out_h) {
  const JobPtr job(ist_job_create(ctx, canvas_w, canvas_h, clear_rgba, ops, n_ops, images, n_images, filter, region));
  if (!job) return g_last_code ? g_last_code : IST_E_INVALID;

  // stage the sources that the job actually samples
  SourceLayout lay;
  int rc = lay.add(images, n_images, src, src_pitch, whole_bitmaps(job->host));
  if (rc) return rc;
  rc = ctx->scratch_src.grow(lay.bytes());
  if (rc) return rc;
  const int64_t rw = job->host.rx1 - job->host.rx0, rh = job->host.ry1 - job->host.ry0;
  const size_t pitch = static_cast<size_t>(rw) * 4;
  rc = ctx->scratch_dst.grow(pitch * static_cast<size_t>(rh));
  if (rc) return rc;
  const SourceLayout::Placed at = lay.place(ctx->scratch_src.p);
  std::vector<RowsCopy> up;
  lay.copy_all(&up);
  rc = stager_of(ctx).upload(up, ctx->stream);
  if (rc) return rc;
  const uintptr_t biased = reinterpret_cast<uintptr_t>(ctx->scratch_dst.p) - (static_cast<uintptr_t>(job->host.ry0) * pitch + static_cast<uintptr_t>(job->host.rx0) * 4);
  rc = ist_job_launch(job.get(), at.ptr.data(), at.pitch.data(), n_images, reinterpret_cast<void*>(biased), pitch, ctx->stream);
  if (rc) return rc;
  // the job's device tables are freed when `job` goes out of scope: the launch must have consumed them
  IST_HIP(hipStreamSynchronize(ctx->stream));
  if (out_w) *out_w = rw;
  if (out_h) *out_h = rh;
  return IST_OK;
}

// The host paths with both directions of PCIe busy (round 4).  The canvas is cut into row bands (ist_shard_row_cuts: ~40 MB each, cuts on
// multiples of 8 rows); band b is the whole op list clipped to its rows, and ist_shard_parts (IST_SPLIT_ROWS) names the source rows it
// samples.  Band by band: the rows not yet on the device go up in 32 MiB pieces on the staging stream (Stager::upload_big), the band is
// launched behind them, and - ist_stitch_rgba8 - its rows go down into the pinned result on the aux stream while the next band's sources go
// up, or - ist_render_png / ist_stitch_png - the PNG encoder compresses it and sends its slabs down meanwhile.  Any layout shards this way: a
// vertical strip (index.js:1522-1538) sends image after image, a horizontal one (1540-1553) a slice of every image per band.  Upload-all,
// launch, download-all costs 8.1 + 7.5 ms for nine 12 MP images; overlapped the two directions hold 48 GB/s each (tools/exp/duplex2.cpp).
// An earlier banded attempt (round 2) sent the uploads as 4 MiB chunks on four streams, which collapses to 12.7 GB/s each way as soon as
// downloads are in flight (tools/exp/duplex.cpp) - the piece size was the problem, not the idea.
struct RowBands {
  ist_ctx* ctx = nullptr;
  bool ok = false;                        // false after prepare(): not applicable (a small canvas, an op list the row cut refuses); nothing was queued
  int nb = 0, n_images = 0;
  int64_t cw = 0, ch = 0;
  size_t row = 0, total = 0;
  const ist_image_desc* images = nullptr;
  std::vector<int32_t> cuts;
  std::vector<std::map<int, RowSpan>> need;   // per band: the rows of every image it samples
  std::vector<JobPtr> jobs;
  SourceLayout lay;                       // the images the bands draw, whole (filled row range by row range)
  SourceLayout::Placed at;
  std::vector<int64_t> lo, hi;            // rows of image i already sent: [lo, hi)
  std::vector<RowsCopy> items;
  uint8_t* canvas = nullptr;
  int64_t y0(int b) const { return cuts[static_cast<size_t>(b)]; }
  int64_t y1(int b) const { return cuts[static_cast<size_t>(b) + 1]; }

  int prepare(ist_ctx* c, int64_t canvas_w, int64_t canvas_h, const uint8_t clear[4], const ist_op* ops, int n_ops, const ist_image_desc* imgs,
              const uint8_t* const* s, const size_t* sp, int n, int filter) {
    static const bool off = tuning_mode() && std::getenv("IST_HOST_DUPLEX") && std::atoi(std::getenv("IST_HOST_DUPLEX")) == 0;
    ctx = c; cw = canvas_w; ch = canvas_h; images = imgs; n_images = n;
    row = static_cast<size_t>(cw) * 4; total = row * static_cast<size_t>(ch);
    if (off || total < (32u << 20) || n_images < 1) return IST_OK;
    nb = static_cast<int>(std::min<size_t>(16, std::max<size_t>(2, total / (40u << 20))));
    cuts.assign(static_cast<size_t>(nb) + 1, 0);
    std::vector<ist_part> parts(static_cast<size_t>(std::max(1, n_ops)) * static_cast<size_t>(nb) + 8);
    int n_parts = 0;
    {
      KeepLastError keep;                                        // not an error of the call: the one-shot path takes it
      if (ist_shard_row_cuts(ch, nb, cuts.data()) != IST_OK ||
          ist_shard_parts(ops, n_ops, cw, ch, images, n_images, filter, nb, IST_SPLIT_ROWS, parts.data(), static_cast<int>(parts.size()), &n_parts) != IST_OK)
        return IST_OK;
    }
    parts.resize(static_cast<size_t>(n_parts));
    // every band compiles the WHOLE op list, clipped to its rows: the flat form looks at every op, so a shorter list could change the band's kernel
    jobs.resize(static_cast<size_t>(nb)); need.resize(static_cast<size_t>(nb));
    for (int b = 0; b < nb; ++b) {
      need[static_cast<size_t>(b)] = shard_holdings(parts_of_slot(parts, b));
      if (y0(b) >= y1(b)) continue;
      const ist_region clip{0, static_cast<int32_t>(y0(b)), static_cast<int32_t>(cw), static_cast<int32_t>(y1(b) - y0(b))};
      jobs[static_cast<size_t>(b)].reset(ist_job_create(ctx, cw, ch, clear, ops, n_ops, images, n_images, filter, &clip));
      if (!jobs[static_cast<size_t>(b)]) return g_last_code ? g_last_code : IST_E_INVALID;
    }
    // device scratch: the images the bands draw, and the canvas
    std::map<int, RowSpan> whole;
    for (const auto& band : need) for (const auto& kv : band) whole[kv.first] = RowSpan{0, bitmap_h(images[kv.first])};
    int rc = lay.add(images, n_images, s, sp, whole);
    if (rc) return rc;
    rc = ctx->scratch_src.grow(lay.bytes());
    if (rc) return rc;
    rc = ctx->scratch_dst.grow(total);
    if (rc) return rc;
    at = lay.place(ctx->scratch_src.p);
    lo.assign(static_cast<size_t>(n_images), -1); hi.assign(static_cast<size_t>(n_images), -1);
    canvas = static_cast<uint8_t*>(ctx->scratch_dst.p);
    ok = true;
    return IST_OK;
  }

  // sends what band b still needs and launches it, all ordered on R
  int submit(int b, hipStream_t R) {
    items.clear();
    auto send = [&](int i, int64_t r0, int64_t r1) { if (r1 > r0) items.push_back(lay.copy(i, r0, r1)); };   // rows [r0, r1) of image i
    for (const auto& kv : need[static_cast<size_t>(b)]) {
      const int i = kv.first;
      const int64_t a = std::max<int64_t>(0, kv.second.y0), e = std::min<int64_t>(bitmap_h(images[i]), kv.second.y1);
      if (e <= a) continue;
      int64_t& L0 = lo[static_cast<size_t>(i)]; int64_t& H0 = hi[static_cast<size_t>(i)];
      if (L0 < 0) { send(i, a, e); L0 = a; H0 = e; }
      else {                                                     // keep ONE interval per image: a band further down extends it (rows between are sent too)
        if (a < L0) { send(i, a, L0); L0 = a; }
        if (e > H0) { send(i, H0, e); H0 = e; }
      }
    }
    if (!items.empty()) { const int rc = stager_of(ctx).upload_big(items, R, &workers_of(ctx)); if (rc) return rc; }
    return ist_job_launch(jobs[static_cast<size_t>(b)].get(), at.ptr.data(), at.pitch.data(), n_images, canvas, row, R);
  }
};

// *done = false: not applicable, nothing was queued and the caller takes the one-shot path.
int stitch_banded_duplex(ist_ctx* ctx, const ist_plan* plan, const ist_op* ops, int n_ops, const ist_image_desc* images,
                         const uint8_t* const* src, const size_t* src_pitch, int n_images, int filter, uint8_t** out_pixels, bool* done) {
  *done = false;
  static const bool print = std::getenv("IST_TIMING") != nullptr;
  const auto t_start = std::chrono::steady_clock::now();
  auto lap = [&](const char* what) { if (print) std::fprintf(stderr, "[ist timing] host stitch: %-34s at %7.2f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count()); };
  RowBands rb;
  int rc = rb.prepare(ctx, plan->canvas_w, plan->canvas_h, kTransparent, ops, n_ops, images, src, src_pitch, n_images, filter);
  if (rc) return rc;
  if (!rb.ok) return IST_OK;
  rc = ensure_aux(ctx);
  if (rc) return rc;
  lap("band jobs compiled, scratch");
  uint8_t* host = static_cast<uint8_t*>(pool_take(rb.total));
  if (!host) return fail(IST_E_NOMEM, "out of pinned host memory for the result");
  std::vector<Event> ev(static_cast<size_t>(rb.nb));   // (made per band that is submitted; they go after the waits below)
  hipStream_t R = ctx->stream, D = ctx->aux;
  // (whatever happens below, the streams are idle before the pinned block or the jobs' tables are given back)
  auto finish = [&](int code) {
    (void)hipStreamSynchronize(R); (void)hipStreamSynchronize(D); (void)stager_of(ctx).sync();
    if (code != IST_OK) pool_give(host);
    return code;
  };
  bool first = true;
  for (int b = 0; b < rb.nb; ++b) {
    const int64_t y0 = rb.y0(b), y1 = rb.y1(b);
    if (y0 >= y1) continue;
    rc = rb.submit(b, R);
    if (rc) return finish(rc);
    Event& e = ev[static_cast<size_t>(b)];
    if (e.ensure() != IST_OK || hipEventRecord(e, R) != hipSuccess || hipStreamWaitEvent(D, e, 0) != hipSuccess ||
        hipMemcpyAsync(host + static_cast<size_t>(y0) * rb.row, rb.canvas + static_cast<size_t>(y0) * rb.row, static_cast<size_t>(y1 - y0) * rb.row, hipMemcpyDeviceToHost, D) != hipSuccess) {
      (void)hipGetLastError();
      return finish(fail(IST_E_HIP, "queueing a band's readback failed"));
    }
    if (first) { lap("first band queued"); first = false; }
  }
  lap("last band queued");
  if (hipStreamSynchronize(D) != hipSuccess || hipStreamSynchronize(R) != hipSuccess) { (void)hipGetLastError(); return finish(fail(IST_E_HIP, "result readback failed")); }
  lap("last band in host memory");
  g_duplex_stitches.fetch_add(1, std::memory_order_relaxed);
  *out_pixels = host;
  *done = true;
  return finish(IST_OK);
}

int render_png_banded(ist_ctx* ctx, const PngForm& form, int64_t canvas_w, int64_t canvas_h, const uint8_t clear_rgba[4], const ist_op* ops, int n_ops,
                      const ist_image_desc* images, const uint8_t* const* src, const size_t* src_pitch, int n_images, int filter,
                      uint8_t** out_png, int64_t* out_len, ist_preview* preview) {
  RowBands rb;
  int rc = rb.prepare(ctx, canvas_w, canvas_h, clear_rgba ? clear_rgba : kTransparent, ops, n_ops, images, src, src_pitch, n_images, filter);
  if (rc) return rc;
  if (!rb.ok) return 1;
  rc = ensure_render(ctx);
  if (rc) return rc;
  hipStream_t R = ctx->render;
  std::vector<Event> ev(static_cast<size_t>(rb.nb));   // (made per band that is submitted; they go after the waits below)
  int next = 0;
  // the encoder is about to read canvas rows [0, y_end) on `reader`: submit the bands they lie in, order the reader behind the last of them
  auto need_rows = [&](int64_t y_end, void* reader_) -> int {
    hipStream_t reader = static_cast<hipStream_t>(reader_);
    int last = -1;
    for (int b = 0; b < rb.nb; ++b) {
      if (rb.y0(b) >= rb.y1(b)) continue;
      if (rb.y0(b) >= y_end) break;
      if (b >= next) {
        const int rc2 = rb.submit(b, R);
        if (rc2) return rc2;
        if (ev[static_cast<size_t>(b)].ensure() != IST_OK || hipEventRecord(ev[static_cast<size_t>(b)], R) != hipSuccess) {
          (void)hipGetLastError(); return fail(IST_E_HIP, "hipEventRecord failed");
        }
        next = b + 1;
      }
      last = b;
    }
    if (last >= 0 && hipStreamWaitEvent(reader, ev[static_cast<size_t>(last)], 0) != hipSuccess) { (void)hipGetLastError(); return fail(IST_E_HIP, "ordering the export behind the render failed"); }
    return IST_OK;
  };
  int64_t hint = 0;
  for (int b = 0; b < rb.nb; ++b) hint = std::max<int64_t>(hint, rb.y1(b) - rb.y0(b));
  rc = png_to_host(ctx, form, rb.canvas, rb.row, canvas_w, canvas_h, nullptr, out_png, out_len, need_rows, hint, preview);
  (void)hipStreamSynchronize(R); (void)stager_of(ctx).sync(); (void)hipStreamSynchronize(ctx->stream);
  if (rc == IST_OK) g_duplex_stitches.fetch_add(1, std::memory_order_relaxed);
  return rc;
}

// PNG of a rendered op list (+ the preview of its canvas): the canvas never leaves the device.  The caller has checked the arguments.
int render_png(ist_ctx* ctx, int64_t canvas_w, int64_t canvas_h, const uint8_t clear_rgba[4], const ist_op* ops, int n_ops,
               const ist_image_desc* images, const uint8_t* const* src, const size_t* src_pitch, int n_images, int filter,
               uint8_t** out_png, int64_t* out_len, ist_preview* preview) {
  *out_png = nullptr; *out_len = 0;
  const PngForm form = settings_of(ctx).png;      // the call's form: read once
  { const int rc = form.check(); if (rc) return rc; }      // (level 0 in RGB: refused before anything is enqueued)
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceGuard g(ctx->device);
  int rc = render_png_banded(ctx, form, canvas_w, canvas_h, clear_rgba, ops, n_ops, images, src, src_pitch, n_images, filter, out_png, out_len, preview);
  if (rc != 1) return rc;                      // (1: not applicable, nothing queued)
  rc = render_to_scratch(ctx, canvas_w, canvas_h, clear_rgba, ops, n_ops, images, src, src_pitch, n_images, filter, nullptr, nullptr, nullptr);
  if (rc) return rc;
  return png_to_host(ctx, form, ctx->scratch_dst.p, static_cast<size_t>(canvas_w) * 4, canvas_w, canvas_h, nullptr, out_png, out_len, nullptr, 0, preview);
}

}  // namespace

extern "C" {

int64_t ist_debug_duplex_stitches(void) { return g_duplex_stitches.load(); }

int ist_render_rgba8(ist_ctx* ctx, int64_t canvas_w, int64_t canvas_h, const uint8_t clear_rgba[4],
                     const ist_op* ops, int n_ops, const ist_image_desc* images, const uint8_t* const* src,
                     const size_t* src_pitch, int n_images, int filter, const ist_region* region, uint8_t* dst,
                     size_t dst_pitch) {
  if (!ctx) return fail(IST_E_NO_CONTEXT, "无法获取绘图上下文");
  if (!dst) return fail(IST_E_INVALID, "ist_render_rgba8: dst is NULL");
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceGuard g(ctx->device);
  // the region that will be read back (same-size export, index.js:1577-1579; or getImageData, 1564): check the caller's
  // pitch before any work is queued
  int64_t rw = canvas_w, rh = canvas_h;
  if (region) {
    const int64_t rx = std::max<int64_t>(0, region->x), ry = std::max<int64_t>(0, region->y);
    rw = std::min<int64_t>(canvas_w, static_cast<int64_t>(region->x) + region->w) - rx;
    rh = std::min<int64_t>(canvas_h, static_cast<int64_t>(region->y) + region->h) - ry;
  }
  if (rw > 0 && dst_pitch < static_cast<size_t>(rw) * 4) return fail(IST_E_INVALID, "dst_pitch too small");
  int rc = render_to_scratch(ctx, canvas_w, canvas_h, clear_rgba, ops, n_ops, images, src, src_pitch, n_images, filter, region, &rw, &rh);
  if (rc) return rc;
  std::vector<RowsCopy> down{RowsCopy{ctx->scratch_dst.p, nullptr, dst, dst_pitch, static_cast<size_t>(rw) * 4, static_cast<size_t>(rh)}};
  return stager_of(ctx).download(down, ctx->stream);
}

// PNG of a rendered op list: the canvas never leaves the device, only the PNG bytes cross PCIe
int ist_render_png(ist_ctx* ctx, int64_t canvas_w, int64_t canvas_h, const uint8_t clear_rgba[4], const ist_op* ops,
                   int n_ops, const ist_image_desc* images, const uint8_t* const* src, const size_t* src_pitch,
                   int n_images, int filter, uint8_t** out_png, int64_t* out_len) {
  if (!ctx) return fail(IST_E_NO_CONTEXT, "无法获取绘图上下文");
  if (!out_png || !out_len) return fail(IST_E_INVALID, "ist_render_png: NULL output");
  return render_png(ctx, canvas_w, canvas_h, clear_rgba, ops, n_ops, images, src, src_pitch, n_images, filter, out_png, out_len, nullptr);
}

// plan + render + PNG: onStitch stages 2-5 including the export (index.js:1251-1581), decode excluded
int ist_stitch_png_preview(ist_ctx* ctx, const ist_image_desc* images, const uint8_t* const* src, const size_t* src_pitch,
                           int n_images, int direction, int mode, double gap, const ist_limits* limits, int filter,
                           ist_plan* out_plan, uint8_t** out_png, int64_t* out_len, ist_preview* preview) {
  preview_clear(preview);
  if (!ctx) return fail(IST_E_NO_CONTEXT, "无法获取绘图上下文");
  if (!out_plan || !out_png || !out_len) return fail(IST_E_INVALID, "ist_stitch_png: NULL output");
  int rc = preview_check(preview);
  if (rc) return rc;
  std::vector<ist_op> ops;
  rc = plan_with_ops(images, n_images, direction, mode, gap, limits, out_plan, &ops);
  if (rc != IST_OK) return rc;
  rc = render_png(ctx, out_plan->canvas_w, out_plan->canvas_h, kTransparent, ops.data(), static_cast<int>(ops.size()), images, src, src_pitch,
                  n_images, filter, out_png, out_len, preview);
  if (rc != IST_OK) ist_plan_free(out_plan);
  return rc;
}

int ist_stitch_png(ist_ctx* ctx, const ist_image_desc* images, const uint8_t* const* src, const size_t* src_pitch,
                   int n_images, int direction, int mode, double gap, const ist_limits* limits, int filter,
                   ist_plan* out_plan, uint8_t** out_png, int64_t* out_len) {
  return ist_stitch_png_preview(ctx, images, src, src_pitch, n_images, direction, mode, gap, limits, filter, out_plan, out_png, out_len, nullptr);
}

int ist_stitch_rgba8(ist_ctx* ctx, const ist_image_desc* images, const uint8_t* const* src, const size_t* src_pitch,
                     int n_images, int direction, int mode, double gap, const ist_limits* limits, int filter,
                     ist_plan* out_plan, uint8_t** out_pixels) {
  if (!ctx) return fail(IST_E_NO_CONTEXT, "无法获取绘图上下文");
  if (!out_plan || !out_pixels) return fail(IST_E_INVALID, "ist_stitch_rgba8: NULL output");
  *out_pixels = nullptr;
  std::vector<ist_op> ops;
  int rc = plan_with_ops(images, n_images, direction, mode, gap, limits, out_plan, &ops);
  if (rc != IST_OK) return rc;
  PlanGuard pg{out_plan};
  const int n_ops = static_cast<int>(ops.size());
  {
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard g(ctx->device);
    bool done = false;
    rc = stitch_banded_duplex(ctx, out_plan, ops.data(), n_ops, images, src, src_pitch, n_images, filter, out_pixels, &done);
    if (rc == IST_OK && !done) {
      rc = render_to_scratch(ctx, out_plan->canvas_w, out_plan->canvas_h, kTransparent, ops.data(), n_ops, images, src, src_pitch,
                             n_images, filter, nullptr, nullptr, nullptr);
      // the export (index.js:1577-1579): the whole canvas in one DMA into a pinned block of the pool
      if (rc == IST_OK)
        rc = read_back_pooled(ctx->scratch_dst.p, static_cast<size_t>(out_plan->canvas_w) * 4 * static_cast<size_t>(out_plan->canvas_h), ctx->stream, out_pixels);
    }
  }
  pg.keep = rc == IST_OK;
  return rc;
}

// plan + render + JPEG: ist_stitch_png with the other export (utils/canvas.js:205-221, fileType 'jpg').  The canvas is rendered in one
// launch into the context's scratch - the pixels every path of ist_stitch_rgba8 delivers - and only the file comes down.
int ist_stitch_jpeg(ist_ctx* ctx, const ist_image_desc* images, const uint8_t* const* src, const size_t* src_pitch,
                    int n_images, int direction, int mode, double gap, const ist_limits* limits, int filter, int quality,
                    int subsampling, ist_plan* out_plan, uint8_t** out_jpeg, int64_t* out_len) {
  if (!ctx) return fail(IST_E_NO_CONTEXT, "无法获取绘图上下文");
  if (!out_plan || !out_jpeg || !out_len) return fail(IST_E_INVALID, "ist_stitch_jpeg: NULL output");
  *out_jpeg = nullptr; *out_len = 0;
  int rc = jpeg_check_options("ist_stitch_jpeg", quality, subsampling);
  if (rc) return rc;
  std::vector<ist_op> ops;
  rc = plan_with_ops(images, n_images, direction, mode, gap, limits, out_plan, &ops);
  if (rc != IST_OK) return rc;
  PlanGuard pg{out_plan};
  rc = jpeg_check_export("ist_stitch_jpeg", out_plan->canvas_w, out_plan->canvas_h, quality, subsampling);
  if (rc) return rc;
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceGuard g(ctx->device);
  rc = render_to_scratch(ctx, out_plan->canvas_w, out_plan->canvas_h, kTransparent, ops.data(), static_cast<int>(ops.size()), images, src, src_pitch,
                         n_images, filter, nullptr, nullptr, nullptr);
  if (rc == IST_OK)
    rc = jpeg_to_host(ctx, ctx->scratch_dst.p, static_cast<size_t>(out_plan->canvas_w) * 4, out_plan->canvas_w, out_plan->canvas_h, quality, subsampling,
                      out_jpeg, out_len);
  pg.keep = rc == IST_OK;
  return rc;
}

// PNG of host pixels (H2D, encode, D2H)
int ist_png_encode_rgba8(ist_ctx* ctx, const uint8_t* pixels, size_t pitch, int64_t w, int64_t h, uint8_t** out_png,
                         int64_t* out_len) {
  if (!ctx) return fail(IST_E_NO_CONTEXT, "无法获取绘图上下文");
  if (!pixels || !out_png || !out_len || w < 1 || h < 1 || pitch < static_cast<size_t>(w) * 4) return fail(IST_E_INVALID, "ist_png_encode_rgba8: bad argument");
  const PngForm form = settings_of(ctx).png;      // the call's form: read once
  { const int rc = form.check(); if (rc) return rc; }
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceGuard g(ctx->device);
  const size_t row = static_cast<size_t>(w) * 4;
  int rc = ctx->scratch_dst.grow(row * static_cast<size_t>(h));
  if (rc) return rc;
  std::vector<RowsCopy> up{RowsCopy{ctx->scratch_dst.p, pixels, nullptr, pitch, row, static_cast<size_t>(h)}};
  rc = stager_of(ctx).upload(up, ctx->stream);
  if (rc) return rc;
  return png_to_host(ctx, form, ctx->scratch_dst.p, row, w, h, nullptr, out_png, out_len);
}

}  // extern "C"
