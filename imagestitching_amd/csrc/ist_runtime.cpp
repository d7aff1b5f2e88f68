// ist_runtime.cpp — the device context and the compiled jobs of the C-ABI, with the helpers every entry point shares (device
// scratch, the context's streams, result readback).  The host-buffer entry points are in ist_host_stitch.cpp, the image
// decoders in ist_decode.cpp, the file pipeline in ist_files.cpp.
//
// Reference anchors (miniprogram-stitch/miniprogram/): the context stands for the canvas node obtained at
// pages/index/index.js:1196-1204; a job for the offscreen canvas + recorded draws (utils/canvas.js:131-150,
// index.js:1391-1428, 1532-1551); launch for the raster flush the export forces (utils/canvas.js:205-242).
// There is deliberately no CPU fallback: without a HIP device every rendering entry point fails.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>

#include "ist_ctx.h"

using namespace ist;

namespace ist {
int ctx_png_scratch(ist_ctx* ctx, size_t need, void** p) { const int rc = ctx->scratch_png.grow(need); *p = ctx->scratch_png.p; return rc; }

static std::atomic<int64_t> g_dev_allocs{0};
std::atomic<int64_t> g_live_handles[4];
int dev_malloc(void** p, size_t bytes) {
  g_dev_allocs.fetch_add(1, std::memory_order_relaxed);
  return static_cast<int>(hipMalloc(p, bytes));
}

// A buffer the library hands to the caller (freed with ist_free): a pinned block from the pool, filled by ONE linear DMA
// from device memory, no host copy.  Synchronises `stream`.
int read_back_pooled(const void* dev, size_t bytes, hipStream_t stream, uint8_t** out) {
  uint8_t* host = static_cast<uint8_t*>(pool_take(bytes));
  if (!host) return fail(IST_E_NOMEM, "out of pinned host memory for the result");
  if (hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) {
    (void)hipGetLastError();
    pool_give(host);
    return fail(IST_E_HIP, "result readback failed");
  }
  *out = host;
  return IST_OK;
}

// the context's second stream (high priority: its small kernels should not queue behind thousands of workgroups of the first)
int ensure_aux(ist_ctx* ctx) {
  static const bool lowest = tuning_mode() && std::getenv("IST_AUX_PRIORITY") && !std::atoi(std::getenv("IST_AUX_PRIORITY"));     // A/B knob: 0 = lowest
  return ctx->aux.ensure(lowest ? Stream::kLowest : Stream::kHighest);
}
// the render stream (high priority: its short kernels should not queue behind the PNG encoder's thousands of workgroups)
int ensure_render(ist_ctx* ctx) { return ctx->render.ensure(Stream::kHighest); }

// The PNG file of a canvas in device memory -> a pooled pinned block (freed with ist_free).  `dfile` = device scratch of
// at least ist_png_bound bytes (nullptr: the context's own).  The compressing encoder hands the file over slab by slab
// while it is still compressing (png_encode_device_deflate); the stored form is encoded whole and copied once.
// Caller holds ctx->mu.  Synchronises ctx->stream.
int png_to_host(ist_ctx* ctx, const PngForm& form, const void* canvas, size_t pitch, int64_t w, int64_t h, void* dfile, uint8_t** out_png, int64_t* out_len,
                const std::function<int(int64_t, void*)>& need_rows_in, int64_t slab_rows_hint, ist_preview* preview) {
  // With a preview: the encoder's request for the canvas's LAST rows is the point behind which every render has been ordered in
  // front of the stream that asked.  The reduce is queued there, on a stream of its own - beside the last slab's compression, not in
  // front of it, and with no host wait.  Without one, need_rows is the caller's, untouched.
  PreviewTail tail(ctx, canvas, pitch, w, h, preview);
  std::function<int(int64_t, void*)> with_preview;
  if (preview) {
    const int rc = tail.prepare();
    if (rc) return rc;
    with_preview = [&](int64_t y_end, void* reader) -> int {
      const int rc2 = need_rows_in ? need_rows_in(y_end, reader) : IST_OK;
      if (rc2 || y_end < h) return rc2;
      return tail.queue(static_cast<hipStream_t>(reader));
    };
  }
  const std::function<int(int64_t, void*)>& need_rows = preview ? with_preview : need_rows_in;
  const int64_t cap = ist_png_bound(w, h);
  if (!dfile) {
    const int rc = ctx->scratch_file.grow(static_cast<size_t>(cap));
    if (rc) return rc;
    dfile = ctx->scratch_file.p;
  }
  int64_t len = 0;
  if (form.compressed()) {
    { const int rc = ensure_aux(ctx); if (rc) return rc; }
    uint8_t* host = static_cast<uint8_t*>(pool_take(static_cast<size_t>(cap)));
    if (!host) return fail(IST_E_NOMEM, "out of pinned host memory for the result");
    { KeepLastError tolerated; (void)ctx->png2.ensure(); }   // (without it the slabs share one stream)
    const int rc = png_encode_device_deflate(ctx, form, canvas, pitch, w, h, dfile, cap, &len, ctx->stream, host, ctx->aux, need_rows, slab_rows_hint, ctx->png2);
    if (rc) { (void)hipStreamSynchronize(ctx->aux); (void)hipStreamSynchronize(ctx->stream); if (ctx->png2) (void)hipStreamSynchronize(ctx->png2); pool_give(host); return rc; }
    if (preview) { const int rc2 = tail.finish(); if (rc2) { pool_give(host); return rc2; } }
    *out_png = host; *out_len = len;
    return IST_OK;
  }
  int rc = need_rows ? need_rows(h, ctx->stream) : IST_OK;   // (the stored form reads the whole canvas in one pass)
  if (rc) return rc;
  rc = png_encode_device_stored(canvas, pitch, w, h, dfile, cap, &len, ctx->stream);
  if (rc) return rc;
  uint8_t* host = nullptr;
  rc = read_back_pooled(dfile, static_cast<size_t>(len), ctx->stream, &host);
  if (rc) return rc;
  if (preview) { rc = tail.finish(); if (rc) { pool_give(host); return rc; } }
  *out_png = host; *out_len = len;
  return IST_OK;
}

}  // namespace ist

extern "C" {

int64_t ist_debug_device_allocs(void) { return g_dev_allocs.load(std::memory_order_relaxed); }

int ist_debug_live_handles(int64_t out[4]) {
  if (!out) return fail(IST_E_INVALID, "ist_debug_live_handles: NULL output");
  for (int k = 0; k < 4; ++k) out[k] = g_live_handles[k].load(std::memory_order_relaxed);
  return IST_OK;
}

int ist_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

ist_ctx* ist_ctx_create(int device) {
  const int n = ist_device_count();
  if (n <= 0) { fail(IST_E_NO_DEVICE, "no HIP device: the stitch path has no CPU fallback"); return nullptr; }
  if (device < 0 || device >= n) { fail(IST_E_INVALID, "device index out of range"); return nullptr; }
  DeviceGuard g(device);
  if (!g.ok) { fail(IST_E_NO_DEVICE, "hipSetDevice failed"); return nullptr; }
  std::unique_ptr<ist_ctx> c(new ist_ctx);
  c->device = device;
  if (c->stream.ensure() != IST_OK) return nullptr;
  return c.release();
}

int ist_ctx_set_png_level(ist_ctx* ctx, int level) {
  if (!ctx) return fail(IST_E_NO_CONTEXT, "无法获取绘图上下文");
  return settings_set(&ctx->settings, kPngLevel, level);
}

int ist_ctx_set_png_color(ist_ctx* ctx, int color) {
  if (!ctx) return fail(IST_E_NO_CONTEXT, "无法获取绘图上下文");
  return settings_set(&ctx->settings, kPngColor, color);
}

int ist_ctx_set_png_filter(ist_ctx* ctx, int filter) {
  if (!ctx) return fail(IST_E_NO_CONTEXT, "无法获取绘图上下文");
  return settings_set(&ctx->settings, kPngFilter, filter);
}

int ist_ctx_set_png_match(ist_ctx* ctx, int match) {
  if (!ctx) return fail(IST_E_NO_CONTEXT, "无法获取绘图上下文");
  return settings_set(&ctx->settings, kPngMatch, match);
}

int ist_debug_png_grid(int64_t w, int64_t h, int color, int64_t out[4]) {
  if (w < 1 || h < 1 || !out || (color != IST_PNG_RGBA && color != IST_PNG_RGB)) return fail(IST_E_INVALID, "ist_debug_png_grid: bad argument");
  png_deflate_grid(w, h, color, out);
  return IST_OK;
}

int ist_ctx_sync(ist_ctx* ctx) {
  if (!ctx) return fail(IST_E_NO_CONTEXT, "无法获取绘图上下文");
  DeviceGuard g(ctx->device);
  // (every stream, the per-image ones included: those are idle on return from every entry point, so a caller observes nothing of it)
  bool ok = true;
  for (hipStream_t st : ctx->streams()) ok = (hipStreamSynchronize(st) == hipSuccess) && ok;
  if (ctx->stager) ok = (ctx->stager->sync() == IST_OK) && ok;
  if (!ok) { (void)hipGetLastError(); return fail(IST_E_HIP, "hipStreamSynchronize failed"); }
  return IST_OK;
}

// Everything the context holds is a member that releases itself (ist_ctx.h: the streams first, each waited for).  What is left to say
// here is the order of what is NOT a plain member: the kept preview job hands its tables to the pool, the workers and the stager stop.
void ist_ctx_destroy(ist_ctx* ctx) {
  if (!ctx) return;
  DeviceGuard g(ctx->device);
  for (hipStream_t st : ctx->streams()) (void)hipStreamSynchronize(st);
  if (ctx->prev_job) ist_job_destroy(ctx->prev_job);
  ctx->workers.reset();
  ctx->stager.reset();
  delete ctx;
}

static std::atomic<int64_t> g_flat_launches{0};

int64_t ist_debug_flat_launches(void) { return g_flat_launches.load(); }

}  // extern "C"

namespace ist {
void count_flat_launches(int64_t n) { g_flat_launches.fetch_add(n, std::memory_order_relaxed); }

ist_job* job_compile(ist_ctx* ctx, int64_t canvas_w, int64_t canvas_h, const uint8_t clear_rgba[4], const ist_op* ops, int n_ops,
                     const ist_image_desc* images, int n_images, int filter, const ist_region* clip) {
  if (!ctx) { fail(IST_E_NO_CONTEXT, "无法获取绘图上下文"); return nullptr; }
  if (n_images > kMaxImages) { fail(IST_E_UNSUPPORTED, "more than 128 images in one launch"); return nullptr; }
  std::unique_ptr<ist_job> job(new ist_job);
  job->ctx = ctx;
  if (compile_ops(canvas_w, canvas_h, clear_rgba ? clear_rgba : kTransparent, ops, n_ops, images, n_images, filter,
                  clip, &job->host) != IST_OK)
    return nullptr;
  for (const DevOp& o : job->host.ops) job->max_image = std::max(job->max_image, o.image);
  job->flat = compile_flat_twin(canvas_w, canvas_h, clear_rgba ? clear_rgba : kTransparent, ops, n_ops, images, n_images, filter, job->host);
  return job.release();
}

TableLayout table_layout(const ist_job& job) {
  TableLayout L;
  const Compiled* hs[2] = {&job.host, job.flat ? &job.flat->host : nullptr};
  for (int t = 0; t < 2; ++t) {
    if (!hs[t]) continue;
    const Compiled& h = *hs[t];
    const size_t b[5] = {h.ops.size() * sizeof(DevOp), h.cells.size() * sizeof(DevCell), h.bands.size() * sizeof(DevBand),
                         h.stacks.size() * sizeof(int32_t), h.tiles.size() * sizeof(DevTile)};
    const void* f[5] = {h.ops.data(), h.cells.data(), h.bands.data(), h.stacks.data(), h.tiles.data()};
    for (int k = 0; k < 5; ++k) { L.bytes[t][k] = b[k]; L.from[t][k] = f[k]; L.at[t][k] = L.total; L.total += round256(b[k]); }
  }
  return L;
}

void pack_tables(const TableLayout& L, uint8_t* blob) {
  for (int t = 0; t < 2; ++t)
    for (int k = 0; k < 5; ++k) if (L.bytes[t][k]) std::memcpy(blob + L.at[t][k], L.from[t][k], L.bytes[t][k]);
}

void point_tables(ist_job* job, const TableLayout& L, uint8_t* base) {
  DevTables* dts[2] = {&job->dt, job->flat ? &job->flat_dt : nullptr};
  for (int t = 0; t < 2; ++t) {
    if (!dts[t]) continue;
    dts[t]->ops = L.bytes[t][0] ? reinterpret_cast<DevOp*>(base + L.at[t][0]) : nullptr;
    dts[t]->cells = L.bytes[t][1] ? reinterpret_cast<DevCell*>(base + L.at[t][1]) : nullptr;
    dts[t]->bands = L.bytes[t][2] ? reinterpret_cast<DevBand*>(base + L.at[t][2]) : nullptr;
    dts[t]->stacks = L.bytes[t][3] ? reinterpret_cast<int32_t*>(base + L.at[t][3]) : nullptr;
    dts[t]->tiles = L.bytes[t][4] ? reinterpret_cast<DevTile*>(base + L.at[t][4]) : nullptr;
  }
}

int job_launch_args(const ist_job* job, const void* const* src, const size_t* src_pitch, int n_images, void* dst, size_t dst_pitch,
                    LaunchArgs* out, const Compiled** out_run, bool* out_flat) {
  if (!job || !dst) return fail(IST_E_INVALID, "ist_job_launch: NULL argument");
  if (n_images <= job->max_image) return fail(IST_E_DECODE, "图片" + std::to_string(job->max_image) + "解码异常: source table too short");
  if (n_images > kMaxImages) return fail(IST_E_UNSUPPORTED, "more than 128 images in one launch");
  const Compiled& h = job->host;
  // only the rendered region is ever addressed, so a compact band buffer (pitch = region width) is legal when the
  // caller biases dst by -(ry0*pitch + rx0*4)
  if (dst_pitch < static_cast<size_t>(h.rx1 - h.rx0) * 4 || (dst_pitch & 3)) return fail(IST_E_INVALID, "dst_pitch too small or not a multiple of 4");
  LaunchArgs& a = *out;
  std::memset(&a, 0, sizeof(a));
  a.dst = static_cast<uint8_t*>(dst);
  a.dst_pitch = dst_pitch;
  bool dense = job->flat && dst_pitch == static_cast<size_t>(h.canvas_w) * 4;      // (a flat twin exists only for draws as wide as the canvas)
  for (const DevOp& o : h.ops) {
    if (o.image < 0) continue;
    const int i = o.image;
    if (!src || !src[i]) return fail(IST_E_DECODE, "图片" + std::to_string(i) + "解码异常");
    const size_t p = src_pitch ? src_pitch[i] : static_cast<size_t>(h.img_w[i]) * 4;
    if (p < static_cast<size_t>(h.img_w[i]) * 4 || (p & 3)) return fail(IST_E_INVALID, "src_pitch too small or not a multiple of 4");
    if ((reinterpret_cast<uintptr_t>(src[i]) & 3) != 0) return fail(IST_E_INVALID, "source pixels must be 4-byte aligned");
    a.src[i] = static_cast<const uint8_t*>(src[i]);
    a.pitch[i] = p;
    dense = dense && p == dst_pitch;
  }
  if ((reinterpret_cast<uintptr_t>(dst) & 3) != 0) return fail(IST_E_INVALID, "dst must be 4-byte aligned");
  // dense rows on both sides: the job's flat twin moves the same bytes as rows of kFlatPitch (validated above on the caller's own table)
  const Compiled& run = dense ? job->flat->host : h;
  const DevTables& dt = dense ? job->flat_dt : job->dt;
  if (dense) {
    LaunchArgs f;
    std::memset(&f, 0, sizeof(f));
    f.dst = a.dst + job->flat->dst_delta;
    f.dst_pitch = kFlatPitch;
    for (size_t k = 0; k < job->flat->src.size(); ++k) {
      f.src[k] = a.src[job->flat->src[k].image] + job->flat->src[k].delta;
      f.pitch[k] = kFlatPitch;
    }
    a = f;
  }
  a.ops = dt.ops; a.cells = dt.cells; a.bands = dt.bands; a.stacks = dt.stacks;
  a.tiles = run.tiles.empty() ? nullptr : dt.tiles;
  a.n_bands = static_cast<int32_t>(run.bands.size());
  a.n_cells = static_cast<int32_t>(run.cells.size());
  a.filter = run.filter;
  a.lds_words = run.lds_words;
  a.lds_half = run.lds_half;
  a.pad_ = 0;
  *out_run = &run;
  *out_flat = dense;
  return IST_OK;
}

void note_launch_stream(ist_job* job, void* stream) {
  std::lock_guard<std::mutex> lk(job->launch_mu);
  job->launched = true;
  hipStream_t st = static_cast<hipStream_t>(stream);
  int k = 0;
  while (k < job->n_launched_on && job->launched_on[k] != st) ++k;
  if (k == job->n_launched_on) {
    if (k < ist_job::kStreams) job->launched_on[job->n_launched_on++] = st;
    else job->launched_many = true;
  }
}
}  // namespace ist

extern "C" {

ist_job* ist_job_create(ist_ctx* ctx, int64_t canvas_w, int64_t canvas_h, const uint8_t clear_rgba[4],
                        const ist_op* ops, int n_ops, const ist_image_desc* images, int n_images,
                        int filter, const ist_region* clip) {
  std::unique_ptr<ist_job> job(job_compile(ctx, canvas_w, canvas_h, clear_rgba, ops, n_ops, images, n_images, filter, clip));
  if (!job) return nullptr;
  DeviceGuard g(ctx->device);
  // the tables (the job's five and, when it has one, its flat twin's five) travel as ONE allocation and ONE copy (256-byte aligned sections)
  const TableLayout lay = table_layout(*job);
  const size_t total = lay.total;
  if (total) {
    std::vector<uint8_t> blob(total, 0);
    pack_tables(lay, blob.data());
    {                                       // a block of an earlier job of this context, if one is large enough
      std::lock_guard<std::mutex> lk(ctx->table_mu);
      for (size_t k = 0; k < ctx->table_pool.size(); ++k)
        if (ctx->table_pool[k].bytes >= total && ctx->table_pool[k].bytes <= 4 * total + (1u << 20)) {
          job->d_tables = std::move(ctx->table_pool[k]);
          ctx->table_pool.erase(ctx->table_pool.begin() + static_cast<std::ptrdiff_t>(k));
          break;
        }
    }
    if (job->d_tables.grow(total) != IST_OK ||
        hipMemcpy(job->d_tables.p, blob.data(), total, hipMemcpyHostToDevice) != hipSuccess) {      // blocking: the tables are in place when this returns
      (void)hipGetLastError();
      fail(IST_E_HIP, "uploading the op tables failed");
      ist_job_destroy(job.release());
      return nullptr;
    }
    point_tables(job.get(), lay, static_cast<uint8_t*>(job->d_tables.p));
  }
  return job.release();
}

int ist_job_info_get(const ist_job* job, ist_job_info* out) {
  if (!job || !out) return fail(IST_E_INVALID, "ist_job_info_get: NULL argument");
  *out = job->host.info;
  return IST_OK;
}

size_t ist_job_preferred_dst_pitch(const ist_job* job) {
  if (!job) return 0;
  const size_t row = static_cast<size_t>(job->host.rx1 - job->host.rx0) * 4;      // (a clipped job renders into a buffer as wide as its region)
  return job->flat ? row : (row + 4095) & ~static_cast<size_t>(4095);
}

int ist_job_launch(ist_job* job, const void* const* src, const size_t* src_pitch, int n_images, void* dst,
                   size_t dst_pitch, void* stream) {
  LaunchArgs a;
  const Compiled* run = nullptr;
  bool flat = false;
  const int rc = job_launch_args(job, src, src_pitch, n_images, dst, dst_pitch, &a, &run, &flat);
  if (rc) return rc;
  if (flat) g_flat_launches.fetch_add(1, std::memory_order_relaxed);
  DeviceGuard g(job->ctx->device);
  if (!g.ok) return fail(IST_E_NO_DEVICE, "hipSetDevice failed");
  note_launch_stream(job, stream);
  return launch_stitch(a, run->info.n_tiles, run->kernel_kind, stream);
}

void ist_job_destroy(ist_job* job) {
  if (!job) return;
  if (job->ctx) {
    DeviceGuard g(job->ctx->device);
    // the tables go to the context's pool for the next job: every launch must have read them first.  (What hipFree did
    // implicitly.  NOT an event per launch: recorded behind every kernel it cost back-to-back launches 3 % — 135 -> 140 us,
    // measured.)  Only the streams the job ran on are waited for: a host that shares the device (torch, the device group's
    // other streams) is not stalled by the death of one job.  One-shot jobs of the host-path entry points arrive here with
    // an idle stream.  A stream the caller has destroyed since makes the wait fail: then, and only then, the device is waited for.
    bool idle = true;
    if (job->launched) {
      bool per_stream = !job->launched_many;
      for (int k = 0; k < job->n_launched_on && per_stream; ++k)
        if (hipStreamSynchronize(job->launched_on[k]) != hipSuccess) { (void)hipGetLastError(); per_stream = false; }
      if (!per_stream) { idle = hipDeviceSynchronize() == hipSuccess; if (!idle) (void)hipGetLastError(); }
    }
    DevBuf evicted;                       // (freed outside the lock)
    if (job->d_tables.p && idle && job->d_tables.bytes <= (64u << 20)) {
      // a full pool gives up its OLDEST block for this one, so that a workload that repeats itself (a restitch of the same
      // layouts) finds the blocks it needs there again instead of allocating on every call behind blocks of earlier work
      std::lock_guard<std::mutex> lk(job->ctx->table_mu);
      std::vector<DevBuf>& pool = job->ctx->table_pool;
      if (static_cast<int>(pool.size()) >= ist_ctx::kTablePool) { evicted = std::move(pool.front()); pool.erase(pool.begin()); }
      pool.push_back(std::move(job->d_tables));
    }
  }
  delete job;
}

// buffers handed out by the library: pinned blocks go back to the pool, anything else was malloc'ed
void ist_free(void* p) {
  if (!p) return;
  if (!pool_give(p)) std::free(p);
}

void ist_pool_trim(void) { pool_trim(); }

}  // extern "C"
