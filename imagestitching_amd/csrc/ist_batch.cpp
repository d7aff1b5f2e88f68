// ist_batch.cpp — many independent stitches per kernel launch (ist_jobs_launch, ist_stitch_rgba8_batch, ist_stitch_png_batch).
//
// Reference anchor: each entry of a batch is one unchanged Page.onStitch (miniprogram-stitch/miniprogram/pages/index/index.js:
// 1186-1633; a request is capped at 9 images by index.js:311).  A service that renders many small requests pays, per request
// and call, a blocking table upload (ist_job_create), a dependent kernel boundary (ist_job_launch) and - on the host path - its
// own uploads, stream synchronisation and readback.  Here N jobs share one table copy and one launch per kernel form.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "ist_ctx.h"
#include "ist_internal.h"
#include "ist_jpeg_enc.h"
#include "ist_launch.h"

using namespace ist;

namespace {

std::atomic<int64_t> g_batch_launches{0};

// The host path splits a batch so that sources + canvases of one sub-batch stay under this many device bytes (a larger
// request runs alone, with the memory its single stitch would take).  Two sub-batches are in flight (Pipeline below), so the
// context keeps at most twice this much device scratch for batches.
// (IST_TUNING=1 IST_BATCH_BYTES=<bytes> overrides, read once, so that small canvases cross sub-batches)
constexpr size_t kSubBatchBytesDefault = size_t(512) << 20;
size_t sub_batch_bytes() {
  static const long long knob = (tuning_mode() && std::getenv("IST_BATCH_BYTES")) ? std::atoll(std::getenv("IST_BATCH_BYTES")) : 0;
  return knob > 0 ? static_cast<size_t>(knob) : kSubBatchBytesDefault;
}

}  // namespace

namespace ist {

// A ring slot large enough for `bytes`, free to be overwritten: the kernels that read it last time have completed.
int batch_take_slot(ist_ctx* ctx, size_t bytes, ist_ctx::BatchSlot** out) {
  ist_ctx::BatchSlot& s = ctx->batch_ring[ctx->batch_next];
  ctx->batch_next = (ctx->batch_next + 1) % ist_ctx::kBatchRing;
  if (s.pending) {
    if (hipEventSynchronize(s.done) != hipSuccess) { (void)hipGetLastError(); return fail(IST_E_HIP, "waiting for an earlier batch failed"); }
    s.pending = false;
  }
  const int rc = s.done.ensure();
  if (rc) return rc;
  size_t want = size_t(64) << 10;           // (a power of two: a slot grows in few steps)
  while (want < bytes) want <<= 1;
  if (s.host.grow(want)) return fail(IST_E_NOMEM, "out of pinned host memory for the batch table");
  if (s.dev.grow(want)) return fail(IST_E_NOMEM, "out of device memory for the batch table");
  *out = &s;
  return IST_OK;
}

}  // namespace ist

extern "C" {

int64_t ist_debug_batch_launches(void) { return g_batch_launches.load(std::memory_order_relaxed); }

int ist_jobs_launch(ist_job* const* jobs, int n_jobs, const void* const* src, const size_t* src_pitch, const int* n_images,
                    void* const* dst, const size_t* dst_pitch, void* stream) {
  if (n_jobs <= 0) return fail(IST_E_INVALID, "ist_jobs_launch: no jobs");
  if (n_jobs > kMaxBatchJobs) return fail(IST_E_UNSUPPORTED, "more than 4096 jobs in one batch");
  if (!jobs || !n_images || !dst || !dst_pitch) return fail(IST_E_INVALID, "ist_jobs_launch: NULL argument");
  ist_ctx* ctx = jobs[0] ? jobs[0]->ctx : nullptr;
  for (int k = 0; k < n_jobs; ++k) {
    if (!jobs[k]) return fail(IST_E_INVALID, "job " + std::to_string(k) + ": NULL job");
    if (jobs[k]->ctx != ctx) return fail(IST_E_INVALID, "job " + std::to_string(k) + " belongs to another context than job 0");
  }
  if (!ctx) return fail(IST_E_NO_CONTEXT, "无法获取绘图上下文");
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(IST_E_NO_DEVICE, "hipSetDevice failed");
  hipStream_t st = static_cast<hipStream_t>(stream);
  {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess) (void)hipGetLastError();
    else if (cs != hipStreamCaptureStatusNone) return fail(IST_E_UNSUPPORTED, "ist_jobs_launch: graph capture of a batch is not supported");
  }
  // every job is checked (and its arguments built) before anything is enqueued
  std::vector<LaunchArgs> args(static_cast<size_t>(n_jobs));
  std::vector<const Compiled*> run(static_cast<size_t>(n_jobs), nullptr);
  std::vector<char> flat_of(static_cast<size_t>(n_jobs), 0);
  size_t first = 0;
  for (int k = 0; k < n_jobs; ++k) {
    if (n_images[k] < 0) return fail(IST_E_INVALID, "job " + std::to_string(k) + ": negative image count");
    bool flat = false;
    const int rc = job_launch_args(jobs[k], src ? src + first : nullptr, src_pitch ? src_pitch + first : nullptr, n_images[k], dst[k],
                                   dst_pitch[k], &args[static_cast<size_t>(k)], &run[static_cast<size_t>(k)], &flat);
    if (rc) { const std::string why = g_last_error; return fail(rc, "job " + std::to_string(k) + ": " + why); }
    flat_of[static_cast<size_t>(k)] = flat ? 1 : 0;
    first += static_cast<size_t>(n_images[k]);
  }
  // one group per kernel form; jobs without tiles (an empty clip) launch nothing
  struct Group { std::vector<int> jobs; int64_t n_tiles = 0; unsigned lds = 0; size_t at_args = 0, at_begin = 0, at_chunk = 0; int64_t n_chunks = 0; };
  Group grp[kKernelKinds];
  for (int k = 0; k < n_jobs; ++k) {
    const Compiled& r = *run[static_cast<size_t>(k)];
    if (r.info.n_tiles <= 0) continue;
    // (a number that names no kind is grouped as the launchers run it, as KIND_GENERAL; the compiler writes none)
    const int kind = r.kernel_kind >= 0 && r.kernel_kind < kKernelKinds ? r.kernel_kind : KIND_GENERAL;
    Group& G = grp[kind];
    G.jobs.push_back(k);
    G.n_tiles += r.info.n_tiles;
    G.lds = std::max(G.lds, static_cast<unsigned>(args[static_cast<size_t>(k)].lds_words) * 4u);
  }
  size_t total = 0;
  for (Group& G : grp) {
    if (G.jobs.empty()) continue;
    if (G.n_tiles > 0x7FFFFFFF) return fail(IST_E_UNSUPPORTED, "a batch of more than 2^31 - 1 tiles of one kernel form");
    const size_t m = G.jobs.size();
    G.n_chunks = (G.n_tiles + (int64_t(1) << kBatchChunkLg) - 1) >> kBatchChunkLg;
    G.at_args = total;  total = round256(total + m * sizeof(LaunchArgs));
    G.at_begin = total; total = round256(total + (m + 1) * sizeof(int64_t));
    G.at_chunk = total; total = round256(total + static_cast<size_t>(G.n_chunks + 1) * sizeof(int32_t));
  }
  if (total == 0) return IST_OK;
  std::lock_guard<std::mutex> lk(ctx->batch_mu);
  ist_ctx::BatchSlot* slot = nullptr;
  int rc = batch_take_slot(ctx, total, &slot);
  if (rc) return rc;
  uint8_t* h = static_cast<uint8_t*>(slot->host.p);
  for (const Group& G : grp) {
    if (G.jobs.empty()) continue;
    const size_t m = G.jobs.size();
    LaunchArgs* ja = reinterpret_cast<LaunchArgs*>(h + G.at_args);
    int64_t* tb = reinterpret_cast<int64_t*>(h + G.at_begin);
    int32_t* cj = reinterpret_cast<int32_t*>(h + G.at_chunk);
    int64_t t = 0;
    for (size_t j = 0; j < m; ++j) {
      const int k = G.jobs[j];
      std::memcpy(&ja[j], &args[static_cast<size_t>(k)], sizeof(LaunchArgs));
      tb[j] = t;
      t += run[static_cast<size_t>(k)]->info.n_tiles;
    }
    tb[m] = t;
    size_t j = 0;
    for (int64_t c = 0; c < G.n_chunks; ++c) {            // the job that holds the chunk's first tile
      const int64_t first_tile = c << kBatchChunkLg;
      while (j + 1 < m && tb[j + 1] <= first_tile) ++j;
      cj[c] = static_cast<int32_t>(j);
    }
    cj[G.n_chunks] = static_cast<int32_t>(m - 1);
  }
  uint8_t* d = static_cast<uint8_t*>(slot->dev.p);
  if (hipMemcpyAsync(d, h, total, hipMemcpyHostToDevice, st) != hipSuccess) { (void)hipGetLastError(); return fail(IST_E_HIP, "uploading the batch table failed"); }
  int launches = 0;
  for (int kind = 0; kind < kKernelKinds && rc == IST_OK; ++kind) {
    const Group& G = grp[kind];
    if (G.jobs.empty()) continue;
    BatchArgs b;
    b.jobs = reinterpret_cast<const LaunchArgs*>(d + G.at_args);
    b.tile_begin = reinterpret_cast<const int64_t*>(d + G.at_begin);
    b.chunk_job = reinterpret_cast<const int32_t*>(d + G.at_chunk);
    b.n_tiles = G.n_tiles;
    rc = launch_stitch_batch(b, kind, G.lds, stream);
    if (rc != IST_OK) break;
    ++launches;
    int64_t flats = 0;                                    // (bookkeeping only for what was launched)
    for (const int k : G.jobs) { note_launch_stream(jobs[k], stream); flats += flat_of[static_cast<size_t>(k)]; }
    count_flat_launches(flats);
  }
  // (recorded whatever happened: the copy is in flight and the slot must not be refilled before it is done)
  if (hipEventRecord(slot->done, st) == hipSuccess) slot->pending = true;
  else { (void)hipGetLastError(); (void)hipStreamSynchronize(st); }
  g_batch_launches.fetch_add(launches, std::memory_order_relaxed);
  return rc;
}

}  // extern "C"

namespace {

// jobs of a sub-batch whose kernel has completed (its half's kernel_done event): they are dropped without the stream wait of
// ist_job_destroy, which would also wait for the launch of the NEXT sub-batch queued behind it on the same stream
void drop_jobs(std::vector<JobPtr>* jobs) {
  for (JobPtr& j : *jobs) { j->launched = false; j->n_launched_on = 0; j->launched_many = false; }
  jobs->clear();
}

// The host path, sub-batch after sub-batch through the two halves of ctx->batch_half: sub-batch i is compiled, its tables and
// sources go up on the staging stream while sub-batch i - 1's canvases come down on the aux stream, then one ist_jobs_launch on
// ctx->stream renders it into half i % 2, and its canvases follow on the aux stream into pooled pinned blocks (the batch class of
// the pool: a batch's caller holds all its results at once).  (What the single-stitch path does band by band, done sub-batch by
// sub-batch: both directions of PCIe busy at once.)
// With out_len (ist_stitch_png_batch) every result is a PNG file instead: the sub-batch's canvases are encoded straight from the
// half's canvas area into its file area by one compression launch (+ one gather launch) on ctx->stream, and the files come down on
// the aux stream, each exactly as long as it is; the few header / trailer bytes no kernel writes are patched into the host copies
// once the downloads are done (apply_patches).
// With quality / subsampling (ist_stitch_jpeg_batch) every result is a JPEG file: the same, through the batch encoder of
// ist_jpeg_encode.hip, whose gather writes every byte of a file - nothing is patched.
struct Pipeline {
  ist_ctx* ctx;
  const ist_stitch_request* reqs;
  const std::vector<std::vector<ist_op>>& ops;
  const std::vector<int>& n_ops;
  const ist_plan* plans;
  uint8_t** out_pixels;
  int64_t* out_len;                       // PNG or JPEG files out (NULL: canvases)
  const int* quality = nullptr;           // JPEG files out: per request (NULL: PNG)
  const int* subsampling = nullptr;
  PngForm png;                            // PNG files out: the form of the call
  std::vector<JobPtr> jobs[2];            // the jobs whose tables live in half 0 / 1
  bool used[2] = {false, false};
  int next = 0;
  std::vector<std::pair<int, std::vector<PngPatch>>> patches;   // (request, its file's patches), applied after finish()

  Pipeline(ist_ctx* c, const ist_stitch_request* r, const std::vector<std::vector<ist_op>>& o, const std::vector<int>& no, const ist_plan* p, uint8_t** out,
           int64_t* len = nullptr)
      : ctx(c), reqs(r), ops(o), n_ops(no), plans(p), out_pixels(out), out_len(len) {}

  void apply_patches() {
    for (const auto& fp : patches)
      for (const PngPatch& pt : fp.second) std::memcpy(out_pixels[fp.first] + pt.at, pt.b, static_cast<size_t>(pt.n));
  }

  // everything queued is done; jobs dropped.  Returns rc.
  int finish(int rc) {
    const bool ok = hipStreamSynchronize(ctx->stream) == hipSuccess && (!ctx->aux || hipStreamSynchronize(ctx->aux) == hipSuccess);
    if (!ok) { (void)hipGetLastError(); if (rc == IST_OK) rc = fail(IST_E_HIP, "result readback failed"); }
    if (ctx->stager) (void)ctx->stager->sync();
    drop_jobs(&jobs[0]); drop_jobs(&jobs[1]);
    return rc;
  }

  int run(const std::vector<int>& idx) {
    const size_t n = idx.size();
    const int hi = next; next ^= 1;
    ist_ctx::BatchHalf& H = ctx->batch_half[hi];
    std::vector<JobPtr> js(n);
    std::vector<TableLayout> lay(n);
    SourceLayout src;                                      // the sources every job samples, request after request
    std::vector<size_t> tab_at(n, 0), dst_at(n, 0), canvas_bytes(n, 0), file_at(n, 0), file_cap(n, 0);
    size_t tab_total = 0, dst_total = 0, file_total = 0;
    for (size_t q = 0; q < n; ++q) {
      const int k = idx[q];
      const ist_stitch_request& r = reqs[k];
      const ist_plan& p = plans[k];
      js[q].reset(job_compile(ctx, p.canvas_w, p.canvas_h, kTransparent, ops[static_cast<size_t>(k)].data(), n_ops[static_cast<size_t>(k)],
                              r.images, r.n_images, r.filter, nullptr));
      int rc = js[q] ? src.add(r.images, r.n_images, r.src, r.src_pitch, whole_bitmaps(js[q]->host)) : (g_last_code ? g_last_code : IST_E_INVALID);
      if (rc) { const std::string why = g_last_error; return fail(rc, "request " + std::to_string(k) + ": " + why); }
      lay[q] = table_layout(*js[q]);
      tab_at[q] = tab_total; tab_total += round256(lay[q].total);
      canvas_bytes[q] = static_cast<size_t>(p.canvas_w) * 4 * static_cast<size_t>(p.canvas_h);
      dst_at[q] = dst_total; dst_total += round256(canvas_bytes[q]);
      if (out_len) {
        file_cap[q] = static_cast<size_t>(quality ? ist_jpeg_bound(p.canvas_w, p.canvas_h, subsampling[k]) : ist_png_bound(p.canvas_w, p.canvas_h));
        file_at[q] = file_total; file_total += round256(file_cap[q]);
      }
    }
    // the half is free once the launch that read it (two sub-batches ago) is done; its canvases must also be down before they
    // are re-allocated (a growth) or overwritten (ordered on the device below)
    if (used[hi]) {
      if (hipEventSynchronize(H.kernel_done) != hipSuccess) { (void)hipGetLastError(); return fail(IST_E_HIP, "waiting for an earlier sub-batch failed"); }
      drop_jobs(&jobs[hi]);
      if ((H.dst.bytes < dst_total || H.file.bytes < file_total) && hipEventSynchronize(H.read_done) != hipSuccess) { (void)hipGetLastError(); return fail(IST_E_HIP, "waiting for an earlier sub-batch failed"); }
    }
    int rc = H.kernel_done.ensure();
    if (!rc) rc = H.read_done.ensure();
    if (!rc) rc = H.tab.grow(tab_total ? tab_total : 256);
    if (!rc) rc = H.src.grow(src.bytes());
    if (!rc) rc = H.dst.grow(dst_total ? dst_total : 256);
    if (!rc && out_len) rc = H.file.grow(file_total ? file_total : 256);
    if (rc) return rc;
    uint8_t* dtab = static_cast<uint8_t*>(H.tab.p);
    uint8_t* ddst = static_cast<uint8_t*>(H.dst.p);
    // every job's tables in one host block: one item of the staged upload
    std::vector<uint8_t> blob(tab_total, 0);
    std::vector<RowsCopy> up;
    for (size_t q = 0; q < n; ++q) {
      pack_tables(lay[q], blob.data() + tab_at[q]);
      point_tables(js[q].get(), lay[q], dtab + tab_at[q]);
    }
    if (tab_total) up.push_back(RowsCopy{dtab, blob.data(), nullptr, tab_total, tab_total, 1});
    const SourceLayout::Placed at = src.place(H.src.p);
    src.copy_all(&up);
    std::vector<ist_job*> ljob(n, nullptr);
    std::vector<int> lcount(n, 0);
    std::vector<void*> ldst(n, nullptr);
    std::vector<size_t> ldst_pitch(n, 0);
    for (size_t q = 0; q < n; ++q) {
      ljob[q] = js[q].get();
      lcount[q] = reqs[idx[q]].n_images;
      ldst[q] = ddst + dst_at[q];
      ldst_pitch[q] = static_cast<size_t>(plans[idx[q]].canvas_w) * 4;
    }
    rc = stager_of(ctx).upload_big(up, ctx->stream, &workers_of(ctx));      // (one stream, big pieces: it shares PCIe with the downloads)
    if (rc) return rc;
    if (used[hi] && hipStreamWaitEvent(ctx->stream, H.read_done, 0) != hipSuccess) { (void)hipGetLastError(); return fail(IST_E_HIP, "ordering a sub-batch failed"); }
    rc = ist_jobs_launch(ljob.data(), static_cast<int>(n), at.ptr.data(), at.pitch.data(), lcount.data(), ldst.data(), ldst_pitch.data(), ctx->stream);
    if (rc) return rc;
    if (hipEventRecord(H.kernel_done, ctx->stream) != hipSuccess) { (void)hipGetLastError(); return fail(IST_E_HIP, "hipEventRecord failed"); }
    used[hi] = true;
    jobs[hi] = std::move(js);                              // (the pipeline drops them once their launch is done)
    if (out_len) return encode_and_read(idx, H, ddst, dst_at, file_at, file_cap);
    // every canvas into a pinned block of its own, on the aux stream behind the launch
    if (hipStreamWaitEvent(ctx->aux, H.kernel_done, 0) != hipSuccess) { (void)hipGetLastError(); return fail(IST_E_HIP, "ordering a readback failed"); }
    for (size_t q = 0; q < n; ++q) {
      uint8_t* host = static_cast<uint8_t*>(pool_take_batch(canvas_bytes[q]));
      if (!host) return fail(IST_E_NOMEM, "out of pinned host memory for the results");
      out_pixels[idx[q]] = host;                           // (the caller's release() gives it back, after finish())
      if (hipMemcpyAsync(host, ddst + dst_at[q], canvas_bytes[q], hipMemcpyDeviceToHost, ctx->aux) != hipSuccess) { (void)hipGetLastError(); return fail(IST_E_HIP, "queueing a readback failed"); }
    }
    if (hipEventRecord(H.read_done, ctx->aux) != hipSuccess) { (void)hipGetLastError(); return fail(IST_E_HIP, "hipEventRecord failed"); }
    return IST_OK;
  }

  // the sub-batch's canvases (rendered on ctx->stream) -> PNG files in the half's file area, ONE compression launch for all of them
  // (the encoder returns with ctx->stream idle); then every file into a pinned block of its real length, on the aux stream
  int encode_and_read(const std::vector<int>& idx, ist_ctx::BatchHalf& H, uint8_t* ddst, const std::vector<size_t>& dst_at,
                      const std::vector<size_t>& file_at, const std::vector<size_t>& file_cap) {
    const size_t n = idx.size();
    uint8_t* dfile = static_cast<uint8_t*>(H.file.p);
    if (quality) return encode_and_read_jpeg(idx, H, ddst, dst_at, file_at, file_cap);
    std::vector<PngBatchFile> files(n);
    for (size_t q = 0; q < n; ++q) {
      const ist_plan& p = plans[idx[q]];
      files[q] = PngBatchFile{ddst + dst_at[q], static_cast<size_t>(p.canvas_w) * 4, p.canvas_w, p.canvas_h, dfile + file_at[q],
                              static_cast<int64_t>(file_cap[q]), 0, {}};
      const int rc = png_batch_check(files[q], idx[q]);
      if (rc) { const std::string why = g_last_error; return fail(rc, "request " + std::to_string(idx[q]) + ": " + why); }
    }
    const int rc = png.compressed() ? png_encode_batch_deflate(ctx, png, files, ctx->stream, true) : png_encode_batch_stored(ctx, png, files, ctx->stream, true);
    if (rc) return rc;
    for (size_t q = 0; q < n; ++q) {
      const size_t len = static_cast<size_t>(files[q].len);
      uint8_t* host = static_cast<uint8_t*>(pool_take_batch(len));
      if (!host) return fail(IST_E_NOMEM, "out of pinned host memory for the results");
      out_pixels[idx[q]] = host;                           // (the caller's release() gives it back, after finish())
      out_len[idx[q]] = files[q].len;
      if (hipMemcpyAsync(host, dfile + file_at[q], len, hipMemcpyDeviceToHost, ctx->aux) != hipSuccess) { (void)hipGetLastError(); return fail(IST_E_HIP, "queueing a readback failed"); }
      patches.emplace_back(idx[q], std::move(files[q].patches));
    }
    if (hipEventRecord(H.read_done, ctx->aux) != hipSuccess) { (void)hipGetLastError(); return fail(IST_E_HIP, "hipEventRecord failed"); }
    return IST_OK;
  }

  // ... -> JPEG files: one transform, one entropy and one gather launch per round of the batch encoder for all of them
  int encode_and_read_jpeg(const std::vector<int>& idx, ist_ctx::BatchHalf& H, uint8_t* ddst, const std::vector<size_t>& dst_at,
                           const std::vector<size_t>& file_at, const std::vector<size_t>& file_cap) {
    const size_t n = idx.size();
    uint8_t* dfile = static_cast<uint8_t*>(H.file.p);
    std::vector<JpegBatchFile> files(n);
    for (size_t q = 0; q < n; ++q) {
      const ist_plan& p = plans[idx[q]];
      files[q] = JpegBatchFile{ddst + dst_at[q], static_cast<size_t>(p.canvas_w) * 4, p.canvas_w, p.canvas_h, quality[idx[q]], subsampling[idx[q]],
                               dfile + file_at[q], static_cast<int64_t>(file_cap[q]), 0};
      const int rc = jpeg_batch_check(files[q], "request", idx[q]);
      if (rc) return rc;
    }
    const int rc = jpeg_encode_batch(ctx, files, ctx->stream, "request", idx.data());
    if (rc) return rc;
    for (size_t q = 0; q < n; ++q) {
      const size_t len = static_cast<size_t>(files[q].len);
      uint8_t* host = static_cast<uint8_t*>(pool_take_batch(len));
      if (!host) return fail(IST_E_NOMEM, "out of pinned host memory for the results");
      out_pixels[idx[q]] = host;                           // (the caller's release() gives it back, after finish())
      out_len[idx[q]] = files[q].len;
      if (hipMemcpyAsync(host, dfile + file_at[q], len, hipMemcpyDeviceToHost, ctx->aux) != hipSuccess) { (void)hipGetLastError(); return fail(IST_E_HIP, "queueing a readback failed"); }
    }
    if (hipEventRecord(H.read_done, ctx->aux) != hipSuccess) { (void)hipGetLastError(); return fail(IST_E_HIP, "hipEventRecord failed"); }
    return IST_OK;
  }
};

// ist_stitch_rgba8_batch (out_len NULL), ist_stitch_png_batch (png: its form) and (quality, subsampling given) ist_stitch_jpeg_batch
int stitch_batch(ist_ctx* ctx, const ist_stitch_request* reqs, int n_reqs, ist_plan* out_plans, uint8_t** out_pixels, int64_t* out_len,
                 const int* quality = nullptr, const int* subsampling = nullptr, const PngForm& png = {}) {
  const size_t n = static_cast<size_t>(n_reqs);
  for (size_t k = 0; k < n; ++k) { out_pixels[k] = nullptr; std::memset(&out_plans[k], 0, sizeof(ist_plan)); if (out_len) out_len[k] = 0; }
  auto release = [&]() {
    for (size_t k = 0; k < n; ++k) {
      ist_plan_free(&out_plans[k]);
      std::memset(&out_plans[k], 0, sizeof(ist_plan));
      if (out_pixels[k]) { ist_free(out_pixels[k]); out_pixels[k] = nullptr; }
      if (out_len) out_len[k] = 0;
    }
  };
  // plan every request (pure CPU): the op list of each, and what it will hold on the device
  std::vector<std::vector<ist_op>> ops(n);
  std::vector<int> n_ops(n, 0);
  std::vector<size_t> bytes(n, 0);
  for (size_t k = 0; k < n; ++k) {
    const ist_stitch_request& r = reqs[k];
    if (r.n_images <= 0) continue;                        // index.js:1189: nothing to do for this entry
    const int rc = plan_with_ops(r.images, r.n_images, r.direction, r.mode, r.gap, r.limits, &out_plans[k], &ops[k]);
    if (rc == IST_NOTHING_TO_DO) { std::memset(&out_plans[k], 0, sizeof(ist_plan)); continue; }
    if (rc < 0) { const std::string why = g_last_error; release(); return fail(rc, "request " + std::to_string(k) + ": " + why); }
    n_ops[k] = static_cast<int>(ops[k].size());
    bytes[k] = static_cast<size_t>(out_plans[k].canvas_w) * 4 * static_cast<size_t>(out_plans[k].canvas_h);
    for (int i = 0; i < r.n_images; ++i)
      bytes[k] += static_cast<size_t>(std::max<int64_t>(0, bitmap_w(r.images[i]))) * 4 * static_cast<size_t>(std::max<int64_t>(0, bitmap_h(r.images[i])));
    if (quality) {                                        // + its file (the encoder's scratch is its own, bounded by its budget)
      const int rcj = jpeg_check_export(("request " + std::to_string(k)).c_str(), out_plans[k].canvas_w, out_plans[k].canvas_h, quality[k], subsampling[k]);
      if (rcj) { KeepLastError keep; release(); return rcj; }
      bytes[k] += static_cast<size_t>(ist_jpeg_bound(out_plans[k].canvas_w, out_plans[k].canvas_h, subsampling[k]));
    } else if (out_len) {                                 // + its file, and at level 1 its chunk slots (~1.01 x the canvas)
      const int64_t cw = out_plans[k].canvas_w, ch = out_plans[k].canvas_h;
      bytes[k] += static_cast<size_t>(ist_png_bound(cw, ch));
      // (the RGBA chunk count whatever the call's colour form: the RGBA count is the documented upper bound for both - the RGB form never
      // has more chunks - and a budget that does not depend on the colour cuts the same sub-batches for both)
      if (png.compressed()) bytes[k] += static_cast<size_t>(png_deflate_chunks(cw, ch) * png_deflate_slot_bytes());
    }
  }
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceGuard g(ctx->device);
  if (!g.ok) { release(); return fail(IST_E_NO_DEVICE, "hipSetDevice failed"); }
  int rc = ensure_aux(ctx);
  if (rc) { release(); return rc; }
  // sub-batches: consecutive requests while their device bytes fit the budget, and at most kMaxBatchJobs of them
  Pipeline pipe(ctx, reqs, ops, n_ops, out_plans, out_pixels, out_len);
  pipe.quality = quality; pipe.subsampling = subsampling; pipe.png = png;
  std::vector<int> idx;
  size_t held = 0;
  const size_t budget = sub_batch_bytes();
  for (size_t k = 0; k <= n && rc == IST_OK; ++k) {
    const bool live = k < n && n_ops[k] > 0;
    const bool flush = !idx.empty() && (k == n || (live && (held + bytes[k] > budget || idx.size() >= static_cast<size_t>(kMaxBatchJobs))));
    if (flush) { rc = pipe.run(idx); idx.clear(); held = 0; }
    if (live) { idx.push_back(static_cast<int>(k)); held += bytes[k]; }
  }
  rc = pipe.finish(rc);
  if (rc) { KeepLastError keep; release(); return rc; }
  pipe.apply_patches();
  return IST_OK;
}

}  // namespace

extern "C" {

int ist_stitch_rgba8_batch(ist_ctx* ctx, const ist_stitch_request* reqs, int n_reqs, ist_plan* out_plans, uint8_t** out_pixels) {
  if (!ctx) return fail(IST_E_NO_CONTEXT, "无法获取绘图上下文");
  if (n_reqs < 0 || (n_reqs > 0 && (!reqs || !out_plans || !out_pixels))) return fail(IST_E_INVALID, "ist_stitch_rgba8_batch: NULL argument");
  return stitch_batch(ctx, reqs, n_reqs, out_plans, out_pixels, nullptr);
}

int ist_stitch_png_batch(ist_ctx* ctx, const ist_stitch_request* reqs, int n_reqs, ist_plan* out_plans, uint8_t** out_png, int64_t* out_len) {
  if (!ctx) return fail(IST_E_NO_CONTEXT, "无法获取绘图上下文");
  if (n_reqs < 0 || (n_reqs > 0 && (!reqs || !out_plans || !out_png || !out_len))) return fail(IST_E_INVALID, "ist_stitch_png_batch: NULL argument");
  const PngForm form = settings_of(ctx).png;      // the call's form: read once
  { const int rc = form.check(); if (rc) return rc; }
  return stitch_batch(ctx, reqs, n_reqs, out_plans, out_png, out_len, nullptr, nullptr, form);
}

int ist_stitch_jpeg_batch(ist_ctx* ctx, const ist_stitch_request* reqs, int n_reqs, const int* quality, const int* subsampling,
                          ist_plan* out_plans, uint8_t** out_jpeg, int64_t* out_len) {
  if (!ctx) return fail(IST_E_NO_CONTEXT, "无法获取绘图上下文");
  if (n_reqs < 0 || (n_reqs > 0 && (!reqs || !quality || !subsampling || !out_plans || !out_jpeg || !out_len)))
    return fail(IST_E_INVALID, "ist_stitch_jpeg_batch: NULL argument");
  // the options of EVERY request, the ones without images included, before anything is planned
  for (int k = 0; k < n_reqs; ++k) { out_jpeg[k] = nullptr; out_len[k] = 0; std::memset(&out_plans[k], 0, sizeof(ist_plan)); }
  for (int k = 0; k < n_reqs; ++k) {
    const int rc = jpeg_check_options(("request " + std::to_string(k)).c_str(), quality[k], subsampling[k]);
    if (rc) return rc;
  }
  return stitch_batch(ctx, reqs, n_reqs, out_plans, out_jpeg, out_len, quality, subsampling);
}

}  // extern "C"
