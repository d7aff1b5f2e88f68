// ist_files.cpp — files -> PNG: the whole onStitch for files, device-resident.  Only file bytes go in and only PNG bytes come out
// over PCIe (ist_stitch_files_png, ist_stitch_paths_png).
//
// decode (index.js:1441-1520) -> plan (1251-1386) -> resample+blit (1532-1551) -> PNG export (1577-1579), PIPELINED: the
// planner needs only the frame headers, so the canvas is laid out first; then every image decodes on its own thread and
// stream (FileDecoder, ist_decode.cpp), band k of the canvas is rendered as soon as image k is there, and the PNG encoder - which
// works slab by slab, each slab crossing PCIe while the next one compresses - asks for canvas rows as it reaches them.  The first
// slabs of the file are on their way to the host while the last images are still in the Huffman decoder.  Which bands there
// are, which of them need no launch and which a request submits is index arithmetic: ist_file_bands.cpp.
#include <hip/hip_runtime_api.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <mutex>

#include "ist_decode.h"
#include "ist_file_bands.h"

using namespace ist;

namespace {
std::atomic<int64_t> g_direct_images{0};

// One stitch cut into a background launch + one launch per draw (cut_file_bands): band k can be rendered - and exported - as
// soon as image k is decoded.  ok = false when the stitch is not cut: the caller then renders the canvas with ONE launch once
// every image is there.
struct BandedJobs {
  bool ok = false;
  std::vector<JobPtr> band;              // per part
  JobPtr bg;                             // (released before the bands)
  std::vector<ist_part> parts;           // sorted by Y0
};

int compile_banded(ist_ctx* ctx, int64_t cw, int64_t ch, const uint8_t clear[4], const ist_op* ops, int n_ops, const ist_image_desc* images,
                   int n_images, int filter, BandedJobs* out) {
  std::vector<ist_part> cut;
  std::vector<ist_region> boxes;
  if (!cut_file_bands(ops, n_ops, cw, ch, images, n_images, filter, &cut, &boxes)) return IST_OK;      // not banded, not an error
  const std::vector<ist_op> bg = shard_root_ops(ops, n_ops, {}, boxes);
  out->bg.reset(ist_job_create(ctx, cw, ch, clear, bg.data(), static_cast<int>(bg.size()), images, n_images, filter, nullptr));
  if (!out->bg) return g_last_code ? g_last_code : IST_E_INVALID;
  for (size_t k = 0; k < cut.size(); ++k) {
    const std::vector<ist_op> one = shard_part_ops(ops, n_ops, cut[k]);
    out->band.emplace_back(ist_job_create(ctx, cw, ch, clear, one.data(), static_cast<int>(one.size()), images, n_images, filter, &boxes[k]));
    if (!out->band.back()) return g_last_code ? g_last_code : IST_E_INVALID;
  }
  out->parts = cut;
  out->ok = true;
  return IST_OK;
}

// (the caller holds ctx->mu and has checked the arguments; set: its snapshot of the context's settings, the PNG form checked)
int stitch_files_png_locked(ist_ctx* ctx, const Settings& set, const uint8_t* const* files, const int64_t* lens, int n_images, int direction, int mode,
                            double gap, const ist_limits* limits, int filter, ist_plan* out_plan, uint8_t** out_png, int64_t* out_len,
                            ist_preview* preview) {
  const int n = n_images;
  DeviceGuard g(ctx->device);
  Phases ph(ctx, set.timing);
  // (IST_TUNING=1 IST_TIMELINE=1: host-side marks of one call on stderr, microseconds from its start)
  const bool tl_outer = tl_active();                      // (ist_stitch_paths_png started the call's clock: its file reads are part of the call)
  if (!tl_outer) tl_begin();
  struct TlEnd { bool mine; ~TlEnd() { if (mine) tl_end("ist_stitch_files_png"); } } tl_end_guard{!tl_outer};
  FileDecoder fd(ctx, files, lens, n, &ph, set.color_profile);
  int rc = fd.headers();
  if (rc) return rc;
  tl_mark("headers parsed");
  const std::vector<ist_image_desc> descs = fd.descs(lens);
  std::vector<ist_op> ops;
  rc = plan_with_ops(descs.data(), n, direction, mode, gap, limits, out_plan, &ops);
  if (rc != IST_OK) return rc;
  PlanGuard pg{out_plan};
  const int n_ops = static_cast<int>(ops.size());

  // one device arena (the context's, grow-only): bitmaps, JPEG coefficient planes + sample planes, canvas, PNG
  size_t off = 0;
  std::vector<size_t> o_img(static_cast<size_t>(n));
  for (int i = 0; i < n; ++i) o_img[static_cast<size_t>(i)] = arena_take(&off, static_cast<size_t>(fd.dec(i).w) * 4 * fd.dec(i).h + 16);
  fd.layout(&off);
  const size_t canvas_pitch = static_cast<size_t>(out_plan->canvas_w) * 4;
  const size_t o_canvas = arena_take(&off, canvas_pitch * static_cast<size_t>(out_plan->canvas_h));
  const int64_t png_cap = ist_png_bound(out_plan->canvas_w, out_plan->canvas_h);
  const size_t o_png = arena_take(&off, static_cast<size_t>(png_cap));
  rc = ctx->scratch_arena.grow(off);
  if (rc) return rc;
  uint8_t* d = static_cast<uint8_t*>(ctx->scratch_arena.p);
  ph.lap(IST_PHASE_PLAN_ARENA, "plan + device arena", nullptr);
  std::vector<uint8_t*> img(static_cast<size_t>(n));
  std::vector<const void*> dsrc(static_cast<size_t>(n));
  std::vector<size_t> dpitch(static_cast<size_t>(n));
  for (int i = 0; i < n; ++i) {
    img[static_cast<size_t>(i)] = d + o_img[static_cast<size_t>(i)];
    dsrc[static_cast<size_t>(i)] = img[static_cast<size_t>(i)];
    dpitch[static_cast<size_t>(i)] = static_cast<size_t>(fd.dec(i).w) * 4;
  }
  tl_mark("plan + arena");
  rc = fd.start(d, img.data(), dpitch.data());          // the images decode from here on
  if (rc) return rc;
  tl_mark("workers started");
  // Two streams: RENDER (Huffman batch, then per image: reconstruction + its band of the canvas) and ctx->stream (the PNG
  // encoder, which waits for band k's event before it compresses the slabs that read it).  On one stream the reconstruction
  // of image k+1 sat between the slabs of band k and band k+1 and cost its full time; on its own stream it runs beside them.
  rc = ensure_aux(ctx);
  if (rc) return rc;
  rc = ensure_render(ctx);
  if (rc) return rc;
  hipStream_t render = ph.on ? ctx->stream : ctx->render;
  // the stitch, cut per image (compiled while the workers parse): background now, band k when image k is there
  BandedJobs bj;
  rc = compile_banded(ctx, out_plan->canvas_w, out_plan->canvas_h, kTransparent, ops.data(), n_ops, descs.data(), n, filter, &bj);
  if (rc) return rc;
  tl_mark("banded jobs compiled");
  JobPtr whole;
  if (!bj.ok) {
    whole.reset(ist_job_create(ctx, out_plan->canvas_w, out_plan->canvas_h, kTransparent, ops.data(), n_ops, descs.data(), n, filter, nullptr));
    if (!whole) return g_last_code ? g_last_code : IST_E_INVALID;
  } else {
    rc = ist_job_launch(bj.bg.get(), dsrc.data(), dpitch.data(), n, d + o_canvas, canvas_pitch, render);
    if (rc) return rc;
  }
  // A draw that only MOVES its image - no scaling, no turn, whole pixels, nothing clipped, an opaque source - needs no bitmap
  // of its own and no launch: the image is reconstructed straight into its box of the canvas (the colour kernel writes with the
  // canvas pitch).  That is every draw of a same-width vertical strip (BASELINE configs[1]): per 12 MP photo 48 MB less to
  // write, 96 MB less to read and write again, and one launch less.  (Pipelined mode only: the phase-timed run keeps the
  // stitch a step of its own; both make the same canvas.)
  std::vector<char> direct(bj.parts.size(), 0);
  if (bj.ok && !ph.on) {
    for (size_t k = 0; k < bj.parts.size(); ++k) {
      const ist_part& p = bj.parts[k];
      ist_job_info info;
      if (!draw_moves_whole_image(ops[static_cast<size_t>(p.op)], p, descs[static_cast<size_t>(p.image)], out_plan->canvas_w, out_plan->canvas_h)) continue;
      if (!fd.dec(p.image).jpeg) continue;               // (an opaque source whose colour kernel writes with any pitch)
      if (ist_job_info_get(bj.band[k].get(), &info) != IST_OK || info.tiles_copy != info.n_tiles || info.n_tiles == 0) continue;      // (the compiler agrees: copy tiles only)
      bool shared = false;                               // (an image drawn twice keeps its bitmap)
      for (size_t q = 0; q < bj.parts.size(); ++q) if (q != k && bj.parts[q].image == p.image) shared = true;
      if (shared) continue;
      direct[k] = 1;
      g_direct_images.fetch_add(1, std::memory_order_relaxed);
      img[static_cast<size_t>(p.image)] = d + o_canvas + static_cast<size_t>(p.Y0) * canvas_pitch + static_cast<size_t>(p.X0) * 4;
      dpitch[static_cast<size_t>(p.image)] = canvas_pitch;
      dsrc[static_cast<size_t>(p.image)] = img[static_cast<size_t>(p.image)];
    }
  }
  bool rendered_whole = false;
  // the export is about to read canvas rows [0, y_end) on `reader` (one of the encoder's two streams): order it behind the
  // render of those rows
  auto ordered = [&](hipStream_t reader, hipEvent_t ev) -> int {
    if (render != reader) IST_HIP_OR(hipStreamWaitEvent(reader, ev, 0), "ordering the export behind the render failed");
    return IST_OK;
  };
  rc = ctx->render_done.ensure();
  if (rc) return rc;
  // The FIRST request renders everything: behind the Huffman batch every image is reconstructed and its band rendered on the
  // render stream, an event per band (the images' upload events are free again by then).  History (rocprofv3 timelines,
  // profiles/r03_file_pipeline_kernels.txt is the last of them): (1) pulling band k+1 only when slab k+1 was about to be
  // submitted put its reconstruction in competition with slab k's compression, which fills every CU - the 40 us colour
  // kernel took 250 us and the slabs ran one after the other at half speed; (2) a render THREAD that submitted the bands while
  // the encoder's thread submitted slabs was slower still (7.2-7.4 ms against 6.6-7.0): the render kernels then trickled in
  // between the slabs' workgroups for 4.4 ms instead of 1.0.  The compressing kernel owns the chip while it runs; the only work
  // that really hides behind it is the file's trip over PCIe.
  BandSchedule sched(bj.parts);
  auto need_rows = [&](int64_t y_end, void* reader_) -> int {
    hipStream_t reader = static_cast<hipStream_t>(reader_);
    if (!bj.ok) {
      if (!rendered_whole) {
        int rc2 = fd.finish(render);
        if (rc2) return rc2;
        rendered_whole = true;
        rc2 = ist_job_launch(whole.get(), dsrc.data(), dpitch.data(), n, d + o_canvas, canvas_pitch, render);
        if (rc2) return rc2;
        IST_HIP_OR(hipEventRecord(ctx->render_done, render), "hipEventRecord failed");
      }
      return ordered(reader, ctx->render_done);
    }
    // first request (the short first slab): only the bands it reads, so that the file's first bytes are on their way while the
    // rest is rendered; every later request: everything that is left
    const BandSchedule::Request r = sched.request(y_end);
    const bool first_request = r.begin == 0;
    if (r.begin < bj.parts.size()) tl_mark(first_request ? "first rows requested" : "rest of the rows requested");
    for (size_t k = r.begin; k < r.end; ++k) {
      int rc2 = fd.take(bj.parts[k].image, render);
      if (rc2) return rc2;
      if (!direct[k]) rc2 = ist_job_launch(bj.band[k].get(), dsrc.data(), dpitch.data(), n, d + o_canvas, canvas_pitch, render);
      if (rc2) return rc2;
      IST_HIP_OR(hipEventRecord(ctx->img_event[k], render), "hipEventRecord failed");       // (band k's event: BandSchedule)
    }
    if (first_request) tl_mark("first band submitted (Huffman batch done)");
    // the last band that rows [0, y_end) touch; rows that no band touches (a gap at the top) are ordered behind the background
    // launch alone
    if (r.cover != BandSchedule::kNone) return ordered(reader, ctx->img_event[r.cover]);
    IST_HIP_OR(hipEventRecord(ctx->render_done, render), "hipEventRecord failed");
    return ordered(reader, ctx->render_done);
  };
  if (ph.on) {                                            // phase timing: the whole canvas first, then the export
    rc = need_rows(out_plan->canvas_h, ctx->stream);
    if (rc) return rc;
    ph.lap(IST_PHASE_STITCH, "compile + stitch launches", ctx->stream);
  }
  // PNG export on the device; the file's slabs cross PCIe (the only D2H of the call) while later slabs compress and -
  // not timing - while later images decode
  int64_t len = 0;
  uint8_t* host = nullptr;
  int64_t hint_rows = 0;
  for (const ist_part& p : bj.parts) hint_rows = std::max<int64_t>(hint_rows, p.Y1 - p.Y0);
  tl_mark("encoder entered");
  rc = png_to_host(ctx, set.png, d + o_canvas, canvas_pitch, out_plan->canvas_w, out_plan->canvas_h, d + o_png, &host, &len, need_rows, hint_rows, preview);
  tl_mark("encoder returned (file in host memory)");
  if (rc == IST_OK) rc = fd.finish(render);               // (images whose draw is clipped away entirely)
  (void)hipStreamSynchronize(render);                     // nothing of this call runs on when the arena is handed to the next
  tl_mark("render stream idle");
  if (rc) { if (host) pool_give(host); if (preview && preview->pixels) { pool_give(preview->pixels); preview->pixels = nullptr; preview->width = preview->height = 0; } (void)hipStreamSynchronize(ctx->stream); return rc; }
  ph.lap(IST_PHASE_PNG, "PNG encode (GPU) + D2H, overlapped", ctx->stream);
  ph.lap(IST_PHASE_D2H, "(D2H: inside the PNG phase)", nullptr);
  if (ph.print) std::fprintf(stderr, "[ist timing] %d of %d images decoded by the GPU entropy decoder\n", fd.gpu_decoded(), n);
  *out_png = host; *out_len = len;
  pg.keep = true;
  return IST_OK;
}

// the argument rules of the two entry points (`who`: the entry point, `in`: its input array, NULL when one is missing); the
// outputs are cleared.  IST_OK: go on
int check_stitch_call(const char* who, ist_ctx* ctx, const void* in, int n_images, ist_plan* out_plan, uint8_t** out_png, int64_t* out_len) {
  if (!ctx) return fail(IST_E_NO_CONTEXT, "无法获取绘图上下文");
  if (!out_plan || !out_png || !out_len) return fail(IST_E_INVALID, std::string(who) + ": NULL output");
  *out_png = nullptr; *out_len = 0;
  std::memset(out_plan, 0, sizeof(*out_plan));
  if (n_images <= 0) return IST_NOTHING_TO_DO;
  if (!in) return fail(IST_E_INVALID, std::string(who) + ": NULL input");
  if (n_images > kMaxImages) return fail(IST_E_UNSUPPORTED, "more than 128 images in one launch");
  return IST_OK;
}

// The files are READ into blocks the context keeps from call to call (grow-only up to kKeepFileBytes each), one parked
// worker per file - not mapped: the decoders parse a file twice (headers for the arena layout, then the scan) and walk it
// with plain loads, so a file that another process rewrites or truncates while it is mapped would change under them
// (a different layout on the second read) or raise SIGBUS in a worker thread and take the host process down.
// A short read - the file shrank between fstat and read - is an error of that image.
constexpr size_t kKeepFileBytes = size_t{64} << 20;
// a block that grew beyond kKeepFileBytes goes when the call that needed it ends
struct TrimFileBufs {
  ist_ctx* c;
  ~TrimFileBufs() { for (ScanBuf& b : c->file_bufs) if (b.capacity() > kKeepFileBytes) { ScanBuf none; b.swap(none); } }
};

// (the caller holds ctx->mu)  ptr[i] / lens[i]: the bytes of file i, in ctx->file_bufs[i]
int read_paths(ist_ctx* ctx, const char* const* paths, int n_images, std::vector<const uint8_t*>* ptr_out, std::vector<int64_t>* lens_out) {
  const size_t n = static_cast<size_t>(n_images);
  if (ctx->file_bufs.size() < n) ctx->file_bufs.resize(n);
  std::vector<int> fds(n, -1);
  std::vector<int64_t>& lens = *lens_out;
  std::vector<const uint8_t*>& ptr = *ptr_out;
  lens.assign(n, 0);
  ptr.assign(n, nullptr);
  std::vector<int> bad(n, 0);                             // 1: out of memory, 2: short read / read error
  struct Close { std::vector<int>& f; ~Close() { for (int d : f) if (d >= 0) (void)close(d); } } closer{fds};
  for (size_t i = 0; i < n; ++i) {
    fds[i] = paths[i] ? open(paths[i], O_RDONLY | O_CLOEXEC) : -1;
    struct stat st;
    if (fds[i] < 0 || fstat(fds[i], &st) != 0 || !S_ISREG(st.st_mode) || st.st_size <= 0)
      return fail(IST_E_DECODE, "图片" + std::to_string(i) + "解码异常: " + (fds[i] < 0 ? "cannot open the file" : "empty file, or not a regular file"));
    // (an image file of more than 1 GiB is no photo: refuse it before a block of that size is allocated for it)
    if (st.st_size > (off_t{1} << 30)) return fail(IST_E_DECODE, "图片" + std::to_string(i) + "解码异常: the file is larger than 1 GiB");
    lens[i] = static_cast<int64_t>(st.st_size);
  }
  auto read_one = [&](int k) {
    const size_t i = static_cast<size_t>(k), want = static_cast<size_t>(lens[i]);
    ScanBuf& b = ctx->file_bufs[i];
    if (!b.reserve(want + want / 8 + 64)) { bad[i] = 1; return; }
    size_t got = 0;
    while (got < want) {
      const ssize_t r = pread(fds[i], b.data() + got, want - got, static_cast<off_t>(got));
      if (r < 0 && errno == EINTR) continue;
      if (r <= 0) { bad[i] = 2; return; }
      got += static_cast<size_t>(r);
    }
    b.set_size(want);
    ptr[i] = b.data();
  };
  if (n_images == 1) read_one(0);
  else {
    WorkerPool& workers = workers_of(ctx);
    tl_mark("paths: files opened");
    workers.run(n_images, read_one);
    tl_mark("paths: read tasks handed out");
    workers.wait();
    tl_mark("paths: files read");
  }
  for (size_t i = 0; i < n; ++i) {
    if (bad[i] == 1) return fail(IST_E_NOMEM, "out of memory for the bytes of image " + std::to_string(i));
    if (bad[i]) return fail(IST_E_DECODE, "图片" + std::to_string(i) + "解码异常: the file changed while it was read");
  }
  return IST_OK;
}

}  // namespace

extern "C" {

int64_t ist_debug_direct_images(void) { return g_direct_images.load(std::memory_order_relaxed); }

int ist_stitch_files_png_preview(ist_ctx* ctx, const uint8_t* const* files, const int64_t* lens, int n_images, int direction, int mode,
                                 double gap, const ist_limits* limits, int filter, ist_plan* out_plan, uint8_t** out_png,
                                 int64_t* out_len, ist_preview* preview) {
  preview_clear(preview);
  int rc = check_stitch_call("ist_stitch_files_png", ctx, lens ? files : nullptr, n_images, out_plan, out_png, out_len);
  if (rc < 0) return rc;
  const int rcp = preview_check(preview);
  if (rcp) return rcp;
  if (rc) return rc;
  const Settings set = settings_of(ctx);      // what this call reads of the context's settings: read once
  { const int rcf = set.png.check(); if (rcf) return rcf; }      // (level 0 in RGB: refused before anything is read or enqueued)
  std::lock_guard<std::mutex> lock(ctx->mu);
  return stitch_files_png_locked(ctx, set, files, lens, n_images, direction, mode, gap, limits, filter, out_plan, out_png, out_len, preview);
}

int ist_stitch_files_png(ist_ctx* ctx, const uint8_t* const* files, const int64_t* lens, int n_images, int direction, int mode,
                         double gap, const ist_limits* limits, int filter, ist_plan* out_plan, uint8_t** out_png,
                         int64_t* out_len) {
  return ist_stitch_files_png_preview(ctx, files, lens, n_images, direction, mode, gap, limits, filter, out_plan, out_png, out_len, nullptr);
}

int ist_stitch_paths_png_preview(ist_ctx* ctx, const char* const* paths, int n_images, int direction, int mode, double gap, const ist_limits* limits,
                                 int filter, ist_plan* out_plan, uint8_t** out_png, int64_t* out_len, ist_preview* preview) {
  preview_clear(preview);
  int rc = check_stitch_call("ist_stitch_paths_png", ctx, paths, n_images, out_plan, out_png, out_len);
  if (rc < 0) return rc;
  const int rcp = preview_check(preview);
  if (rcp) return rcp;
  if (rc) return rc;
  const Settings set = settings_of(ctx);      // what this call reads of the context's settings: read once
  { const int rcf = set.png.check(); if (rcf) return rcf; }      // (level 0 in RGB: refused before anything is read or enqueued)
  tl_begin();
  struct TlEnd { ~TlEnd() { tl_end("ist_stitch_paths_png"); } } tl_end_guard;
  std::lock_guard<std::mutex> lock(ctx->mu);
  tl_mark("paths: context locked");
  TrimFileBufs trim{ctx};
  std::vector<const uint8_t*> ptr;
  std::vector<int64_t> lens;
  rc = read_paths(ctx, paths, n_images, &ptr, &lens);
  if (rc) return rc;
  return stitch_files_png_locked(ctx, set, ptr.data(), lens.data(), n_images, direction, mode, gap, limits, filter, out_plan, out_png, out_len, preview);
}

int ist_stitch_paths_png(ist_ctx* ctx, const char* const* paths, int n_images, int direction, int mode, double gap, const ist_limits* limits,
                         int filter, ist_plan* out_plan, uint8_t** out_png, int64_t* out_len) {
  return ist_stitch_paths_png_preview(ctx, paths, n_images, direction, mode, gap, limits, filter, out_plan, out_png, out_len, nullptr);
}

}  // extern "C"
