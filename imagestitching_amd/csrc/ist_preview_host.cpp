// ist_preview_host.cpp — previews of the C-ABI: the fit rule, the device entry point, and the tail every *_png_preview call shares.
// Reference anchor: steps 7-8 of Page.onStitch (pages/index/index.js:1593-1603): the exported file is loaded back into a bitmap and
// drawn into the preview node, shrunk to fit.  Here the canvas never left HBM, so the preview is one reduce of it (ist_preview.hip)
// queued behind the last render, beside the encoder.
#include <atomic>
#include <cmath>
#include <cstring>
#include <mutex>

#include "ist_ctx.h"

using namespace ist;

namespace ist {

namespace {
std::atomic<int64_t> g_preview_launches{0};
}  // namespace

// Workgroup shape of the reduce for a shape.  A group of per_group output pixels has an x footprint of at most per_group * kx + 2
// source columns (+ 1 for a rounding error at either end): one 256-column pass while that fits, otherwise one pixel per group and as
// many passes as its box needs.  A chunk is 64 rows (16 per wave); boxes taller than 64 chunks get taller chunks, so that stage 2 never
// adds more than 64 partial sums.
bool preview_geometry(int64_t w, int64_t h, int32_t pw, int32_t ph, PreviewArgs* out) {
  if (pw < 1 || ph < 1 || w <= pw || h <= ph || w > (int64_t{1} << 30) || h > (int64_t{1} << 30)) return false;
  PreviewArgs& a = *out;
  std::memset(&a, 0, sizeof(a));
  a.w = static_cast<int32_t>(w); a.h = static_cast<int32_t>(h); a.pw = pw; a.ph = ph;
  a.kx = static_cast<double>(w) / static_cast<double>(pw);
  a.ky = static_cast<double>(h) / static_cast<double>(ph);
  a.per_group = static_cast<int32_t>(std::max(1.0, std::floor(253.0 / a.kx)));
  a.groups = (pw + a.per_group - 1) / a.per_group;
  a.passes = a.per_group > 1 ? 1 : static_cast<int32_t>((static_cast<int64_t>(std::ceil(a.kx)) + 3 + 255) / 256);
  const int64_t box_cols = std::min<int64_t>(64, static_cast<int64_t>(std::ceil(a.kx)) + 1);
  a.sub = 1;
  while (a.sub < box_cols) a.sub <<= 1;
  const int64_t box_rows = static_cast<int64_t>(std::ceil(a.ky)) + 2;
  a.chunk_rows = static_cast<int32_t>(std::max<int64_t>(64, ((box_rows + 63) / 64 + 3) & ~int64_t{3}));
  a.chunks = static_cast<int32_t>((box_rows + a.chunk_rows - 1) / a.chunk_rows);
  return true;
}

int preview_check(ist_preview* pv) {
  if (!pv) return IST_OK;
  pv->width = pv->height = 0;
  pv->pixels = nullptr;
  if (!std::isfinite(pv->box_w) || !std::isfinite(pv->box_h) || !(pv->box_w > 0.0) || !(pv->box_h > 0.0))
    return fail(IST_E_INVALID, "preview: the box sides must be finite and > 0");
  return IST_OK;
}

int preview_enqueue(ist_ctx* ctx, const void* src, size_t src_pitch, int64_t w, int64_t h, bool opaque, void* dst, size_t dst_pitch,
                    int32_t pw, int32_t ph, hipStream_t stream) {
  std::lock_guard<std::mutex> lock(ctx->prev_mu);
  PreviewArgs a;
  if (preview_geometry(w, h, pw, ph, &a)) {
    const size_t need = static_cast<size_t>(ph) * static_cast<size_t>(a.chunks) * static_cast<size_t>(pw) * 16;
    // (growing frees the old block, which waits for the device: a reduce still in flight has finished with it by then)
    int rc = ctx->scratch_prev.grow(need);
    if (rc) return rc;
    rc = ctx->prev_done.ensure();
    if (rc) return rc;
    // one reduce owns the partial sums at a time: a call on another stream than the last one starts behind it
    if (ctx->prev_pending && ctx->prev_last != stream) IST_HIP_OR(hipStreamWaitEvent(stream, ctx->prev_done, 0), "ordering a preview behind the previous one failed");
    a.src = static_cast<const uint8_t*>(src); a.src_pitch = src_pitch;
    a.dst = static_cast<uint8_t*>(dst); a.dst_pitch = dst_pitch;
    a.partial = static_cast<float*>(ctx->scratch_prev.p);
    rc = launch_preview(a, opaque, stream);
    if (rc) return rc;
    IST_HIP_OR(hipEventRecord(ctx->prev_done, stream), "hipEventRecord failed");
    ctx->prev_pending = true; ctx->prev_last = stream;
    g_preview_launches.fetch_add(1, std::memory_order_relaxed);
    return IST_OK;
  }
  // an axis that does not shrink (a result smaller than its box): the existing path, one draw under IST_FILTER_AREA.  The job of the
  // last such shape is kept, so that a repeated preview compiles and allocates nothing.
  const int64_t key[5] = {w, h, pw, ph, opaque ? 1 : 0};
  if (!ctx->prev_job || std::memcmp(key, ctx->prev_job_key, sizeof(key)) != 0) {
    if (ctx->prev_job) { ist_job_destroy(ctx->prev_job); ctx->prev_job = nullptr; }
    if (w > 2147483647ll || h > 2147483647ll) return fail(IST_E_INVALID, "preview: the source is too large");
    ist_image_desc desc;
    std::memset(&desc, 0, sizeof(desc));
    desc.width = static_cast<int32_t>(w); desc.height = static_cast<int32_t>(h); desc.orientation = 1; desc.opaque = opaque ? 1 : 0;
    ist_op op;
    std::memset(&op, 0, sizeof(op));
    op.kind = IST_OP_DRAW; op.image = 0;
    op.m[0] = 1.0; op.m[3] = 1.0;
    op.s[2] = static_cast<double>(w); op.s[3] = static_cast<double>(h);
    op.d[2] = static_cast<double>(pw); op.d[3] = static_cast<double>(ph);
    ctx->prev_job = ist_job_create(ctx, pw, ph, kTransparent, &op, 1, &desc, 1, IST_FILTER_AREA, nullptr);
    if (!ctx->prev_job) return g_last_code ? g_last_code : IST_E_INVALID;
    std::memcpy(ctx->prev_job_key, key, sizeof(key));
  }
  return ist_job_launch(ctx->prev_job, &src, &src_pitch, 1, dst, dst_pitch, stream);
}

PreviewTail::~PreviewTail() {
  if (queued) (void)hipStreamSynchronize(ctx->prev_stream);
  if (host) pool_give(host);
}

int PreviewTail::prepare() {
  int rc = ist_preview_fit(w, h, pv->box_w, pv->box_h, &pw, &ph);
  if (rc) return rc;
  const size_t bytes = static_cast<size_t>(pw) * 4 * static_cast<size_t>(ph);
  rc = ctx->prev_out.grow(bytes);
  if (rc) return rc;
  rc = ctx->prev_stream.ensure();
  if (rc) return rc;
  rc = ctx->prev_ready.ensure();
  if (rc) return rc;
  host = static_cast<uint8_t*>(pool_take(bytes));
  if (!host) return fail(IST_E_NOMEM, "out of pinned host memory for the preview");
  return IST_OK;
}

int PreviewTail::queue(hipStream_t reader) {
  if (queued) return IST_OK;
  IST_HIP_OR(hipEventRecord(ctx->prev_ready, reader), "hipEventRecord failed");
  IST_HIP_OR(hipStreamWaitEvent(ctx->prev_stream, ctx->prev_ready, 0), "ordering the preview behind the render failed");
  queued = true;                                            // (from here on the destructor waits for the stream)
  // (not `opaque`: a canvas rendered from a recorded op list may hold translucent pixels; for an opaque one the bytes are the same rule)
  const int rc = preview_enqueue(ctx, canvas, pitch, w, h, false, ctx->prev_out.p, static_cast<size_t>(pw) * 4, pw, ph, ctx->prev_stream);
  if (rc) return rc;
  IST_HIP_OR(hipMemcpyAsync(host, ctx->prev_out.p, static_cast<size_t>(pw) * 4 * static_cast<size_t>(ph), hipMemcpyDeviceToHost, ctx->prev_stream), "queueing the preview's readback failed");
  return IST_OK;
}

int PreviewTail::finish() {
  if (!queued) return fail(IST_E_HIP, "preview: the export never asked for the canvas's last rows");
  IST_HIP_OR(hipStreamSynchronize(ctx->prev_stream), "preview readback failed");
  queued = false;
  pv->width = pw; pv->height = ph; pv->pixels = host;
  host = nullptr;
  return IST_OK;
}

}  // namespace ist

extern "C" {

int64_t ist_debug_preview_launches(void) { return g_preview_launches.load(std::memory_order_relaxed); }

int ist_debug_preview_geometry(int64_t w, int64_t h, int32_t pw, int32_t ph, int32_t out[6]) {
  if (!out) return fail(IST_E_INVALID, "ist_debug_preview_geometry: NULL output");
  std::memset(out, 0, 6 * sizeof(int32_t));
  PreviewArgs a;
  if (!preview_geometry(w, h, pw, ph, &a)) return 1;         // the job path
  out[0] = a.per_group; out[1] = a.groups; out[2] = a.passes; out[3] = a.sub; out[4] = a.chunk_rows; out[5] = a.chunks;
  return IST_OK;
}

int ist_preview_fit(int64_t w, int64_t h, double box_w, double box_h, int32_t* out_w, int32_t* out_h) {
  if (!out_w || !out_h) return fail(IST_E_INVALID, "ist_preview_fit: NULL output");
  *out_w = *out_h = 0;
  if (w < 1 || h < 1) return fail(IST_E_INVALID, "ist_preview_fit: empty image");
  if (!std::isfinite(box_w) || !std::isfinite(box_h) || !(box_w > 0.0) || !(box_h > 0.0)) return fail(IST_E_INVALID, "preview: the box sides must be finite and > 0");
  const double ew = static_cast<double>(w), eh = static_cast<double>(h);
  const double scale_fit = std::fmin(box_w / ew, box_h / eh);                 // index.js:1600
  const double pvw = std::floor(ew * scale_fit + 0.5), pvh = std::floor(eh * scale_fit + 0.5);   // :1601-1602 (Math.round)
  if (pvw > 2147483647.0 || pvh > 2147483647.0) return fail(IST_E_INVALID, "ist_preview_fit: the preview is too large");
  *out_w = static_cast<int32_t>(std::fmax(pvw, 1.0));                         // (the deviation: never 0)
  *out_h = static_cast<int32_t>(std::fmax(pvh, 1.0));
  return IST_OK;
}

int ist_preview_device(ist_ctx* ctx, const void* src, size_t src_pitch, int64_t w, int64_t h, int opaque, void* dst, size_t dst_pitch,
                       int32_t pw, int32_t ph, void* stream) {
  if (!ctx) return fail(IST_E_NO_CONTEXT, "无法获取绘图上下文");
  if (!src || !dst) return fail(IST_E_INVALID, "ist_preview_device: NULL buffer");
  if (w < 1 || h < 1 || w > 2147483647ll || h > 2147483647ll) return fail(IST_E_INVALID, "ist_preview_device: bad source size");
  if (pw < 1 || ph < 1) return fail(IST_E_INVALID, "ist_preview_device: the preview must be at least 1 x 1");
  if (src_pitch < static_cast<size_t>(w) * 4 || (src_pitch & 3)) return fail(IST_E_INVALID, "src_pitch too small or not a multiple of 4");
  if (dst_pitch < static_cast<size_t>(pw) * 4 || (dst_pitch & 3)) return fail(IST_E_INVALID, "dst_pitch too small or not a multiple of 4");
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(IST_E_NO_DEVICE, "hipSetDevice failed");
  return preview_enqueue(ctx, src, src_pitch, w, h, opaque != 0, dst, dst_pitch, pw, ph, static_cast<hipStream_t>(stream));
}

}  // extern "C"
