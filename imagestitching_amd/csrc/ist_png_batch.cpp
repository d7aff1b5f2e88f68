// ist_png_batch.cpp — many canvases resident in HBM -> many PNG files, one compression launch for all of them
// (ist_png_encode_batch_device).  The kernels and the per-file host layout are the single-file encoder's (ist_png_deflate.hip,
// ist_png.hip); this file checks the arguments and picks the form.
//
// Reference anchor: the export step of onStitch, wx.canvasToTempFilePath({fileType:'png', quality:1}) (utils/canvas.js:205-242,
// pages/index/index.js:1577-1579), for N independent requests.
#include <hip/hip_runtime_api.h>

#include <atomic>
#include <string>
#include <vector>

#include "ist_ctx.h"
#include "ist_internal.h"
#include "ist_launch.h"

namespace ist {

namespace { std::atomic<int64_t> g_png_batch_launches{0}; }

void count_png_batch_launch() { g_png_batch_launches.fetch_add(1, std::memory_order_relaxed); }

int png_batch_check(const PngBatchFile& f, int k) {
  const std::string who = "file " + std::to_string(k) + ": ";
  if (!f.canvas || !f.out || f.w < 1 || f.h < 1 || f.pitch < static_cast<size_t>(f.w) * 4 || (f.pitch & 3))
    return fail(IST_E_INVALID, who + "bad argument");
  if (f.w > (1ll << 29) || f.h > 2147483647ll) return fail(IST_E_OUTPUT_SIZE, who + "image too large for PNG");
  if ((reinterpret_cast<uintptr_t>(f.out) & 15) != 0) return fail(IST_E_INVALID, who + "PNG output buffer must be 16-byte aligned");
  if (f.cap < ist_png_bound(f.w, f.h)) return fail(IST_E_INVALID, who + "PNG output buffer too small (see ist_png_bound)");
  return IST_OK;
}

}  // namespace ist

using namespace ist;

extern "C" {

int64_t ist_debug_png_batch_launches(void) { return g_png_batch_launches.load(std::memory_order_relaxed); }

int ist_png_encode_batch_device(ist_ctx* ctx, const void* const* canvases, const size_t* pitch, const int64_t* w, const int64_t* h, int n,
                                void* const* out, const int64_t* out_cap, int64_t* out_len, void* stream) {
  if (n <= 0) return fail(IST_E_INVALID, "ist_png_encode_batch_device: no canvases");
  if (n > kMaxBatchJobs) return fail(IST_E_UNSUPPORTED, "more than 4096 canvases in one batch");
  if (!canvases || !pitch || !w || !h || !out || !out_cap || !out_len) return fail(IST_E_INVALID, "ist_png_encode_batch_device: NULL argument");
  if (!ctx) return fail(IST_E_NO_CONTEXT, "无法获取绘图上下文");
  // every file is checked before anything is enqueued
  std::vector<PngBatchFile> files(static_cast<size_t>(n));
  for (int k = 0; k < n; ++k) {
    PngBatchFile& f = files[static_cast<size_t>(k)];
    f.canvas = canvases[k]; f.pitch = pitch[k]; f.w = w[k]; f.h = h[k];
    f.out = static_cast<uint8_t*>(out[k]); f.cap = out_cap[k]; f.len = 0;
    const int rc = png_batch_check(f, k);
    if (rc) return rc;
  }
  const PngForm form = settings_of(ctx).png;      // the call's form: read once
  { const int rc = form.check(); if (rc) return rc; }      // (level 0 in RGB: refused before anything is enqueued)
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(IST_E_NO_DEVICE, "hipSetDevice failed");
  const int rc = form.compressed() ? png_encode_batch_deflate(ctx, form, files, stream, false) : png_encode_batch_stored(ctx, form, files, stream, false);
  if (rc) return rc;
  for (int k = 0; k < n; ++k) out_len[k] = files[static_cast<size_t>(k)].len;
  return IST_OK;
}

}  // extern "C"
