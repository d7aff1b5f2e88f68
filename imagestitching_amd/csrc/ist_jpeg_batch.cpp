// ist_jpeg_batch.cpp — many canvases resident in HBM -> many JPEG files, one launch per kernel and round for all of them
// (ist_jpeg_encode_batch_device).  The kernels and the rounds are the encoder's (ist_jpeg_encode.hip, ist_jpeg_enc_host.cpp); this file
// checks the arguments.
//
// Reference anchor: the export seam, safeCanvasToTempFilePath(canvas, prefer) -> wx.canvasToTempFilePath({fileType: prefer})
// (utils/canvas.js:205-221), for N independent requests.
#include <hip/hip_runtime_api.h>

#include <atomic>
#include <string>
#include <vector>

#include "ist_ctx.h"
#include "ist_jpeg_enc.h"

namespace ist {

namespace { std::atomic<int64_t> g_jpeg_batch_launches{0}; }

void count_jpeg_batch_launch() { g_jpeg_batch_launches.fetch_add(1, std::memory_order_relaxed); }

}  // namespace ist

using namespace ist;

extern "C" {

int64_t ist_debug_jpeg_batch_launches(void) { return g_jpeg_batch_launches.load(std::memory_order_relaxed); }

int ist_jpeg_encode_batch_device(ist_ctx* ctx, const void* const* canvases, const size_t* pitch, const int64_t* w, const int64_t* h,
                                 const int* quality, const int* subsampling, int n, void* const* out, const int64_t* out_cap, int64_t* out_len,
                                 void* stream) {
  if (n <= 0) return fail(IST_E_INVALID, "ist_jpeg_encode_batch_device: no canvases");
  if (n > kMaxBatchJobs) return fail(IST_E_UNSUPPORTED, "more than 4096 canvases in one batch");
  if (!canvases || !pitch || !w || !h || !quality || !subsampling || !out || !out_cap || !out_len)
    return fail(IST_E_INVALID, "ist_jpeg_encode_batch_device: NULL argument");
  if (!ctx) return fail(IST_E_NO_CONTEXT, "无法获取绘图上下文");
  // every file is checked before anything is enqueued
  std::vector<JpegBatchFile> files(static_cast<size_t>(n));
  for (int k = 0; k < n; ++k) {
    files[static_cast<size_t>(k)] = JpegBatchFile{canvases[k], pitch[k], w[k], h[k], quality[k], subsampling[k], static_cast<uint8_t*>(out[k]), out_cap[k], 0};
    const int rc = jpeg_batch_check(files[static_cast<size_t>(k)], "file", k);
    if (rc) return rc;
  }
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(IST_E_NO_DEVICE, "hipSetDevice failed");
  const int rc = jpeg_encode_batch(ctx, files, stream);
  if (rc) return rc;
  for (int k = 0; k < n; ++k) out_len[k] = files[static_cast<size_t>(k)].len;
  return IST_OK;
}

}  // extern "C"
