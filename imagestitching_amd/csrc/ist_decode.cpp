// ist_decode.cpp — files -> bitmaps in HBM: the image decoders' front door of the C-ABI (ist_jpeg_* / ist_image_*), the per-call
// FileDecoder the file pipeline (ist_files.cpp) pulls its bitmaps from, and ist_decode_files_device.
//
// Reference anchors (miniprogram-stitch/miniprogram/): the Image.src step (utils/canvas.js:27-121) and the per-image decode loop
// of onStitch (pages/index/index.js:1441-1520).
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "ist_decode.h"
#include "ist_webp.h"

using namespace ist;

namespace {
std::atomic<int64_t> g_gpu_entropy_files{0};
std::atomic<int64_t> g_gpu_entropy_sync_launches{0};

// ---- JPEG decode: entropy decoding on the host, reconstruction on the GPU (ist_jpeg.cpp / ist_jpeg_kernels.hip) ----------
// denom > 1: a component's sample plane holds S x S bytes per block, S = its reduced IDCT size
void jpeg_layout(const JpegImage& J, size_t* off, JpegDevLayout* L, int denom = 1) {
  std::memset(L, 0, sizeof(*L));
  for (int c = 0; c < J.ncomp; ++c) {
    const JpegComp& C = J.comp[c];
    const size_t nblk = static_cast<size_t>(C.blocks_x) * C.blocks_y;
    const size_t S = denom > 1 ? static_cast<size_t>(jpeg_scaled_idct_size(8 / denom, C.h, C.v, J.hmax, J.vmax)) : 8;
    L->coef[c] = arena_take(off, nblk * 128);
    L->q[c] = arena_take(off, 128);
    L->plane[c] = arena_take(off, nblk * S * S);
  }
}
// the `ent` arena part of a host-decoded image (components in sparse form)
void jpeg_layout_sparse(const JpegImage& J, size_t* off, JpegDevLayout* L) {
  for (int c = 0; c < J.ncomp; ++c) {
    const JpegComp& C = J.comp[c];
    if (!C.sparse) continue;
    const size_t nblk = static_cast<size_t>(C.blocks_x) * C.blocks_y;
    L->ent[c] = arena_take(off, C.ent.size() * 4 + 4); L->start[c] = arena_take(off, nblk * 4); L->cnt[c] = arena_take(off, nblk);
  }
}

// H2D of the coefficients (sparse entries are scattered into a zeroed plane on the GPU) + the reconstruction launches
// (the quantisation tables go to the kernels by value: no upload)
// what the reconstruction kernels need to know of an image whose coefficient planes are (or will be) in the arena at L
JpegDeviceJob jpeg_device_job(const JpegImage& J, uint8_t* d, const JpegDevLayout& L, uint8_t* d_out, size_t out_pitch) {
  JpegDeviceJob job;
  job.width = J.width; job.height = J.height; job.ncomp = J.ncomp; job.hmax = J.hmax; job.vmax = J.vmax; job.rgb = J.rgb;
  for (int c = 0; c < 3; ++c) { job.d_coef[c] = nullptr; job.q_host[c] = nullptr; job.d_plane[c] = nullptr; job.h[c] = job.v[c] = 1; job.blocks_x[c] = job.blocks_y[c] = 0; }
  for (int c = 0; c < J.ncomp; ++c) {
    const JpegComp& C = J.comp[c];
    job.d_coef[c] = reinterpret_cast<int16_t*>(d + L.coef[c]);
    job.q_host[c] = C.q;
    job.d_plane[c] = d + L.plane[c];
    job.h[c] = C.h; job.v[c] = C.v; job.blocks_x[c] = C.blocks_x; job.blocks_y[c] = C.blocks_y;
  }
  job.out = d_out; job.out_pitch = out_pitch;
  return job;
}

// the coefficients of an image into its dense device planes at L.coef (coef_on_device: the GPU entropy decoder already filled them)
int jpeg_upload_coefficients(const JpegImage& J, uint8_t* d, uint8_t* d_ent, const JpegDevLayout& L, hipStream_t stream, bool coef_on_device) {
  for (int c = 0; c < J.ncomp; ++c) {
    const JpegComp& C = J.comp[c];
    const size_t nblk = static_cast<size_t>(C.blocks_x) * C.blocks_y;
    int16_t* d_coef = reinterpret_cast<int16_t*>(d + L.coef[c]);
    if (coef_on_device) {
      // the GPU entropy decoder already filled the plane
    } else if (C.sparse) {
      IST_HIP(hipMemsetAsync(d_coef, 0, nblk * 128, stream));
      if (!d_ent) return fail(IST_E_INVALID, "JPEG sparse coefficients without a device arena");
      if (!C.ent.empty()) IST_HIP(hipMemcpyAsync(d_ent + L.ent[c], C.ent.data(), C.ent.size() * 4, hipMemcpyHostToDevice, stream));
      IST_HIP(hipMemcpyAsync(d_ent + L.start[c], C.start.data(), nblk * 4, hipMemcpyHostToDevice, stream));
      IST_HIP(hipMemcpyAsync(d_ent + L.cnt[c], C.cnt.data(), nblk, hipMemcpyHostToDevice, stream));
      const int rc = jpeg_launch_scatter(reinterpret_cast<const uint32_t*>(d_ent + L.ent[c]), reinterpret_cast<const uint32_t*>(d_ent + L.start[c]), d_ent + L.cnt[c], d_coef, static_cast<int>(nblk), stream);
      if (rc) return rc;
    } else {
      if (C.coef.size() != nblk * 64) return fail(IST_E_DECODE, "JPEG component without coefficients");
      IST_HIP(hipMemcpyAsync(d_coef, C.coef.data(), nblk * 128, hipMemcpyHostToDevice, stream));
    }
  }
  return IST_OK;
}

int jpeg_enqueue(const JpegImage& J, uint8_t* d, uint8_t* d_ent, const JpegDevLayout& L, uint8_t* d_out, size_t out_pitch, hipStream_t stream, bool coef_on_device = false,
                 bool chroma_done = false, int denom = 1) {
  JpegDeviceJob job = jpeg_device_job(J, d, L, d_out, out_pitch);
  job.chroma_done = chroma_done; job.denom = denom;
  const int rc = jpeg_upload_coefficients(J, d, d_ent, L, stream, coef_on_device);
  if (rc) return rc;
  return denom > 1 ? jpeg_launch_reconstruct_scaled(job, stream) : jpeg_launch_reconstruct(job, stream);      // (1 / 1: the full-size launches and nothing else)
}

bool valid_denom(int d) { return d == 1 || d == 2 || d == 4 || d == 8; }

// one JPEG file -> RGBA8 in host memory at 1 / denom
int jpeg_decode_rgba8(const char* who, ist_ctx* ctx, const uint8_t* file, int64_t len, int denom, uint8_t* out, size_t out_pitch, int64_t out_rows) {
  if (!ctx) return fail(IST_E_NO_CONTEXT, "无法获取绘图上下文");
  JpegImage J;
  int rc = jpeg_parse_and_entropy_decode(file, len, &J, false);
  if (rc) return rc;
  int sw = J.width, sh = J.height;
  jpeg_scaled_size(J.width, J.height, denom, &sw, &sh);
  if (!out || out_pitch < static_cast<size_t>(sw) * 4 || out_rows < sh) return fail(IST_E_INVALID, std::string(who) + ": output buffer too small");
  const bool to_srgb = settings_of(ctx).color_profile == IST_COLOR_PROFILE_SRGB;      // the call's setting: read once
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceGuard g(ctx->device);
  // one device allocation: coefficients + tables + sample planes + RGBA
  size_t off = 0;
  JpegDevLayout L;
  jpeg_layout(J, &off, &L, denom);
  jpeg_layout_sparse(J, &off, &L);                      // (one arena holds both parts here)
  const size_t row = static_cast<size_t>(sw) * 4;
  const size_t o_out = arena_take(&off, row * sh);
  uint8_t* d = nullptr;
  rc = ctx->scratch_arena.grow(off);
  if (rc) return rc;
  d = static_cast<uint8_t*>(ctx->scratch_arena.p);
  rc = jpeg_enqueue(J, d, d, L, d + o_out, row, ctx->stream, false, false, denom);
  if (rc) return rc;
  if (to_srgb) {
    ist_color_tables t;
    if (image_color_tables(file, len, &t) == IST_COLOR_CONVERT) { rc = launch_color_convert(d + o_out, row, sw, sh, t, ctx->stream); if (rc) return rc; }
  }
  std::vector<RowsCopy> down{RowsCopy{d + o_out, nullptr, out, out_pitch, row, static_cast<size_t>(sh)}};
  rc = stager_of(ctx).download(down, ctx->stream);
  (void)hipStreamSynchronize(ctx->stream);              // nothing of this call may still read the arena when the next call reuses it
  return rc;
}

bool is_jpeg(const uint8_t* f, int64_t n) { return f && n >= 2 && f[0] == 0xFF && f[1] == 0xD8; }
bool is_misc(const uint8_t* f, int64_t n) { return f && n >= 4 && ((f[0] == 'B' && f[1] == 'M') || !std::memcmp(f, "GIF8", 4)); }
}  // namespace

extern "C" {

int ist_jpeg_info(const uint8_t* file, int64_t len, int32_t* width, int32_t* height, int32_t* orientation) {
  JpegImage J;
  const int rc = jpeg_parse_and_entropy_decode(file, len, &J, true);
  if (rc) return rc;
  if (width) *width = J.width;
  if (height) *height = J.height;
  if (orientation) *orientation = J.orientation;
  return IST_OK;
}

int ist_jpeg_decode_rgba8(ist_ctx* ctx, const uint8_t* file, int64_t len, uint8_t* out, size_t out_pitch, int64_t out_rows) {
  return jpeg_decode_rgba8("ist_jpeg_decode_rgba8", ctx, file, len, 1, out, out_pitch, out_rows);
}

// format-agnostic front door: PNG (host decode) or JPEG (host entropy decode + GPU reconstruction)
int ist_misc_info(const uint8_t* file, int64_t len, int32_t* w, int32_t* h);
int ist_misc_decode_rgba8(const uint8_t* file, int64_t len, uint8_t* out, size_t pitch, int64_t out_rows);

int ist_image_info(const uint8_t* file, int64_t len, int32_t* width, int32_t* height, int32_t* orientation) {
  if (is_jpeg(file, len)) return ist_jpeg_info(file, len, width, height, orientation);
  if (is_webp(file, len)) return webp_info(file, len, width, height, orientation);      // EXIF chunk of the container
  if (orientation) *orientation = 0;
  if (is_misc(file, len)) return ist_misc_info(file, len, width, height);
  return ist_png_info(file, len, width, height);
}

int ist_image_decode_rgba8(ist_ctx* ctx, const uint8_t* file, int64_t len, uint8_t* out, size_t out_pitch, int64_t out_rows) {
  if (is_jpeg(file, len)) return ist_jpeg_decode_rgba8(ctx, file, len, out, out_pitch, out_rows);
  if (is_misc(file, len)) return ist_misc_decode_rgba8(file, len, out, out_pitch, out_rows);
  if (is_webp(file, len)) return webp_decode_rgba8(file, len, out, out_pitch, out_rows);
  return ist_png_decode_rgba8(file, len, out, out_pitch, out_rows);
}

int ist_image_decode_rgba8_scaled(ist_ctx* ctx, const uint8_t* file, int64_t len, int32_t denom, uint8_t* out, size_t out_pitch, int64_t out_rows) {
  if (!valid_denom(denom)) return fail(IST_E_INVALID, "ist_image_decode_rgba8_scaled: the file's denominator " + std::to_string(denom) + " is not 1, 2, 4 or 8");
  if (is_jpeg(file, len)) return jpeg_decode_rgba8("ist_image_decode_rgba8_scaled", ctx, file, len, denom, out, out_pitch, out_rows);
  return ist_image_decode_rgba8(ctx, file, len, out, out_pitch, out_rows);      // other file types decode at 1 / 1
}

int ist_jpeg_scaled_size(int32_t w, int32_t h, int32_t denom, int32_t* sw, int32_t* sh) {
  if (w < 1 || h < 1 || !valid_denom(denom) || !sw || !sh) return fail(IST_E_INVALID, "ist_jpeg_scaled_size: bad argument");
  int a = 0, b = 0;
  jpeg_scaled_size(w, h, denom, &a, &b);
  *sw = a; *sh = b;
  return IST_OK;
}

int ist_decode_scale_fit(int32_t w, int32_t h, int32_t min_w, int32_t min_h) {
  if (w < 1 || h < 1 || min_w < 1 || min_h < 1) return fail(IST_E_INVALID, "ist_decode_scale_fit: bad argument");
  for (int d = 8; d > 1; d /= 2)
    if ((static_cast<int64_t>(w) + d - 1) / d >= min_w && (static_cast<int64_t>(h) + d - 1) / d >= min_h) return d;
  return 1;
}

}  // extern "C"

// ---- files -> bitmaps in HBM: the decode stage shared by ist_stitch_files_png and ist_decode_files_device ------------
// (index.js:1441-1520 decodes image after image; :1559-1571 flushes and releases each one.)  Every image has a host thread:
// container parse + de-stuffing, and - baseline JPEG - the upload of its scan on a stream of its own, so that the uploads
// run while other images are still being parsed.  The Huffman passes of ALL eligible images then run as ONE batch on the
// consumer's stream: the decoder is latency-bound per workgroup (a 12 MP photo is 58 workgroups), so nine images in one
// launch take as long as one, whereas one chain per image on nine streams took 2x longer than the batch (measured: the
// runtime multiplexes streams onto four hardware queues, three chains per queue ran back to back).  Behind the batch the
// images are reconstructed one by one as the consumer asks for them, so (ist_stitch_files_png) band k of the canvas is
// rendered and exported while the images behind it are still being reconstructed.  Files the GPU entropy decoder does not
// take (progressive, non-interleaved scans, more than 2048 restart intervals, PNG / BMP / GIF / WebP) are decoded on their thread and uploaded when the consumer
// asks for the image.  With phase timing on, the same steps run with a stream sync between them.
namespace ist {

Phases::Phases(ist_ctx* c, bool timing) : ctx(c), record(timing) {
  static const bool env = std::getenv("IST_TIMING") != nullptr;
  print = env; on = env || record;
  if (record) for (double& v : c->last_ms) v = 0.0;
  t_prev = std::chrono::steady_clock::now();
}
void Phases::lap(int phase, const char* what, hipStream_t st) {
  if (!on) return;
  if (st) (void)hipStreamSynchronize(st);
  const auto t = std::chrono::steady_clock::now();
  const double ms = std::chrono::duration<double, std::milli>(t - t_prev).count();
  if (print) std::fprintf(stderr, "[ist timing] %-28s %8.2f ms\n", what, ms);
  if (record && phase >= 0 && phase < IST_PHASE_COUNT) ctx->last_ms[phase] += ms;
  t_prev = t;
}

constexpr int kImgStreams = 8;           // image i runs on stream i mod kImgStreams

static int ensure_image_lanes(ist_ctx* ctx, int n) {
  const size_t want = static_cast<size_t>(std::min(n, kImgStreams));
  while (ctx->img_stream.size() < want) {
    Stream st;
    const int rc = st.ensure();
    if (rc) return rc;
    ctx->img_stream.push_back(std::move(st));
  }
  while (ctx->img_event.size() < static_cast<size_t>(n)) {
    Event ev;
    const int rc = ev.ensure();
    if (rc) return rc;
    ctx->img_event.push_back(std::move(ev));
  }
  if (ctx->img_huff.size() < static_cast<size_t>(n)) ctx->img_huff.resize(static_cast<size_t>(n));
  if (ctx->scan_bufs.size() < static_cast<size_t>(n)) ctx->scan_bufs.resize(static_cast<size_t>(n));
  return IST_OK;
}

FileDecoder::FileDecoder(ist_ctx* ctx, const uint8_t* const* files, const int64_t* lens, int n, Phases* ph, int color_profile, const int32_t* denom)
    : ctx_(ctx), files_(files), lens_(lens), n_(n), ph_(ph), to_srgb_(color_profile == IST_COLOR_PROFILE_SRGB), denom_(denom), dec_(static_cast<size_t>(n)),
      on_gpu_(static_cast<size_t>(n), 0), taken_(static_cast<size_t>(n), 0), uploaded_(static_cast<size_t>(n), 0), started_(static_cast<size_t>(n), 0),
      chroma_done_(static_cast<size_t>(n), 0), jo_(static_cast<size_t>(n)) {}
FileDecoder::~FileDecoder() {
  join_all();
  for (int i = 0; i < n_; ++i) if (started_[static_cast<size_t>(i)]) (void)hipStreamSynchronize(stream_of(i));
  for (int i = 0; i < n_ && static_cast<size_t>(i) < ctx_->scan_bufs.size(); ++i) {      // keep the scans' memory for the next call (at most 8 MiB per image)
    ScanBuf& mine = dec_[static_cast<size_t>(i)].G.stream;
    if (mine.capacity() > ctx_->scan_bufs[static_cast<size_t>(i)].capacity() && mine.capacity() <= (8u << 20)) ctx_->scan_bufs[static_cast<size_t>(i)].swap(mine);
  }
}

int FileDecoder::headers() {
  static const bool gpu_huffman = std::getenv("IST_JPEG_HOST_HUFFMAN") == nullptr;
  gpu_huffman_ = gpu_huffman;
  for (int i = 0; i < n_; ++i) {
    Dec& D = dec_[static_cast<size_t>(i)];
    const uint8_t* f = files_[i]; const int64_t len = lens_[i];
    D.jpeg = is_jpeg(f, len);
    int rc;
    if (D.jpeg) {
      rc = jpeg_parse_and_entropy_decode(f, len, &D.J, true);
      D.w = D.J.width; D.h = D.J.height; D.orient = D.J.orientation;
    } else {
      int32_t w = 0, h = 0, o = 0;
      rc = ist_image_info(f, len, &w, &h, &o);
      D.w = w; D.h = h; D.orient = o;                    // WebP carries EXIF in its container
    }
    if (rc != IST_OK) return fail(rc, "图片" + std::to_string(i) + "解码异常: " + g_last_error);   // index.js:1512-1514
  }
  return IST_OK;
}
std::vector<ist_image_desc> FileDecoder::descs(const int64_t* lens) const {
  std::vector<ist_image_desc> descs(static_cast<size_t>(n_));
  for (int i = 0; i < n_; ++i) {
    const Dec& D = dec(i);
    ist_image_desc& d = descs[static_cast<size_t>(i)];
    std::memset(&d, 0, sizeof d);
    d.width = D.w; d.height = D.h; d.orientation = D.orient ? D.orient : 1; d.opaque = D.jpeg ? 1 : 0; d.file_size = lens[i];
    if (denom_of(i) > 1) { int sw = 0, sh = 0; jpeg_scaled_size(D.w, D.h, denom_of(i), &sw, &sh); d.bmp_width = sw; d.bmp_height = sh; }
  }
  return descs;
}
void FileDecoder::layout(size_t* off) { for (int i = 0; i < n_; ++i) if (dec_[static_cast<size_t>(i)].jpeg) jpeg_layout(dec_[static_cast<size_t>(i)].J, off, &jo_[static_cast<size_t>(i)], denom_of(i)); }
int FileDecoder::denom_of(int i) const { return denom_ && dec_[static_cast<size_t>(i)].jpeg ? denom_[i] : 1; }      // (other file types decode at 1 / 1)

int FileDecoder::start(uint8_t* arena, uint8_t* const* img, const size_t* pitch) {
  arena_ = arena; img_ = img; pitch_ = pitch;
  const int rc = ensure_image_lanes(ctx_, n_);
  if (rc) return rc;
  workers_of(ctx_).run(n_, [this](int i) { worker(i); });
  running_ = true;
  if (!ph_->on) return IST_OK;
  // phase timing: the steps one after the other
  join_all();
  int rc2 = first_error(); if (rc2) return rc2;
  for (int i = 0; i < n_; ++i) if (uploaded_[static_cast<size_t>(i)]) (void)hipStreamSynchronize(stream_of(i));
  ph_->lap(IST_PHASE_HOST_DECODE, "decode on host threads (+ scan uploads)", nullptr);
  rc2 = huffman_all(ctx_->stream); if (rc2) return rc2;
  ph_->lap(IST_PHASE_ENTROPY_GPU, "entropy decode (GPU)", ctx_->stream);
  if (coef_only_) return IST_OK;                  // (no bitmap is made: coefficients() does the rest)
  for (int i = 0; i < n_; ++i) { rc2 = take(i, ctx_->stream); if (rc2) return rc2; }
  ph_->lap(IST_PHASE_RECONSTRUCT, "H2D + JPEG reconstruct (GPU)", ctx_->stream);
  return IST_OK;
}

int FileDecoder::take(int i, hipStream_t consumer) {
  const size_t k = static_cast<size_t>(i);
  if (taken_[k]) return IST_OK;
  int rc = huffman_all(consumer);
  if (rc) return rc;
  rc = chroma_all(consumer);
  if (rc) return rc;
  taken_[k] = 1;
  rc = place(i, consumer);
  if (rc) return rc;
  // the one place where bitmap i lands: a file tagged with a profile the contract takes is converted to sRGB behind it, in place
  const Dec& D = dec_[k];
  if (!to_srgb_ || D.color.kind != IST_COLOR_CONVERT) return IST_OK;
  int bw = D.w, bh = D.h;
  if (denom_of(i) > 1) jpeg_scaled_size(D.w, D.h, denom_of(i), &bw, &bh);
  return launch_color_convert(img_[i], pitch_[i], bw, bh, D.color, consumer);
}

int FileDecoder::place(int i, hipStream_t consumer) {
  const size_t k = static_cast<size_t>(i);
  int rc = IST_OK;
  Dec& D = dec_[k];
  if (on_gpu_[k]) return jpeg_enqueue(D.J, arena_, nullptr, jo_[k], img_[i], pitch_[i], consumer, true, chroma_done_[k] != 0, denom_of(i));
  const size_t row = static_cast<size_t>(D.w) * 4;
  if (!D.jpeg) {                                  // PNG / BMP / GIF / WebP: decoded on the thread, uploaded here
    std::vector<RowsCopy> up;
    if (pitch_[i] != row) for (int y = 0; y < D.h; ++y) up.push_back(RowsCopy{img_[i] + static_cast<size_t>(y) * pitch_[i], D.px.data() + static_cast<size_t>(y) * row, nullptr, row, row, 1});
    else up.push_back(RowsCopy{img_[i], D.px.data(), nullptr, row, row, static_cast<size_t>(D.h)});
    return stager_of(ctx_).upload(up, consumer);
  }
  JpegDevLayout L;
  rc = host_coefficients(i, consumer, &L);
  if (rc) return rc;
  return jpeg_enqueue(D.J, arena_, static_cast<uint8_t*>(ctx_->scratch_ent.p), L, img_[i], pitch_[i], consumer, false, false, denom_of(i));
}

// A JPEG whose coefficients are on the host (progressive, non-interleaved scans, thousands of restart intervals, or a file that
// failed the GPU decoder's validation and is decoded again by the host decoder here): *L = its layout with the sparse part in the
// context's entry block, which is grown for it
int FileDecoder::host_coefficients(int i, hipStream_t consumer, JpegDevLayout* out) {
  const size_t k = static_cast<size_t>(i);
  int rc = IST_OK;
  Dec& D = dec_[k];
  if (D.G.eligible) {
    D.G.eligible = false;
    JpegImage host;
    rc = jpeg_parse_and_entropy_decode(files_[i], lens_[i], &host, false, nullptr);
    if (rc) return fail(rc, "图片" + std::to_string(i) + "解码异常: " + g_last_error);
    D.J = std::move(host);
  }
  size_t need = 0;
  JpegDevLayout L = jo_[k];
  jpeg_layout_sparse(D.J, &need, &L);
  if (need) {                                      // one block serves the host-decoded images in turn
    (void)hipStreamSynchronize(consumer);
    rc = ctx_->scratch_ent.grow(need, need / 2);
    if (rc) return rc;
  }
  *out = L;
  return IST_OK;
}

void FileDecoder::layout_coefficients(size_t* off) {
  coef_only_ = true;
  for (int i = 0; i < n_; ++i) {
    const Dec& D = dec_[static_cast<size_t>(i)];
    if (!D.jpeg) continue;
    JpegDevLayout& L = jo_[static_cast<size_t>(i)];
    std::memset(&L, 0, sizeof L);
    for (int c = 0; c < D.J.ncomp; ++c) L.coef[c] = arena_take(off, static_cast<size_t>(D.J.comp[c].blocks_x) * D.J.comp[c].blocks_y * 128);
  }
}

int FileDecoder::coefficients(hipStream_t consumer, std::vector<JpegCoefPlanes>* out) {
  int rc = huffman_all(consumer);
  if (rc) return rc;
  out->assign(static_cast<size_t>(n_), JpegCoefPlanes{});
  for (int i = 0; i < n_; ++i) {
    const size_t k = static_cast<size_t>(i);
    if (!dec_[k].jpeg) return fail(IST_E_INVALID, "image " + std::to_string(i) + " is not a JPEG: it has no coefficients");
    if (!on_gpu_[k] && !taken_[k]) {
      JpegDevLayout L;
      rc = host_coefficients(i, consumer, &L);
      if (rc) return rc;
      rc = jpeg_upload_coefficients(dec_[k].J, arena_, static_cast<uint8_t*>(ctx_->scratch_ent.p), L, consumer, false);
      if (rc) return rc;
    }
    taken_[k] = 1;
    const JpegImage& J = dec_[k].J;
    JpegCoefPlanes& P = (*out)[k];
    for (int c = 0; c < J.ncomp; ++c) {
      P.coef[c] = reinterpret_cast<const int16_t*>(arena_ + jo_[k].coef[c]);
      P.blocks_x[c] = J.comp[c].blocks_x; P.blocks_y[c] = J.comp[c].blocks_y;
    }
  }
  return IST_OK;
}

int FileDecoder::finish(hipStream_t consumer) {
  for (int i = 0; i < n_; ++i) { const int rc = take(i, consumer); if (rc) { join_all(); return rc; } }
  return IST_OK;
}
int FileDecoder::gpu_decoded() const { int g = 0; for (char v : on_gpu_) g += v ? 1 : 0; return g; }

hipStream_t FileDecoder::stream_of(int i) const { return ctx_->img_stream[static_cast<size_t>(i % kImgStreams) % ctx_->img_stream.size()]; }
void FileDecoder::join_all() { if (running_) { ctx_->workers->wait(); running_ = false; } }
int FileDecoder::first_error() {
  for (int i = 0; i < n_; ++i) if (dec_[static_cast<size_t>(i)].rc != IST_OK) return fail(dec_[static_cast<size_t>(i)].rc, "图片" + std::to_string(i) + "解码异常: " + dec_[static_cast<size_t>(i)].err);
  return IST_OK;
}
// every worker has returned; ONE Huffman batch over the eligible images on `consumer`, behind their scan uploads
int FileDecoder::huffman_all(hipStream_t consumer) {
  if (huff_done_) return IST_OK;
  tl_mark("decoder: waiting for the per-image host work");
  join_all();
  tl_mark("decoder: host work of every image done");
  int rc = first_error();
  if (rc) return rc;
  huff_done_ = true;
  std::vector<JpegGpuItem> items; std::vector<int> who;
  for (int i = 0; i < n_; ++i) {
    const size_t k = static_cast<size_t>(i);
    Dec& D = dec_[k];
    if (!D.jpeg || !D.G.eligible) continue;
    JpegGpuItem it; it.J = &D.J; it.S = &D.G;
    for (int c = 0; c < 3; ++c) it.d_coef[c] = c < D.J.ncomp ? reinterpret_cast<int16_t*>(arena_ + jo_[k].coef[c]) : nullptr;
    if (uploaded_[k]) {
      it.d_stream = static_cast<const uint8_t*>(ctx_->img_huff[k].p);
      IST_HIP_OR(hipStreamWaitEvent(consumer, ctx_->img_event[k], 0), "hipStreamWaitEvent failed");
    }
    items.push_back(it); who.push_back(i);
  }
  std::vector<uint8_t> okv;
  int launches = 0;
  rc = jpeg_gpu_entropy_decode(items, &okv, consumer, &ctx_->scratch_huff, &launches);
  g_gpu_entropy_sync_launches.fetch_add(launches, std::memory_order_relaxed);
  if (rc) return rc;
  for (size_t q = 0; q < who.size(); ++q) {
    on_gpu_[static_cast<size_t>(who[q])] = okv[q] ? 1 : 0;
    if (okv[q]) g_gpu_entropy_files.fetch_add(1, std::memory_order_relaxed);
  }
  return IST_OK;
}
// the chroma planes of every image the GPU decoded, in ONE launch behind the batch (the first take() runs it: part of the
// reconstruction phase): each image then costs one fused launch
int FileDecoder::chroma_all(hipStream_t consumer) {
  if (chroma_batch_done_) return IST_OK;
  chroma_batch_done_ = true;
  std::vector<JpegDeviceJob> chroma;
  for (int i = 0; i < n_; ++i) {
    const size_t k = static_cast<size_t>(i);
    if (!on_gpu_[k] || dec_[k].J.ncomp != 3 || denom_of(i) > 1) continue;      // (a reduced image makes its own planes, sized by its IDCTs)
    chroma.push_back(jpeg_device_job(dec_[k].J, arena_, jo_[k], nullptr, 0));
    chroma_done_[k] = 1;
  }
  if (!chroma.empty()) return jpeg_launch_chroma_idct(chroma.data(), static_cast<int>(chroma.size()), consumer);
  return IST_OK;
}
// container + host entropy stage of image i; a baseline JPEG's de-stuffed scan goes up on the image's own stream
void FileDecoder::worker(int i) {
  const size_t k = static_cast<size_t>(i);
  Dec& D = dec_[k];
  DeviceGuard dg(ctx_->device);
  const uint8_t* f = files_[i]; const int64_t len = lens_[i];
  auto failed = [&](int rc) { D.rc = rc; D.err = g_last_error; };     // (thread-local message: carry it out)
  if (to_srgb_) image_color_tables(f, len, &D.color);      // (a bad profile never fails a decode)
  if (!D.jpeg) {
    D.px.resize(static_cast<size_t>(D.w) * D.h * 4);
    const int rc = ist_image_decode_rgba8(nullptr, f, len, D.px.data(), static_cast<size_t>(D.w) * 4, D.h);
    if (rc) failed(rc);
    return;
  }
  JpegImage full;
  // The scan is de-stuffed (SSE2, 16 bytes a step) into a heap block the context keeps from call to call and goes to the
  // device in ONE copy.  (measured, 120 calls each, twice: from a page-locked block of the context instead - a true DMA, no
  // bounce buffer - the call's median was the same, 2.35 vs 2.34-2.37 ms, so the simpler path stayed; in 256 KB pieces sent
  // while the rest was still being de-stuffed, half of the calls took 8 ms.)
  if (k < ctx_->scan_bufs.size()) D.G.stream.swap(ctx_->scan_bufs[k]);            // (a recycled block: capacity, no contents)
  // (IST_TUNING=1 IST_JPEG_SECOND_READ_444=1, tests only: the second read sees the luma sampling factors as 1x1 - what a
  // caller's buffer rewritten between the two parses would look like)
  static const bool flip = tuning_mode() && std::getenv("IST_JPEG_SECOND_READ_444") != nullptr;
  std::vector<uint8_t> flipped;
  if (flip) {
    flipped.assign(f, f + len);
    for (int64_t q = 2; q + 12 < len; ++q) if (flipped[static_cast<size_t>(q)] == 0xFF && flipped[static_cast<size_t>(q) + 1] == 0xC0) { flipped[static_cast<size_t>(q) + 11] = 0x11; break; }
    f = flipped.data();
  }
  const int rc = jpeg_parse_and_entropy_decode(f, len, &full, false, gpu_huffman_ ? &D.G : nullptr);
  if (rc) { failed(rc); return; }
  // The arena (coefficient + sample planes, layout()) was sized from the header-only parse: every input of that layout must
  // be the same on this second read, or the Huffman write kernel, the IDCT and the scatter would run past their planes
  // (4:2:0 turning 4:4:4 doubles blocks_x * blocks_y).  The bytes may be a caller's buffer another thread is still writing.
  bool same = full.width == D.w && full.height == D.h && full.ncomp == D.J.ncomp && full.hmax == D.J.hmax && full.vmax == D.J.vmax &&
              full.mcus_x == D.J.mcus_x && full.mcus_y == D.J.mcus_y;
  for (int c = 0; same && c < full.ncomp; ++c)
    same = full.comp[c].h == D.J.comp[c].h && full.comp[c].v == D.J.comp[c].v && full.comp[c].blocks_x == D.J.comp[c].blocks_x &&
           full.comp[c].blocks_y == D.J.comp[c].blocks_y;
  if (!same) { g_last_error = "JPEG frame header changed between two reads"; failed(IST_E_DECODE); return; }
  D.J = std::move(full);
  if (!D.G.eligible) return;
  const size_t bytes = D.G.stream.size();
  if (ctx_->img_huff[k].grow(bytes, bytes / 4)) return;
  hipStream_t st = stream_of(i);
  started_[k] = 1;
  if (hipMemcpyAsync(ctx_->img_huff[k].p, D.G.stream.data(), bytes, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipEventRecord(ctx_->img_event[k], st) != hipSuccess) { (void)hipGetLastError(); return; }
  uploaded_[k] = 1;
}

int check_denoms(const char* who, const int32_t* denom, int n) {
  for (int i = 0; denom && i < n; ++i)
    if (!valid_denom(denom[i])) return fail(IST_E_INVALID, std::string(who) + ": the denominator of image " + std::to_string(i) + " is " + std::to_string(denom[i]) + ", not 1, 2, 4 or 8");
  return IST_OK;
}

int decode_files_locked(ist_ctx* ctx, const uint8_t* const* files, const int64_t* lens, int n, const int32_t* denom,
                        const std::function<int(const std::vector<ist_image_desc>&, uint8_t**, size_t*)>& place) {
  DeviceGuard g(ctx->device);
  const Settings set = settings_of(ctx);      // what this call reads of the context's settings: read once
  Phases ph(ctx, set.timing);
  FileDecoder fd(ctx, files, lens, n, &ph, set.color_profile, denom);
  int rc = fd.headers();
  if (rc) return rc;
  const std::vector<ist_image_desc> descs = fd.descs(lens);
  std::vector<uint8_t*> img(static_cast<size_t>(n), nullptr);
  std::vector<size_t> pitch(static_cast<size_t>(n), 0);
  rc = place(descs, img.data(), pitch.data());
  if (rc) return rc;
  size_t off = 0;
  fd.layout(&off);
  rc = ctx->scratch_dec.grow(off ? off : 256);
  if (rc) return rc;
  ph.lap(IST_PHASE_PLAN_ARENA, "device arena", nullptr);
  rc = fd.start(static_cast<uint8_t*>(ctx->scratch_dec.p), img.data(), pitch.data());
  if (rc == IST_OK) rc = fd.finish(ctx->stream);
  // the bitmaps are complete (or, on a failure, nothing of this call writes them any more); the host coefficients in flight may go
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) { (void)hipGetLastError(); if (rc == IST_OK) rc = fail(IST_E_HIP, "hipStreamSynchronize failed"); }
  return rc;
}

}  // namespace ist

extern "C" {

int64_t ist_debug_gpu_entropy_files(void) { return g_gpu_entropy_files.load(std::memory_order_relaxed); }
int64_t ist_debug_gpu_entropy_sync_launches(void) { return g_gpu_entropy_sync_launches.load(std::memory_order_relaxed); }

// The GPU entropy decoder's coefficients of ONE file, read back: the same parse, the same jpeg_gpu_entropy_decode and the same dense
// planes the file pipeline hands to the reconstruction kernels - minus the reconstruction.  A file the decoder hands back (ok = 0)
// leaves the caller's planes untouched.
int ist_debug_jpeg_gpu_coefficients(ist_ctx* ctx, const uint8_t* file, int64_t len, int16_t* const* planes, const int64_t* plane_elems,
                                    ist_jpeg_coef_info* info) {
  if (!file || len <= 0 || !info || (planes && !plane_elems)) return fail(IST_E_INVALID, "ist_debug_jpeg_gpu_coefficients: bad argument");
  std::memset(info, 0, sizeof *info);
  JpegImage J;
  JpegGpuScan G;
  int rc = jpeg_parse_and_entropy_decode(file, len, &J, false, &G);
  if (rc) return rc;
  if (!G.eligible) return fail(IST_E_UNSUPPORTED, "ist_debug_jpeg_gpu_coefficients: not a file the GPU entropy decoder takes");
  info->ncomp = J.ncomp;
  for (int c = 0; c < J.ncomp; ++c) { info->blocks_x[c] = J.comp[c].blocks_x; info->blocks_y[c] = J.comp[c].blocks_y; }
  if (!planes) return IST_OK;                           // the geometry only: what the caller sizes its planes from
  size_t off = 0, o_coef[3] = {0, 0, 0}, nblk[3] = {0, 0, 0};
  for (int c = 0; c < J.ncomp; ++c) {
    nblk[c] = static_cast<size_t>(J.comp[c].blocks_x) * J.comp[c].blocks_y;
    if (!planes[c] || plane_elems[c] < 0 || static_cast<uint64_t>(plane_elems[c]) < nblk[c] * 64) return fail(IST_E_INVALID, "ist_debug_jpeg_gpu_coefficients: plane " + std::to_string(c) + " is too small");
    o_coef[c] = arena_take(&off, nblk[c] * 128);
  }
  if (!ctx) return fail(IST_E_NO_CONTEXT, "无法获取绘图上下文");
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceGuard g(ctx->device);
  rc = ctx->scratch_arena.grow(off);
  if (rc) return rc;
  uint8_t* d = static_cast<uint8_t*>(ctx->scratch_arena.p);
  JpegGpuItem it; it.J = &J; it.S = &G;
  for (int c = 0; c < 3; ++c) it.d_coef[c] = c < J.ncomp ? reinterpret_cast<int16_t*>(d + o_coef[c]) : nullptr;
  std::vector<JpegGpuItem> items(1, it);
  std::vector<uint8_t> okv;
  int launches = 0;
  rc = jpeg_gpu_entropy_decode(items, &okv, ctx->stream, &ctx->scratch_huff, &launches);
  g_gpu_entropy_sync_launches.fetch_add(launches, std::memory_order_relaxed);
  if (rc) return rc;
  info->launches = launches;
  info->ok = !okv.empty() && okv[0] ? 1 : 0;
  if (info->ok)
    for (int c = 0; c < J.ncomp; ++c) IST_HIP(hipMemcpyAsync(planes[c], d + o_coef[c], nblk[c] * 128, hipMemcpyDeviceToHost, ctx->stream));
  IST_HIP(hipStreamSynchronize(ctx->stream));           // nothing of this call may still read the arena when the next call reuses it
  return IST_OK;
}

int ist_ctx_set_color_profile(ist_ctx* ctx, int profile) {
  if (!ctx) return fail(IST_E_NO_CONTEXT, "无法获取绘图上下文");
  return settings_set(&ctx->settings, kColorProfile, profile);
}

int ist_color_convert_device(ist_ctx* ctx, void* ptr, size_t pitch, int64_t w, int64_t h, const ist_color_tables* tables, void* stream) {
  if (!ctx) return fail(IST_E_NO_CONTEXT, "无法获取绘图上下文");
  if (!ptr || !tables || w < 1 || h < 1) return fail(IST_E_INVALID, "ist_color_convert_device: bad argument");
  if (pitch / 4 < static_cast<uint64_t>(w) || (pitch & 3) || (reinterpret_cast<uintptr_t>(ptr) & 3)) return fail(IST_E_INVALID, "ist_color_convert_device: a short or unaligned pitch, or an unaligned pointer");
  if (tables->kind == IST_COLOR_IDENTITY) return IST_OK;
  if (tables->kind != IST_COLOR_CONVERT) return fail(IST_E_INVALID, "ist_color_convert_device: the tables are neither IST_COLOR_CONVERT nor IST_COLOR_IDENTITY");
  DeviceGuard g(ctx->device);
  return launch_color_convert(static_cast<uint8_t*>(ptr), pitch, w, h, *tables, stream);
}

int ist_ctx_set_timing(ist_ctx* ctx, int on) {
  if (!ctx) return fail(IST_E_NO_CONTEXT, "无法获取绘图上下文");
  return settings_set(&ctx->settings, kTiming, on != 0);
}

int ist_ctx_last_timing(ist_ctx* ctx, double* ms, int n) {
  if (!ctx || !ms || n < 0) return fail(IST_E_INVALID, "ist_ctx_last_timing: bad argument");
  for (int k = 0; k < n; ++k) ms[k] = k < IST_PHASE_COUNT ? ctx->last_ms[k] : 0.0;
  return IST_OK;
}

// files -> decoded bitmaps in caller-owned device memory (the Image.src step, utils/canvas.js:27-121, ending in HBM)
int ist_decode_files_device_scaled(ist_ctx* ctx, const uint8_t* const* files, const int64_t* lens, int n_images, const int32_t* denom, void* const* dst,
                                   const size_t* dst_pitch, const int64_t* dst_rows, ist_image_desc* out_descs) {
  if (!ctx) return fail(IST_E_NO_CONTEXT, "无法获取绘图上下文");
  if (n_images <= 0) return IST_NOTHING_TO_DO;
  if (!files || !lens || !dst || !dst_pitch || !dst_rows) return fail(IST_E_INVALID, "ist_decode_files_device: NULL argument");
  if (n_images > kMaxImages) return fail(IST_E_UNSUPPORTED, "more than 128 images in one call");
  const int rc = check_denoms("ist_decode_files_device_scaled", denom, n_images);
  if (rc) return rc;
  std::lock_guard<std::mutex> lock(ctx->mu);
  return decode_files_locked(ctx, files, lens, n_images, denom, [&](const std::vector<ist_image_desc>& descs, uint8_t** img, size_t* pitch) -> int {
    for (int i = 0; i < n_images; ++i) {
      const ist_image_desc& D = descs[static_cast<size_t>(i)];
      const int bw = bitmap_w(D), bh = bitmap_h(D);      // (the scaled size of a reduced JPEG)
      // the file's own header is untrusted: the caller states what its buffer holds
      if (!dst[i] || dst_pitch[i] < static_cast<size_t>(bw) * 4 || (dst_pitch[i] & 3) || dst_rows[i] < bh || (reinterpret_cast<uintptr_t>(dst[i]) & 3))
        return fail(IST_E_INVALID, "ist_decode_files_device: the buffer of image " + std::to_string(i) + " is too small for " + std::to_string(bw) + "x" + std::to_string(bh));
      img[i] = static_cast<uint8_t*>(dst[i]);
      pitch[i] = dst_pitch[i];
      if (out_descs) out_descs[i] = D;
    }
    return IST_OK;
  });
}

int ist_decode_files_device(ist_ctx* ctx, const uint8_t* const* files, const int64_t* lens, int n_images, void* const* dst,
                            const size_t* dst_pitch, const int64_t* dst_rows, ist_image_desc* out_descs) {
  return ist_decode_files_device_scaled(ctx, files, lens, n_images, nullptr, dst, dst_pitch, dst_rows, out_descs);
}

}  // extern "C"
