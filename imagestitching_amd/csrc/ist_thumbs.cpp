// ist_thumbs.cpp — thumbnails of the C-ABI: the crop / turn / fit rule, the batch of reduces, and the form over resident bitmaps.
// Reference anchor: the grid of chosen images (pages/index/index.wxml:4-22: one <image mode="aspectFill"> per image at thumbWpx x
// thumbWpx; the cell size from pages/index/index.js:313-343, laid out again at :457-474, awaited image by image at :1155) and the modal
// image (index.wxml:202, aspectFit).  The grid is redrawn on every add, delete and drag, so its cost is per GRID here: one launch pair
// of the preview reduce's batch twins per form (ist_preview.hip), one table copy, and - over bitmaps - one copy down.
#include <atomic>
#include <cmath>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "ist_ctx.h"

using namespace ist;

namespace {

std::atomic<int64_t> g_thumb_launches{0};

// the item's turn goes into PreviewArgs::turn as it is: the public bits are the kernel's
static_assert(IST_TURN_FLIP_X == kTurnFlipX && IST_TURN_FLIP_Y == kTurnFlipY && IST_TURN_TRANSPOSE == kTurnTranspose, "IST_TURN_* and kTurn* must agree");

constexpr int kMaxThumbs = 4096;
// the partial sums of one sub-batch stay within this much of the context's preview scratch (an item that needs more runs alone, with
// what its single preview would take)
constexpr size_t kPartialBudget = size_t(256) << 20;

// EXIF orientation 1..8 -> the turn that takes the stored array to the displayed one (mirrors in stored space, then the transposition)
constexpr int32_t kTurnOf[9] = {0,
                                0,
                                IST_TURN_FLIP_X,
                                IST_TURN_FLIP_X | IST_TURN_FLIP_Y,
                                IST_TURN_FLIP_Y,
                                IST_TURN_TRANSPOSE,
                                IST_TURN_FLIP_Y | IST_TURN_TRANSPOSE,
                                IST_TURN_FLIP_X | IST_TURN_FLIP_Y | IST_TURN_TRANSPOSE,
                                IST_TURN_FLIP_X | IST_TURN_TRANSPOSE};

int64_t clamp_round(double v, int64_t hi) {
  const double r = std::floor(v + 0.5);
  return r < 1.0 ? 1 : r > static_cast<double>(hi) ? hi : static_cast<int64_t>(r);
}

int layout_check(const ist_image_desc* descs, int n, const ist_thumb_spec* spec, const ist_thumb_item* out) {
  if (n > kMaxThumbs) return fail(IST_E_UNSUPPORTED, "more than 4096 thumbnails in one call");
  if (n < 0 || !spec || (n > 0 && (!descs || !out))) return fail(IST_E_INVALID, "ist_thumb_layout: NULL argument or negative count");
  if (spec->cell_w < 1 || spec->cell_h < 1) return fail(IST_E_INVALID, "thumbnails: the cell must be at least 1 x 1");
  if (spec->mode != IST_THUMB_FILL && spec->mode != IST_THUMB_FIT) return fail(IST_E_INVALID, "thumbnails: unknown mode");
  return IST_OK;
}

int layout_one(const ist_image_desc& d, const ist_thumb_spec& sp, int k, ist_thumb_item* it) {
  const int64_t bw = bitmap_w(d), bh = bitmap_h(d);
  if (bw < 1 || bh < 1) return fail(IST_E_INVALID, "image " + std::to_string(k) + ": empty image");
  const int o = sp.apply_orientation && d.orientation >= 1 && d.orientation <= 8 ? d.orientation : 1;
  const int32_t turn = kTurnOf[o];
  const bool t = (turn & IST_TURN_TRANSPOSE) != 0;
  const int64_t W = t ? bh : bw, H = t ? bw : bh;                   // displayed
  int64_t cx = 0, cy = 0, cw = W, ch = H;
  int32_t ow = sp.cell_w, oh = sp.cell_h;
  if (sp.mode == IST_THUMB_FILL) {
    const double tw = static_cast<double>(sp.cell_w), th = static_cast<double>(sp.cell_h);
    const double dW = static_cast<double>(W), dH = static_cast<double>(H);
    if (tw / dW >= th / dH) ch = clamp_round(th * dW / tw, H);
    else cw = clamp_round(tw * dH / th, W);
    cx = (W - cw) / 2; cy = (H - ch) / 2;
  } else {
    const int rc = ist_preview_fit(W, H, static_cast<double>(sp.cell_w), static_cast<double>(sp.cell_h), &ow, &oh);
    if (rc) return rc;
  }
  // back into stored space: undo the transposition, then the mirrors (a mirrored axis counts from the other end)
  const int64_t xs = t ? cy : cx, ys = t ? cx : cy, ws = t ? ch : cw, hs = t ? cw : ch;
  it->width = ow; it->height = oh;
  it->src_x = static_cast<int32_t>((turn & IST_TURN_FLIP_X) ? bw - xs - ws : xs);
  it->src_y = static_cast<int32_t>((turn & IST_TURN_FLIP_Y) ? bh - ys - hs : ys);
  it->src_w = static_cast<int32_t>(ws); it->src_h = static_cast<int32_t>(hs);
  it->turn = turn; it->reserved = 0; it->offset = 0;
  return IST_OK;
}

int layout_all(const ist_image_desc* descs, int n, const ist_thumb_spec* spec, ist_thumb_item* out, int64_t* out_bytes) {
  if (out_bytes) *out_bytes = 0;
  int rc = layout_check(descs, n, spec, out);
  if (rc) return rc;
  int64_t at = 0;
  for (int k = 0; k < n; ++k) {
    rc = layout_one(descs[k], *spec, k, &out[k]);
    if (rc) return rc;
    out[k].offset = at;
    at += int64_t{4} * out[k].width * out[k].height;
  }
  if (out_bytes) *out_bytes = at;
  return IST_OK;
}

// the one draw of an image that does not shrink on both axes: the stored window at (0, 0, pw_s, ph_s) under the turn's CTM
ist_op turned_draw(const ist_thumb_item& it, int32_t pw_s, int32_t ph_s) {
  ist_op op;
  std::memset(&op, 0, sizeof(op));
  op.kind = IST_OP_DRAW; op.image = 0;
  const double sx = (it.turn & IST_TURN_FLIP_X) ? -1.0 : 1.0, tx = (it.turn & IST_TURN_FLIP_X) ? static_cast<double>(pw_s) : 0.0;
  const double sy = (it.turn & IST_TURN_FLIP_Y) ? -1.0 : 1.0, ty = (it.turn & IST_TURN_FLIP_Y) ? static_cast<double>(ph_s) : 0.0;
  if (it.turn & IST_TURN_TRANSPOSE) { op.m[2] = sy; op.m[4] = ty; op.m[1] = sx; op.m[5] = tx; }      // X = sy * v + ty, Y = sx * u + tx
  else { op.m[0] = sx; op.m[4] = tx; op.m[3] = sy; op.m[5] = ty; }
  op.s[2] = static_cast<double>(it.src_w); op.s[3] = static_cast<double>(it.src_h);
  op.d[2] = static_cast<double>(pw_s); op.d[3] = static_cast<double>(ph_s);
  return op;
}

struct Reduce { PreviewArgs a; size_t partial_bytes; bool opaque; };

// one sub-batch of reduces on `stream`: per form one table section, one stage-1 and one stage-2 launch (ctx->prev_mu held)
int launch_sub_batch(ist_ctx* ctx, std::vector<Reduce>& items, size_t first, size_t last, hipStream_t stream) {
  struct Form { std::vector<size_t> idx; size_t at_items = 0, at_wg = 0, at_px = 0; int64_t wgs = 0, px = 0; };
  Form form[2];
  size_t at = 0;
  for (size_t q = first; q < last; ++q) {                   // every item its own range of the partial sums
    items[q].a.partial = reinterpret_cast<float*>(static_cast<uint8_t*>(ctx->scratch_prev.p) + at);
    at += items[q].partial_bytes;
    form[items[q].opaque ? 1 : 0].idx.push_back(q);
  }
  size_t total = 0;
  for (Form& F : form) {
    if (F.idx.empty()) continue;
    const size_t m = F.idx.size();
    F.at_items = total; total = round256(total + m * sizeof(PreviewArgs));
    F.at_wg = total;    total = round256(total + (m + 1) * sizeof(int64_t));
    F.at_px = total;    total = round256(total + (m + 1) * sizeof(int64_t));
  }
  std::lock_guard<std::mutex> lk(ctx->batch_mu);
  ist_ctx::BatchSlot* slot = nullptr;
  int rc = batch_take_slot(ctx, total, &slot);
  if (rc) return rc;
  uint8_t* h = static_cast<uint8_t*>(slot->host.p);
  for (Form& F : form) {
    if (F.idx.empty()) continue;
    const size_t m = F.idx.size();
    PreviewArgs* pa = reinterpret_cast<PreviewArgs*>(h + F.at_items);
    int64_t* wb = reinterpret_cast<int64_t*>(h + F.at_wg);
    int64_t* pb = reinterpret_cast<int64_t*>(h + F.at_px);
    for (size_t j = 0; j < m; ++j) {
      const PreviewArgs& a = items[F.idx[j]].a;
      std::memcpy(&pa[j], &a, sizeof(PreviewArgs));
      wb[j] = F.wgs; pb[j] = F.px;
      F.wgs += static_cast<int64_t>(a.groups) * a.chunks * a.ph;
      F.px += (static_cast<int64_t>(a.pw) * a.ph + 255) / 256 * 256;
    }
    wb[m] = F.wgs; pb[m] = F.px;
  }
  uint8_t* d = static_cast<uint8_t*>(slot->dev.p);
  if (hipMemcpyAsync(d, h, total, hipMemcpyHostToDevice, stream) != hipSuccess) { (void)hipGetLastError(); return fail(IST_E_HIP, "uploading the thumbnail table failed"); }
  int launches = 0;
  for (int f = 0; f < 2 && rc == IST_OK; ++f) {
    const Form& F = form[f];
    if (F.idx.empty()) continue;
    PreviewBatchArgs b;
    b.items = reinterpret_cast<const PreviewArgs*>(d + F.at_items);
    b.wg_begin = reinterpret_cast<const int64_t*>(d + F.at_wg);
    b.px_begin = reinterpret_cast<const int64_t*>(d + F.at_px);
    b.n = static_cast<int32_t>(F.idx.size()); b.pad_ = 0;
    rc = launch_preview_batch(b, F.wgs, F.px, f == 1, stream);
    if (rc == IST_OK) ++launches;
  }
  // (recorded whatever happened: the copy is in flight and the slot must not be refilled before it is done)
  if (hipEventRecord(slot->done, stream) == hipSuccess) slot->pending = true;
  else { (void)hipGetLastError(); (void)hipStreamSynchronize(stream); }
  g_thumb_launches.fetch_add(launches, std::memory_order_relaxed);
  return rc;
}

// every thumbnail of a laid-out call enqueued on `stream` (arguments checked by the caller, the context's device current)
int thumbs_enqueue(ist_ctx* ctx, const ist_image_desc* descs, const void* const* src, const size_t* pitch, int n, const ist_thumb_item* lay,
                   uint8_t* dst, hipStream_t stream) {
  std::vector<Reduce> red;
  std::vector<int> drawn;                                   // the images that do not shrink on both axes
  for (int k = 0; k < n; ++k) {
    const ist_thumb_item& it = lay[k];
    const bool t = (it.turn & IST_TURN_TRANSPOSE) != 0;
    const int32_t pw_s = t ? it.height : it.width, ph_s = t ? it.width : it.height;
    Reduce r;
    if (!preview_geometry(it.src_w, it.src_h, pw_s, ph_s, &r.a)) { drawn.push_back(k); continue; }
    r.a.src = static_cast<const uint8_t*>(src[k]) + static_cast<size_t>(it.src_y) * pitch[k] + static_cast<size_t>(it.src_x) * 4;
    r.a.src_pitch = pitch[k];
    r.a.dst = dst + it.offset; r.a.dst_pitch = static_cast<size_t>(it.width) * 4;
    r.a.turn = it.turn;
    r.partial_bytes = static_cast<size_t>(ph_s) * static_cast<size_t>(r.a.chunks) * static_cast<size_t>(pw_s) * 16;
    r.opaque = descs[k].opaque != 0;
    red.push_back(r);
  }
  // the one-draw jobs first: compiling one may fail, and nothing of the call is in flight then
  const size_t m = drawn.size();
  std::vector<JobPtr> jobs(m);                              // (destroyed on return, which waits for `stream`)
  std::vector<ist_job*> ljob(m, nullptr);
  std::vector<const void*> lsrc(m, nullptr);
  std::vector<size_t> lpitch(m, 0), ldst_pitch(m, 0);
  std::vector<int> lcount(m, 1);
  std::vector<void*> ldst(m, nullptr);
  for (size_t q = 0; q < m; ++q) {
    const int k = drawn[q];
    const ist_thumb_item& it = lay[k];
    const bool t = (it.turn & IST_TURN_TRANSPOSE) != 0;
    const int32_t pw_s = t ? it.height : it.width, ph_s = t ? it.width : it.height;
    ist_image_desc desc;                                    // the window is the job's whole image: nothing outside it is sampled
    std::memset(&desc, 0, sizeof(desc));
    desc.width = it.src_w; desc.height = it.src_h; desc.orientation = 1; desc.opaque = descs[k].opaque ? 1 : 0;
    const ist_op op = turned_draw(it, pw_s, ph_s);
    jobs[q].reset(ist_job_create(ctx, it.width, it.height, kTransparent, &op, 1, &desc, 1, IST_FILTER_AREA, nullptr));
    if (!jobs[q]) { const std::string why = g_last_error; return fail(g_last_code ? g_last_code : IST_E_INVALID, "image " + std::to_string(k) + ": " + why); }
    ljob[q] = jobs[q].get();
    lsrc[q] = static_cast<const uint8_t*>(src[k]) + static_cast<size_t>(it.src_y) * pitch[k] + static_cast<size_t>(it.src_x) * 4;
    lpitch[q] = pitch[k];
    ldst[q] = dst + it.offset; ldst_pitch[q] = static_cast<size_t>(it.width) * 4;
  }
  if (!red.empty()) {
    // sub-batches: consecutive items while their partial sums fit the budget
    std::vector<size_t> cut{0};
    size_t held = 0, most = 0;
    for (size_t q = 0; q < red.size(); ++q) {
      if (q > cut.back() && held + red[q].partial_bytes > kPartialBudget) { cut.push_back(q); held = 0; }
      held += red[q].partial_bytes;
      most = std::max(most, held);
    }
    cut.push_back(red.size());
    std::lock_guard<std::mutex> lock(ctx->prev_mu);
    // (growing frees the old block, which waits for the device: a reduce still in flight has finished with it by then)
    int rc = ctx->scratch_prev.grow(most);
    if (rc) return rc;
    rc = ctx->prev_done.ensure();
    if (rc) return rc;
    // one reduce owns the partial sums at a time: a call on another stream than the last one starts behind it (the sub-batches of this
    // call follow each other on `stream`)
    if (ctx->prev_pending && ctx->prev_last != stream) IST_HIP_OR(hipStreamWaitEvent(stream, ctx->prev_done, 0), "ordering the thumbnails behind the previous preview failed");
    for (size_t c = 0; c + 1 < cut.size() && rc == IST_OK; ++c) rc = launch_sub_batch(ctx, red, cut[c], cut[c + 1], stream);
    // (recorded even after a failure: what was launched reads the scratch)
    if (hipEventRecord(ctx->prev_done, stream) != hipSuccess) { (void)hipGetLastError(); (void)hipStreamSynchronize(stream); ctx->prev_pending = false; }
    else { ctx->prev_pending = true; ctx->prev_last = stream; }
    if (rc) return rc;
  }
  if (drawn.empty()) return IST_OK;
  return ist_jobs_launch(ljob.data(), static_cast<int>(m), lsrc.data(), lpitch.data(), lcount.data(), ldst.data(), ldst_pitch.data(), stream);
}

}  // namespace

extern "C" {

int64_t ist_debug_thumb_launches(void) { return g_thumb_launches.load(std::memory_order_relaxed); }

int ist_thumb_layout(const ist_image_desc* descs, int n, const ist_thumb_spec* spec, ist_thumb_item* out, int64_t* out_bytes) {
  return layout_all(descs, n, spec, out, out_bytes);
}

int ist_thumbs_device(ist_ctx* ctx, const ist_image_desc* descs, const void* const* src, const size_t* pitch, int n, const ist_thumb_spec* spec,
                      void* dst, int64_t dst_cap, ist_thumb_item* out, void* stream) {
  if (!ctx) return fail(IST_E_NO_CONTEXT, "无法获取绘图上下文");
  if (n < 1) return fail(IST_E_INVALID, "ist_thumbs_device: no images");
  if (!src || !pitch || !dst) return fail(IST_E_INVALID, "ist_thumbs_device: NULL argument");
  int64_t total = 0;
  const int rc = layout_all(descs, n, spec, out, &total);
  if (rc) return rc;
  if (dst_cap < total) return fail(IST_E_INVALID, "ist_thumbs_device: dst_cap is smaller than the thumbnails (" + std::to_string(total) + " bytes)");
  for (int k = 0; k < n; ++k) {
    if (!src[k]) return fail(IST_E_DECODE, "图片" + std::to_string(k) + "解码异常");
    if (pitch[k] < static_cast<size_t>(bitmap_w(descs[k])) * 4 || (pitch[k] & 3)) return fail(IST_E_INVALID, "image " + std::to_string(k) + ": pitch too small or not a multiple of 4");
  }
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(IST_E_NO_DEVICE, "hipSetDevice failed");
  return thumbs_enqueue(ctx, descs, src, pitch, n, out, static_cast<uint8_t*>(dst), static_cast<hipStream_t>(stream));
}

int ist_bitmaps_thumbs(ist_ctx* ctx, ist_bitmap* const* bitmaps, int n, const ist_thumb_spec* spec, ist_thumb_item* out, uint8_t** out_pixels) {
  if (out_pixels) *out_pixels = nullptr;
  if (!ctx) return fail(IST_E_NO_CONTEXT, "无法获取绘图上下文");
  if (n < 1) return fail(IST_E_INVALID, "ist_bitmaps_thumbs: no bitmaps");
  if (n > kMaxThumbs) return fail(IST_E_UNSUPPORTED, "more than 4096 thumbnails in one call");
  if (!bitmaps || !out || !out_pixels) return fail(IST_E_INVALID, "ist_bitmaps_thumbs: NULL argument");
  const size_t m = static_cast<size_t>(n);
  std::vector<ist_image_desc> descs(m);
  std::vector<const void*> src(m);
  std::vector<size_t> pitch(m);
  for (int i = 0; i < n; ++i)
    if (!bitmaps[i]) return fail(IST_E_DECODE, "图片" + std::to_string(i) + "解码异常");
  // the call's own references: a host may release a bitmap while this runs
  struct Held { std::vector<ist_bitmap*> b; ~Held() { for (ist_bitmap* x : b) ist_bitmap_release(x); } } held;
  held.b.reserve(m);
  for (int i = 0; i < n; ++i) { ist_bitmap_retain(bitmaps[i]); held.b.push_back(bitmaps[i]); }
  for (size_t i = 0; i < m; ++i) {
    int device = 0;
    const uint8_t* row0 = nullptr;
    bitmap_view(held.b[i], &device, &row0, &pitch[i], &descs[i]);
    src[i] = row0;
    if (device != ctx->device)
      return fail(IST_E_INVALID, "bitmap " + std::to_string(i) + " lives on device " + std::to_string(device) + ", the context on device " + std::to_string(ctx->device));
  }
  int64_t total = 0;
  int rc = layout_all(descs.data(), n, spec, out, &total);
  if (rc) return rc;
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(IST_E_NO_DEVICE, "hipSetDevice failed");
  rc = ctx->prev_out.grow(static_cast<size_t>(total));
  if (rc) return rc;
  rc = thumbs_enqueue(ctx, descs.data(), src.data(), pitch.data(), n, out, static_cast<uint8_t*>(ctx->prev_out.p), ctx->stream);
  if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }      // (nothing of this call is in flight when it returns)
  return read_back_pooled(ctx->prev_out.p, static_cast<size_t>(total), ctx->stream, out_pixels);
}

}  // extern "C"
