// ist_overlap_host.cpp — overlap removal for scrolled screenshots: the three host rules of the contract (include/imagestitch.h: the edge
// rule, the selection, the crop rule; pure functions) and the call that runs the three launches of ist_overlap.hip around them.
// One call: tables up, signatures, edge sums, edge sums down, WAIT, the host's edge rule, pair table up again, costs + flags, both
// down, WAIT, the host's selection.  Three launches, two waits, whatever the number of images.
#include <algorithm>
#include <atomic>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "ist_ctx.h"
#include "ist_overlap.h"

using namespace ist;

namespace {

std::atomic<int64_t> g_overlap_launches{0};

constexpr ist_overlap_opts kDefaults = {8, 16, 8, 0};
constexpr int64_t kMaxWidth = int64_t{1} << 20;   // a row's sums stay below 2^31, so D of two rows fits 32 bits (ist_overlap.hip, row_diff)

int check_opts(const char* who, const ist_overlap_opts* o) {
  if (o && (o->tolerance < 0 || o->min_rows < 0 || o->min_informative < 0)) return fail(IST_E_INVALID, std::string(who) + ": negative option");
  return IST_OK;
}

int32_t edge_rule(const int64_t* d, int n, int64_t T) {
  int32_t best = 0, bad = 0;
  for (int32_t y = 0; y < n; ++y) {
    const bool m = d[y] <= T;
    if (!m) ++bad;
    if (m && bad <= (y + 1) / 4) best = y + 1;
  }
  return best;
}

int32_t select_rule(const int64_t* cost, const int32_t* inf, int kmax, int64_t T, const ist_overlap_opts& o) {
  int32_t best = 0;
  for (int32_t k = std::max(o.min_rows, 1); k <= kmax; ++k) {
    if (static_cast<__int128>(cost[k]) > static_cast<__int128>(T) * k || inf[k] < o.min_informative) continue;
    // ascending k and a strict comparison: an exact tie keeps the smaller k
    if (best == 0 || static_cast<__int128>(cost[k]) * best < static_cast<__int128>(cost[best]) * k) best = k;
  }
  return best;
}

// where the call's tables and results sit: the same offsets in the pinned block and in the device block, the signatures (device only) last
struct Layout { size_t images, row_begin, pairs, tables_end, edge, cost, flag, host_end, sig, total; };

}  // namespace

namespace ist {

int overlap_run(ist_ctx* ctx, const void* const* src, const size_t* pitch, const ist_image_desc* descs, int n, const ist_overlap_opts* opts,
                ist_overlap* out) {
  const ist_overlap_opts o = opts ? *opts : kDefaults;
  const size_t m = static_cast<size_t>(n), np = m - 1;
  for (int i = 0; i < n; ++i)
    if (bitmap_w(descs[i]) > kMaxWidth) return fail(IST_E_UNSUPPORTED, "image " + std::to_string(i) + ": wider than 1048576 pixels");
  std::vector<OvlImage> images(m);
  std::vector<int64_t> row_begin(m + 1);
  int64_t rows = 0;
  for (size_t i = 0; i < m; ++i) {
    images[i] = OvlImage{static_cast<const uint8_t*>(src[i]), pitch[i], static_cast<int32_t>(bitmap_w(descs[i])), static_cast<int32_t>(bitmap_h(descs[i])), rows};
    row_begin[i] = rows;
    rows += images[i].h;
  }
  row_begin[m] = rows;
  std::vector<OvlPair> pairs(np);
  int64_t n_edge = 0, n_cost = 0, n_flag = 0;
  int max_l = 0;
  for (size_t i = 0; i < np; ++i) {
    OvlPair& P = pairs[i];
    std::memset(&P, 0, sizeof(P));
    const OvlImage &A = images[i], &B = images[i + 1];
    const int32_t hm = std::min(A.h, B.h);
    P.sig_a = A.row0; P.sig_b = B.row0; P.ha = A.h; P.hb = B.h;
    P.T = static_cast<int64_t>(o.tolerance) * A.w;
    P.L = A.w == B.w ? hm / 2 : 0;
    P.kmax = -1;
    P.edge_at = n_edge; P.cost_at = n_cost; P.flag_at = n_flag;
    n_edge += 2 * int64_t{P.L}; n_cost += int64_t{hm} + 1; n_flag += B.h;
    max_l = std::max(max_l, P.L);
  }
  Layout L;
  size_t at = 0;
  L.images = arena_take(&at, m * sizeof(OvlImage));
  L.row_begin = arena_take(&at, (m + 1) * sizeof(int64_t));
  L.pairs = arena_take(&at, np * sizeof(OvlPair));
  L.tables_end = at;
  L.edge = arena_take(&at, static_cast<size_t>(n_edge) * sizeof(int64_t));
  L.cost = arena_take(&at, static_cast<size_t>(n_cost) * sizeof(int64_t));
  L.flag = arena_take(&at, static_cast<size_t>(n_flag) * sizeof(int32_t));
  L.host_end = at;
  L.sig = arena_take(&at, static_cast<size_t>(rows) * kOvlCells * sizeof(uint32_t));
  L.total = at;

  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(IST_E_NO_DEVICE, "hipSetDevice failed");
  int rc = ctx->stream.ensure();
  if (rc) return rc;
  ctx->ovl_rows = 0;
  rc = ctx->scratch_ovl.grow(L.total);
  if (rc) return rc;
  rc = ctx->ovl_host.grow(L.host_end);
  if (rc) return rc;
  uint8_t* h = static_cast<uint8_t*>(ctx->ovl_host.p);
  uint8_t* d = static_cast<uint8_t*>(ctx->scratch_ovl.p);
  hipStream_t s = ctx->stream;
  std::memcpy(h + L.images, images.data(), m * sizeof(OvlImage));
  std::memcpy(h + L.row_begin, row_begin.data(), (m + 1) * sizeof(int64_t));
  std::memcpy(h + L.pairs, pairs.data(), np * sizeof(OvlPair));
  OvlArgs a;
  a.images = reinterpret_cast<const OvlImage*>(d + L.images);
  a.row_begin = reinterpret_cast<const int64_t*>(d + L.row_begin);
  a.pairs = reinterpret_cast<const OvlPair*>(d + L.pairs);
  a.sig = reinterpret_cast<uint32_t*>(d + L.sig);
  a.edge = reinterpret_cast<int64_t*>(d + L.edge);
  a.cost = reinterpret_cast<int64_t*>(d + L.cost);
  a.flag = reinterpret_cast<int32_t*>(d + L.flag);
  a.n_images = n; a.n_pairs = static_cast<int32_t>(np);
  // whatever fails from here on, the stream is idle when the call returns: the next call rewrites the pinned block
  struct Idle { hipStream_t s; ~Idle() { (void)hipStreamSynchronize(s); } } idle{s};

  IST_HIP_OR(hipMemcpyAsync(d, h, L.tables_end, hipMemcpyHostToDevice, s), "uploading the overlap tables failed");
  rc = launch_overlap_signatures(a, rows, s);
  if (rc) return rc;
  g_overlap_launches.fetch_add(1, std::memory_order_relaxed);
  rc = launch_overlap_edges(a, max_l, s);
  if (rc) return rc;
  g_overlap_launches.fetch_add(1, std::memory_order_relaxed);
  if (n_edge > 0) IST_HIP_OR(hipMemcpyAsync(h + L.edge, d + L.edge, static_cast<size_t>(n_edge) * sizeof(int64_t), hipMemcpyDeviceToHost, s), "reading the edge sums failed");
  IST_HIP(hipStreamSynchronize(s));

  const int64_t* edge = reinterpret_cast<const int64_t*>(h + L.edge);
  int max_k = 0, max_body = 0;
  for (size_t i = 0; i < np; ++i) {
    OvlPair& P = pairs[i];
    if (P.L == 0) continue;
    P.H = edge_rule(edge + P.edge_at, P.L, P.T);
    P.F = edge_rule(edge + P.edge_at + P.L, P.L, P.T);
    const int32_t body_a = P.ha - P.F - P.H;
    P.body_b = P.hb - P.F - P.H;
    P.kmax = std::min(body_a, P.body_b - 1);
    max_k = std::max(max_k, P.kmax); max_body = std::max(max_body, P.body_b);
  }
  std::memcpy(h + L.pairs, pairs.data(), np * sizeof(OvlPair));
  IST_HIP_OR(hipMemcpyAsync(d + L.pairs, h + L.pairs, np * sizeof(OvlPair), hipMemcpyHostToDevice, s), "uploading the overlap pairs failed");
  rc = launch_overlap_costs(a, max_k, max_body, s);
  if (rc) return rc;
  g_overlap_launches.fetch_add(1, std::memory_order_relaxed);
  IST_HIP_OR(hipMemcpyAsync(h + L.cost, d + L.cost, L.host_end - L.cost, hipMemcpyDeviceToHost, s), "reading the overlap costs failed");
  IST_HIP(hipStreamSynchronize(s));
  ctx->ovl_rows = rows; ctx->ovl_sig_at = L.sig;

  const int64_t* cost = reinterpret_cast<const int64_t*>(h + L.cost);
  const int32_t* flag = reinterpret_cast<const int32_t*>(h + L.flag);
  std::vector<int32_t> inf;
  for (size_t i = 0; i < np; ++i) {
    const OvlPair& P = pairs[i];
    out[i] = ist_overlap{0, 0, 0, 0, 0};
    if (P.L == 0) continue;
    out[i].header = P.H; out[i].footer = P.F;
    if (P.kmax < 1) continue;
    inf.assign(static_cast<size_t>(P.kmax) + 1, 0);
    for (int32_t k = 1; k <= P.kmax; ++k) inf[static_cast<size_t>(k)] = inf[static_cast<size_t>(k) - 1] + (k - 1 < P.body_b - 1 ? flag[P.flag_at + k - 1] : 0);
    const int32_t K = select_rule(cost + P.cost_at, inf.data(), P.kmax, P.T, o);
    out[i].overlap = K;
    out[i].cost = K > 0 ? cost[P.cost_at + K] : 0;
  }
  return IST_OK;
}

}  // namespace ist

extern "C" {

int64_t ist_debug_overlap_launches(void) { return g_overlap_launches.load(std::memory_order_relaxed); }

int ist_overlap_edge(const int64_t* d, int n, int64_t T, int32_t* t) {
  if (!t || n < 0 || (n > 0 && !d)) return fail(IST_E_INVALID, "ist_overlap_edge: NULL argument or negative count");
  *t = edge_rule(d, n, T);
  return IST_OK;
}

int ist_overlap_select(const int64_t* cost, const int32_t* inf, int kmax, int64_t T, const ist_overlap_opts* opts, int32_t* k) {
  if (!k) return fail(IST_E_INVALID, "ist_overlap_select: NULL argument");
  *k = 0;
  if (kmax >= 0 && (!cost || !inf)) return fail(IST_E_INVALID, "ist_overlap_select: NULL argument");
  const int rc = check_opts("ist_overlap_select", opts);
  if (rc) return rc;
  *k = select_rule(cost, inf, kmax, T, opts ? *opts : kDefaults);
  return IST_OK;
}

int ist_overlap_rows(const ist_overlap* pairs, const int32_t* heights, int n, int32_t* top, int32_t* bot) {
  if (n < 1 || !heights || !top || !bot || (n > 1 && !pairs)) return fail(IST_E_INVALID, "ist_overlap_rows: NULL argument or no images");
  for (int i = 0; i < n; ++i) { top[i] = 0; bot[i] = heights[i]; }
  for (int i = 0; i + 1 < n; ++i) {
    if (pairs[i].overlap <= 0) continue;
    top[i + 1] = pairs[i].header + pairs[i].overlap;
    bot[i] = heights[i] - pairs[i].footer;
  }
  for (int i = 1; i + 1 < n; ++i)
    if (bot[i] - top[i] < 1) { bot[i] = heights[i]; top[i + 1] = 0; }
  return IST_OK;
}

int ist_overlap_device(ist_ctx* ctx, const void* const* src, const size_t* pitch, const ist_image_desc* descs, int n, const ist_overlap_opts* opts,
                       ist_overlap* out) {
  if (!ctx) return fail(IST_E_NO_CONTEXT, "无法获取绘图上下文");
  if (n < 2) return fail(IST_E_INVALID, "ist_overlap_device: an overlap needs at least two images");
  if (!src || !pitch || !descs || !out) return fail(IST_E_INVALID, "ist_overlap_device: NULL argument");
  if (n > kMaxImages) return fail(IST_E_UNSUPPORTED, "more than 128 images in one call");
  int rc = check_opts("ist_overlap_device", opts);
  if (rc) return rc;
  for (int i = 0; i < n; ++i) {
    if (!src[i] || bitmap_w(descs[i]) < 1 || bitmap_h(descs[i]) < 1) return fail(IST_E_DECODE, "图片" + std::to_string(i) + "解码异常");
    rc = overlap_check_desc(descs[i], i);
    if (rc) return rc;
    if (pitch[i] < static_cast<size_t>(bitmap_w(descs[i])) * 4 || (pitch[i] & 3)) return fail(IST_E_INVALID, "image " + std::to_string(i) + ": pitch too small or not a multiple of 4");
    if (reinterpret_cast<uintptr_t>(src[i]) & 3) return fail(IST_E_INVALID, "image " + std::to_string(i) + ": the pixels must be 4-byte aligned");
  }
  return overlap_run(ctx, src, pitch, descs, n, opts, out);
}

int ist_debug_overlap_signatures(ist_ctx* ctx, uint32_t* out, int64_t rows) {
  if (!ctx) return fail(IST_E_NO_CONTEXT, "无法获取绘图上下文");
  if (!out || rows < 0) return fail(IST_E_INVALID, "ist_debug_overlap_signatures: NULL argument or negative count");
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (rows > ctx->ovl_rows) return fail(IST_E_INVALID, "ist_debug_overlap_signatures: the last overlap call made " + std::to_string(ctx->ovl_rows) + " rows");
  if (rows == 0) return IST_OK;
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(IST_E_NO_DEVICE, "hipSetDevice failed");
  IST_HIP(hipMemcpy(out, static_cast<const uint8_t*>(ctx->scratch_ovl.p) + ctx->ovl_sig_at, static_cast<size_t>(rows) * kOvlCells * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return IST_OK;
}

}  // extern "C"

namespace ist {

int overlap_check_desc(const ist_image_desc& d, int i) {
  if (d.orientation > 1) return fail(IST_E_UNSUPPORTED, "image " + std::to_string(i) + ": EXIF orientation " + std::to_string(d.orientation) + " (overlaps are searched between stored rows)");
  if (bitmap_w(d) != d.width || bitmap_h(d) != d.height) return fail(IST_E_UNSUPPORTED, "image " + std::to_string(i) + ": decoded at a reduced scale");
  return IST_OK;
}

}  // namespace ist
