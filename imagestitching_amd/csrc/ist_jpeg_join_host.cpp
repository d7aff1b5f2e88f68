// ist_jpeg_join_host.cpp — the lossless JPEG join's host side that needs no device: which sets of files are eligible (from their headers
// alone, read by the decoder's own parser), the joined file's geometry, and the per-image table the kernel reads.  Nothing here calls
// the runtime, so all of it runs, and is checked under sanitizers, without a GPU (tools/check_jpeg_join_host.cpp).  The rule is stated
// in include/imagestitch.h ("lossless JPEG joins") and restated in tests/jpeg_join_reference.py.
//
// Reference anchor: the page has no such route - its only way from files to a file is decode, draw, export (pages/index/index.js:
// 1441-1579); this is the export seam (utils/canvas.js:205-221) reached without a canvas.
#include <cstring>
#include <string>

#include "ist_internal.h"
#include "ist_jpeg_enc.h"
#include "ist_jpeg_join.h"

namespace ist {

const char* jpeg_join_reason_text(int reason) {
  switch (reason) {
    case IST_JOIN_OK: return "eligible";
    case IST_JOIN_NOT_JPEG: return "not a JPEG the decoder takes";
    case IST_JOIN_LAYOUT: return "not a YCbCr file sampled 4:4:4 or 4:2:0";
    case IST_JOIN_MIXED: return "its sampling layout differs from image 0's";
    case IST_JOIN_TABLES: return "its quantisation tables cannot be carried (they differ from image 0's, Cb's differs from Cr's, or an entry is 0 or above 255)";
    case IST_JOIN_SIZE: return "its size across the join differs from image 0's";
    case IST_JOIN_ALIGN: return "its size along the join is not a multiple of the MCU size and it is not the last image";
    case IST_JOIN_ORIENT: return "it has an EXIF orientation above 1";
    case IST_JOIN_LIMIT: return "more than 128 images, or a joined side above 65535";
    case IST_JOIN_RANGE: return "a coefficient is outside the range a baseline file codes";
    default: return "unknown reason";
  }
}

int jpeg_join_eligible(const uint8_t* const* files, const int64_t* lens, int n, int direction, ist_jpeg_join_info* info, JoinPlan* plan) {
  std::memset(info, 0, sizeof *info);
  info->image = -1; info->subsampling = -1;
  auto refuse = [&](int reason, int image, const std::string& more = std::string()) {
    info->reason = reason; info->image = image;
    return fail(IST_E_UNSUPPORTED, "image " + std::to_string(image) + ": " + jpeg_join_reason_text(reason) + (more.empty() ? "" : " (" + more + ")"));
  };
  if (n > kJoinMaxImages) return refuse(IST_JOIN_LIMIT, kJoinMaxImages);
  const bool horizontal = direction == IST_HORIZONTAL;
  *plan = JoinPlan();
  plan->n = n; plan->direction = direction;
  plan->files.resize(static_cast<size_t>(n));
  JpegImage first;                               // image 0's header: what every other image is held against
  int64_t along = 0;                             // the joined side so far
  for (int i = 0; i < n; ++i) {
    JpegImage cur;
    JpegImage& J = i == 0 ? first : cur;
    if (!files[i] || lens[i] < 2 || files[i][0] != 0xFF || files[i][1] != 0xD8) return refuse(IST_JOIN_NOT_JPEG, i);
    if (jpeg_parse_tables(files[i], lens[i], &J) != IST_OK) return refuse(IST_JOIN_NOT_JPEG, i, g_last_error);
    if (J.ncomp != 3 || J.rgb || !((J.hmax == 1 && J.vmax == 1) || (J.hmax == 2 && J.vmax == 2))) return refuse(IST_JOIN_LAYOUT, i);
    if (J.hmax != first.hmax || J.vmax != first.vmax) return refuse(IST_JOIN_MIXED, i);
    if (i == 0) {
      info->subsampling = plan->subsampling = J.hmax == 2 ? IST_JPEG_420 : IST_JPEG_444;
      if (std::memcmp(J.comp[1].q, J.comp[2].q, sizeof J.comp[1].q) != 0) return refuse(IST_JOIN_TABLES, i);
      for (int c = 0; c < 2; ++c)
        for (int k = 0; k < 64; ++k) {
          if (J.comp[c].q[k] < 1 || J.comp[c].q[k] > 255) return refuse(IST_JOIN_TABLES, i);
          plan->q[c][k] = static_cast<uint8_t>(J.comp[c].q[k]);
        }
    } else {
      for (int c = 0; c < 3; ++c)
        if (std::memcmp(J.comp[c].q, first.comp[c].q, sizeof J.comp[c].q) != 0) return refuse(IST_JOIN_TABLES, i);
    }
    if (horizontal ? J.height != first.height : J.width != first.width) return refuse(IST_JOIN_SIZE, i);
    const int mcu = 8 * J.hmax;
    if (i < n - 1 && (horizontal ? J.width : J.height) % mcu != 0) return refuse(IST_JOIN_ALIGN, i);
    if (J.orientation > 1) return refuse(IST_JOIN_ORIENT, i);
    along += horizontal ? J.width : J.height;
    if (along > 65535) return refuse(IST_JOIN_LIMIT, i);
    plan->files[static_cast<size_t>(i)] = JoinFile{J.width, J.height, J.mcus_x, J.mcus_y};
  }
  plan->width = horizontal ? along : first.width;
  plan->height = horizontal ? first.height : along;
  const JpegGeometry g = jpeg_geometry(plan->width, plan->height, plan->subsampling);
  plan->mcus_x = g.mcus_x; plan->mcus_y = g.mcus_y;
  info->width = plan->width; info->height = plan->height;
  return IST_OK;
}

int jpeg_join_table(const JoinPlan& plan, const JpegCoefPlanes* planes, JoinTable* out) {
  std::memset(out, 0, sizeof *out);
  const bool horizontal = plan.direction == IST_HORIZONTAL, is420 = jpeg_ss_420(plan.subsampling);
  out->n = plan.n;
  int32_t at = 0;
  for (int i = 0; i < plan.n; ++i) {
    const JoinFile& f = plan.files[static_cast<size_t>(i)];
    out->first[i] = at;
    at += horizontal ? f.mcus_x : f.mcus_y;
    JoinImage& I = out->img[i];
    for (int c = 0; c < 3; ++c) {
      const int s = is420 && c == 0 ? 2 : 1;
      if (!planes[i].coef[c] || planes[i].blocks_x[c] != f.mcus_x * s || planes[i].blocks_y[c] != f.mcus_y * s)
        return fail(IST_E_DECODE, "图片" + std::to_string(i) + "解码异常: JPEG frame header changed between two reads");
      I.coef[c] = planes[i].coef[c]; I.blocks_x[c] = planes[i].blocks_x[c]; I.blocks_y[c] = planes[i].blocks_y[c];
    }
    // across the join every image has the joined file's MCU count (equal widths or heights: the eligibility rule)
    if ((horizontal ? f.mcus_y : f.mcus_x) != (horizontal ? plan.mcus_y : plan.mcus_x)) return fail(IST_E_INVALID, "join plan: image " + std::to_string(i) + " does not span the joined file");
  }
  if (at != (horizontal ? plan.mcus_x : plan.mcus_y)) return fail(IST_E_INVALID, "join plan: the images do not add up to the joined file");
  for (int i = plan.n; i <= kJoinMaxImages; ++i) out->first[i] = at;
  return IST_OK;
}

}  // namespace ist

using namespace ist;

extern "C" {

int ist_jpeg_join_check(const uint8_t* const* files, const int64_t* lens, int n, int direction, ist_jpeg_join_info* out) {
  if (!files || !lens || n <= 0 || (direction != IST_VERTICAL && direction != IST_HORIZONTAL)) return fail(IST_E_INVALID, "ist_jpeg_join_check: bad argument");
  ist_jpeg_join_info info;
  JoinPlan plan;
  const int rc = jpeg_join_eligible(files, lens, n, direction, &info, &plan);
  if (out) *out = info;
  return rc;
}

}  // extern "C"
