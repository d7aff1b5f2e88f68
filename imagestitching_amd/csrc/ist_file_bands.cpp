// ist_file_bands.cpp — the cut, the direct-placement test and the band schedule of the file pipeline (ist_file_bands.h).  Pure CPU.
#include "ist_file_bands.h"

#include <algorithm>
#include <cmath>

namespace ist {

bool cut_file_bands(const ist_op* ops, int n_ops, int64_t canvas_w, int64_t canvas_h, const ist_image_desc* images, int n_images, int filter,
                    std::vector<ist_part>* parts, std::vector<ist_region>* boxes) {
  std::vector<ist_part> cut(static_cast<size_t>(n_ops) + 8);
  int n_parts = 0;
  if (ist_shard_parts(ops, n_ops, canvas_w, canvas_h, images, n_images, filter, std::max(1, n_images), IST_SPLIT_IMAGE, cut.data(),
                      static_cast<int>(cut.size()), &n_parts) != IST_OK || n_parts < 2)
    return false;                        // overlapping draws (or a single image)
  if (n_parts > n_images) return false;  // an image drawn twice, a draw split in two: more bands than events
  cut.resize(static_cast<size_t>(n_parts));
  std::stable_sort(cut.begin(), cut.end(), [](const ist_part& a, const ist_part& b) { return a.Y0 < b.Y0; });
  boxes->clear();
  for (const ist_part& p : cut) boxes->push_back(ist_region{p.X0, p.Y0, p.X1 - p.X0, p.Y1 - p.Y0});
  parts->swap(cut);
  return true;
}

bool draw_moves_whole_image(const ist_op& o, const ist_part& p, const ist_image_desc& desc, int64_t canvas_w, int64_t canvas_h) {
  const int32_t w = desc.width, h = desc.height;
  const double X = o.m[4] + o.d[0], Y = o.m[5] + o.d[1];
  if (desc.orientation != 1 || o.kind != IST_OP_DRAW || o.image != p.image) return false;
  if (o.m[0] != 1.0 || o.m[1] != 0.0 || o.m[2] != 0.0 || o.m[3] != 1.0) return false;
  if (o.s[0] != 0.0 || o.s[1] != 0.0 || o.s[2] != w || o.s[3] != h || o.d[2] != w || o.d[3] != h) return false;
  if (X != std::floor(X) || Y != std::floor(Y) || X < 0 || Y < 0 || X + w > canvas_w || Y + h > canvas_h) return false;
  return p.X0 == static_cast<int32_t>(X) && p.Y0 == static_cast<int32_t>(Y) && p.X1 - p.X0 == w && p.Y1 - p.Y0 == h;
}

BandSchedule::Request BandSchedule::request(int64_t y_end) {
  Request r{next_, next_, kNone};
  const bool first_request = next_ == 0;
  while (next_ < y0_.size() && (!first_request || y0_[next_] < y_end)) ++next_;
  r.end = next_;
  // (the parts are sorted by Y0 and the background launch precedes them all on the render stream)
  for (size_t k = 0; k < y0_.size(); ++k) if (y0_[k] < y_end) r.cover = k;
  if (r.cover != kNone && r.cover >= next_) r.cover = kNone;
  return r;
}

}  // namespace ist
