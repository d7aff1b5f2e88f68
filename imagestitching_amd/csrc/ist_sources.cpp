// ist_sources.cpp — where the caller's source images sit in device scratch (SourceLayout, ist_internal.h).  Pure CPU.
#include "ist_internal.h"

namespace ist {

int SourceLayout::add(const ist_image_desc* images, int n_images, const uint8_t* const* src, const size_t* src_pitch,
                      const std::map<int, RowSpan>& held) {
  for (const auto& kv : held) {
    const int i = kv.first;
    if (!src || !src[i] || bitmap_w(images[i]) < 1 || bitmap_h(images[i]) < 1) return fail(IST_E_DECODE, "图片" + std::to_string(i) + "解码异常");
    if (src_pitch && src_pitch[i] < static_cast<size_t>(bitmap_w(images[i])) * 4) return fail(IST_E_INVALID, "src_pitch too small");
  }
  const size_t first = img_.size();
  img_.resize(first + static_cast<size_t>(n_images));
  for (const auto& kv : held) {
    const size_t row = static_cast<size_t>(bitmap_w(images[kv.first])) * 4;
    img_[first + static_cast<size_t>(kv.first)] = Image{src[kv.first], src_pitch ? src_pitch[kv.first] : row, row, total_, kv.second};
    total_ += round256(row * static_cast<size_t>(kv.second.y1 - kv.second.y0) + kSourceTail);
  }
  return IST_OK;
}

SourceLayout::Placed SourceLayout::place(void* base) {
  base_ = static_cast<uint8_t*>(base);
  Placed p{std::vector<const void*>(img_.size(), nullptr), std::vector<size_t>(img_.size(), 0)};
  for (size_t i = 0; i < img_.size(); ++i) {
    const Image& m = img_[i];
    if (m.src) { p.ptr[i] = reinterpret_cast<const void*>(reinterpret_cast<uintptr_t>(base_ + m.at) - static_cast<uintptr_t>(m.rows.y0) * m.row); p.pitch[i] = m.row; }
  }
  return p;
}

RowsCopy SourceLayout::copy(int i, int64_t r0, int64_t r1) const {
  const Image& m = img_[static_cast<size_t>(i)];
  return RowsCopy{base_ + m.at + static_cast<size_t>(r0 - m.rows.y0) * m.row, m.src + static_cast<size_t>(r0) * m.pitch, nullptr, m.pitch, m.row,
                  static_cast<size_t>(r1 - r0)};
}

void SourceLayout::copy_all(std::vector<RowsCopy>* items) const {
  for (size_t i = 0; i < img_.size(); ++i)
    if (img_[i].src) items->push_back(copy(static_cast<int>(i), img_[i].rows.y0, img_[i].rows.y1));
}

std::map<int, RowSpan> whole_bitmaps(const Compiled& job) {
  std::map<int, RowSpan> held;
  for (const DevOp& o : job.ops) if (o.image >= 0) held[o.image] = RowSpan{0, job.img_h[static_cast<size_t>(o.image)]};
  return held;
}

}  // namespace ist
