// shard_ops.cpp — prints what the C++ side builds from a cut (ist_shard.cpp: the sub-jobs' op lists and clips, the rows every slot
// holds, the rows the root delivers), for tests/test_shard_ops.py to hold against imagestitching_amd/dist.py.  Pure CPU, no HIP:
//   g++ -std=c++17 -Iinclude -Iimagestitching_amd/csrc tools/shard_ops.cpp imagestitching_amd/csrc/{ist_plan,ist_shard,ist_compile}.cpp
// stdin, any number of cases, whitespace separated:
//   canvas_w canvas_h filter split n_slots n_images n_ops
//   n_images x (width height orientation bmp_width bmp_height opaque)
//   n_ops x (kind image m0..m5 s0..s3 d0..d3 r g b a)
// stdout per case (units in the order dist.py's ShardedStitch.parts lists them: the parts, or under IST_SPLIT_ROWS the bands):
//   case <rc>                                 ist_shard_parts' return code; nothing else follows unless it is 0
//   unit <slot> <x> <y> <w> <h> <n>           + n op lines: the unit's op list, clipped to (x, y, w, h)
//   root <n>                                  + n op lines: the root's list (no clip)
//   hold <slot> <image> <y0> <y1>             per slot, per image
//   uncovered <y0> <y1>                       the rows no unit of another slot covers
//   end
// op lines: op <kind> <image> m0..m5 s0..s3 d0..d3 r g b a (doubles in %.17g)
#include <cstdio>
#include <vector>

#include "ist_internal.h"

using namespace ist;

static void print_ops(const std::vector<ist_op>& ops) {
  for (const ist_op& o : ops) {
    std::printf("op %d %d", o.kind, o.image);
    for (double v : o.m) std::printf(" %.17g", v);
    for (double v : o.s) std::printf(" %.17g", v);
    for (double v : o.d) std::printf(" %.17g", v);
    for (uint8_t v : o.rgba) std::printf(" %d", v);
    std::printf("\n");
  }
}

int main() {
  long long cw, ch;
  int filter, split, n_slots, n_images, n_ops;
  while (std::scanf("%lld %lld %d %d %d %d %d", &cw, &ch, &filter, &split, &n_slots, &n_images, &n_ops) == 7) {
    std::vector<ist_image_desc> images(static_cast<size_t>(n_images));
    for (ist_image_desc& d : images) {
      d = ist_image_desc{};
      if (std::scanf("%d %d %d %d %d %d", &d.width, &d.height, &d.orientation, &d.bmp_width, &d.bmp_height, &d.opaque) != 6) return 2;
    }
    std::vector<ist_op> ops(static_cast<size_t>(n_ops));
    for (ist_op& o : ops) {
      o = ist_op{};
      int c[4];
      if (std::scanf("%d %d", &o.kind, &o.image) != 2) return 2;
      for (double& v : o.m) if (std::scanf("%lf", &v) != 1) return 2;
      for (double& v : o.s) if (std::scanf("%lf", &v) != 1) return 2;
      for (double& v : o.d) if (std::scanf("%lf", &v) != 1) return 2;
      if (std::scanf("%d %d %d %d", &c[0], &c[1], &c[2], &c[3]) != 4) return 2;
      for (int k = 0; k < 4; ++k) o.rgba[k] = static_cast<uint8_t>(c[k]);
    }
    std::vector<ist_part> parts(static_cast<size_t>(n_ops) * static_cast<size_t>(n_slots) + static_cast<size_t>(n_slots) + 8);
    int n_parts = 0;
    const int rc = ist_shard_parts(ops.data(), n_ops, cw, ch, images.data(), n_images, filter, n_slots, split, parts.data(),
                                   static_cast<int>(parts.size()), &n_parts);
    std::printf("case %d\n", rc);
    if (rc != IST_OK) continue;
    parts.resize(static_cast<size_t>(n_parts));
    std::vector<ist_region> remote;
    auto unit = [&](int slot, const ist_region& box, const std::vector<ist_op>& list) {
      std::printf("unit %d %d %d %d %d %zu\n", slot, box.x, box.y, box.w, box.h, list.size());
      print_ops(list);
      if (slot != 0) remote.push_back(box);
    };
    if (split == IST_SPLIT_ROWS) {
      std::vector<int32_t> cuts(static_cast<size_t>(n_slots) + 1);
      if (ist_shard_row_cuts(ch, n_slots, cuts.data()) != IST_OK) return 3;
      for (int s = 0; s < n_slots; ++s) {
        const int32_t y0 = cuts[static_cast<size_t>(s)], y1 = cuts[static_cast<size_t>(s) + 1];
        if (y1 > y0) unit(s, ist_region{0, y0, static_cast<int32_t>(cw), y1 - y0}, shard_band_ops(ops.data(), n_ops, parts_of_slot(parts, s)));
      }
    } else {
      for (const ist_part& p : parts) unit(p.slot, ist_region{p.X0, p.Y0, p.X1 - p.X0, p.Y1 - p.Y0}, shard_part_ops(ops.data(), n_ops, p));
    }
    const std::vector<ist_op> root = shard_root_ops(ops.data(), n_ops, parts_of_slot(parts, 0), remote);
    std::printf("root %zu\n", root.size());
    print_ops(root);
    for (int s = 0; s < n_slots; ++s)
      for (const auto& kv : shard_holdings(parts_of_slot(parts, s)))
        std::printf("hold %d %d %lld %lld\n", s, kv.first, static_cast<long long>(kv.second.y0), static_cast<long long>(kv.second.y1));
    for (const RowSpan& r : uncovered_rows(remote, ch)) std::printf("uncovered %lld %lld\n", static_cast<long long>(r.y0), static_cast<long long>(r.y1));
    std::printf("end\n");
  }
  return 0;
}
