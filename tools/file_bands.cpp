// file_bands.cpp — prints what the file pipeline's index rules decide (ist_file_bands.cpp: the cut into bands, the draws that only
// move their image, the band schedule), for tests/test_file_bands.py to hold against its own statement of them.  Pure CPU, no HIP:
//   g++ -std=c++17 -Iinclude -Iimagestitching_amd/csrc tools/file_bands.cpp imagestitching_amd/csrc/{ist_file_bands,ist_plan,ist_shard,ist_compile}.cpp
// stdin, any number of cases, whitespace separated:
//   canvas_w canvas_h filter n_images n_ops n_seq
//   n_images x (width height orientation bmp_width bmp_height opaque)
//   n_ops x (kind image m0..m5 s0..s3 d0..d3 r g b a)
//   n_seq x (k y_end_1 .. y_end_k)                  the requests one call of the encoder would make
// stdout per case:
//   case <banded>                                   cut_file_bands' answer; only `end` follows when it is 0
//   part <k> <image> <op> <X0> <Y0> <X1> <Y1>       the sorted parts
//   box <k> <x> <y> <w> <h>
//   moves <k> <0|1> <0|1>                           draw_moves_whole_image; the band's compiled job has copy tiles only
//   seq <j>                                         a fresh BandSchedule, then one line per request:
//   req <y_end> <begin> <end> <cover>               cover -1: none
//   end
#include <cstdio>
#include <vector>

#include "ist_file_bands.h"

using namespace ist;

int main() {
  long long cw, ch;
  int filter, n_images, n_ops, n_seq;
  while (std::scanf("%lld %lld %d %d %d %d", &cw, &ch, &filter, &n_images, &n_ops, &n_seq) == 6) {
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
    std::vector<std::vector<long long>> seqs(static_cast<size_t>(n_seq));
    for (std::vector<long long>& s : seqs) {
      int k = 0;
      if (std::scanf("%d", &k) != 1 || k < 0) return 2;
      s.resize(static_cast<size_t>(k));
      for (long long& y : s) if (std::scanf("%lld", &y) != 1) return 2;
    }
    std::vector<ist_part> parts;
    std::vector<ist_region> boxes;
    const bool banded = cut_file_bands(ops.data(), n_ops, cw, ch, images.data(), n_images, filter, &parts, &boxes);
    std::printf("case %d\n", banded ? 1 : 0);
    if (banded) {
      for (size_t k = 0; k < parts.size(); ++k) {
        const ist_part& p = parts[k];
        std::printf("part %zu %d %d %d %d %d %d\n", k, p.image, p.op, p.X0, p.Y0, p.X1, p.Y1);
        std::printf("box %zu %d %d %d %d\n", k, boxes[k].x, boxes[k].y, boxes[k].w, boxes[k].h);
        const std::vector<ist_op> one = shard_part_ops(ops.data(), n_ops, p);
        Compiled job;
        if (compile_ops(cw, ch, kTransparent, one.data(), static_cast<int>(one.size()), images.data(), n_images, filter, &boxes[k], &job) != IST_OK) return 3;
        std::printf("moves %zu %d %d\n", k, draw_moves_whole_image(ops[static_cast<size_t>(p.op)], p, images[static_cast<size_t>(p.image)], cw, ch) ? 1 : 0,
                    job.info.n_tiles != 0 && job.info.tiles_copy == job.info.n_tiles ? 1 : 0);
      }
      for (size_t j = 0; j < seqs.size(); ++j) {
        std::printf("seq %zu\n", j);
        BandSchedule sched(parts);
        for (long long y : seqs[j]) {
          const BandSchedule::Request r = sched.request(y);
          std::printf("req %lld %zu %zu %lld\n", y, r.begin, r.end, r.cover == BandSchedule::kNone ? -1LL : static_cast<long long>(r.cover));
        }
      }
    }
    std::printf("end\n");
  }
  return 0;
}
