// ist_file_bands.h — the index arithmetic of the file pipeline (ist_files.cpp): how one stitch is cut into bands, which draws
// need no bitmap of their own, and which bands a request of the PNG encoder submits.  Pure CPU, no HIP: tools/file_bands.cpp
// prints what these decide and tests/test_file_bands.py holds it against the planner's op list.
#ifndef IST_FILE_BANDS_H_
#define IST_FILE_BANDS_H_

#include <vector>

#include "ist_internal.h"

namespace ist {

// One stitch cut into one part per draw (the cut the device group uses: ist_shard_parts with a slot per image, IST_SPLIT_IMAGE),
// sorted by Y0 (stable: op order among equals), and the parts' canvas boxes.  false - nothing is written - when the draws overlap,
// when there is nothing to cut (fewer than two parts), or when the cut has more parts than images: band k signals its render
// through the context's event k, and there is one event per IMAGE (see BandSchedule).
bool cut_file_bands(const ist_op* ops, int n_ops, int64_t canvas_w, int64_t canvas_h, const ist_image_desc* images, int n_images, int filter,
                    std::vector<ist_part>* parts, std::vector<ist_region>* boxes);

// The draw `op` of `part` only MOVES its image (`desc`): unit transform, the whole source rectangle, a whole-pixel offset, nothing
// clipped by the canvas, the part's box is the image's box, the image upright (orientation 1).
bool draw_moves_whole_image(const ist_op& op, const ist_part& part, const ist_image_desc& desc, int64_t canvas_w, int64_t canvas_h);

// Which bands a request for canvas rows [0, y_end) submits, and which band's event covers those rows.  The FIRST request (nothing
// submitted yet) takes only the bands that start above y_end, so that the file's first bytes are on their way while the rest is
// rendered; every later request takes everything that is left.
// Event indexing: band k (position in the sorted parts) records ctx->img_event[k] - the events FileDecoder indexes by IMAGE while
// the scans upload.  The two uses do not meet: every upload event has been waited for (the Huffman batch of the first take())
// before the first band is recorded, and cut_file_bands never yields more parts than images.
class BandSchedule {
 public:
  static constexpr size_t kNone = ~size_t{0};
  struct Request {
    size_t begin, end;      // parts [begin, end) are submitted now, in this order
    size_t cover;           // the last part that rows [0, y_end) touch: order the reader behind ITS event.  kNone: no part starts
                            // above y_end (a gap at the top) - order the reader behind a fresh event on the render stream
  };
  explicit BandSchedule(const std::vector<ist_part>& sorted_parts) { for (const ist_part& p : sorted_parts) y0_.push_back(p.Y0); }
  Request request(int64_t y_end);

 private:
  std::vector<int64_t> y0_;
  size_t next_ = 0;         // parts [0, next_) have been submitted
};

}  // namespace ist

#endif  // IST_FILE_BANDS_H_
