// ist_overlap.h — the device tables and launch entries of the overlap search, shared by ist_overlap.hip and ist_overlap_host.cpp
#ifndef IST_OVERLAP_H_
#define IST_OVERLAP_H_

#include "ist_internal.h"

namespace ist {

constexpr int kOvlCells = 32;             // cells of a row's signature (the contract in include/imagestitch.h)

// one image of a call: its pixels and the first of its rows in the signature table (the images' rows follow each other)
struct OvlImage {
  const uint8_t* src;
  size_t pitch;
  int32_t w, h;
  int64_t row0;
};

// one pair (A above, B below).  The edge launch reads everything but H, F, kmax, body_b and T_pos, which the host fills in between.
struct OvlPair {
  int64_t sig_a, sig_b;     // first signature rows of A and B
  int64_t edge_at;          // first of the pair's 2 * L edge sums (L from the top, then L from the bottom)
  int64_t cost_at;          // first of the pair's cost(k), k = 0 .. min(hA, hB)
  int64_t flag_at;          // first of the pair's informative flags, one per row of B
  int64_t T;                // tolerance * w
  int32_t ha, hb;
  int32_t L;                // 0: the widths differ, nothing is computed for the pair
  int32_t H, F, kmax, body_b;
  int32_t pad_;
};

struct OvlArgs {
  const OvlImage* images;
  const int64_t* row_begin;   // images + 1 entries: OvlImage::row0 of every image, then the number of rows
  const OvlPair* pairs;
  uint32_t* sig;              // rows x kOvlCells
  int64_t* edge;
  int64_t* cost;
  int32_t* flag;
  int32_t n_images, n_pairs;
};

constexpr int kOvlSigRows = 4;            // rows per signature workgroup (one per wave)
constexpr int kOvlCostKs = 4;             // k per cost workgroup (one per wave)
int launch_overlap_signatures(const OvlArgs& a, int64_t rows, void* stream);
int launch_overlap_edges(const OvlArgs& a, int max_l, void* stream);
// max_k: the largest kmax of the call; max_body: the largest body_b
int launch_overlap_costs(const OvlArgs& a, int max_k, int max_body, void* stream);

}  // namespace ist

#endif  // IST_OVERLAP_H_
