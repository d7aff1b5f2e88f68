// ist_overlap.hip — the overlap search between neighbouring screenshots for gfx950 (MI355X, CDNA4).  The contract is stated in
// include/imagestitch.h ("overlap removal for scrolled screenshots"); everything here is integer, so no sum depends on its order.
//
//   signatures  ONE launch for all images of a call: one wave per image row (four rows per 256-thread workgroup; a wave finds its image
//               by binary search over the images' first rows).  Lane = 4 neighbouring pixels, one 16-byte load, 256 pixels per wave and
//               step, four steps in flight.  A pixel's cell is floor((32 x + 31) / w) - the c with e(c) <= x < e(c + 1) - found once
//               per load when its four pixels share a cell, per pixel otherwise; the values meet in the wave's 32 LDS counters
//               (integer adds), which lanes 0..31 store as the row's 128 bytes.  Every pixel is read once: the time is the bytes'.
//   edges       one thread per (pair, row counted from the top or from the bottom): D of the two rows, 2 x 128 bytes of the table.
//   costs       one wave per (pair, k): lane r, r + 64, ... adds D(A row hA - F - k + r, B row H + r), the wave folds the 64 sums.
//               Behind the k-workgroups of a pair come the workgroups of B's informative flags, one thread per body row.
// LDS: 512 bytes (signatures); no private segment; nothing is allocated or waited for here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "ist_overlap.h"

namespace ist {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_a4 __attribute__((aligned(4)));   // RGBA rows are only pixel (4-byte) aligned in general

#define IST_DEV static __device__ __forceinline__

typedef const __attribute__((address_space(4))) OvlImage ConstOvlImage;
typedef const __attribute__((address_space(4))) OvlPair ConstOvlPair;
typedef const __attribute__((address_space(4))) int64_t ConstI64;

IST_DEV uint32_t value_of(uint32_t px) { return (px & 0xFFu) + 2u * ((px >> 8) & 0xFFu) + ((px >> 16) & 0xFFu); }
IST_DEV uint32_t cell_of(uint32_t x, uint32_t w) { return (32u * x + 31u) / w; }

__global__ __launch_bounds__(256) void ist_overlap_signature_kernel(const OvlArgs A, const int64_t rows) {
  __shared__ uint32_t bins[kOvlSigRows][kOvlCells];
  const int tid = static_cast<int>(threadIdx.x);
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t g = static_cast<int64_t>(blockIdx.x) * kOvlSigRows + wave;      // this wave's row of the table
  if (lane < kOvlCells) bins[wave][lane] = 0u;
  __syncthreads();
  if (g < rows) {                                             // (wave-uniform)
    ConstI64* begin = (ConstI64*)A.row_begin;
    int lo = 0, hi = A.n_images - 1;
    while (lo < hi) {                                         // the last image whose first row is <= g
      const int mid = (lo + hi + 1) >> 1;
      if (begin[mid] <= g) lo = mid; else hi = mid - 1;
    }
    const int j = __builtin_amdgcn_readfirstlane(lo);
    const OvlImage& im = *(const OvlImage*)((ConstOvlImage*)A.images + j);
    const uint32_t w = static_cast<uint32_t>(im.w);
    const uint8_t* row = im.src + static_cast<size_t>(g - im.row0) * im.pitch;
    const uint32_t chunks = (w + 3u) >> 2;
    for (uint32_t c0 = 0; c0 < chunks; c0 += 256u) {
      u32x4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const uint32_t x = 4u * (c0 + 64u * u + lane);
        v[u] = u32x4{0u, 0u, 0u, 0u};
        if (x + 3u < w) v[u] = *reinterpret_cast<const u32x4_a4*>(row + static_cast<size_t>(x) * 4);
        else {                                                // the row's right edge: nothing behind it may be read
          if (x < w) v[u].x = *reinterpret_cast<const uint32_t*>(row + static_cast<size_t>(x) * 4);
          if (x + 1u < w) v[u].y = *reinterpret_cast<const uint32_t*>(row + static_cast<size_t>(x) * 4 + 4);
          if (x + 2u < w) v[u].z = *reinterpret_cast<const uint32_t*>(row + static_cast<size_t>(x) * 4 + 8);
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const uint32_t x = 4u * (c0 + 64u * u + lane);
        if (x >= w) continue;
        const uint32_t a = value_of(v[u].x), b = value_of(v[u].y), c = value_of(v[u].z), d = value_of(v[u].w);
        const uint32_t first = cell_of(x, w);
        if (x + 3u < w && cell_of(x + 3u, w) == first) atomicAdd(&bins[wave][first], a + b + c + d);
        else {
          atomicAdd(&bins[wave][first], a);
          if (x + 1u < w) atomicAdd(&bins[wave][cell_of(x + 1u, w)], b);
          if (x + 2u < w) atomicAdd(&bins[wave][cell_of(x + 2u, w)], c);
          if (x + 3u < w) atomicAdd(&bins[wave][cell_of(x + 3u, w)], d);
        }
      }
    }
  }
  __syncthreads();
  if (g < rows && lane < kOvlCells) A.sig[g * kOvlCells + lane] = bins[wave][lane];
}

// D of two rows of the table.  (A row's sums add up to at most 1020 w and w <= 2^20 is the host's rule, so D fits 32 bits.)
IST_DEV uint32_t row_diff(const uint32_t* __restrict__ p, const uint32_t* __restrict__ q) {
  uint32_t s = 0u;
#pragma unroll
  for (int i = 0; i < kOvlCells / 4; ++i) {
    const u32x4 a = reinterpret_cast<const u32x4*>(p)[i], b = reinterpret_cast<const u32x4*>(q)[i];
    s += (a.x > b.x ? a.x - b.x : b.x - a.x) + (a.y > b.y ? a.y - b.y : b.y - a.y);
    s += (a.z > b.z ? a.z - b.z : b.z - a.z) + (a.w > b.w ? a.w - b.w : b.w - a.w);
  }
  return s;
}

__global__ __launch_bounds__(256) void ist_overlap_edge_kernel(const OvlArgs A) {
  const OvlPair& P = *(const OvlPair*)((ConstOvlPair*)A.pairs + blockIdx.y);
  const int t = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
  if (t >= 2 * P.L) return;
  const bool bottom = t >= P.L;
  const int y = bottom ? t - P.L : t;
  const int64_t ra = P.sig_a + (bottom ? P.ha - 1 - y : y), rb = P.sig_b + (bottom ? P.hb - 1 - y : y);
  A.edge[P.edge_at + t] = static_cast<int64_t>(row_diff(A.sig + ra * kOvlCells, A.sig + rb * kOvlCells));
}

__global__ __launch_bounds__(256) void ist_overlap_cost_kernel(const OvlArgs A, const int k_blocks) {
  const OvlPair& P = *(const OvlPair*)((ConstOvlPair*)A.pairs + blockIdx.y);
  if (P.L == 0) return;
  const int tid = static_cast<int>(threadIdx.x);
  if (static_cast<int>(blockIdx.x) < k_blocks) {
    const int lane = tid & 63;
    const int k = static_cast<int>(blockIdx.x) * kOvlCostKs + __builtin_amdgcn_readfirstlane(tid >> 6);
    if (k > P.kmax) return;                                   // (wave-uniform; kmax may be -1)
    const uint32_t* a = A.sig + (P.sig_a + (P.ha - P.F - k)) * kOvlCells;
    const uint32_t* b = A.sig + (P.sig_b + P.H) * kOvlCells;
    uint64_t s = 0;
    for (int r = lane; r < k; r += 64) s += row_diff(a + static_cast<int64_t>(r) * kOvlCells, b + static_cast<int64_t>(r) * kOvlCells);
    uint32_t lo = static_cast<uint32_t>(s), hi = static_cast<uint32_t>(s >> 32);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const uint64_t o = (static_cast<uint64_t>(__shfl_xor(hi, m)) << 32) | __shfl_xor(lo, m);
      s += o;
      lo = static_cast<uint32_t>(s); hi = static_cast<uint32_t>(s >> 32);
    }
    if (lane == 0) A.cost[P.cost_at + k] = static_cast<int64_t>(s);
  } else {
    const int r = (static_cast<int>(blockIdx.x) - k_blocks) * 256 + tid;
    if (r >= P.body_b - 1) return;
    const uint32_t* b = A.sig + (P.sig_b + P.H + r) * kOvlCells;
    A.flag[P.flag_at + r] = static_cast<int64_t>(row_diff(b, b + kOvlCells)) > P.T ? 1 : 0;
  }
}

int launched(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(IST_E_HIP, std::string(what) + " launch failed: " + hipGetErrorString(e));
  return IST_OK;
}

}  // namespace

int launch_overlap_signatures(const OvlArgs& a, int64_t rows, void* stream) {
  const int64_t wgs = (rows + kOvlSigRows - 1) / kOvlSigRows;
  if (wgs < 1 || wgs > 2147483647ll) return fail(IST_E_OUTPUT_SIZE, "overlap: too many rows for one launch");
  hipLaunchKernelGGL(ist_overlap_signature_kernel, dim3(static_cast<unsigned>(wgs)), dim3(256), 0, static_cast<hipStream_t>(stream), a, rows);
  return launched("overlap signature");
}

int launch_overlap_edges(const OvlArgs& a, int max_l, void* stream) {
  const unsigned gx = static_cast<unsigned>(std::max(1, (2 * max_l + 255) / 256));
  hipLaunchKernelGGL(ist_overlap_edge_kernel, dim3(gx, static_cast<unsigned>(a.n_pairs)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  return launched("overlap edge");
}

int launch_overlap_costs(const OvlArgs& a, int max_k, int max_body, void* stream) {
  const int k_blocks = (std::max(max_k, 0) + 1 + kOvlCostKs - 1) / kOvlCostKs;
  const int f_blocks = (std::max(max_body - 1, 0) + 255) / 256;
  hipLaunchKernelGGL(ist_overlap_cost_kernel, dim3(static_cast<unsigned>(k_blocks + f_blocks), static_cast<unsigned>(a.n_pairs)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), a, k_blocks);
  return launched("overlap cost");
}

}  // namespace ist
