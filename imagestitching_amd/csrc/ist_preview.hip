// ist_preview.hip — the preview shrink for gfx950 (MI355X, CDNA4): a source-stationary box reduce.
//
// Stands in for the redraw that follows the export (reference: pages/index/index.js:1597-1603): the exported image drawn into the
// preview node, shrunk to fit.  The raster rule is IST_FILTER_AREA with integer edges on a fresh transparent canvas: a preview pixel
// is the overlap-weighted mean of the premultiplied source under its box of kx x ky source pixels (kx = w / pw, ky = h / ph, both
// > 1 here; every other draw takes the job path, ist_preview_host.cpp), rounded once, read back with straight alpha.
//
// The kernels of ist_kernels.hip are output-stationary: a thread owns canvas pixels and walks their footprints.  A preview turns
// that inside out - a few thousand output pixels, each under thousands of source pixels - so the work here is laid out over the
// SOURCE, and its time follows 4 * w * h whatever the ratio:
//
//   stage 1   one 256-thread workgroup per (output row Y, row chunk c, group g of J neighbouring output pixels).
//             It reads rows [iy0 + c * RC, iy0 + (c + 1) * RC) of the row's box over the group's x footprint: lane = 4 neighbouring
//             source pixels (one 16-byte load), 256 source pixels per wave, wave v the rows v, v + 4, ...; every row is weighted by its
//             overlap with the box.  The four waves' column sums meet in LDS; then SUB lanes per output pixel (a power of two that
//             covers the box) sum the pixel's columns with the columns' overlap weights and fold over a fixed xor tree.
//             One float4 per (Y, c, X) goes to scratch with a plain store.  A footprint wider than 256 columns (J = 1) is walked
//             in passes.  Only the rows and columns that two boxes share are read twice.
//   stage 2   one thread per output pixel: adds its C partial sums in chunk order, normalises, rounds once, un-premultiplies, stores.
//
// No atomics: every sum has one owner and a fixed order, so the same input gives the same bytes.  The sums are hierarchical
// (at most RC / 4 rows per lane, four waves, a tree over the columns, C chunks): integer-valued until the fractional end weights
// come in, so that a box of 705 600 taps keeps its mean to well under an LSB where one running fp32 sum loses half of one.
// Weights, clamping and rounding are those of the area branch of tile_area_stream (opaque) and pixel_general (ist_kernels.hip).
// Both stages are __device__ bodies of a PreviewArgs: the single-image kernels run one reduce per launch, their batch twins (the
// thumbnails of a grid of images, ist_thumbs.cpp) many - each workgroup looks its item up first - and stage 2 of a twin stores the
// pixel where the item's turn (mirrors, transposition: an EXIF orientation) puts it.
// Build: hipcc --offload-arch=gfx950 -ffp-contract=off (the fp64 coordinate math must not be fused).
#include <hip/hip_runtime.h>

#include <string>

#include "ist_internal.h"
#include "ist_launch.h"

namespace ist {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_a4 __attribute__((aligned(4)));   // RGBA rows are only pixel (4-byte) aligned in general
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define IST_DEV static __device__ __forceinline__

IST_DEV int clamp_int(double v) { return static_cast<int>(fmin(fmax(v, -2.0e9), 2.0e9)); }

// one source axis of one output coordinate: the box [lo, hi) and the source indices it touches, clipped to the source
// (a box that overhangs the source by a rounding error would put that sliver on the edge pixel: dropped, it is < 1e-9 of a pixel)
struct Box { double lo, hi; int i0, i1; };
IST_DEV Box box_of(double k, int out, int n) {
  Box b;
  const double c = k * (static_cast<double>(out) + 0.5);
  b.lo = c - 0.5 * k; b.hi = c + 0.5 * k;
  b.i0 = max(clamp_int(floor(b.lo)), 0);
  b.i1 = min(clamp_int(ceil(b.hi)) - 1, n - 1);
  return b;
}
IST_DEV float overlap(const Box& b, int i) {
  return static_cast<float>(fmin(static_cast<double>(i) + 1.0, b.hi) - fmax(static_cast<double>(i), b.lo));
}

template <bool OPAQUE>
IST_DEV void add_px(f32x4& acc, uint32_t px, float wy) {
  f32x4 v = {static_cast<float>(px & 0xFFu), static_cast<float>((px >> 8) & 0xFFu), static_cast<float>((px >> 16) & 0xFFu), 0.f};
  if (!OPAQUE) { const float a = static_cast<float>(px >> 24); v = v * a; v.w = a; }
  acc += v * wy;
}

// stage 1 of one reduce: workgroup `id` of its groups * chunks * ph
template <bool OPAQUE>
IST_DEV void preview_partial(const PreviewArgs& A, const int64_t id) {
  __shared__ f32x4 wave_sum[4][256];     // per wave: the column sums of its rows
  __shared__ f32x4 col_sum[256];         // the four waves together
  const int tid = static_cast<int>(threadIdx.x);
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // workgroup -> (Y, c, g), g fastest: neighbours in the grid read neighbouring columns of the same rows
  const int g = static_cast<int>(id % A.groups);
  const int64_t yc = id / A.groups;
  const int c = static_cast<int>(yc % A.chunks);
  const int Y = static_cast<int>(yc / A.chunks);
  const Box by = box_of(A.ky, Y, A.h);
  const int ra = by.i0 + c * A.chunk_rows, rb = min(ra + A.chunk_rows - 1, by.i1);     // this chunk's rows (none: rb < ra)
  const int X0 = g * A.per_group, X1 = min(X0 + A.per_group, A.pw);
  const int fx0 = box_of(A.kx, X0, A.w).i0, fx1 = box_of(A.kx, X1 - 1, A.w).i1;         // the group's x footprint
  f32x4* part = reinterpret_cast<f32x4*>(A.partial) + (static_cast<int64_t>(Y) * A.chunks + c) * A.pw;
  const int sub = tid & (A.sub - 1), per_round = 256 / A.sub;
  f32x4 carried = {0.f, 0.f, 0.f, 0.f};   // (passes > 1: the one output pixel's sum so far, in the lanes that own it)
  for (int p = 0; p < A.passes; ++p) {
    const int cbase = fx0 + 256 * p;
    // ---- rows: lane = 4 source pixels, wave = every fourth row of the chunk, four rows in flight per lane
    const int xx = cbase + 4 * lane;
    const bool whole = xx + 3 <= A.w - 1 && xx <= fx1;      // (beyond fx1 nothing is needed; beyond w nothing may be read)
    f32x4 acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    const uint8_t* col = A.src + static_cast<size_t>(min(xx, A.w - 1)) * 4;
    for (int y = ra + wave; y <= rb; y += 16) {
      u32x4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (y + 4 * u > rb) break;                          // (wave-uniform)
        const uint8_t* r = col + static_cast<size_t>(y + 4 * u) * A.src_pitch;
        if (whole) v[u] = *reinterpret_cast<const u32x4_a4*>(r);
        else {                                              // the source's right edge, or columns nobody sums: pixel by pixel
          v[u].x = xx <= fx1 ? *reinterpret_cast<const uint32_t*>(r) : 0u;
          v[u].y = xx + 1 <= fx1 ? *reinterpret_cast<const uint32_t*>(r + 4) : 0u;
          v[u].z = xx + 2 <= fx1 ? *reinterpret_cast<const uint32_t*>(r + 8) : 0u;
          v[u].w = xx + 3 <= fx1 ? *reinterpret_cast<const uint32_t*>(r + 12) : 0u;
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (y + 4 * u > rb) break;
        const float wy = overlap(by, y + 4 * u);
        add_px<OPAQUE>(acc[0], v[u].x, wy); add_px<OPAQUE>(acc[1], v[u].y, wy);
        add_px<OPAQUE>(acc[2], v[u].z, wy); add_px<OPAQUE>(acc[3], v[u].w, wy);
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) wave_sum[wave][4 * lane + q] = acc[q];
    __syncthreads();
    col_sum[tid] = (wave_sum[0][tid] + wave_sum[1][tid]) + (wave_sum[2][tid] + wave_sum[3][tid]);
    __syncthreads();
    // ---- columns: A.sub lanes per output pixel, per_round pixels at a time
    for (int j0 = 0; j0 < X1 - X0; j0 += per_round) {
      const int X = X0 + j0 + tid / A.sub;
      f32x4 s = {0.f, 0.f, 0.f, 0.f};
      if (X < X1) {
        const Box bx = box_of(A.kx, X, A.w);
        const int hi = min(bx.i1, cbase + 255);
        for (int i = max(bx.i0, cbase) + sub; i <= hi; i += A.sub) s += col_sum[i - cbase] * overlap(bx, i);
      }
      for (int m = A.sub >> 1; m >= 1; m >>= 1) {           // (the same tree for every pixel: the order of the sum is fixed)
        s.x += __shfl_xor(s.x, m); s.y += __shfl_xor(s.y, m); s.z += __shfl_xor(s.z, m); s.w += __shfl_xor(s.w, m);
      }
      if (A.passes > 1) carried += s;
      else if (X < X1 && sub == 0) part[X] = s;
    }
    // (the next pass writes wave_sum only after every wave has passed the second barrier above, and col_sum only after the first
    // barrier of that pass, which no wave reaches before it has finished reading here)
  }
  if (A.passes > 1 && tid == 0) part[X0] = carried;        // (passes > 1 only with one output pixel per group)
}

// round half up to a byte (v in [0, 255]: to_u8 of ist_kernels.hip)
IST_DEV uint32_t to_u8(float v) { return static_cast<uint32_t>(v + 0.5f); }

// stage 2 of one reduce: thread `idx` of its pw * ph (or beyond them: nothing).  turn: where the pixel is stored (ist_launch.h)
template <bool OPAQUE>
IST_DEV void preview_finish(const PreviewArgs& A, const int64_t idx, const int turn) {
  if (idx >= static_cast<int64_t>(A.pw) * A.ph) return;
  const int X = static_cast<int>(idx % A.pw), Y = static_cast<int>(idx / A.pw);
  const f32x4* part = reinterpret_cast<const f32x4*>(A.partial) + static_cast<int64_t>(Y) * A.chunks * A.pw + X;
  f32x4 s = part[0];
  for (int c = 1; c < A.chunks; ++c) s += part[static_cast<int64_t>(c) * A.pw];
  uint32_t o;
  if (OPAQUE) {                                             // the mean replaces the (transparent) canvas: tile_area_stream
    const float normf = static_cast<float>(1.0 / (A.kx * A.ky));
    o = 0xFF000000u | to_u8(fminf(s.x * normf, 255.f)) | (to_u8(fminf(s.y * normf, 255.f)) << 8) | (to_u8(fminf(s.z * normf, 255.f)) << 16);
  } else {                                                  // premultiplied mean over nothing, one rounding, straight-alpha readback: pixel_general
    const double norm = 1.0 / (A.kx * A.ky);
    const uint32_t a = static_cast<uint32_t>(fmin(fmax(floor(static_cast<double>(s.w) * norm + 0.5), 0.0), 255.0));
    const uint32_t r = static_cast<uint32_t>(fmin(fmax(floor(static_cast<double>(s.x) * norm / 255.0 + 0.5), 0.0), 255.0));
    const uint32_t gg = static_cast<uint32_t>(fmin(fmax(floor(static_cast<double>(s.y) * norm / 255.0 + 0.5), 0.0), 255.0));
    const uint32_t b = static_cast<uint32_t>(fmin(fmax(floor(static_cast<double>(s.z) * norm / 255.0 + 0.5), 0.0), 255.0));
    if (a == 255u) o = r | (gg << 8) | (b << 16) | 0xFF000000u;
    else if (a == 0u) o = 0u;
    else o = min(255u, (r * 255u + a / 2u) / a) | (min(255u, (gg * 255u + a / 2u) / a) << 8) | (min(255u, (b * 255u + a / 2u) / a) << 16) | (a << 24);
  }
  const int Xf = (turn & kTurnFlipX) ? A.pw - 1 - X : X, Yf = (turn & kTurnFlipY) ? A.ph - 1 - Y : Y;
  const int col = (turn & kTurnTranspose) ? Yf : Xf, row = (turn & kTurnTranspose) ? Xf : Yf;
  *reinterpret_cast<uint32_t*>(A.dst + static_cast<size_t>(row) * A.dst_pitch + static_cast<size_t>(col) * 4) = o;
}

template <bool OPAQUE>
__global__ __launch_bounds__(256) void ist_preview_partial_kernel(const PreviewArgs A) {
  preview_partial<OPAQUE>(A, static_cast<int64_t>(blockIdx.x));
}

template <bool OPAQUE>
__global__ __launch_bounds__(256) void ist_preview_finish_kernel(const PreviewArgs A) {
  preview_finish<OPAQUE>(A, static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x, 0);
}

// ------------------------------------------------------------------------------------------------ batch
// Many reduces in one launch per stage (ist_thumbs_device): the workgroups of all items are numbered item-major, a workgroup finds its
// item by binary search over the items' first workgroups (stage 2: their first threads, whole workgroups each) and runs the body
// above on that item's PreviewArgs.  The lookup is wave-uniform; the tables are read through the constant address space, so the
// item's arguments arrive in scalar registers as a kernarg PreviewArgs does.
typedef const __attribute__((address_space(4))) PreviewArgs ConstPreviewArgs;
typedef const __attribute__((address_space(4))) int64_t ConstI64;

IST_DEV int batch_item_of(ConstI64* begin, int n, int64_t at) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {                                   // the last item whose first entry is <= at
    const int mid = (lo + hi + 1) >> 1;
    if (begin[mid] <= at) lo = mid; else hi = mid - 1;
  }
  return __builtin_amdgcn_readfirstlane(lo);
}

template <bool OPAQUE>
__global__ __launch_bounds__(256) void ist_preview_partial_batch_kernel(const PreviewBatchArgs B) {
  const int64_t wg = static_cast<int64_t>(blockIdx.x);
  ConstI64* begin = (ConstI64*)B.wg_begin;
  const int j = batch_item_of(begin, B.n, wg);
  const PreviewArgs& A = *(const PreviewArgs*)((ConstPreviewArgs*)B.items + j);
  preview_partial<OPAQUE>(A, wg - begin[j]);
}

template <bool OPAQUE>
__global__ __launch_bounds__(256) void ist_preview_finish_batch_kernel(const PreviewBatchArgs B) {
  const int64_t first = static_cast<int64_t>(blockIdx.x) * 256;
  ConstI64* begin = (ConstI64*)B.px_begin;
  const int j = batch_item_of(begin, B.n, first);
  const PreviewArgs& A = *(const PreviewArgs*)((ConstPreviewArgs*)B.items + j);
  preview_finish<OPAQUE>(A, first - begin[j] + threadIdx.x, A.turn);
}

}  // namespace

int launch_preview(const PreviewArgs& A, bool opaque, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t wgs = static_cast<int64_t>(A.groups) * A.chunks * A.ph;
  const int64_t fin = (static_cast<int64_t>(A.pw) * A.ph + 255) / 256;
  if (wgs > 2147483647ll || fin > 2147483647ll) return fail(IST_E_OUTPUT_SIZE, "preview too large for one launch");
  if (opaque) {
    hipLaunchKernelGGL(ist_preview_partial_kernel<true>, dim3(static_cast<unsigned>(wgs)), dim3(256), 0, s, A);
    hipLaunchKernelGGL(ist_preview_finish_kernel<true>, dim3(static_cast<unsigned>(fin)), dim3(256), 0, s, A);
  } else {
    hipLaunchKernelGGL(ist_preview_partial_kernel<false>, dim3(static_cast<unsigned>(wgs)), dim3(256), 0, s, A);
    hipLaunchKernelGGL(ist_preview_finish_kernel<false>, dim3(static_cast<unsigned>(fin)), dim3(256), 0, s, A);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(IST_E_HIP, std::string("preview launch failed: ") + hipGetErrorString(e));
  return IST_OK;
}

int launch_preview_batch(const PreviewBatchArgs& B, int64_t n_wgs, int64_t n_px, bool opaque, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t fin = (n_px + 255) / 256;
  if (n_wgs < 1 || fin < 1 || n_wgs > 2147483647ll || fin > 2147483647ll) return fail(IST_E_OUTPUT_SIZE, "thumbnails too large for one launch");
  if (opaque) {
    hipLaunchKernelGGL(ist_preview_partial_batch_kernel<true>, dim3(static_cast<unsigned>(n_wgs)), dim3(256), 0, s, B);
    hipLaunchKernelGGL(ist_preview_finish_batch_kernel<true>, dim3(static_cast<unsigned>(fin)), dim3(256), 0, s, B);
  } else {
    hipLaunchKernelGGL(ist_preview_partial_batch_kernel<false>, dim3(static_cast<unsigned>(n_wgs)), dim3(256), 0, s, B);
    hipLaunchKernelGGL(ist_preview_finish_batch_kernel<false>, dim3(static_cast<unsigned>(fin)), dim3(256), 0, s, B);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(IST_E_HIP, std::string("thumbnail launch failed: ") + hipGetErrorString(e));
  return IST_OK;
}

}  // namespace ist
