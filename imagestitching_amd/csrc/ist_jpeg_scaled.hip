// ist_jpeg_scaled.hip — reduced-size JPEG reconstruction on gfx950: a file decoded at 1/2, 1/4 or 1/8 of its natural size from the SAME
// coefficient planes the full-size kernels (ist_jpeg_kernels.hip) read.  Reference anchor: the decoded bitmap that is smaller than the
// image (bmp.width / bmp.height against width / height, pages/index/index.js:1522-1523).
//
// The arithmetic is libjpeg-turbo's decode-to-scale (scale_num / scale_denom, what Pillow's Image.draft asks for), restated in
// include/imagestitch.h and tests/jpeg_scaled_reference.py: with N = 8 / denominator every component gets an S x S inverse DCT,
// S in {1, 2, 4, 8}, that reads the low frequencies of the 8 x 8 block (the reduced "slow" integer IDCTs: 13-bit constants, 2-bit
// pass-1 scaling); a component that is still coarser than the output is doubled along one axis by the triangle filter (h2v1 / h1v2)
// or, at 1/8 and for planes at most 2 samples wide, by replication; colour conversion is the full-size one.
//
// Two kernels.  ist_jpeg_scaled_idct_kernel<S> (S = 4, 2, 1) turns coefficient blocks into sample planes of pitch blocks_x * S;
// components with S = 8 (4:2:0 chroma at 1/2) go through ist_jpeg_idct_kernel of the full-size path.  ist_jpeg_scaled_planes_kernel
// turns the planes into RGBA8.  Luma goes through a plane here: it is at most a quarter of the pixels, and the coefficient reads
// (every block, whatever S) dominate the traffic.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstring>

#include "ist_internal.h"
#include "ist_jpeg.h"

namespace ist {

namespace {

std::atomic<int64_t> g_scaled_launches{0};

constexpr int fix(double x) { return static_cast<int>(x * 8192.0 + 0.5); }      // F(x) = round(8192 x)
constexpr int CONST_BITS = 13, PASS1_BITS = 2;

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// one 1-D pass of the 4-point reduced IDCT: in[4] is not read
__device__ __forceinline__ void idct4(const int in[8], int out[4], int shift) {
  const int t0 = in[0] << (CONST_BITS + 1);
  const int t2 = in[2] * fix(1.847759065) + in[6] * (-fix(0.765366865));
  const int t10 = t0 + t2, t12 = t0 - t2;
  const int z1 = in[7], z2 = in[5], z3 = in[3], z4 = in[1];
  const int o0 = z1 * (-fix(0.211164243)) + z2 * fix(1.451774981) + z3 * (-fix(2.172734803)) + z4 * fix(1.061594337);
  const int o2 = z1 * (-fix(0.509795579)) + z2 * (-fix(0.601344887)) + z3 * fix(0.899976223) + z4 * fix(2.562915447);
  out[0] = descale(t10 + o2, shift); out[3] = descale(t10 - o2, shift);
  out[1] = descale(t12 + o0, shift); out[2] = descale(t12 - o0, shift);
}
// the 2-point one: in[2], in[4], in[6] are not read
__device__ __forceinline__ void idct2(const int in[8], int out[2], int shift) {
  const int t10 = in[0] << (CONST_BITS + 2);
  const int t0 = in[7] * (-fix(0.720959822)) + in[5] * fix(0.850430095) + in[3] * (-fix(1.272758580)) + in[1] * fix(3.624509785);
  out[0] = descale(t10 + t0, shift); out[1] = descale(t10 - t0, shift);
}

// the lanes of a block hand their rows and columns to each other through LDS; they sit in one wave.  Nothing but this point
// orders a lane's reads behind the other lanes' writes (the compiler can prove that the addresses differ and would be free to
// move the reads up): a release / acquire pair at wave scope around a wave barrier, which costs no instruction.
__device__ __forceinline__ void wave_lds_order() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- coefficient blocks -> S x S samples per block ---------------------------------------------------------------------------
// S = 4, 2: 32 blocks per 256-thread workgroup, 8 lanes per block, as the full-size kernel lays them out.  Lane (b, i):
//   1. reads ROW i of its block with one 16-byte load (a wave reads eight whole blocks = 1 KiB contiguous), dequantises it and
//      writes it to the block's LDS image (72 dwords, element (y, x) at 9 y + x: rows and columns of the 32 lanes of an LDS
//      cycle fall on 32 different banks);
//   2. runs pass 1 on COLUMN i (it reads rows 0-3, 5-7 for S = 4 and 0, 1, 3, 5, 7 for S = 2) and writes the S results back to
//      rows 0 .. S-1 of the column; the columns pass 2 never reads (4; for S = 2 also 2 and 6) are computed and ignored;
//   3. lanes i < S run pass 2 on ROW i, level-shift, clamp and store S bytes of row i of the block.
// S = 1: a sample is DESCALE(dequantised DC, 3); one thread per block, 256 blocks per workgroup.
constexpr int kBlocks = 32, kPitch = 72, kComps = 18;
struct ScaledComp { const int16_t* coef; uint8_t* plane; int blocks_x, n_blocks; uint16_t q[64]; };
struct ScaledIdctArgs { ScaledComp comp[kComps]; int wg0[kComps + 1]; };      // wg0[c] = first workgroup of component c; wg0[n] = the grid

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <int S>
__global__ __launch_bounds__(256) void ist_jpeg_scaled_idct_kernel(const ScaledIdctArgs P) {
  const int wg = static_cast<int>(blockIdx.x), t = static_cast<int>(threadIdx.x);
  int ci = 0;
  while (ci + 1 < kComps && wg >= P.wg0[ci + 1]) ++ci;                      // (workgroup-uniform: scalar loads of the arguments)
  const ScaledComp& A = P.comp[ci];
  if constexpr (S == 1) {
    const int b = (wg - P.wg0[ci]) * 256 + t;
    if (b >= A.n_blocks) return;
    const int dc = static_cast<int>(A.coef[static_cast<size_t>(b) * 64]) * static_cast<int>(A.q[0]);
    A.plane[b] = static_cast<uint8_t>(clampi(descale(dc, 3) + 128, 0, 255));      // (pitch = blocks_x: sample (by, bx) is byte b)
    return;
  } else {
    __shared__ int ws[kBlocks * kPitch];
    __shared__ int q9[72];
    const int lb = t >> 3, i = t & 7;
    const int b = (wg - P.wg0[ci]) * kBlocks + lb;
    const bool live = b < A.n_blocks;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (live) v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(A.coef + static_cast<size_t>(b) * 64) + i);      // (read once)
    if (t < 64) q9[9 * (t >> 3) + (t & 7)] = A.q[t];
    __syncthreads();
    int* W = ws + lb * kPitch;
    {
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int x = 0; x < 8; ++x) {
        const int c = static_cast<int>(static_cast<int16_t>((w[x >> 1] >> (16 * (x & 1))) & 0xFFFFu));
        W[9 * i + x] = __mul24(c, q9[9 * i + x]);      // (int16 x uint16: exact in 24-bit operands)
      }
    }
    wave_lds_order();
    int in[8], o[4];
#pragma unroll
    for (int y = 0; y < 8; ++y) in[y] = (y == 4 || (S == 2 && (y == 2 || y == 6))) ? 0 : W[9 * y + i];
    if (S == 4) idct4(in, o, CONST_BITS - PASS1_BITS + 1); else idct2(in, o, CONST_BITS - PASS1_BITS + 2);
    // (a lane writes the column it has just read and no other: nothing to order between the two)
#pragma unroll
    for (int y = 0; y < S; ++y) W[9 * y + i] = o[y];
    wave_lds_order();
#pragma unroll
    for (int x = 0; x < 8; ++x) in[x] = (x == 4 || (S == 2 && (x == 2 || x == 6))) ? 0 : W[9 * (i & (S - 1)) + x];      // (lanes i >= S: a row of their own block again, result unused)
    if (S == 4) idct4(in, o, CONST_BITS + PASS1_BITS + 3 + 1); else idct2(in, o, CONST_BITS + PASS1_BITS + 3 + 2);
    if (!live || i >= S) return;
    const int by = b / A.blocks_x, bx = b - by * A.blocks_x;
    uint8_t* dst = A.plane + (static_cast<size_t>(by) * S + i) * (static_cast<size_t>(A.blocks_x) * S) + static_cast<size_t>(bx) * S;
    uint32_t r = 0u;
#pragma unroll
    for (int x = 0; x < S; ++x) r |= static_cast<uint32_t>(clampi(o[x] + 128, 0, 255)) << (8 * x);
    if (S == 4) *reinterpret_cast<uint32_t*>(dst) = r;                    // (the plane is 256-byte aligned, its pitch a multiple of 4)
    else *reinterpret_cast<uint16_t*>(dst) = static_cast<uint16_t>(r);    // (pitch a multiple of 2)
  }
}

// ---- sample planes -> RGBA8 ---------------------------------------------------------------------------------------------------
// A thread converts 4 pixels of one row: thread t of a 256-thread workgroup takes group t & 63 of row t >> 6 of a 256 x 4 pixel tile,
// so a wave writes 1 KiB of one bitmap row with 16-byte stores.  Component 0 always has the output's size; components 1 and 2
// (chroma, or G and B) have it too (ux = uy = 1: 4:4:4 and - the IDCT size makes up for the sampling - 4:2:0) or are half as wide
// (ux = 2, 4:2:2) or half as high (uy = 2, 4:4:0).  Every branch on the arguments is uniform over the launch.
enum { kGrey = 0, kYcc = 1, kRgb = 2 };
struct PlanesArgs {
  const uint8_t* p[3]; int pitch[3];
  int sw, sh;                      // output size = true size of plane 0
  int cw, ch;                      // true size of planes 1, 2
  int ux, uy;                      // 1 or 2, never both 2
  int fancy;                       // triangle filter (else replication) where ux or uy is 2
  int kind;
  uint8_t* out; size_t out_pitch;
};

// columns x0 .. x0+3 of a plane row as four bytes; columns past w - 1 repeat the last one (they are never shown).  A pitch that
// is a multiple of 4 lets the four come as one dword (x0 is a multiple of 4 and below w <= pitch, rows start 4-byte aligned).
__device__ __forceinline__ uint32_t row4(const uint8_t* row, int pitch, int x0, int w) {
  if ((pitch & 3) == 0) return *reinterpret_cast<const uint32_t*>(row + x0);
  uint32_t v = 0u;
#pragma unroll
  for (int k = 0; k < 4; ++k) v |= static_cast<uint32_t>(row[min(x0 + k, w - 1)]) << (8 * k);
  return v;
}

__device__ __forceinline__ uint32_t ycc_to_rgba(int Yv, int cb, int cr) {
  // 16-bit fixed point: FIX(1.40200)=91881, FIX(1.77200)=116130, FIX(0.71414)=46802, FIX(0.34414)=22554
  const int r = Yv + ((91881 * cr + 32768) >> 16);
  const int b = Yv + ((116130 * cb + 32768) >> 16);
  const int g = Yv + ((-22554 * cb + 32768 - 46802 * cr) >> 16);
  return static_cast<uint32_t>(clampi(r, 0, 255)) | (static_cast<uint32_t>(clampi(g, 0, 255)) << 8) |
         (static_cast<uint32_t>(clampi(b, 0, 255)) << 16) | 0xFF000000u;
}

// the four samples of plane pl (1 or 2) under pixels x0 .. x0+3 of row y, upsampled, as four bytes
__device__ __forceinline__ uint32_t upsampled4(const PlanesArgs& A, int pl, int x0, int y) {
  const uint8_t* P = A.p[pl];
  const size_t pitch = static_cast<size_t>(A.pitch[pl]);
  if (A.ux == 2) {                                  // h2v1: 3/4 nearer + 1/4 further column; a clamped neighbour reproduces the edge rule ((4 c + 1 or 2) >> 2 = c)
    const uint8_t* row = P + static_cast<size_t>(y) * pitch;
    const int i0 = x0 >> 1;
    int c[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) c[k] = row[clampi(i0 - 1 + k, 0, A.cw - 1)];      // columns i0-1 .. i0+2
    if (!A.fancy) return static_cast<uint32_t>(c[1]) * 0x0101u | static_cast<uint32_t>(c[2]) * 0x01010000u;
    return static_cast<uint32_t>((3 * c[1] + c[0] + 1) >> 2) | static_cast<uint32_t>((3 * c[1] + c[2] + 2) >> 2) << 8 |
           static_cast<uint32_t>((3 * c[2] + c[1] + 1) >> 2) << 16 | static_cast<uint32_t>((3 * c[2] + c[3] + 2) >> 2) << 24;
  }
  if (A.uy == 2) {                                  // h1v2: 3/4 nearer + 1/4 further row, rows clamped to the plane
    const int j = y >> 1;
    const uint32_t a = row4(P + static_cast<size_t>(j) * pitch, A.pitch[pl], x0, A.cw);
    if (!A.fancy) return a;
    const int jn = clampi((y & 1) ? j + 1 : j - 1, 0, A.ch - 1);
    const uint32_t f = row4(P + static_cast<size_t>(jn) * pitch, A.pitch[pl], x0, A.cw);
    const uint32_t rnd = (y & 1) ? 2u : 1u;
    uint32_t v = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) v |= ((3u * ((a >> (8 * k)) & 255u) + ((f >> (8 * k)) & 255u) + rnd) >> 2) << (8 * k);
    return v;
  }
  return row4(P + static_cast<size_t>(y) * pitch, A.pitch[pl], x0, A.cw);
}

__global__ __launch_bounds__(256) void ist_jpeg_scaled_planes_kernel(const PlanesArgs A) {
  const int t = static_cast<int>(threadIdx.x);
  const int x0 = (static_cast<int>(blockIdx.x) * 64 + (t & 63)) * 4, y = static_cast<int>(blockIdx.y) * 4 + (t >> 6);
  if (x0 >= A.sw || y >= A.sh) return;
  const uint32_t c0 = row4(A.p[0] + static_cast<size_t>(y) * static_cast<size_t>(A.pitch[0]), A.pitch[0], x0, A.sw);
  uint32_t px[4];
  if (A.kind == kGrey) {
#pragma unroll
    for (int k = 0; k < 4; ++k) px[k] = ((c0 >> (8 * k)) & 255u) * 0x010101u | 0xFF000000u;
  } else {
    const uint32_t c1 = upsampled4(A, 1, x0, y), c2 = upsampled4(A, 2, x0, y);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int a = static_cast<int>((c0 >> (8 * k)) & 255u), b = static_cast<int>((c1 >> (8 * k)) & 255u), c = static_cast<int>((c2 >> (8 * k)) & 255u);
      if (A.kind == kRgb) px[k] = static_cast<uint32_t>(a) | (static_cast<uint32_t>(b) << 8) | (static_cast<uint32_t>(c) << 16) | 0xFF000000u;
      else px[k] = ycc_to_rgba(a, b - 128, c - 128);
    }
  }
  uint8_t* o = A.out + static_cast<size_t>(y) * A.out_pitch + static_cast<size_t>(x0) * 4;
  const int nv = A.sw - x0;
  if (nv >= 4 && (reinterpret_cast<uintptr_t>(o) & 15) == 0) {
    uint4 v; v.x = px[0]; v.y = px[1]; v.z = px[2]; v.w = px[3];
    *reinterpret_cast<uint4*>(o) = v;
  } else {
    for (int k = 0; k < 4 && k < nv; ++k) *reinterpret_cast<uint32_t*>(o + 4 * k) = px[k];
  }
}

template <int S>
int launch_idct(const JpegDeviceJob& J, const int* sizes, hipStream_t stream) {
  ScaledIdctArgs a;
  std::memset(&a, 0, sizeof a);
  constexpr int per_wg = S == 1 ? 256 : kBlocks;
  int nc = 0, wgs = 0;
  for (int c = 0; c < J.ncomp; ++c) {
    const int n_blocks = J.blocks_x[c] * J.blocks_y[c];
    if (sizes[c] != S || n_blocks <= 0) continue;
    ScaledComp& C = a.comp[nc];
    a.wg0[nc] = wgs;
    C.coef = J.d_coef[c]; C.plane = J.d_plane[c]; C.blocks_x = J.blocks_x[c]; C.n_blocks = n_blocks;
    for (int q = 0; q < 64; ++q) C.q[q] = J.q_host[c] ? J.q_host[c][q] : 1;
    wgs += (n_blocks + per_wg - 1) / per_wg;
    ++nc;
  }
  if (nc == 0) return IST_OK;
  for (int c = nc; c <= kComps; ++c) a.wg0[c] = c == nc ? wgs : 0x7fffffff;
  hipLaunchKernelGGL(ist_jpeg_scaled_idct_kernel<S>, dim3(static_cast<unsigned>(wgs)), dim3(256), 0, stream, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(IST_E_HIP, std::string("JPEG reduced IDCT launch failed: ") + hipGetErrorString(e));
  g_scaled_launches.fetch_add(1, std::memory_order_relaxed);
  return IST_OK;
}

}  // namespace

int jpeg_launch_reconstruct_scaled(const JpegDeviceJob& J, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (J.denom != 2 && J.denom != 4 && J.denom != 8) return fail(IST_E_INVALID, "JPEG reduced reconstruction: the denominator is not 2, 4 or 8");
  if (J.ncomp != 1 && J.ncomp != 3) return fail(IST_E_UNSUPPORTED, "JPEG reduced reconstruction: 1 or 3 components");
  const int N = 8 / J.denom;
  int S[3] = {N, N, N};
  for (int c = 0; c < J.ncomp; ++c) S[c] = jpeg_scaled_idct_size(N, J.h[c], J.v[c], J.hmax, J.vmax);
  PlanesArgs pa;
  std::memset(&pa, 0, sizeof pa);
  jpeg_scaled_size(J.width, J.height, J.denom, &pa.sw, &pa.sh);
  pa.ux = pa.uy = 1;
  if (J.ncomp == 3) {
    // what the decoder takes (ist_jpeg.cpp): components 1 and 2 sampled 1 x 1, component 0 hmax x vmax
    if (S[1] != S[2] || S[0] != N) return fail(IST_E_UNSUPPORTED, "JPEG reduced reconstruction: unexpected sampling");
    pa.ux = J.hmax * N / (J.h[1] * S[1]); pa.uy = J.vmax * N / (J.v[1] * S[1]);
    if ((pa.ux != 1 && pa.ux != 2) || (pa.uy != 1 && pa.uy != 2) || (pa.ux == 2 && pa.uy == 2)) return fail(IST_E_UNSUPPORTED, "JPEG reduced reconstruction: unexpected sampling");
    pa.cw = static_cast<int>((static_cast<int64_t>(J.width) * J.h[1] * S[1] + J.hmax * 8 - 1) / (J.hmax * 8));
    pa.ch = static_cast<int>((static_cast<int64_t>(J.height) * J.v[1] * S[1] + J.vmax * 8 - 1) / (J.vmax * 8));
    // libjpeg drops the triangle filter when the smallest IDCT is 1 x 1; h2v1 replicates a plane at most 2 samples wide
    pa.fancy = N > 1 && !(pa.ux == 2 && pa.cw <= 2);
    if (S[1] == 8 && !J.chroma_done) {                 // the full-size chroma planes: the full-size launch
      const int rc = jpeg_launch_chroma_idct(&J, 1, stream_);
      if (rc) return rc;
    }
  }
  int rc = launch_idct<4>(J, S, stream);
  if (rc == IST_OK) rc = launch_idct<2>(J, S, stream);
  if (rc == IST_OK) rc = launch_idct<1>(J, S, stream);
  if (rc) return rc;
  for (int c = 0; c < J.ncomp; ++c) { pa.p[c] = J.d_plane[c]; pa.pitch[c] = J.blocks_x[c] * S[c]; }
  pa.kind = J.ncomp == 1 ? kGrey : (J.rgb ? kRgb : kYcc);
  pa.out = J.out; pa.out_pitch = J.out_pitch;
  const dim3 grid(static_cast<unsigned>((pa.sw + 255) / 256), static_cast<unsigned>((pa.sh + 3) / 4));
  hipLaunchKernelGGL(ist_jpeg_scaled_planes_kernel, grid, dim3(256), 0, stream, pa);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(IST_E_HIP, std::string("JPEG reduced reconstruct launch failed: ") + hipGetErrorString(e));
  return IST_OK;
}

}  // namespace ist

extern "C" int64_t ist_debug_jpeg_scaled_launches(void) { return ist::g_scaled_launches.load(std::memory_order_relaxed); }
