// ist_color.hip — a decoded bitmap through the tables of its ICC profile to sRGB, in place, for gfx950 (MI355X, CDNA4).  The contract is
// stated in include/imagestitch.h ("colour profiles"); everything here is integer, so the bytes are those of tests/icc_reference.py.
//
//   One launch per image over a w x h box of RGBA8 at any pitch.  A workgroup of 256 threads owns kColorRows rows x 1024 pixels.  A row's
//   base is only pixel (4-byte) aligned - the file pipeline reconstructs some images straight into their box of the canvas, which
//   begins at any X0 - so every row is cut at its own 16-byte boundaries: up to 3 head pixels, nb groups of 4 pixels that one lane
//   moves with one 16-byte load and one 16-byte store, up to 3 tail pixels.  Item t < nb of a row is group t; item nb is the row's
//   head and tail, pixel by pixel.  Nothing outside the box is read or written.
//   Tables in LDS, 19 KiB: dec[3][256] widened to a dword per entry (the bank of a code v is v mod 32, whatever the channel), from
//   the launch's by-value argument; enc[4096], a dword per 16 linear values, from a constant of the module: the code count c at the
//   bucket's first value in the low byte and the next threshold T[c + 1] above it (65536 behind the last).  No two thresholds
//   share a bucket (the narrowest step is 19), so the count of o is c + (o >= next): one LDS read per channel instead of a search.
//   The lookups are data-dependent; neighbouring lanes hold neighbouring pixels, whose codes are mostly close (same dword: broadcast).
//   The matrix is wave-uniform (scalar registers); 64-bit sums by v_mad_i64_i32.
// LDS: 19456 bytes; no private segment; nothing is allocated or waited for here.
#include <hip/hip_runtime.h>

#include <atomic>
#include <string>

#include "ist_icc.h"
#include "ist_internal.h"

namespace ist {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

#define IST_DEV static __device__ __forceinline__

constexpr int kColorRows = 16;               // rows per workgroup
constexpr int kColorThreads = 256;           // items (16-byte groups) of a row per workgroup
constexpr int kColorFlight = 2;              // rows whose loads a lane has in flight

struct alignas(16) EncTable { uint32_t v[4096]; };
constexpr EncTable make_enc() {
  EncTable t{};
  uint32_t c = 0;
  for (uint32_t k = 0; k < 4096; ++k) {
    while (c < 255 && kSrgbEncodeT[c + 1] <= 16u * k) ++c;
    const uint32_t next = c < 255 ? kSrgbEncodeT[c + 1] : 65536u;
    t.v[k] = c | (next << 8);
  }
  return t;
}
__device__ const EncTable kEnc = make_enc();

struct ColorArgs {
  uint8_t* px;
  size_t pitch;
  int32_t w, h;
  ist_color_tables t;
};

IST_DEV uint32_t encode(const uint32_t* enc, int64_t s) {
  s >>= 16;
  const uint32_t o = s < 0 ? 0u : s > 65535 ? 65535u : static_cast<uint32_t>(s);
  const uint32_t e = enc[o >> 4];
  return (e & 255u) + (o >= (e >> 8) ? 1u : 0u);
}

IST_DEV uint32_t convert(uint32_t p, const uint32_t* dec, const uint32_t* enc, const ColorArgs& A) {
  const int32_t r = static_cast<int32_t>(dec[p & 255u]), g = static_cast<int32_t>(dec[256u + ((p >> 8) & 255u)]),
                b = static_cast<int32_t>(dec[512u + ((p >> 16) & 255u)]);
  uint32_t out = p & 0xFF000000u;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int64_t s = static_cast<int64_t>(A.t.mq[i][0]) * r + static_cast<int64_t>(A.t.mq[i][1]) * g + static_cast<int64_t>(A.t.mq[i][2]) * b + 32768;
    out |= encode(enc, s) << (8 * i);
  }
  return out;
}

__global__ __launch_bounds__(kColorThreads) void ist_color_convert_kernel(const ColorArgs A) {
  __shared__ uint32_t enc[4096];
  __shared__ uint32_t dec[768];
  const int tid = static_cast<int>(threadIdx.x);
#pragma unroll
  for (int j = 0; j < 4; ++j) reinterpret_cast<u32x4*>(enc)[tid + kColorThreads * j] = reinterpret_cast<const u32x4*>(kEnc.v)[tid + kColorThreads * j];
#pragma unroll
  for (int c = 0; c < 3; ++c) dec[256 * c + tid] = A.t.dec[c][tid];
  __syncthreads();
  const uint32_t item = blockIdx.y * kColorThreads + static_cast<uint32_t>(tid);
  const uint32_t y0 = blockIdx.x * kColorRows;
  const uint32_t w = static_cast<uint32_t>(A.w), h = static_cast<uint32_t>(A.h);
  for (uint32_t dy = 0; dy < kColorRows; dy += kColorFlight) {
    u32x4 v[kColorFlight];
    uint8_t* at[kColorFlight];
#pragma unroll
    for (int u = 0; u < kColorFlight; ++u) {                 // the loads of kColorFlight rows go out before the first conversion
      at[u] = nullptr;
      const uint32_t y = y0 + dy + u;
      if (y >= h) continue;
      uint8_t* row = A.px + static_cast<size_t>(y) * A.pitch;
      const uint32_t head = min(w, ((16u - (static_cast<uint32_t>(reinterpret_cast<uintptr_t>(row)) & 15u)) & 15u) >> 2);
      const uint32_t nb = (w - head) >> 2;
      if (item < nb) {
        at[u] = row + static_cast<size_t>(head + 4u * item) * 4;
        v[u] = *reinterpret_cast<const u32x4*>(at[u]);
      } else if (item == nb) {                             // the row's head and tail (at most 6 pixels), pixel by pixel
        const uint32_t edge = w - 4u * nb;
        for (uint32_t k = 0; k < edge; ++k) {
          uint32_t* q = reinterpret_cast<uint32_t*>(row) + (k < head ? k : 4u * nb + k);
          *q = convert(*q, dec, enc, A);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kColorFlight; ++u) {
      if (!at[u]) continue;
      u32x4 o;
      o.x = convert(v[u].x, dec, enc, A); o.y = convert(v[u].y, dec, enc, A);
      o.z = convert(v[u].z, dec, enc, A); o.w = convert(v[u].w, dec, enc, A);
      *reinterpret_cast<u32x4*>(at[u]) = o;
    }
  }
}

std::atomic<int64_t> g_color_launches{0};

}  // namespace

int launch_color_convert(uint8_t* px, size_t pitch, int64_t w, int64_t h, const ist_color_tables& t, void* stream) {
  const int64_t bands = (h + kColorRows - 1) / kColorRows;
  const int64_t chunks = (w / 4 + 1 + kColorThreads - 1) / kColorThreads;      // items of a row: at most w / 4 groups + the edge item
  if (bands < 1 || bands > 2147483647ll || chunks < 1 || chunks > 65535 || w > 2147483647ll || h > 2147483647ll)
    return fail(IST_E_OUTPUT_SIZE, "colour conversion: the box is too large for one launch");
  ColorArgs a;
  a.px = px; a.pitch = pitch; a.w = static_cast<int32_t>(w); a.h = static_cast<int32_t>(h); a.t = t;
  hipLaunchKernelGGL(ist_color_convert_kernel, dim3(static_cast<unsigned>(bands), static_cast<unsigned>(chunks)), dim3(kColorThreads), 0,
                     static_cast<hipStream_t>(stream), a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(IST_E_HIP, std::string("colour conversion launch failed: ") + hipGetErrorString(e));
  g_color_launches.fetch_add(1, std::memory_order_relaxed);
  return IST_OK;
}

}  // namespace ist

extern "C" int64_t ist_debug_color_launches(void) { return ist::g_color_launches.load(std::memory_order_relaxed); }
