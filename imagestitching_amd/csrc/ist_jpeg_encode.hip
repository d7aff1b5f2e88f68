// ist_jpeg_encode.hip — the JPEG export: a baseline JFIF file of a canvas in HBM, transform and entropy code on the GPU.
//
// Reference anchor: the export seam, safeCanvasToTempFilePath(canvas, prefer) -> wx.canvasToTempFilePath({fileType: prefer})
// (utils/canvas.js:205-221); the page's other file producer, wx.compressImage (utils/canvas.js:262), writes JPEGs.  The file is
// pinned in integers by include/imagestitch.h ("export: baseline JPEG"); tests/jpeg_encode_reference.py states the same in numpy
// and the two must agree byte for byte.
//
// Decomposition (the one of ist_png_deflate.hip: independent units into bounded slots, an O(units) host layout, a gather):
//   * one restart interval = one MCU row: its DC predictors start at zero and it ends on a byte, so no interval needs another;
//   * transform kernel: a workgroup owns one 16x16 MCU (4:2:0) or four 8x8 MCUs (4:4:4) - one pixel per thread, read coordinates
//     clamped (that IS the edge padding) - converts, forms the 2x2 chroma means, runs both FDCT passes through LDS, quantises and
//     writes int16 coefficients, zig-zag order, blocks in coding order, to scratch;
//   * entropy kernel: a workgroup walks one interval in batches of 256 blocks, one block per lane: bits counted, block-wide scan,
//     codes OR-ed into a zeroed LDS image of the batch, then the batch's whole bytes are 0xFF-stuffed (a second scan, over the 0xFF
//     counts) into the interval's slot; the partial last byte carries into the next batch.  The DC predictor of a block is read
//     from the coefficient scratch (the previous block of its component), so nothing but that byte is carried;
//   * the host prefix-sums the interval lengths and a gather kernel copies every interval behind its RSTn marker.
// The canvas is encoded in slabs of MCU rows so that coefficients + slots stay within kBudget of the context's scratch.
//
// IST_JPEG_OPTIMIZE (the file's own Huffman tables) puts "whole file counted" in front of "first interval coded":
//   * histogram kernel: one wave per block, lane k = coefficient k; the ballot of the non-zero AC lanes is the block's run structure,
//     so every lane finds its own run/size symbol; counts go into a histogram per wave in LDS and from there, once per workgroup and
//     non-zero bin, into the file's 544 64-bit counters (integer adds commute: the counts do not depend on the order);
//   * the host builds the four tables from the counts (jpeg_enc_tables_optimal), writes the header from them and sends both up;
//   * the entropy kernel's wide instantiation (a DC code may be 16 bits: 1665 bits per block) codes with them.  It reports a symbol
//     without a code as an interval of length 0, which the host refuses.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "ist_ctx.h"
#include "ist_jpeg_enc.h"

namespace ist {

namespace {

std::atomic<int64_t> g_launches{0}, g_hist_launches{0};

// (the tables, the header and the geometry are host code without a device: ist_jpeg_enc.h)
constexpr size_t kBudget = kJpegEncBudget;
constexpr int kBlockBits = kJpegBlockBits;
constexpr int kBatch = 256;                // blocks per batch of the entropy kernel = its threads
constexpr int img_words(int block_bits) { return (7 + kBatch * block_bits + 31) / 32 + 2; }      // LDS bit image of a batch behind a carried partial byte
typedef JpegGeometry Geometry;
inline Geometry geometry(int64_t w, int64_t h, int subsampling) { return jpeg_geometry(w, h, subsampling); }

// ---- transform ---------------------------------------------------------------------------------------------------------
struct XformArgs {
  const uint8_t* canvas; size_t pitch; int32_t w, h;
  const JpegTables* tab;
  int16_t* coef;                 // the slab's blocks in coding order, 64 coefficients each (zig-zag order)
  int32_t mcus_x, mcu_row0, is420;
};

// T[u][x] of the contract: 2896 for u = 0, else sign * {4017, ...}[k - 1] with k = (2x+1) u mod 32 folded into the first quadrant
__device__ __forceinline__ int fdct_coef(int u, int x) {
  if (u == 0) return 2896;
  int k = ((2 * x + 1) * u) & 31, sign = 1;
  if (k > 16) k = 32 - k;
  if (k > 8) { k = 16 - k; sign = -1; }
  const int c = k == 1 ? 4017 : k == 2 ? 3784 : k == 3 ? 3406 : k == 4 ? 2896 : k == 5 ? 2276 : k == 6 ? 1567 : 799;
  return sign * c;
}

// one workgroup of the transform: MCUs [bx * (1 or 4), ...) of MCU row A.mcu_row0 + by; by counts from the first row of A.coef
__device__ __forceinline__ void jpeg_transform(const XformArgs& A, const int bx, const int by) {
  __shared__ int sT[64], sQ[128], sZ[64];
  __shared__ int sS[12 * 64], sR[12 * 64];        // level-shifted samples / row-pass results (later: the quantised blocks), block by block
  __shared__ int sC[2][256];                      // 4:2:0: full-resolution chroma of the MCU
  const int tid = threadIdx.x;
  if (tid < 64) { sT[tid] = fdct_coef(tid >> 3, tid & 7); sZ[tid] = A.tab->zz_of[tid]; }
  if (tid < 128) sQ[tid] = A.tab->q[tid >> 6][tid & 63];
  const int tw = A.is420 ? 16 : 32, sh = A.is420 ? 4 : 5;
  const int px = tid & (tw - 1), py = tid >> sh;
  const int64_t mcu_y = static_cast<int64_t>(A.mcu_row0) + by;
  const int x = min(bx * tw + px, A.w - 1);                 // (clamped reads: the edge padding)
  const int y = static_cast<int>(min(mcu_y * (A.is420 ? 16 : 8) + py, static_cast<int64_t>(A.h) - 1));
  const uint32_t p = *reinterpret_cast<const uint32_t*>(A.canvas + static_cast<size_t>(y) * A.pitch + 4 * static_cast<size_t>(x));
  const int R = p & 255u, G = (p >> 8) & 255u, B = (p >> 16) & 255u;                  // (alpha is not read)
  const int Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
  const int Cb = (-11059 * R - 21709 * G + 32768 * B + 8388608 + 32767) >> 16;
  const int Cr = (32768 * R - 27439 * G - 5329 * B + 8388608 + 32767) >> 16;
  const int in_block = (py & 7) * 8 + (px & 7);
  if (A.is420) {
    sS[((py >> 3) * 2 + (px >> 3)) * 64 + in_block] = Y - 128;
    sC[0][tid] = Cb; sC[1][tid] = Cr;
  } else {
    const int b = (px >> 3) * 3;
    sS[b * 64 + in_block] = Y - 128; sS[(b + 1) * 64 + in_block] = Cb - 128; sS[(b + 2) * 64 + in_block] = Cr - 128;
  }
  __syncthreads();
  if (A.is420 && tid < 128) {
    const int c = tid >> 6, i = tid & 63, at = (i >> 3) * 32 + (i & 7) * 2;
    sS[(4 + c) * 64 + i] = ((sC[c][at] + sC[c][at + 1] + sC[c][at + 16] + sC[c][at + 17] + 2) >> 2) - 128;
  }
  if (A.is420) __syncthreads();                   // (uniform)
  const int n = (A.is420 ? 6 : 12) * 64;
  for (int i = tid; i < n; i += 256) {            // rows: r[y][u] = (sum_x T[u][x] s[y][x] + 512) >> 10
    const int* s = sS + (i & ~7); const int* t = sT + (i & 7) * 8;
    int acc = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) acc += t[k] * s[k];
    sR[i] = (acc + 512) >> 10;
  }
  __syncthreads();
  for (int i = tid; i < n; i += 256) {            // columns: c[v][u] = (sum_y T[v][y] r[y][u] + 4096) >> 13, then the quantiser
    const int b = i >> 6, v = (i >> 3) & 7, u = i & 7;
    const int* r = sR + b * 64 + u; const int* t = sT + v * 8;
    int acc = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) acc += t[k] * r[8 * k];
    const int c = (acc + 4096) >> 13;
    const int comp = A.is420 ? (b >= 4) : (b % 3 != 0);
    const uint32_t q = static_cast<uint32_t>(sQ[comp * 64 + (i & 63)]);
    int k = static_cast<int>((static_cast<uint32_t>(c < 0 ? -c : c) + 4u * q) / (8u * q));
    if ((i & 63) != 0) k = min(k, 1023);
    sS[b * 64 + sZ[i & 63]] = c < 0 ? -k : k;     // (every thread has read its samples: two barriers ago)
  }
  __syncthreads();
  // the workgroup's blocks are consecutive in coding order: one run of 32-bit stores
  const int64_t mcu0 = static_cast<int64_t>(bx) * (A.is420 ? 1 : 4);
  const int mcus = static_cast<int>(min(static_cast<int64_t>(A.is420 ? 1 : 4), static_cast<int64_t>(A.mcus_x) - mcu0));
  const int words = mcus * (A.is420 ? 6 : 3) * 32;
  uint32_t* dst = reinterpret_cast<uint32_t*>(A.coef) + ((static_cast<int64_t>(by) * A.mcus_x + mcu0) * (A.is420 ? 6 : 3)) * 32;
  for (int i = tid; i < words; i += 256)
    dst[i] = (static_cast<uint32_t>(sS[2 * i]) & 0xFFFFu) | (static_cast<uint32_t>(sS[2 * i + 1]) << 16);
}

__global__ __launch_bounds__(256) void ist_jpeg_transform_kernel(const XformArgs A) {
  jpeg_transform(A, static_cast<int>(blockIdx.x), static_cast<int>(blockIdx.y));
}

// ---- entropy code ------------------------------------------------------------------------------------------------------
struct EntropyArgs {
  const int16_t* coef;
  const JpegTables* tab;
  uint8_t* slots;                // one per interval of the slab
  uint32_t* len;                 // per interval of the slab: bytes written
  int32_t row_blocks, bpm;
  int64_t slot;
};

// MSB-first bit writer into 32-bit words whose most significant byte is the first byte of the stream
struct BitWriter {
  uint32_t* w; unsigned long long acc; int n, wp;
  __device__ void init(uint32_t* words, int bitpos) { w = words; wp = bitpos >> 5; n = bitpos & 31; acc = 0; }
  __device__ void put(uint32_t v, int bits) {            // bits <= 27
    acc = (acc << bits) | v; n += bits;
    if (n >= 32) { n -= 32; atomicOr(&w[wp++], static_cast<uint32_t>(acc >> n)); acc &= (1ull << n) - 1ull; }
  }
  __device__ void flush() { if (n > 0 && acc) atomicOr(&w[wp], static_cast<uint32_t>(acc << (32 - n))); }
};

__device__ __forceinline__ int size_of(int a) { return a ? 32 - __clz(a) : 0; }      // a >= 0

// one block: its bit count (EMIT false) or its codes into the image.  c: 64 coefficients, zig-zag order, two per word
// GUARD (counting pass only): *bad becomes non-zero when the block holds a symbol that the tables have no code for
template <bool EMIT, bool GUARD = false>
__device__ __forceinline__ int code_block(const uint32_t (&c)[32], int diff, const uint32_t* dc, const uint32_t* ac, BitWriter* bw, int* bad = nullptr) {
  int bits;
  {
    const int s = size_of(diff < 0 ? -diff : diff);
    const uint32_t h = dc[s];
    if (GUARD) *bad |= h == 0u;
    bits = static_cast<int>(h >> 16) + s;
    if (EMIT) bw->put(((h & 0xFFFFu) << s) | (static_cast<uint32_t>(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1u)), bits);
  }
  int run = 0;
#pragma unroll
  for (int k = 1; k < 64; ++k) {
    int v = static_cast<int16_t>((k & 1) ? (c[k >> 1] >> 16) : (c[k >> 1] & 0xFFFFu));
    if (v == 0) { ++run; continue; }
    while (run >= 16) {                                   // ZRL
      const uint32_t z = ac[0xF0];
      if (GUARD) *bad |= z == 0u;
      bits += static_cast<int>(z >> 16);
      if (EMIT) bw->put(z & 0xFFFFu, static_cast<int>(z >> 16));
      run -= 16;
    }
    v = max(-1023, min(1023, v));                          // (the transform clamps already: this keeps the slot bound whatever the scratch holds)
    const int s = size_of(v < 0 ? -v : v);
    const uint32_t h = ac[run * 16 + s];
    if (GUARD) *bad |= h == 0u;
    const int l = static_cast<int>(h >> 16) + s;
    bits += l;
    if (EMIT) bw->put(((h & 0xFFFFu) << s) | (static_cast<uint32_t>(v < 0 ? v - 1 : v) & ((1u << s) - 1u)), l);
    run = 0;
  }
  if (run > 0) {                                           // EOB
    const uint32_t e = ac[0];
    if (GUARD) *bad |= e == 0u;
    bits += static_cast<int>(e >> 16);
    if (EMIT) bw->put(e & 0xFFFFu, static_cast<int>(e >> 16));
  }
  return bits;
}

__device__ __forceinline__ uint32_t img_byte(const uint32_t* img, int i) { return (img[i >> 2] >> (24 - 8 * (i & 3))) & 255u; }

// block-wide exclusive scan of one int per thread (256 threads); *total = the sum.  ws: 4 words of LDS nobody else touches
__device__ __forceinline__ int block_scan(int v, uint32_t* ws, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) { const int t = __shfl_up(incl, off); if (lane >= off) incl += t; }
  if (lane == 63) ws[wave] = static_cast<uint32_t>(incl);
  __syncthreads();
  int base = 0;
  for (int k = 0; k < wave; ++k) base += static_cast<int>(ws[k]);
  *total = static_cast<int>(ws[0] + ws[1] + ws[2] + ws[3]);
  return base + incl - v;
}

// one workgroup of the entropy coder: interval iv of A (its coefficients, its slot, its length).  BLOCK_BITS: the most bits of a
// block under the tables in use (it sizes the image); GUARD: the tables may lack a code (optimised tables): such an interval gets
// length 0
template <int BLOCK_BITS, bool GUARD>
__device__ __forceinline__ void jpeg_entropy(const EntropyArgs& A, const int iv) {
  __shared__ uint32_t img[img_words(BLOCK_BITS)];
  __shared__ uint32_t sDc[32], sAc[512];
  __shared__ uint32_t ws_bits[4], ws_ff[4];
  const int tid = threadIdx.x;
  if (tid < 32) sDc[tid] = A.tab->dc[tid >> 4][tid & 15];
  for (int i = tid; i < 512; i += 256) sAc[i] = A.tab->ac[i >> 8][i & 255];
  __syncthreads();
  const int16_t* coef = A.coef + static_cast<int64_t>(iv) * A.row_blocks * 64;
  uint8_t* slot = A.slots + static_cast<int64_t>(iv) * A.slot;
  int64_t out_pos = 0;
  int carry_bits = 0; uint32_t carry_val = 0;            // the partial last byte of the batches so far (its bits at the top of a byte)
  int bad = 0;
  for (int base = 0; base < A.row_blocks; base += kBatch) {
    const int j = base + tid;
    const bool on = j < A.row_blocks;
    const bool last = base + kBatch >= A.row_blocks;
    uint32_t c[32];
    int diff = 0, comp = 0;
    if (on) {
      const uint4* src = reinterpret_cast<const uint4*>(coef + static_cast<int64_t>(j) * 64);
#pragma unroll
      for (int q = 0; q < 8; ++q) { const uint4 v = src[q]; c[4 * q] = v.x; c[4 * q + 1] = v.y; c[4 * q + 2] = v.z; c[4 * q + 3] = v.w; }
      // the previous block of the same component in coding order (4:2:0: Y Y Y Y Cb Cr per MCU)
      const int pos = j % A.bpm;
      comp = A.bpm == 6 ? (pos >= 4) : (pos != 0);
      const int back = A.bpm == 3 ? 3 : (pos == 0 ? 3 : (pos < 4 ? 1 : 6));
      const int pred = j >= back ? coef[static_cast<int64_t>(j - back) * 64] : 0;
      diff = max(-2047, min(2047, static_cast<int>(static_cast<int16_t>(c[0] & 0xFFFFu)) - pred));
    } else {
#pragma unroll
      for (int q = 0; q < 32; ++q) c[q] = 0;
    }
    const uint32_t* dc = sDc + comp * 16; const uint32_t* ac = sAc + comp * 256;
    const int mybits = on ? code_block<false, GUARD>(c, diff, dc, ac, nullptr, &bad) : 0;
    int sum;
    const int start = carry_bits + block_scan(mybits, ws_bits, &sum);      // (its barrier: the last batch's image has been read by everybody)
    const int total = carry_bits + sum;
    const int pad = (last && (total & 7)) ? 8 - (total & 7) : 0;
    for (int i = tid; i < ((total + pad + 31) >> 5) + 1; i += 256) img[i] = 0;
    __syncthreads();
    if (tid == 0) {
      if (carry_bits) atomicOr(&img[0], carry_val << 24);
      if (pad) atomicOr(&img[total >> 5], ((1u << pad) - 1u) << (32 - (total & 31) - pad));     // the interval ends on a byte: 1 bits
    }
    if (on) { BitWriter bw; bw.init(img, start); code_block<true>(c, diff, dc, ac, &bw); bw.flush(); }
    __syncthreads();
    // the batch's whole bytes, each 0xFF followed by 0x00: thread t owns bytes [t * span, t * span + span)
    const int nb = (total + pad) >> 3;
    const int span = (((nb + 255) >> 8) + 3) & ~3;
    const int b0 = min(nb, tid * span), b1 = min(nb, b0 + span);
    int ff = 0;
    for (int i = b0; i < b1; ++i) ff += img_byte(img, i) == 255u;
    int ff_total;
    const int ff_before = block_scan(ff, ws_ff, &ff_total);
    int64_t at = out_pos + b0 + ff_before;
    for (int i = b0; i < b1; ++i) {
      const uint32_t v = img_byte(img, i);
      if (at < A.slot) slot[at] = static_cast<uint8_t>(v);
      ++at;
      if (v == 255u) { if (at < A.slot) slot[at] = 0; ++at; }
    }
    out_pos += nb + ff_total;
    carry_bits = (total + pad) & 7;
    carry_val = carry_bits ? (img_byte(img, nb) & (0xFF00u >> carry_bits) & 255u) : 0u;
  }
  if (GUARD) bad = __syncthreads_or(bad);
  if (tid == 0) A.len[iv] = bad ? 0u : static_cast<uint32_t>(min(out_pos, A.slot));
}

__global__ __launch_bounds__(256) void ist_jpeg_entropy_kernel(const EntropyArgs A) { jpeg_entropy<kBlockBits, false>(A, static_cast<int>(blockIdx.x)); }
// ... for files with optimised tables
__global__ __launch_bounds__(256) void ist_jpeg_entropy_wide_kernel(const EntropyArgs A) {
  jpeg_entropy<kJpegBlockBitsWide, true>(A, static_cast<int>(blockIdx.x));
}

// ---- symbol counts (IST_JPEG_OPTIMIZE) ---------------------------------------------------------------------------------
struct HistArgs {
  const int16_t* coef;           // the intervals of a slab, as the entropy kernel reads them
  int64_t* counters;             // the file's kJpegCounters counters
  int32_t row_blocks, bpm;
};
constexpr int kHistBlocks = 128;         // blocks of one workgroup: part `part` of an interval is its blocks [part * kHistBlocks, ...)
constexpr int kHistStep = 8;             // blocks a wave has in flight: its loads are issued before the first of them is counted

// one block by one wave: v = coefficient `lane` (zig-zag order), pred = the DC predictor (read by lane 0 only); h: the wave's own
// counters of the block's component (16 DC sizes, then 256 AC symbols)
__device__ __forceinline__ void count_block(int v, int pred, int lane, uint32_t* h) {
  const bool nz = lane > 0 && v != 0;
  const unsigned long long m = __ballot(nz);                 // bit k: AC coefficient k is not zero
  if (nz) {
    const unsigned long long lower = m & ((1ull << lane) - 1ull);
    const int prev = lower ? 63 - __clzll(lower) : 0;        // the non-zero coefficient before this one (0: the DC)
    const int run = lane - prev - 1;
    const int s = size_of(min(v < 0 ? -v : v, 1023));
    atomicAdd(&h[16 + (((run & 15) << 4) | s)], 1u);
    if (run >= 16) atomicAdd(&h[16 + 0xF0], static_cast<uint32_t>(run >> 4));      // ZRLs
  }
  if (lane == 0) {
    const int d = max(-2047, min(2047, v - pred));
    atomicAdd(&h[size_of(d < 0 ? -d : d)], 1u);
    if (!(m >> 63)) atomicAdd(&h[16], 1u);                   // EOB: the block ends in zeros
  }
}

// one workgroup of the histogram: part `part` of interval iv.  A wave takes kHistStep blocks (contiguous bytes) per step.
__device__ __forceinline__ void jpeg_histogram(const HistArgs& A, const int iv, const int part) {
  __shared__ uint32_t h[4][kJpegCounters];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b0 = part * kHistBlocks, b1 = min(A.row_blocks, b0 + kHistBlocks);
  if (b0 >= A.row_blocks) return;                            // (uniform)
  for (int i = tid; i < 4 * kJpegCounters; i += 256) (&h[0][0])[i] = 0;
  __syncthreads();
  const int16_t* coef = A.coef + static_cast<int64_t>(iv) * A.row_blocks * 64;
  for (int j0 = b0 + kHistStep * wave; j0 < b1; j0 += 4 * kHistStep) {
    int v[kHistStep], pred[kHistStep], comp[kHistStep];
#pragma unroll
    for (int u = 0; u < kHistStep; ++u) {
      const int j = j0 + u;
      v[u] = 0; pred[u] = 0; comp[u] = 0;
      if (j < b1) {                                           // (uniform)
        v[u] = coef[static_cast<int64_t>(j) * 64 + lane];
        const int pos = j % A.bpm;                            // as jpeg_entropy: the previous block of the same component
        comp[u] = A.bpm == 6 ? (pos >= 4) : (pos != 0);
        const int back = A.bpm == 3 ? 3 : (pos == 0 ? 3 : (pos < 4 ? 1 : 6));
        if (j >= back) pred[u] = coef[static_cast<int64_t>(j - back) * 64];
      }
    }
#pragma unroll
    for (int u = 0; u < kHistStep; ++u)
      if (j0 + u < b1) count_block(v[u], pred[u], lane, h[wave] + comp[u] * (16 + 256));
  }
  __syncthreads();
  for (int i = tid; i < kJpegCounters; i += 256) {
    const uint32_t n = h[0][i] + h[1][i] + h[2][i] + h[3][i];      // (at most kHistBlocks x 64 symbols)
    if (n) atomicAdd(reinterpret_cast<unsigned long long*>(A.counters) + i, static_cast<unsigned long long>(n));
  }
}

__global__ __launch_bounds__(256) void ist_jpeg_histogram_kernel(const HistArgs A) {
  jpeg_histogram(A, static_cast<int>(blockIdx.x), static_cast<int>(blockIdx.y));
}

// ---- gather ------------------------------------------------------------------------------------------------------------
struct GatherArgs { const uint8_t* slots; int64_t slot; uint8_t* out; const int64_t* dst; const uint32_t* len; int32_t first; };

// interval first + i: len bytes from its slot to file offset dst (any alignment, so bytes: the 16-byte units of the
// PNG gather need slots that are multiples of 16), behind RST((k - 1) mod 8) for every interval but the file's first
__device__ __forceinline__ void jpeg_gather(const GatherArgs& G, const int i) {
  const int k = G.first + i;
  const uint8_t* s = G.slots + static_cast<int64_t>(i) * G.slot;
  uint8_t* d = G.out + G.dst[i];
  const int n = static_cast<int>(G.len[i]);
  if (k > 0 && threadIdx.x < 2) d[static_cast<int>(threadIdx.x) - 2] = threadIdx.x == 0 ? 0xFF : static_cast<uint8_t>(0xD0 + ((k - 1) & 7));
  for (int j = threadIdx.x; j < n; j += 256) d[j] = s[j];
}

__global__ __launch_bounds__(256) void ist_jpeg_gather_kernel(const GatherArgs G) { jpeg_gather(G, static_cast<int>(blockIdx.x)); }

// ---- batch -------------------------------------------------------------------------------------------------------------
// The intervals of many files in one grid per kernel (ist_jpeg_encode_batch_device).  The unit is the PIECE, a run of MCU rows of one
// file (JpegPiece, ist_jpeg_enc.h); the workgroups of all pieces are numbered piece-major, a workgroup finds its piece by binary
// search over the pieces' first workgroups (transform) or first intervals (entropy, gather) and runs the body above on arguments made
// from the piece's record.  The search is wave-uniform and the record is read through the constant address space, so the arguments
// arrive in scalar registers as a kernarg struct does (the thumbnail twins of ist_preview.hip are the model).
struct JpegBatchArgs {
  const JpegPiece* pieces; int32_t n;
  uint32_t* len;                 // per interval of the round: bytes written (pinned host memory, as the single encoder's)
  const int64_t* dst;            // ... and its place in its file, laid out by the host between entropy and gather
};
typedef const __attribute__((address_space(4))) JpegPiece ConstPiece;

template <bool BY_WG>
__device__ __forceinline__ int jpeg_piece_of(ConstPiece* pieces, int n, int at) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {                                   // the last piece whose first entry is <= at
    const int mid = (lo + hi + 1) >> 1;
    if ((BY_WG ? pieces[mid].wg0 : pieces[mid].iv0) <= at) lo = mid; else hi = mid - 1;
  }
  return __builtin_amdgcn_readfirstlane(lo);
}

__global__ __launch_bounds__(256) void ist_jpeg_transform_batch_kernel(const JpegBatchArgs B) {
  const int wg = static_cast<int>(blockIdx.x);
  ConstPiece* P = (ConstPiece*)B.pieces + jpeg_piece_of<true>((ConstPiece*)B.pieces, B.n, wg);
  const int local = wg - P->wg0, by = local / P->gx;
  XformArgs A;
  A.canvas = P->canvas; A.pitch = P->pitch; A.w = P->w; A.h = P->h; A.tab = P->tab; A.coef = P->coef;
  A.mcus_x = P->mcus_x; A.mcu_row0 = P->mcu_row0; A.is420 = P->is420;
  jpeg_transform(A, local - by * P->gx, by);
}

// the entropy twin's body: interval iv of the round, coded by jpeg_entropy<BLOCK_BITS, GUARD> on its piece's arguments
template <int BLOCK_BITS, bool GUARD>
__device__ __forceinline__ void jpeg_entropy_batch(const JpegBatchArgs& B, const int iv) {
  ConstPiece* P = (ConstPiece*)B.pieces + jpeg_piece_of<false>((ConstPiece*)B.pieces, B.n, iv);
  EntropyArgs A;
  A.coef = P->coef; A.tab = P->tab; A.slots = P->slots; A.len = B.len + P->iv0;
  A.row_blocks = P->row_blocks; A.bpm = P->bpm; A.slot = P->slot;
  jpeg_entropy<BLOCK_BITS, GUARD>(A, iv - P->iv0);
}

__global__ __launch_bounds__(256) void ist_jpeg_entropy_batch_kernel(const JpegBatchArgs B) {
  jpeg_entropy_batch<kBlockBits, false>(B, static_cast<int>(blockIdx.x));
}
// ... for a round that holds a file with optimised tables (bits are bits, and the slot sizes are the pieces' own)
__global__ __launch_bounds__(256) void ist_jpeg_entropy_wide_batch_kernel(const JpegBatchArgs B) {
  jpeg_entropy_batch<kJpegBlockBitsWide, true>(B, static_cast<int>(blockIdx.x));
}

// the histogram of the round's optimised pieces: interval blockIdx.x of the round, part blockIdx.y of it
struct JpegHistBatchArgs { const JpegPiece* pieces; int32_t n; int64_t* counters; };
__global__ __launch_bounds__(256) void ist_jpeg_histogram_batch_kernel(const JpegHistBatchArgs B) {
  const int iv = static_cast<int>(blockIdx.x);
  ConstPiece* P = (ConstPiece*)B.pieces + jpeg_piece_of<false>((ConstPiece*)B.pieces, B.n, iv);
  if (P->hist < 0) return;                                   // (uniform: a file with the Annex K tables)
  HistArgs A;
  A.coef = P->coef; A.counters = B.counters + static_cast<int64_t>(P->hist) * kJpegCounters;
  A.row_blocks = P->row_blocks; A.bpm = P->bpm;
  jpeg_histogram(A, iv - P->iv0, static_cast<int>(blockIdx.y));
}

// ... and the gather writes what no interval holds: the file's header (by the workgroup of the file's interval 0) and its EOI marker
// (behind the file's last interval), so that every byte of a file comes from this launch
__global__ __launch_bounds__(256) void ist_jpeg_gather_batch_kernel(const JpegBatchArgs B) {
  const int iv = static_cast<int>(blockIdx.x);
  ConstPiece* P = (ConstPiece*)B.pieces + jpeg_piece_of<false>((ConstPiece*)B.pieces, B.n, iv);
  const int i = iv - P->iv0, k = P->mcu_row0 + i;
  const GatherArgs G{P->slots, P->slot, P->out, B.dst + P->iv0, B.len + P->iv0, P->mcu_row0};
  jpeg_gather(G, i);
  if (k == 0) {
    const uint8_t* head = P->head; uint8_t* out = P->out;
    const int n = static_cast<int>(min(static_cast<int64_t>(P->head_len), P->out_cap));
    for (int j = threadIdx.x; j < n; j += 256) out[j] = head[j];
  }
  if (k == P->mcus_y - 1 && threadIdx.x < 2) {
    const int64_t at = G.dst[i] + static_cast<int64_t>(G.len[i]) + threadIdx.x;
    if (at < P->out_cap) P->out[at] = threadIdx.x == 0 ? 0xFF : 0xD9;
  }
}

// ---- host --------------------------------------------------------------------------------------------------------------
// MCU rows per slab: what kBudget holds (IST_TUNING=1 IST_JPEG_ENC_ROWS=<rows> overrides, so that a small canvas crosses slabs)
int64_t slab_rows_of(const Geometry& g) {
  static const int64_t knob = (tuning_mode() && std::getenv("IST_JPEG_ENC_ROWS")) ? std::atoll(std::getenv("IST_JPEG_ENC_ROWS")) : 0;
  const int64_t per_row = g.row_blocks * 128 + g.slot;
  int64_t rows = std::max<int64_t>(1, static_cast<int64_t>(kBudget) / per_row);
  if (knob > 0) rows = knob;
  return std::min<int64_t>(std::min<int64_t>(rows, g.mcus_y), 65535);
}

// every rule of ist_jpeg_encode_device but the context's
int check_args(const char* who, const void* canvas, size_t pitch, int64_t w, int64_t h, int quality, int subsampling) {
  if (quality < 1 || quality > 100) return fail(IST_E_INVALID, std::string(who) + ": quality must be 1..100");
  if (!jpeg_ss_known(subsampling)) return fail(IST_E_INVALID, std::string(who) + ": unknown subsampling");
  if (!canvas || w < 1 || h < 1) return fail(IST_E_INVALID, std::string(who) + ": bad argument");
  if (w > 65535) return fail(IST_E_UNSUPPORTED, std::string(who) + ": a JPEG is at most 65535 wide (width " + std::to_string(w) + ")");
  if (h > 65535) return fail(IST_E_UNSUPPORTED, std::string(who) + ": a JPEG is at most 65535 high (height " + std::to_string(h) + ")");
  if (pitch < static_cast<size_t>(w) * 4 || (pitch & 3)) return fail(IST_E_INVALID, std::string(who) + ": pitch below 4 * w or not a multiple of 4");
  return IST_OK;
}

}  // namespace

int64_t jpeg_slab_rows(const JpegGeometry& g) { return slab_rows_of(g); }

int jpeg_batch_check(const JpegBatchFile& f, const char* what, int k) {
  const std::string who = std::string(what) + " " + std::to_string(k);
  const int rc = check_args(who.c_str(), f.canvas, f.pitch, f.w, f.h, f.quality, f.subsampling);
  if (rc) return rc;
  if (!f.out) return fail(IST_E_INVALID, who + ": NULL output");
  if ((reinterpret_cast<uintptr_t>(f.out) & 15) != 0) return fail(IST_E_INVALID, who + ": JPEG output buffer must be 16-byte aligned");
  if (f.cap < ist_jpeg_bound(f.w, f.h, f.subsampling)) return fail(IST_E_INVALID, who + ": JPEG output buffer too small (see ist_jpeg_bound)");
  return IST_OK;
}

// The file of a canvas in device memory into `out` (device, out_cap bytes).  The arguments have been checked.  Synchronises `stream`.
// The loop is jpeg_encode_slabs; what fills a slab here is the transform kernel.
int jpeg_encode_device(ist_ctx* ctx, const void* canvas, size_t pitch, int64_t w, int64_t h, int quality, int subsampling, void* out,
                       int64_t out_cap, int64_t* out_len, hipStream_t stream) {
  const Geometry g = geometry(w, h, subsampling);
  JpegTables T;
  jpeg_enc_tables(quality, &T);
  XformArgs X;
  X.canvas = static_cast<const uint8_t*>(canvas); X.pitch = pitch; X.w = static_cast<int32_t>(w); X.h = static_cast<int32_t>(h);
  X.tab = nullptr; X.coef = nullptr;
  X.mcus_x = static_cast<int32_t>(g.mcus_x); X.mcu_row0 = 0; X.is420 = jpeg_ss_420(subsampling);
  const unsigned gx = static_cast<unsigned>(X.is420 ? g.mcus_x : (g.mcus_x + 3) / 4);
  JpegSlabSource src;
  src.fill = [&](int64_t r0, int64_t rows, int16_t* coef, const JpegTables* tab, void* st) -> int {
    X.mcu_row0 = static_cast<int32_t>(r0); X.coef = coef; X.tab = tab;
    hipLaunchKernelGGL(ist_jpeg_transform_kernel, dim3(gx, static_cast<unsigned>(rows)), dim3(256), 0, static_cast<hipStream_t>(st), X);
    IST_HIP(hipGetLastError());
    g_launches.fetch_add(1, std::memory_order_relaxed);
    return IST_OK;
  };
  return jpeg_encode_slabs(ctx, w, h, subsampling, T, out, out_cap, out_len, stream, src);
}

// One file, slab by slab; src.fill leaves a slab's coefficients in the scratch (ist_jpeg_enc.h).
// IST_JPEG_OPTIMIZE: every slab is filled and counted first (no host wait between slabs: stream order protects the scratch), one
// synchronisation brings the counts down, the tables and the header go up, and the slab loop runs with the wide entropy kernel.  A
// file of one slab keeps its coefficients; a file of N > 1 slabs is filled twice.
int jpeg_encode_slabs(ist_ctx* ctx, int64_t w, int64_t h, int subsampling, const JpegTables& T0, void* out, int64_t out_cap, int64_t* out_len,
                      void* stream_, const JpegSlabSource& src) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const Geometry g = geometry(w, h, subsampling);
  const bool optimize = jpeg_ss_optimize(subsampling);
  const int64_t slab_rows = slab_rows_of(g);
  JpegTables T = T0;
  std::vector<uint8_t> head = jpeg_enc_header(w, h, subsampling, T, g.mcus_x);      // (optimised: no header is longer than this one)
  if (static_cast<int64_t>(head.size()) + 2 > out_cap) return fail(IST_E_INVALID, "JPEG output buffer too small (see ist_jpeg_bound)");

  const size_t o_coef = round256(sizeof T), coef_bytes = round256(static_cast<size_t>(slab_rows * g.row_blocks) * 128);
  const size_t o_slots = o_coef + coef_bytes, total = o_slots + static_cast<size_t>(slab_rows * g.slot);
  int rc = ctx->scratch_jpg.grow(total);
  if (rc) return rc;
  constexpr size_t kCountBytes = static_cast<size_t>(kJpegCounters) * 8;
  if (optimize) { rc = ctx->scratch_jpg_counts.grow(kCountBytes); if (rc) return rc; }
  uint8_t* const scratch = static_cast<uint8_t*>(ctx->scratch_jpg.p);
  // per interval of a slab: its length (written by the kernel) and its place in the file (read by the gather), in pinned memory;
  // behind them the counts of an optimised file
  const size_t o_counts = static_cast<size_t>(slab_rows) * 16;
  PoolBlock res;
  if (!res.take(o_counts + (optimize ? kCountBytes : 0))) return fail(IST_E_NOMEM, "out of pinned host memory for the JPEG encoder");
  int64_t* const dst = res.at<int64_t>();
  uint32_t* const len = res.at<uint32_t>(8 * static_cast<size_t>(slab_rows));
  // (every way out below leaves the stream idle: kernels in flight write `res` and read the tables)
  StreamDrain drain(stream);
  IST_HIP(hipMemcpyAsync(scratch, &T, sizeof T, hipMemcpyHostToDevice, stream));
  struct { const JpegTables* tab; int16_t* coef; } X{reinterpret_cast<const JpegTables*>(scratch), reinterpret_cast<int16_t*>(scratch + o_coef)};
  auto transform = [&](int64_t r0, int64_t rows) -> int { return src.fill(r0, rows, X.coef, X.tab, stream); };
  auto synced = [&]() -> int { return src.synced ? src.synced() : IST_OK; };
  bool kept = false;                                 // the (only) slab's coefficients are in the scratch already
  if (optimize) {
    int64_t* const counters = static_cast<int64_t*>(ctx->scratch_jpg_counts.p);
    IST_HIP(hipMemsetAsync(counters, 0, kCountBytes, stream));
    const HistArgs H{X.coef, counters, static_cast<int32_t>(g.row_blocks), g.bpm};
    const unsigned parts = static_cast<unsigned>((g.row_blocks + kHistBlocks - 1) / kHistBlocks);
    for (int64_t r0 = 0; r0 < g.mcus_y; r0 += slab_rows) {
      const int64_t rows = std::min(slab_rows, g.mcus_y - r0);
      rc = transform(r0, rows);
      if (rc) return rc;
      hipLaunchKernelGGL(ist_jpeg_histogram_kernel, dim3(static_cast<unsigned>(rows), parts), dim3(256), 0, stream, H);
      IST_HIP(hipGetLastError());
      g_hist_launches.fetch_add(1, std::memory_order_relaxed);
    }
    IST_HIP(hipMemcpyAsync(res.at(o_counts), counters, kCountBytes, hipMemcpyDeviceToHost, stream));
    IST_HIP(hipStreamSynchronize(stream));
    rc = synced();
    if (rc) return rc;
    JpegHuffSpec spec;
    jpeg_enc_codes_optimal(res.at<const int64_t>(o_counts), &T, &spec);
    head = jpeg_enc_header(w, h, subsampling, T, g.mcus_x, &spec);
    IST_HIP(hipMemcpyAsync(scratch, &T, sizeof T, hipMemcpyHostToDevice, stream));
    kept = g.mcus_y <= slab_rows;
  }
  IST_HIP(hipMemcpyAsync(out, head.data(), head.size(), hipMemcpyHostToDevice, stream));
  int64_t pos = static_cast<int64_t>(head.size());
  for (int64_t r0 = 0; r0 < g.mcus_y; r0 += slab_rows) {
    const int64_t rows = std::min(slab_rows, g.mcus_y - r0);
    if (!kept) { rc = transform(r0, rows); if (rc) return rc; }
    EntropyArgs E;
    E.coef = X.coef; E.tab = X.tab; E.slots = scratch + o_slots; E.len = len;
    E.row_blocks = static_cast<int32_t>(g.row_blocks); E.bpm = g.bpm; E.slot = g.slot;
    if (optimize) hipLaunchKernelGGL(ist_jpeg_entropy_wide_kernel, dim3(static_cast<unsigned>(rows)), dim3(kBatch), 0, stream, E);
    else hipLaunchKernelGGL(ist_jpeg_entropy_kernel, dim3(static_cast<unsigned>(rows)), dim3(kBatch), 0, stream, E);
    IST_HIP(hipGetLastError());
    IST_HIP(hipStreamSynchronize(stream));
    rc = synced();
    if (rc) return rc;
    for (int64_t k = 0; k < rows; ++k) {
      if (r0 + k > 0) pos += 2;                      // RSTn
      // (length 0 is also what the wide kernel reports for a symbol that the file's tables have no code for)
      if (len[k] < 1 || static_cast<int64_t>(len[k]) >= g.slot) return fail(IST_E_HIP, "JPEG entropy kernel returned an impossible interval length");
      dst[k] = pos;
      pos += len[k];
    }
    if (pos + 2 > out_cap) return fail(IST_E_INVALID, "JPEG output buffer too small (see ist_jpeg_bound)");
    const GatherArgs G{scratch + o_slots, g.slot, static_cast<uint8_t*>(out), dst, len, static_cast<int32_t>(r0)};
    hipLaunchKernelGGL(ist_jpeg_gather_kernel, dim3(static_cast<unsigned>(rows)), dim3(256), 0, stream, G);
    IST_HIP(hipGetLastError());
    if (r0 + rows < g.mcus_y) IST_HIP(hipStreamSynchronize(stream));      // the next slab's kernels rewrite len[]; dst[] is rewritten by the host
  }
  static const uint8_t eoi[2] = {0xFF, 0xD9};
  IST_HIP(hipMemcpyAsync(static_cast<uint8_t*>(out) + pos, eoi, 2, hipMemcpyHostToDevice, stream));
  IST_HIP(hipStreamSynchronize(stream));
  *out_len = pos + 2;
  return IST_OK;
}

// Many canvases, round by round (jpeg_batch_pieces): the round's tables, headers and piece records go up in ONE copy through the
// ring of ist_jobs_launch, then one transform and one entropy launch for all its pieces, one synchronisation in which the host lays the
// intervals out per file, and one gather launch, which also writes headers and EOI markers.  Nothing else is copied.
// Files with IST_JPEG_OPTIMIZE have tables and a header of their own, which need the file's counts.  A batch of one round counts
// between its transform and its entropy launch (one more synchronisation, the counts down, the table block up again); a batch of
// several rounds first transforms and counts every round that holds an optimised piece, then runs its rounds as ever.
int jpeg_encode_batch(ist_ctx* ctx, std::vector<JpegBatchFile>& files, void* stream_, const char* what, const int* ids) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int n = static_cast<int>(files.size());
  const std::vector<ist_jpeg_piece> pieces = jpeg_batch_pieces(files.data(), n, jpeg_batch_budget());
  const int n_pieces = static_cast<int>(pieces.size());
  std::vector<JpegOptFile> opt(static_cast<size_t>(n));
  int n_opt = 0;
  for (int k = 0; k < n; ++k)
    if (jpeg_ss_optimize(files[static_cast<size_t>(k)].subsampling)) opt[static_cast<size_t>(k)].hist = n_opt++;
  std::vector<JpegRound> rounds;
  std::vector<unsigned> hist_parts;                  // per round: the parts of the longest interval among its optimised pieces
  int64_t max_ivs = 0;
  size_t max_scratch = 0;
  for (int p0 = 0; p0 < n_pieces;) {
    int p1 = p0 + 1;
    while (p1 < n_pieces && pieces[p1].round == pieces[p0].round) ++p1;
    rounds.push_back(jpeg_round_plan(files.data(), pieces.data(), p0, p1));
    const JpegRound& R = rounds.back();
    if (R.wgs > 2147483647ll) return fail(IST_E_UNSUPPORTED, "a JPEG batch round of more than 2^31 - 1 workgroups");
    max_ivs = std::max(max_ivs, R.ivs); max_scratch = std::max(max_scratch, R.scratch_bytes);
    int64_t longest = 0;
    for (int f : R.opt_files) longest = std::max(longest, geometry(files[static_cast<size_t>(f)].w, files[static_cast<size_t>(f)].h, files[static_cast<size_t>(f)].subsampling).row_blocks);
    hist_parts.push_back(static_cast<unsigned>((longest + kHistBlocks - 1) / kHistBlocks));
    p0 = p1;
  }
  // The ring and the scratch are held for the whole call: a second batch encode on this context waits here, so neither grows
  // nor overwrites the scratch under this one's kernels.  A slot is refilled two rounds later at the earliest, behind the
  // synchronisation of the round in between, which is queued behind this round's gather: no event is needed WHILE the lock is held
  // through the last synchronisation (Drain below; whoever drops that must record slot->done and set slot->pending instead).
  // (A counted round is synchronised before the next one starts.)
  std::lock_guard<std::mutex> lk(ctx->batch_mu);
  int rc = ctx->scratch_jpg.grow(max_scratch);
  if (rc) return rc;
  const size_t count_bytes = static_cast<size_t>(n_opt) * kJpegCounters * 8;
  if (n_opt) { rc = ctx->scratch_jpg_counts.grow(count_bytes); if (rc) return rc; }
  uint8_t* const scratch = static_cast<uint8_t*>(ctx->scratch_jpg.p);
  int64_t* const counters = static_cast<int64_t*>(ctx->scratch_jpg_counts.p);
  // per interval of a round: its length (written by the kernel) and its place in its file (read by the gather), in pinned memory;
  // behind them the counts of the optimised files
  const size_t o_counts = static_cast<size_t>(max_ivs) * 16;
  PoolBlock res;
  if (!res.take(o_counts + count_bytes)) return fail(IST_E_NOMEM, "out of pinned host memory for the JPEG encoder");
  int64_t* const dst = res.at<int64_t>();
  uint32_t* const len = res.at<uint32_t>(8 * static_cast<size_t>(max_ivs));
  std::vector<int64_t> pos(static_cast<size_t>(n), kJpegHeaderBytes);      // (an optimised file's: its own header's length, below)
  // Every way out leaves the stream idle (kernels in flight read the slot and write `res`).
  StreamDrain drain(stream);
  // one round's table block up, its transform and, for its optimised pieces, their histogram
  auto transform = [&](const JpegRound& R, ist_ctx::BatchSlot* slot, bool count, unsigned parts) -> int {
    uint8_t* const d = static_cast<uint8_t*>(slot->dev.p);
    jpeg_round_pack(R, files.data(), pieces.data(), static_cast<uint8_t*>(slot->host.p), d, scratch, opt.data());
    IST_HIP(hipMemcpyAsync(d, slot->host.p, R.table_bytes, hipMemcpyHostToDevice, stream));
    const JpegBatchArgs B{reinterpret_cast<const JpegPiece*>(d + R.at_pieces), R.p1 - R.p0, len, dst};
    hipLaunchKernelGGL(ist_jpeg_transform_batch_kernel, dim3(static_cast<unsigned>(R.wgs)), dim3(256), 0, stream, B);
    IST_HIP(hipGetLastError());
    count_jpeg_batch_launch();
    if (count) {
      const JpegHistBatchArgs HB{B.pieces, B.n, counters};
      hipLaunchKernelGGL(ist_jpeg_histogram_batch_kernel, dim3(static_cast<unsigned>(R.ivs), parts), dim3(256), 0, stream, HB);
      IST_HIP(hipGetLastError());
      g_hist_launches.fetch_add(1, std::memory_order_relaxed);
    }
    return IST_OK;
  };
  // the counts down (one synchronisation), then every optimised file's tables and header
  auto build_tables = [&]() -> int {
    IST_HIP(hipMemcpyAsync(res.at(o_counts), counters, count_bytes, hipMemcpyDeviceToHost, stream));
    IST_HIP(hipStreamSynchronize(stream));
    for (int k = 0; k < n; ++k) {
      JpegOptFile& o = opt[static_cast<size_t>(k)];
      if (o.hist < 0) continue;
      const JpegBatchFile& f = files[static_cast<size_t>(k)];
      JpegHuffSpec spec;
      jpeg_enc_tables_optimal(f.quality, res.at<const int64_t>(o_counts) + static_cast<size_t>(o.hist) * kJpegCounters, &o.T, &spec);
      o.head = jpeg_enc_header(f.w, f.h, f.subsampling, o.T, geometry(f.w, f.h, f.subsampling).mcus_x, &spec);
      o.built = true;
      pos[static_cast<size_t>(k)] = static_cast<int64_t>(o.head.size());
    }
    return IST_OK;
  };
  const bool one_round = rounds.size() == 1;
  if (n_opt) {
    IST_HIP(hipMemsetAsync(counters, 0, count_bytes, stream));
    if (!one_round) {
      for (size_t r = 0; r < rounds.size(); ++r) {
        if (rounds[r].opt_files.empty()) continue;
        ist_ctx::BatchSlot* slot = nullptr;
        rc = batch_take_slot(ctx, rounds[r].table_bytes, &slot);
        if (rc) return rc;
        rc = transform(rounds[r], slot, true, hist_parts[r]);
        if (rc) return rc;
        IST_HIP(hipStreamSynchronize(stream));       // the next round rewrites the scratch (and, two rounds on, the slot)
      }
      rc = build_tables();
      if (rc) return rc;
    }
  }
  for (size_t r = 0; r < rounds.size(); ++r) {
    const JpegRound& R = rounds[r];
    const bool wide = !R.opt_files.empty();
    ist_ctx::BatchSlot* slot = nullptr;
    rc = batch_take_slot(ctx, R.table_bytes, &slot);
    if (rc) return rc;
    uint8_t* const d = static_cast<uint8_t*>(slot->dev.p);
    rc = transform(R, slot, wide && one_round, hist_parts[r]);
    if (rc) return rc;
    const JpegBatchArgs B{reinterpret_cast<const JpegPiece*>(d + R.at_pieces), R.p1 - R.p0, len, dst};
    if (wide && one_round) {                         // the coefficients stay; the block goes up again with the files' own tables and headers
      rc = build_tables();
      if (rc) return rc;
      jpeg_round_pack(R, files.data(), pieces.data(), static_cast<uint8_t*>(slot->host.p), d, scratch, opt.data());
      IST_HIP(hipMemcpyAsync(d, slot->host.p, R.table_bytes, hipMemcpyHostToDevice, stream));
    }
    if (wide) hipLaunchKernelGGL(ist_jpeg_entropy_wide_batch_kernel, dim3(static_cast<unsigned>(R.ivs)), dim3(kBatch), 0, stream, B);
    else hipLaunchKernelGGL(ist_jpeg_entropy_batch_kernel, dim3(static_cast<unsigned>(R.ivs)), dim3(kBatch), 0, stream, B);
    IST_HIP(hipGetLastError());
    IST_HIP(hipStreamSynchronize(stream));
    int64_t iv = 0;
    for (int p = R.p0; p < R.p1; ++p) {
      const ist_jpeg_piece& pc = pieces[static_cast<size_t>(p)];
      JpegBatchFile& f = files[static_cast<size_t>(pc.file)];
      const Geometry g = geometry(f.w, f.h, f.subsampling);
      int64_t at = pos[static_cast<size_t>(pc.file)];
      for (int64_t k = 0; k < pc.mcu_rows; ++k, ++iv) {
        if (pc.mcu_row0 + k > 0) at += 2;              // RSTn
        // (length 0 is also what the wide kernel reports for a symbol that the file's tables have no code for)
        if (len[iv] < 1 || static_cast<int64_t>(len[iv]) >= g.slot) return fail(IST_E_HIP, "JPEG entropy kernel returned an impossible interval length");
        dst[iv] = at;
        at += len[iv];
      }
      if (at + 2 > f.cap) return fail(IST_E_INVALID, std::string(what) + " " + std::to_string(ids ? ids[pc.file] : pc.file) + ": JPEG output buffer too small (see ist_jpeg_bound)");
      pos[static_cast<size_t>(pc.file)] = at;
      if (pc.mcu_row0 + pc.mcu_rows == g.mcus_y) f.len = at + 2;
    }
    hipLaunchKernelGGL(ist_jpeg_gather_batch_kernel, dim3(static_cast<unsigned>(R.ivs)), dim3(256), 0, stream, B);
    IST_HIP(hipGetLastError());
  }
  IST_HIP(hipStreamSynchronize(stream));
  return IST_OK;
}

// ... into a pooled pinned block of the file's real length.  Caller holds ctx->mu; the canvas is complete on ctx->stream.
int jpeg_to_host(ist_ctx* ctx, const void* canvas, size_t pitch, int64_t w, int64_t h, int quality, int subsampling, uint8_t** out_jpeg,
                 int64_t* out_len) {
  const int64_t cap = ist_jpeg_bound(w, h, subsampling);
  int rc = ctx->scratch_file.grow(static_cast<size_t>(cap));
  if (rc) return rc;
  int64_t len = 0;
  rc = jpeg_encode_device(ctx, canvas, pitch, w, h, quality, subsampling, ctx->scratch_file.p, cap, &len, ctx->stream);
  if (rc) return rc;
  uint8_t* host = nullptr;
  rc = read_back_pooled(ctx->scratch_file.p, static_cast<size_t>(len), ctx->stream, &host);
  if (rc) return rc;
  *out_jpeg = host; *out_len = len;
  return IST_OK;
}

int jpeg_check_export(const char* who, int64_t w, int64_t h, int quality, int subsampling) {
  static const uint8_t some = 0;
  return check_args(who, &some, static_cast<size_t>(std::max<int64_t>(w, 1)) * 4, w, h, quality, subsampling);
}

int jpeg_check_options(const char* who, int quality, int subsampling) { return check_args(who, who, 4, 1, 1, quality, subsampling); }

}  // namespace ist

using namespace ist;

extern "C" {

int64_t ist_debug_jpeg_encode_launches(void) { return g_launches.load(std::memory_order_relaxed); }
int64_t ist_debug_jpeg_histogram_launches(void) { return g_hist_launches.load(std::memory_order_relaxed); }

int ist_debug_jpeg_counts(ist_ctx* ctx, int64_t* out, int64_t n) {
  if (!ctx) return fail(IST_E_NO_CONTEXT, "无法获取绘图上下文");
  if (!out || n < 0 || n % kJpegCounters != 0) return fail(IST_E_INVALID, "ist_debug_jpeg_counts: NULL argument or a count that is no multiple of " + std::to_string(kJpegCounters));
  std::lock_guard<std::mutex> lock(ctx->mu);
  const int64_t held = static_cast<int64_t>(ctx->scratch_jpg_counts.bytes / 8);
  if (n > held) return fail(IST_E_INVALID, "ist_debug_jpeg_counts: the block holds " + std::to_string(held) + " counters");
  if (n == 0) return IST_OK;
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(IST_E_NO_DEVICE, "hipSetDevice failed");
  IST_HIP(hipStreamSynchronize(ctx->stream));
  IST_HIP(hipMemcpy(out, ctx->scratch_jpg_counts.p, static_cast<size_t>(n) * 8, hipMemcpyDeviceToHost));
  return IST_OK;
}

int ist_jpeg_quant_tables(int quality, uint8_t luma[64], uint8_t chroma[64]) {
  if (quality < 1 || quality > 100) return fail(IST_E_INVALID, "ist_jpeg_quant_tables: quality must be 1..100");
  if (!luma || !chroma) return fail(IST_E_INVALID, "ist_jpeg_quant_tables: NULL table");
  jpeg_quant_tables(quality, luma, chroma);
  return IST_OK;
}

int ist_jpeg_optimal_table(const int64_t freq[256], uint8_t bits[16], uint8_t vals[256], int* n_vals) {
  if (!freq || !bits || !vals || !n_vals) return fail(IST_E_INVALID, "ist_jpeg_optimal_table: NULL argument");
  for (int s = 0; s < 256; ++s)
    if (freq[s] < 0) return fail(IST_E_INVALID, "ist_jpeg_optimal_table: negative count");
  *n_vals = jpeg_optimal_table(freq, bits, vals);
  return IST_OK;
}

int64_t ist_jpeg_bound(int64_t w, int64_t h, int subsampling) {
  if (w < 1 || h < 1 || w > 65535 || h > 65535 || !jpeg_ss_known(subsampling)) return -1;
  const Geometry g = geometry(w, h, subsampling);
  return 1024 + g.mcus_y * (g.row_blocks * g.block_bytes + 16);
}

int ist_jpeg_encode_device(ist_ctx* ctx, const void* canvas, size_t pitch, int64_t w, int64_t h, int quality, int subsampling, void* out,
                           int64_t out_cap, int64_t* out_len, void* stream) {
  if (!ctx) return fail(IST_E_NO_CONTEXT, "无法获取绘图上下文");
  const int rc = check_args("ist_jpeg_encode_device", canvas, pitch, w, h, quality, subsampling);
  if (rc) return rc;
  if (!out || !out_len) return fail(IST_E_INVALID, "ist_jpeg_encode_device: NULL output");
  if ((reinterpret_cast<uintptr_t>(out) & 15) != 0) return fail(IST_E_INVALID, "JPEG output buffer must be 16-byte aligned");
  if (out_cap < ist_jpeg_bound(w, h, subsampling)) return fail(IST_E_INVALID, "JPEG output buffer too small (see ist_jpeg_bound)");
  return jpeg_encode_device(ctx, canvas, pitch, w, h, quality, subsampling, out, out_cap, out_len, static_cast<hipStream_t>(stream));
}

int ist_jpeg_encode_rgba8(ist_ctx* ctx, const uint8_t* pixels, size_t pitch, int64_t w, int64_t h, int quality, int subsampling,
                          uint8_t** out_jpeg, int64_t* out_len) {
  if (!ctx) return fail(IST_E_NO_CONTEXT, "无法获取绘图上下文");
  int rc = check_args("ist_jpeg_encode_rgba8", pixels, pitch, w, h, quality, subsampling);
  if (rc) return rc;
  if (!out_jpeg || !out_len) return fail(IST_E_INVALID, "ist_jpeg_encode_rgba8: NULL output");
  *out_jpeg = nullptr; *out_len = 0;
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(IST_E_NO_DEVICE, "hipSetDevice failed");
  const size_t row = static_cast<size_t>(w) * 4;
  rc = ctx->scratch_dst.grow(row * static_cast<size_t>(h));
  if (rc) return rc;
  std::vector<RowsCopy> up{RowsCopy{ctx->scratch_dst.p, pixels, nullptr, pitch, row, static_cast<size_t>(h)}};
  rc = stager_of(ctx).upload(up, ctx->stream);
  if (rc) return rc;
  return jpeg_to_host(ctx, ctx->scratch_dst.p, row, w, h, quality, subsampling, out_jpeg, out_len);
}

}  // extern "C"
