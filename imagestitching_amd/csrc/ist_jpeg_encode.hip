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
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "ist_ctx.h"

namespace ist {

namespace {

std::atomic<int64_t> g_launches{0};

constexpr size_t kBudget = 256u << 20;     // coefficient scratch + interval slots of one slab
constexpr int kBlockBits = 22 + 63 * 26;   // most bits of one block: DC code 11 + 11 magnitude bits, 63 x (AC code 16 + 10)
constexpr int kBlockBytes = 2 * kBlockBits / 8;      // ... as bytes when every byte is 0xFF and stuffed: 415
static_assert(kBlockBits == 1660 && kBlockBytes * 8 == 2 * kBlockBits, "slot bound");
constexpr int kBatch = 256;                // blocks per batch of the entropy kernel = its threads
constexpr int kImgWords = (7 + kBatch * kBlockBits + 31) / 32 + 2;      // LDS bit image of a batch behind a carried partial byte

// T.81 Annex K: the example quantisation tables K.1 / K.2 (natural order) and the Huffman tables K.3 - K.6 (BITS, HUFFVAL)
const uint8_t kQLuma[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                            14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                            49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const uint8_t kQChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                              47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                              99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
const uint8_t kZigzag[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13,
                             6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38,
                             31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};       // zig-zag position -> natural index
const uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
const uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
const uint8_t kAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
     0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
     0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
     0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
     0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
     0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
     0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
     0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
     0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
     0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
     0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
     0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
     0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// what the kernels read beside the canvas: one block at the head of the context's JPEG scratch
struct JpegTables {
  uint32_t dc[2][16];        // Huffman code of a DC size: length << 16 | code (slot 0 luma, 1 chroma)
  uint32_t ac[2][256];       // ... of an AC run/size symbol (0: the symbol has no code)
  uint8_t q[2][64];          // quantisation tables, natural order
  uint8_t zz_of[64];         // natural index -> zig-zag position
};

void huff_codes(const uint8_t* bits, const uint8_t* vals, uint32_t* out) {       // T.81 C.2: canonical codes
  uint32_t code = 0; int k = 0;
  for (int l = 1; l <= 16; ++l) {
    for (int i = 0; i < bits[l - 1]; ++i) out[vals[k++]] = (static_cast<uint32_t>(l) << 16) | code++;
    code <<= 1;
  }
}

void quant_tables(int quality, uint8_t luma[64], uint8_t chroma[64]) {           // libjpeg: jpeg_quality_scaling, jpeg_add_quant_table
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int i = 0; i < 64; ++i) {
    luma[i] = static_cast<uint8_t>(std::min(255, std::max(1, (kQLuma[i] * scale + 50) / 100)));
    chroma[i] = static_cast<uint8_t>(std::min(255, std::max(1, (kQChroma[i] * scale + 50) / 100)));
  }
}

struct Geometry {
  int mcu_w, mcu_h, bpm;         // MCU size in pixels, blocks per MCU
  int64_t mcus_x, mcus_y, row_blocks;
  int64_t slot;                  // bytes of one interval's slot (a multiple of 16)
};
Geometry geometry(int64_t w, int64_t h, int subsampling) {
  Geometry g;
  g.mcu_w = g.mcu_h = subsampling == IST_JPEG_420 ? 16 : 8;
  g.bpm = subsampling == IST_JPEG_420 ? 6 : 3;
  g.mcus_x = (w + g.mcu_w - 1) / g.mcu_w; g.mcus_y = (h + g.mcu_h - 1) / g.mcu_h;
  g.row_blocks = g.mcus_x * g.bpm;
  g.slot = (g.row_blocks * kBlockBytes + 2 + 15) & ~15ll;      // + the byte the pad can add, and one so that no real length reaches it
  return g;
}

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

__global__ __launch_bounds__(256) void ist_jpeg_transform_kernel(const XformArgs A) {
  __shared__ int sT[64], sQ[128], sZ[64];
  __shared__ int sS[12 * 64], sR[12 * 64];        // level-shifted samples / row-pass results (later: the quantised blocks), block by block
  __shared__ int sC[2][256];                      // 4:2:0: full-resolution chroma of the MCU
  const int tid = threadIdx.x;
  if (tid < 64) { sT[tid] = fdct_coef(tid >> 3, tid & 7); sZ[tid] = A.tab->zz_of[tid]; }
  if (tid < 128) sQ[tid] = A.tab->q[tid >> 6][tid & 63];
  const int tw = A.is420 ? 16 : 32, sh = A.is420 ? 4 : 5;
  const int px = tid & (tw - 1), py = tid >> sh;
  const int64_t mcu_y = static_cast<int64_t>(A.mcu_row0) + blockIdx.y;
  const int x = min(static_cast<int>(blockIdx.x) * tw + px, A.w - 1);                 // (clamped reads: the edge padding)
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
  const int64_t mcu0 = static_cast<int64_t>(blockIdx.x) * (A.is420 ? 1 : 4);
  const int mcus = static_cast<int>(min(static_cast<int64_t>(A.is420 ? 1 : 4), static_cast<int64_t>(A.mcus_x) - mcu0));
  const int words = mcus * (A.is420 ? 6 : 3) * 32;
  uint32_t* dst = reinterpret_cast<uint32_t*>(A.coef) + ((static_cast<int64_t>(blockIdx.y) * A.mcus_x + mcu0) * (A.is420 ? 6 : 3)) * 32;
  for (int i = tid; i < words; i += 256)
    dst[i] = (static_cast<uint32_t>(sS[2 * i]) & 0xFFFFu) | (static_cast<uint32_t>(sS[2 * i + 1]) << 16);
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
template <bool EMIT>
__device__ __forceinline__ int code_block(const uint32_t (&c)[32], int diff, const uint32_t* dc, const uint32_t* ac, BitWriter* bw) {
  int bits;
  {
    const int s = size_of(diff < 0 ? -diff : diff);
    const uint32_t h = dc[s];
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
      bits += static_cast<int>(z >> 16);
      if (EMIT) bw->put(z & 0xFFFFu, static_cast<int>(z >> 16));
      run -= 16;
    }
    v = max(-1023, min(1023, v));                          // (the transform clamps already: this keeps the slot bound whatever the scratch holds)
    const int s = size_of(v < 0 ? -v : v);
    const uint32_t h = ac[run * 16 + s];
    const int l = static_cast<int>(h >> 16) + s;
    bits += l;
    if (EMIT) bw->put(((h & 0xFFFFu) << s) | (static_cast<uint32_t>(v < 0 ? v - 1 : v) & ((1u << s) - 1u)), l);
    run = 0;
  }
  if (run > 0) {                                           // EOB
    const uint32_t e = ac[0];
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

__global__ __launch_bounds__(256) void ist_jpeg_entropy_kernel(const EntropyArgs A) {
  __shared__ uint32_t img[kImgWords];
  __shared__ uint32_t sDc[32], sAc[512];
  __shared__ uint32_t ws_bits[4], ws_ff[4];
  const int tid = threadIdx.x;
  if (tid < 32) sDc[tid] = A.tab->dc[tid >> 4][tid & 15];
  for (int i = tid; i < 512; i += 256) sAc[i] = A.tab->ac[i >> 8][i & 255];
  __syncthreads();
  const int16_t* coef = A.coef + static_cast<int64_t>(blockIdx.x) * A.row_blocks * 64;
  uint8_t* slot = A.slots + static_cast<int64_t>(blockIdx.x) * A.slot;
  int64_t out_pos = 0;
  int carry_bits = 0; uint32_t carry_val = 0;            // the partial last byte of the batches so far (its bits at the top of a byte)
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
    const int mybits = on ? code_block<false>(c, diff, dc, ac, nullptr) : 0;
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
  if (tid == 0) A.len[blockIdx.x] = static_cast<uint32_t>(min(out_pos, A.slot));
}

// ---- gather ------------------------------------------------------------------------------------------------------------
struct GatherArgs { const uint8_t* slots; int64_t slot; uint8_t* out; const int64_t* dst; const uint32_t* len; int32_t first; };

// interval first + blockIdx.x: len bytes from its slot to file offset dst (any alignment, so bytes: the 16-byte units of the
// PNG gather need slots that are multiples of 16), behind RST((k - 1) mod 8) for every interval but the file's first
__global__ __launch_bounds__(256) void ist_jpeg_gather_kernel(const GatherArgs G) {
  const int k = G.first + static_cast<int>(blockIdx.x);
  const uint8_t* s = G.slots + static_cast<int64_t>(blockIdx.x) * G.slot;
  uint8_t* d = G.out + G.dst[blockIdx.x];
  const int n = static_cast<int>(G.len[blockIdx.x]);
  if (k > 0 && threadIdx.x < 2) d[static_cast<int>(threadIdx.x) - 2] = threadIdx.x == 0 ? 0xFF : static_cast<uint8_t>(0xD0 + ((k - 1) & 7));
  for (int i = threadIdx.x; i < n; i += 256) d[i] = s[i];
}

// ---- host --------------------------------------------------------------------------------------------------------------
void seg(std::vector<uint8_t>* o, int marker, const std::vector<uint8_t>& body) {
  o->push_back(0xFF); o->push_back(static_cast<uint8_t>(marker));
  o->push_back(static_cast<uint8_t>((body.size() + 2) >> 8)); o->push_back(static_cast<uint8_t>((body.size() + 2) & 255));
  o->insert(o->end(), body.begin(), body.end());
}

// SOI, APP0, DQT x 2, DHT x 4, DRI, SOF0, SOS
std::vector<uint8_t> header(int64_t w, int64_t h, int subsampling, const JpegTables& T, int64_t restart) {
  std::vector<uint8_t> o{0xFF, 0xD8};
  seg(&o, 0xE0, {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
  for (int s = 0; s < 2; ++s) {
    std::vector<uint8_t> b{static_cast<uint8_t>(s)};
    for (int k = 0; k < 64; ++k) b.push_back(T.q[s][kZigzag[k]]);
    seg(&o, 0xDB, b);
  }
  for (int tc = 0; tc < 2; ++tc)
    for (int s = 0; s < 2; ++s) {
      std::vector<uint8_t> b{static_cast<uint8_t>(tc * 16 + s)};
      const uint8_t* bits = tc ? kAcBits[s] : kDcBits[s];
      b.insert(b.end(), bits, bits + 16);
      if (tc) b.insert(b.end(), kAcVals[s], kAcVals[s] + 162); else b.insert(b.end(), kDcVals, kDcVals + 12);
      seg(&o, 0xC4, b);
    }
  seg(&o, 0xDD, {static_cast<uint8_t>(restart >> 8), static_cast<uint8_t>(restart & 255)});
  const uint8_t hv = subsampling == IST_JPEG_420 ? 0x22 : 0x11;
  seg(&o, 0xC0, {8, static_cast<uint8_t>(h >> 8), static_cast<uint8_t>(h & 255), static_cast<uint8_t>(w >> 8), static_cast<uint8_t>(w & 255), 3,
                 1, hv, 0, 2, 0x11, 1, 3, 0x11, 1});
  seg(&o, 0xDA, {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
  return o;
}

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
  if (subsampling != IST_JPEG_444 && subsampling != IST_JPEG_420) return fail(IST_E_INVALID, std::string(who) + ": unknown subsampling");
  if (!canvas || w < 1 || h < 1) return fail(IST_E_INVALID, std::string(who) + ": bad argument");
  if (w > 65535) return fail(IST_E_UNSUPPORTED, std::string(who) + ": a JPEG is at most 65535 wide (width " + std::to_string(w) + ")");
  if (h > 65535) return fail(IST_E_UNSUPPORTED, std::string(who) + ": a JPEG is at most 65535 high (height " + std::to_string(h) + ")");
  if (pitch < static_cast<size_t>(w) * 4 || (pitch & 3)) return fail(IST_E_INVALID, std::string(who) + ": pitch below 4 * w or not a multiple of 4");
  return IST_OK;
}

}  // namespace

// The file of a canvas in device memory into `out` (device, out_cap bytes).  The arguments have been checked.  Synchronises `stream`.
int jpeg_encode_device(ist_ctx* ctx, const void* canvas, size_t pitch, int64_t w, int64_t h, int quality, int subsampling, void* out,
                       int64_t out_cap, int64_t* out_len, hipStream_t stream) {
  const Geometry g = geometry(w, h, subsampling);
  const int64_t slab_rows = slab_rows_of(g);
  JpegTables T;
  std::memset(&T, 0, sizeof T);
  for (int s = 0; s < 2; ++s) { huff_codes(kDcBits[s], kDcVals, T.dc[s]); huff_codes(kAcBits[s], kAcVals[s], T.ac[s]); }
  quant_tables(quality, T.q[0], T.q[1]);
  for (int k = 0; k < 64; ++k) T.zz_of[kZigzag[k]] = static_cast<uint8_t>(k);
  const std::vector<uint8_t> head = header(w, h, subsampling, T, g.mcus_x);
  if (static_cast<int64_t>(head.size()) + 2 > out_cap) return fail(IST_E_INVALID, "JPEG output buffer too small (see ist_jpeg_bound)");

  const size_t o_coef = round256(sizeof T), coef_bytes = round256(static_cast<size_t>(slab_rows * g.row_blocks) * 128);
  const size_t o_slots = o_coef + coef_bytes, total = o_slots + static_cast<size_t>(slab_rows * g.slot);
  int rc = grow_device(&ctx->scratch_jpg, &ctx->scratch_jpg_bytes, total);
  if (rc) return rc;
  uint8_t* const scratch = static_cast<uint8_t*>(ctx->scratch_jpg);
  // per interval of a slab: its length (written by the kernel) and its place in the file (read by the gather), in pinned memory
  struct Pinned { uint8_t* p; ~Pinned() { if (p) pool_give(p); } } res{static_cast<uint8_t*>(pool_take(static_cast<size_t>(slab_rows) * 16))};
  if (!res.p) return fail(IST_E_NOMEM, "out of pinned host memory for the JPEG encoder");
  int64_t* const dst = reinterpret_cast<int64_t*>(res.p);
  uint32_t* const len = reinterpret_cast<uint32_t*>(res.p + 8 * static_cast<size_t>(slab_rows));
  // (every way out below leaves the stream idle: kernels in flight write `res` and read the tables)
  struct Drain { hipStream_t s; ~Drain() { (void)hipStreamSynchronize(s); } } drain{stream};
  IST_HIP(hipMemcpyAsync(scratch, &T, sizeof T, hipMemcpyHostToDevice, stream));
  IST_HIP(hipMemcpyAsync(out, head.data(), head.size(), hipMemcpyHostToDevice, stream));
  int64_t pos = static_cast<int64_t>(head.size());
  for (int64_t r0 = 0; r0 < g.mcus_y; r0 += slab_rows) {
    const int64_t rows = std::min(slab_rows, g.mcus_y - r0);
    XformArgs X;
    X.canvas = static_cast<const uint8_t*>(canvas); X.pitch = pitch; X.w = static_cast<int32_t>(w); X.h = static_cast<int32_t>(h);
    X.tab = reinterpret_cast<const JpegTables*>(scratch); X.coef = reinterpret_cast<int16_t*>(scratch + o_coef);
    X.mcus_x = static_cast<int32_t>(g.mcus_x); X.mcu_row0 = static_cast<int32_t>(r0); X.is420 = subsampling == IST_JPEG_420;
    const unsigned gx = static_cast<unsigned>(X.is420 ? g.mcus_x : (g.mcus_x + 3) / 4);
    hipLaunchKernelGGL(ist_jpeg_transform_kernel, dim3(gx, static_cast<unsigned>(rows)), dim3(256), 0, stream, X);
    IST_HIP(hipGetLastError());
    g_launches.fetch_add(1, std::memory_order_relaxed);
    EntropyArgs E;
    E.coef = X.coef; E.tab = X.tab; E.slots = scratch + o_slots; E.len = len;
    E.row_blocks = static_cast<int32_t>(g.row_blocks); E.bpm = g.bpm; E.slot = g.slot;
    hipLaunchKernelGGL(ist_jpeg_entropy_kernel, dim3(static_cast<unsigned>(rows)), dim3(kBatch), 0, stream, E);
    IST_HIP(hipGetLastError());
    IST_HIP(hipStreamSynchronize(stream));
    for (int64_t k = 0; k < rows; ++k) {
      if (r0 + k > 0) pos += 2;                      // RSTn
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

// ... into a pooled pinned block of the file's real length.  Caller holds ctx->mu; the canvas is complete on ctx->stream.
int jpeg_to_host(ist_ctx* ctx, const void* canvas, size_t pitch, int64_t w, int64_t h, int quality, int subsampling, uint8_t** out_jpeg,
                 int64_t* out_len) {
  const int64_t cap = ist_jpeg_bound(w, h, subsampling);
  int rc = grow_device(&ctx->scratch_file, &ctx->scratch_file_bytes, static_cast<size_t>(cap));
  if (rc) return rc;
  int64_t len = 0;
  rc = jpeg_encode_device(ctx, canvas, pitch, w, h, quality, subsampling, ctx->scratch_file, cap, &len, ctx->stream);
  if (rc) return rc;
  uint8_t* host = nullptr;
  rc = read_back_pooled(ctx->scratch_file, static_cast<size_t>(len), ctx->stream, &host);
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

int ist_jpeg_quant_tables(int quality, uint8_t luma[64], uint8_t chroma[64]) {
  if (quality < 1 || quality > 100) return fail(IST_E_INVALID, "ist_jpeg_quant_tables: quality must be 1..100");
  if (!luma || !chroma) return fail(IST_E_INVALID, "ist_jpeg_quant_tables: NULL table");
  quant_tables(quality, luma, chroma);
  return IST_OK;
}

int64_t ist_jpeg_bound(int64_t w, int64_t h, int subsampling) {
  if (w < 1 || h < 1 || w > 65535 || h > 65535 || (subsampling != IST_JPEG_444 && subsampling != IST_JPEG_420)) return -1;
  const Geometry g = geometry(w, h, subsampling);
  return 1024 + g.mcus_y * (g.row_blocks * kBlockBytes + 16);
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
  rc = grow_device(&ctx->scratch_dst, &ctx->scratch_dst_bytes, row * static_cast<size_t>(h));
  if (rc) return rc;
  std::vector<RowsCopy> up{RowsCopy{ctx->scratch_dst, pixels, nullptr, pitch, row, static_cast<size_t>(h)}};
  rc = stager_of(ctx).upload(up, ctx->stream);
  if (rc) return rc;
  return jpeg_to_host(ctx, ctx->scratch_dst, row, w, h, quality, subsampling, out_jpeg, out_len);
}

}  // extern "C"
