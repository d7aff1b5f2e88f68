// ist_png_deflate.hip — the COMPRESSING PNG export: Paeth filter + run-length matches + dynamic Huffman, on the GPU.
//
// Reference anchor: the export step of onStitch — wx.canvasToTempFilePath({fileType:'png', quality:1})
// (utils/canvas.js:205-242, pages/index/index.js:1577-1579).  The reference's encoder is the WeChat client; a PNG that
// decodes to the same pixels is the same result, so the bit stream is designed for the hardware:
//
//   * the filtered stream (per row: filter byte 4 = Paeth, then the Paeth residuals of the RGBA bytes) is cut into
//     CHUNKS of at most 16 KiB — whole rows when a row fits, otherwise pieces of one row.  One 256-thread workgroup
//     compresses one chunk into its own deflate block, entirely in LDS, independently of every other chunk.
//   * tokens: thread t owns bytes [64 t, 64 t + 64) of the chunk.  A run of equal bytes becomes one literal + matches
//     of distance 1 (what zlib calls Z_RLE, its recommended strategy for PNG); flat areas — gaps, margins, screenshots
//     — filter to zeros and collapse to a few bits per 64 bytes.  Runs do not cross a thread's span, so no thread
//     needs its neighbour's state.
//   * code: one dynamic Huffman code per chunk over the 286 literal/length symbols, built from the chunk's histogram
//     (bitonic sort + two-queue merge + the zlib length-limit fix-up); the code-length alphabet uses a fixed 4-bit code
//     so no third code has to be built.  Every thread re-walks its span twice more: once to count its bits (block-wide
//     exclusive scan gives its bit offset), once to emit them (LDS atomicOr).
//   * a chunk whose Huffman form is not smaller than its bytes is written as a stored block (random data stays 1:1).
//   * every chunk ends byte-aligned (empty stored block = zlib's sync flush) and is padded with further empty stored
//     blocks (5 bytes each, coprime with 16) to a multiple of 16 bytes, so chunks concatenate with 16-byte copies.
//   * each workgroup also returns the Adler-32 partial sums of its filtered bytes and the raw CRC-32 of its output
//     bytes; the host combines them (O(chunks)), lays the chunks out behind one another (several IDAT chunks if the
//     stream exceeds the IDAT limit), a second kernel copies them into place, and ~100 header/trailer bytes are patched.
//
// ADAPTIVE ROW FILTERS (ist_ctx_set_png_filter, IST_PNG_FILTER_ADAPTIVE; the default stays Paeth on every row).  For a canvas in a
// colour form of bpp bytes per pixel (4 RGBA, 3 RGB: alpha is not read) row y gets the filter type f of {0 None, 1 Sub, 2 Up,
// 3 Average, 4 Paeth} with the least
//     cost_f(y) = sum over the row's bpp w residual bytes r of (r < 128 ? r : 256 - r)
// (the minimum sum of absolute differences; the filter byte itself is not counted).  Residuals are those of the PNG specification
// 9.2 - 9.4: left / up / upper left are the same channel of the neighbouring pixel, zero outside the image; Average is
// (left + up) >> 1 on the unwrapped 0..255 values; Paeth breaks its ties as above.  Ties between filters go to the first of
// 4, 1, 2, 3, 0: Paeth wins ties, so a canvas on which nothing beats Paeth gives the default form's stream bit for bit, and flat
// rows stay type 4 (on row 0, where Sub is Paeth and None is Up, neither Sub nor None is ever chosen).  The choice is a function
// of the row's pixels and of the row above alone - not of the chunk grid, not of the slabs - and is made by a pre-pass kernel (ist_png_row_filter_kernel) that writes one byte per row; the compressing
// kernels' adaptive twins read that byte in step A, form the residual with that predictor and store the type as the row's filter
// byte.  Everything behind the filter - grid, spans, tokens, code rule, stored against Huffman, pads, Adler-32, slabs, IDAT layout,
// IHDR (filter method 0 allows a type per row) - is unchanged.
//
// WINDOW MATCHES (ist_ctx_set_png_match, IST_PNG_MATCH_WINDOW; the default stays the run form above).  A chunk may also copy from its
// own earlier spans - what rendered text needs, whose residual patterns return at a distance, not next to each other.  In a chunk of n
// bytes b every position p with p + 4 <= n has a key, the little-endian word b[p..p+3], and H(p) = (key * 2654435761 mod 2^32) >> 20.
// cand(p) = the greatest q with a key, H(q) == H(p) and q < 64 (p / 64): the latest position of that hash in an EARLIER span, or none;
// a function of the chunk's bytes alone.  Every span is parsed on its own from its first byte; at p: run = the bytes from p on equal to
// b[p] inside the span; m = the bytes for which b[cand(p) + i] == b[p + i], at most 63 and not past the span's end, 0 without a
// candidate (the source may run into the destination span: an overlapping copy).  m >= 4 and m >= run: one match of m bytes at
// distance p - cand(p); otherwise run >= 4: the run form's literal + match of run - 1 at distance 1; otherwise a literal.  Codes: the
// literal/length code by the rule of step C; a second code over the 30 distance symbols by the same rule (one symbol in use: length
// 1; none: symbol 0 with length 1); one of them incomplete after 16 rounds: no window form.  Block: the run form's with HDIST = the
// highest distance symbol in use and its HDIST + 1 lengths behind the 286 in the same 4-bit code; a match is length code, extra bits,
// distance code, extra bits.  Choice per chunk: stored or run form exactly as the default setting decides; the window form replaces
// that only where its chunk WITH lead bytes and pads is smaller (the 5-byte pads are not monotone in the body), a tie keeps the
// default's bytes - so no chunk and no file grows, SLOT and ist_png_bound stand, and a chunk that keeps the run or stored form is the
// default setting's chunk bit for bit.  Filter, colour form, grid, checksums, len16, slots, gather and slabs are untouched.  The
// kernels are window twins of their own (deflate_chunk_window below); tests/png_match_reference.py restates the rule on the CPU.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <functional>
#include <mutex>
#include <vector>

#include "ist_crc.h"
#include "ist_host.h"
#include "ist_ctx.h"

namespace ist {

namespace {

constexpr int kCopyGrid = 0;             // workgroups of the device-to-host copy kernel (0: the runtime's copy); IST_PNG_COPY_GRID overrides in tuning mode
constexpr int CH = 16384;              // most filtered-stream bytes in one chunk
constexpr int SPAN = 64;               // bytes per thread
constexpr int SLOT = CH + 128;         // bytes per chunk in the scratch area (stored form + framing + alignment pads)
constexpr int NSYM = 286;              // literal/length symbols
constexpr int HDR_BITS = 3 + 5 + 5 + 4 + 19 * 3 + (NSYM + 1) * 4;      // block header with every code length sent in 4 bits
constexpr int PADDED = CH + CH / 16;   // LDS bytes of the filtered chunk: 4 pad bytes after every 64 (bank spread)

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_a4 __attribute__((aligned(4)));

struct DeflArgs {
  const uint8_t* canvas; size_t pitch; int64_t w, h;
  uint8_t* slots;                // n_chunks * SLOT
  uint32_t* len16;               // per chunk: bytes written / 16
  uint32_t* crc;                 // per chunk: raw CRC (register from 0) of the bytes written
  uint32_t* ad_a; uint32_t* ad_b; uint32_t* ad_n;    // per chunk: sum of bytes, index-weighted sum mod 65521, byte count
  const uint32_t* tables;        // 4 x 256 CRC slicing tables
  const uint32_t* xpow16;        // x^(128 i) mod P: shift of a CRC register over 16 i zero bytes
  int32_t rows_per_chunk;        // > 0: a chunk is this many whole rows; 0: a chunk is a piece of one row
  int32_t pieces_per_row, piece_px;
  int64_t chunk0;                // first chunk of this launch (the canvas is encoded in slabs of chunks)
  unsigned long long* dbg;       // IST_PNG_PHASES (tuning): 8 clock samples per chunk
};
// the batch kernels' arguments: the chunks of many canvases in ONE launch (png_encode_batch_deflate), see "batch twins" below
struct DeflJob { const uint8_t* canvas; size_t pitch; int64_t w, h; int32_t rows_per_chunk, pieces_per_row, piece_px, pad_; };
struct DeflBatchArgs {
  const DeflJob* jobs;           // per file (device memory)
  const int64_t* chunk_begin;    // n_files + 1 (device memory)
  int32_t n_files;
  uint8_t* slots;
  uint32_t* len16; uint32_t* crc; uint32_t* ad_a; uint32_t* ad_b; uint32_t* ad_n;
  const uint32_t* tables; const uint32_t* xpow16;
};

__device__ __forceinline__ int padpos(int p) { return p + ((p >> 6) << 2); }

// Paeth residuals of one RGBA pixel (PNG spec 9.4): per channel the neighbour - left, up or upper left - closest to left +
// up - upper left, ties in that order.  Two channels at a time as packed 16-bit lanes (v_pk_sub_i16 / v_pk_max_i16 /
// v_pk_ashrrev_i16): pa = |up - ul|, pb = |left - ul|, pc = |(up - ul) + (left - ul)|; a comparison is the sign of a packed
// difference spread over its lane, a selection is a bit-field insert.  52 operations per pixel instead of ~85 byte-wise ones; the
// kernel is instruction-issue-bound (87 % of its issue slots busy, profiles/r03_counters_png.txt).
typedef short s16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ s16x2 as_s16x2(uint32_t v) { return __builtin_bit_cast(s16x2, v); }
__device__ __forceinline__ uint32_t as_u32(s16x2 v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ uint32_t paeth_pred2(uint32_t l, uint32_t u, uint32_t ul) {      // two channels, 16-bit lanes holding 0..255
  const s16x2 zero = {0, 0};
  const s16x2 d1 = as_s16x2(u) - as_s16x2(ul), d2 = as_s16x2(l) - as_s16x2(ul), d3 = d1 + d2;
  const s16x2 pa = __builtin_elementwise_max(d1, zero - d1), pb = __builtin_elementwise_max(d2, zero - d2), pc = __builtin_elementwise_max(d3, zero - d3);
  const uint32_t a_gt_b = as_u32((pb - pa) >> 15), a_gt_c = as_u32((pc - pa) >> 15), b_gt_c = as_u32((pc - pb) >> 15);      // all ones where greater
  const uint32_t not_a = a_gt_b | a_gt_c;
  const uint32_t u_or_ul = (ul & b_gt_c) | (u & ~b_gt_c);
  return (u_or_ul & not_a) | (l & ~not_a);
}
__device__ __forceinline__ uint32_t paeth4(uint32_t cur, uint32_t a, uint32_t b, uint32_t c) {
  const uint32_t m = 0x00FF00FFu;
  const uint32_t pe = paeth_pred2(a & m, b & m, c & m), po = paeth_pred2((a >> 8) & m, (b >> 8) & m, (c >> 8) & m);
  const uint32_t pred = pe | (po << 8);
  // cur - pred in every byte: borrow-free subtraction of the low seven bits, the top bits by xor
  return ((cur | 0x80808080u) - (pred & 0x7F7F7F7Fu)) ^ ((cur ^ ~pred) & 0x80808080u);
}
// the residuals of one pixel under filter type ft (the adaptive kernels): None, Sub, Up, Average = (left + up) >> 1 per channel in
// 16-bit lanes (the bit a shift carries out of the upper lane falls into the masked half of the lower one), Paeth as above
__device__ __forceinline__ uint32_t filter4(uint32_t ft, uint32_t cur, uint32_t a, uint32_t b, uint32_t c) {
  const uint32_t m = 0x00FF00FFu;
  uint32_t pred;
  if (ft == 4) pred = paeth_pred2(a & m, b & m, c & m) | (paeth_pred2((a >> 8) & m, (b >> 8) & m, (c >> 8) & m) << 8);
  else if (ft == 3) pred = ((((a & m) + (b & m)) >> 1) & m) | ((((((a >> 8) & m) + ((b >> 8) & m)) >> 1) & m) << 8);
  else pred = ft == 1 ? a : (ft == 2 ? b : 0u);
  return ((cur | 0x80808080u) - (pred & 0x7F7F7F7Fu)) ^ ((cur ^ ~pred) & 0x80808080u);
}

// deflate length symbol for a match of l bytes (3 <= l <= 63: a match never leaves its 64-byte span, whose first byte is a literal;
// symbols 257 .. 276, at most 3 extra bits): symbol, extra-bit count, extra-bit value
__device__ __forceinline__ void len_code(int l, int* sym, int* eb, int* ev) {
  const int m = l - 3;
  if (m < 8) { *sym = 257 + m; *eb = 0; *ev = 0; return; }
  const int e = (31 - __builtin_clz(m)) - 2;
  *sym = 257 + 4 * (e + 1) + ((m >> e) & 3); *eb = e; *ev = m & ((1 << e) - 1);
}

struct BitWriter {
  uint32_t* w; unsigned long long acc; int n; int wp;
  __device__ void init(uint32_t* words, int bitpos) { w = words; wp = bitpos >> 5; n = bitpos & 31; acc = 0; }
  __device__ void put(uint32_t v, int bits) {
    acc |= static_cast<unsigned long long>(v) << n; n += bits;
    if (n >= 32) { atomicOr(&w[wp++], static_cast<uint32_t>(acc)); acc >>= 32; n -= 32; }
  }
  __device__ void flush() { if (n > 0 && acc) atomicOr(&w[wp], static_cast<uint32_t>(acc)); }
};

__device__ __forceinline__ void or_bits(uint32_t* w, int bitpos, uint32_t v, int bits) {
  const int wp = bitpos >> 5, sh = bitpos & 31;
  if (v) {
    atomicOr(&w[wp], v << sh);
    if (sh + bits > 32) atomicOr(&w[wp + 1], v >> (32 - sh));
  }
}

__device__ __forceinline__ uint32_t rev_bits(uint32_t code, int len) { return __brev(code) >> (32 - len); }

// The span lives in REGISTERS (16 dwords): the LDS image of the filtered chunk is dead once every thread holds its span, so
// the output bit buffer takes its place (one 17 KiB buffer instead of two: 6 workgroups per CU instead of 4 - the kernel's
// clock is LDS latency, so residency is throughput).  The walk's dword loop has a wave-uniform trip count, which makes the
// register pick a scalar jump.
__device__ __forceinline__ uint32_t span_word(const uint32_t (&sp)[16], int d) {
  switch (d) {
    case 0: return sp[0]; case 1: return sp[1]; case 2: return sp[2]; case 3: return sp[3];
    case 4: return sp[4]; case 5: return sp[5]; case 6: return sp[6]; case 7: return sp[7];
    case 8: return sp[8]; case 9: return sp[9]; case 10: return sp[10]; case 11: return sp[11];
    case 12: return sp[12]; case 13: return sp[13]; case 14: return sp[14]; default: return sp[15];
  }
}

// Which bytes of a span are literals and where its matches start, as 64-bit masks - computed once per walk, so that the walk
// itself carries no run state from byte to byte (the stateful walk cost ~23 instructions per byte in each of the three
// passes; this one ~6).  eq bit i: byte i equals byte i-1.  A run of R >= 4 equal bytes is its first byte as a literal + ONE
// match of R - 1 bytes at distance 1, shorter runs are literals: `covered` = the bytes inside matches = every eq position that
// belongs to three consecutive eq bits; a match starts where a covered stretch starts and is as long as the stretch.
// (eq is returned too: the window parse measures its runs on it.  Splitting the function into eq and the run masks adds an instruction
// to each of deflate_chunk's kernels.)
struct SpanMasks { unsigned long long lit, mstart, covered, eq; };
__device__ __forceinline__ SpanMasks span_masks(const uint32_t (&sp)[16], int n) {
  unsigned long long eq = 0;
#pragma unroll
  for (int d = 0; d < 16; ++d) {
    const uint32_t w = sp[d];
    const uint32_t prev = d ? (sp[d ? d - 1 : 0] >> 24) : (~w & 0xFFu);            // (byte 0 has no predecessor: never equal)
    const uint32_t x = w ^ ((w << 8) | prev);                                      // a zero byte where a byte equals the one before it
    const uint32_t nz = (((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;     // 0x80 in every NON-zero byte (exact)
    const uint32_t z = (nz ^ 0x80808080u) >> 7;                                    // bit 0 / 8 / 16 / 24: the byte is zero
    const uint32_t nib = ((z * 0x00204081u) >> 21) & 15u;                          // those four bits side by side
    eq |= static_cast<unsigned long long>(nib) << (4 * d);
  }
  const unsigned long long valid = n >= 64 ? ~0ull : ((1ull << n) - 1ull);
  eq &= valid & ~1ull;
  const unsigned long long t = eq & (eq >> 1) & (eq >> 2);                         // bit i: bytes i-1 .. i+2 are equal
  SpanMasks m;
  m.covered = (t | (t << 1) | (t << 2)) & valid;
  m.lit = valid & ~m.covered;
  m.mstart = m.covered & ~(m.covered << 1);
  m.eq = eq;
  return m;
}

// One pass of a thread over its span.  PASS 0: histogram; 1: count bits; 2: emit.  The span is read as 16 dwords (the
// padded layout keeps every span 4-byte aligned); the dword loop has a wave-uniform trip count, which makes the register
// pick a scalar jump.
template <int PASS>
__device__ __forceinline__ int walk_span(const uint32_t (&sp)[16], int n, const SpanMasks& M, uint32_t* hist, const uint32_t* clen, const uint32_t* code, BitWriter* bw) {
  int bits = 0;
  if (PASS != 2) {                                   // matches in any order: a loop over the (few) places where one starts
    unsigned long long ms = M.mstart;
    while (ms) {
      const int i = __ffsll(static_cast<long long>(ms)) - 1;
      ms &= ms - 1ull;
      const unsigned long long rest = ~(M.covered >> i);
      const int mlen = rest ? __ffsll(static_cast<long long>(rest)) - 1 : 64 - i;       // 3 .. 63 covered bytes in a row
      int msym, meb, mev;
      len_code(mlen, &msym, &meb, &mev);
      if (PASS == 0) atomicAdd(&hist[msym], 1u);
      else bits += static_cast<int>(clen[msym]) + meb + 1;
    }
  }
#pragma unroll 1
  for (int d = 0; d < 16; ++d) {
    if (4 * d >= n) break;                           // (wave-uniform only in full chunks; a scalar branch there)
    const uint32_t w = span_word(sp, d);
    const uint32_t lit4 = static_cast<uint32_t>(M.lit >> (4 * d)) & 15u;
    if (PASS != 2) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t b = (w >> (8 * k)) & 255u;
        if (lit4 & (1u << k)) {
          if (PASS == 0) atomicAdd(&hist[b], 1u);
          else bits += static_cast<int>(clen[b]);
        }
      }
    } else {
      // emission, two bytes per put: a byte that is no literal contributes zero bits (a select, not a branch), so the pair's
      // codes go out as ONE word of at most 30 bits; the match that starts at one of the two positions - its bytes are no
      // literals, so the order inside the pair does not matter - follows in a rarely taken branch
      const uint32_t ms4 = static_cast<uint32_t>(M.mstart >> (4 * d)) & 15u;
#pragma unroll
      for (int k = 0; k < 4; k += 2) {
        const uint32_t p0 = code[(w >> (8 * k)) & 255u], p1 = code[(w >> (8 * k + 8)) & 255u];      // (code[] carries the length in its upper half)
        const uint32_t c0 = (lit4 & (1u << k)) ? p0 : 0u, c1 = (lit4 & (2u << k)) ? p1 : 0u;
        const uint32_t l0 = c0 >> 16;
        bw->put((c0 & 0xFFFFu) | ((c1 & 0xFFFFu) << l0), static_cast<int>(l0 + (c1 >> 16)));
        if (ms4 & (3u << k)) {                       // the match behind a run's first byte (distance 1: one zero bit)
          const int i = 4 * d + k + ((ms4 >> k) & 1u ? 0 : 1);
          const unsigned long long rest = ~(M.covered >> i);
          const int mlen = rest ? __ffsll(static_cast<long long>(rest)) - 1 : 64 - i;
          int msym, meb, mev;
          len_code(mlen, &msym, &meb, &mev);
          const uint32_t pm = code[msym];
          bw->put(pm & 0xFFFFu, static_cast<int>(pm >> 16));
          if (meb) bw->put(static_cast<uint32_t>(mev), meb);
          bw->put(0u, 1);
        }
      }
    }
  }
  return bits;
}

// ---- The steps of a chunk as functions: deflate_chunk_window below is made of them, deflate_chunk of those that leave the machine
// code of its eight kernels as it was (span load, span masks, block header, pads, Adler report, step E; the batch kernels' unpack) -
// the other steps it states inline, each with a note.  Whether a step can be shared there is decided by compiling, not by reading:
// a function is simplified on its own before it is inlined, and with the constants of ALL its callers (block_header is a template
// for that reason: the window body's call would otherwise change what the run form's call compiles to).  The LDS arrays belong to
// the two bodies and come in as pointers.

// which pixels: rows [y0, y0 + nrows) x columns [x0, x0 + npr); the filter byte belongs to the piece with x0 == 0.  bpp: bytes of a
// pixel in the filtered stream; rowlen and len = rowlen * nrows (<= CH by construction) are counted in those
struct ChunkRect { int64_t y0; int nrows, x0, npr, hasf, rowlen, len; };
__device__ __forceinline__ ChunkRect chunk_rect(const DeflArgs& P, const int64_t chunk, const int bpp) {
  ChunkRect R;
  if (P.rows_per_chunk > 0) {
    R.y0 = chunk * P.rows_per_chunk; R.nrows = static_cast<int>(min(static_cast<int64_t>(P.rows_per_chunk), P.h - R.y0)); R.x0 = 0; R.npr = static_cast<int>(P.w);
  } else {
    R.y0 = chunk / P.pieces_per_row; R.nrows = 1;
    const int piece = static_cast<int>(chunk - R.y0 * P.pieces_per_row);
    R.x0 = piece * P.piece_px; R.npr = static_cast<int>(min(static_cast<int64_t>(P.piece_px), P.w - R.x0));
  }
  R.hasf = R.x0 == 0 ? 1 : 0;
  R.rowlen = R.hasf + bpp * R.npr;
  R.len = R.rowlen * R.nrows;
  return R;
}

// A. load + filter into the padded LDS image.  bpp: 4 (RGBA, colour type 6) or 3 (RGB, colour type 2: the canvas is still read a
// dword per pixel, the alpha byte of the residual is not stored).  ftab: the filter type of canvas row y is ftab[y] (written by the
// row-filter pre-pass); null: 4 on every row.  Four pixels per thread and round, all sixteen loads issued before the first filter.
__device__ __forceinline__ void filter_chunk(const DeflArgs& P, const ChunkRect& R, const uint8_t* ftab, const int bpp, uint8_t* filt) {
  const int npix = R.npr * R.nrows;
  for (int q0 = threadIdx.x; q0 < npix; q0 += 1024) {
    uint32_t cur[4], a[4], b[4], c[4], ft[4]; int pos[4]; bool on[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int q = q0 + 256 * u;
      on[u] = q < npix;
      cur[u] = a[u] = b[u] = c[u] = 0u; pos[u] = 0; ft[u] = 4u;
      if (on[u]) {
        const int r = R.nrows == 1 ? 0 : q / R.npr, xx = q - r * R.npr;      // (one row per chunk - every image wider than 2047 px - needs no division)
        const int64_t y = R.y0 + r; const int x = R.x0 + xx;
        const uint8_t* row = P.canvas + static_cast<size_t>(y) * P.pitch;
        cur[u] = *reinterpret_cast<const uint32_t*>(row + 4 * static_cast<size_t>(x));
        if (x > 0) a[u] = *reinterpret_cast<const uint32_t*>(row + 4 * static_cast<size_t>(x - 1));
        if (y > 0) {
          b[u] = *reinterpret_cast<const uint32_t*>(row - P.pitch + 4 * static_cast<size_t>(x));
          if (x > 0) c[u] = *reinterpret_cast<const uint32_t*>(row - P.pitch + 4 * static_cast<size_t>(x - 1));
        }
        pos[u] = r * R.rowlen + R.hasf + bpp * xx;
        if (ftab) ft[u] = static_cast<uint32_t>(ftab[y]);
        if (R.hasf && xx == 0) filt[padpos(r * R.rowlen)] = static_cast<uint8_t>(ft[u]);      // filter type of the row
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (!on[u]) continue;
      const uint32_t fv = filter4(ft[u], cur[u], a[u], b[u], c[u]);
#pragma unroll
      for (int k = 0; k < 4; ++k) if (k < bpp) filt[padpos(pos[u] + k)] = static_cast<uint8_t>(fv >> (8 * k));
    }
  }
}

// a thread's span out of the padded LDS image into registers
__device__ __forceinline__ void load_span(const uint8_t* filt, const int tid, uint32_t (&sp)[16]) {
  const u32x4* mine = reinterpret_cast<const u32x4*>(filt + tid * (SPAN + 4));      // (68-byte pitch: 4-byte aligned)
  const uint32_t* mw = reinterpret_cast<const uint32_t*>(mine);
#pragma unroll
  for (int d = 0; d < 16; ++d) sp[d] = mw[d];
}

// Adler-32 partials of the chunk's filtered bytes: the sum of the bytes and their sum weighted with the distance from the chunk's end,
// mod 65521, per wave into wsum[0..3] and wsum[4..7]; behind a barrier thread 0 reports their totals and the byte count
__device__ __forceinline__ void adler_partials(const uint32_t (&sp)[16], const int n, const int base, const int len, uint32_t* wsum) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t a1 = 0, a2 = 0;
#pragma unroll
  for (int d = 0; d < 16; ++d)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = 4 * d + k;
      const uint32_t b = i < n ? (sp[d] >> (8 * k)) & 255u : 0u;
      a1 += b; a2 += static_cast<uint32_t>(len - (base + i)) * b;
    }
  a2 %= 65521u;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { a1 += __shfl_xor(a1, off); a2 += __shfl_xor(a2, off); }
  if (lane == 0) { wsum[wave] = a1; wsum[4 + wave] = a2; }
}
__device__ __forceinline__ void adler_report(const DeflArgs& P, const int64_t chunk, const uint32_t* wsum, const int len) {
  P.ad_a[chunk] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  P.ad_b[chunk] = (wsum[4] + wsum[5] + wsum[6] + wsum[7]) % 65521u;
  P.ad_n[chunk] = static_cast<uint32_t>(len);
}

// C. The code rule (Shannon lengths, then the slack handed back in up to 16 rounds; canonical codes) for ONE WAVE over nsym <= 320
// symbols: lane j holds symbols j, 64 + j, ... 256 + j.  Writes clen[] and code[] (code | length << 16, bit-reversed) and returns whether
// the code is complete.  single: the distance code's two special cases - one symbol in use gets length 1, none in use gives symbol 0
// length 1 (what the run form's header says).
__device__ __forceinline__ bool build_code(const uint32_t* hist, uint32_t* clen, uint32_t* code, const int nsym, const int lane, const bool single) {
  uint32_t cnt[5]; int ln[5];
  uint32_t tot = 0;
  int used = 0;
#pragma unroll
  for (int q = 0; q < 5; ++q) { const int sy = 64 * q + lane; cnt[q] = sy < nsym ? hist[sy] : 0u; tot += cnt[q]; used += __popcll(__ballot(cnt[q] != 0u)); }
  if (single && used <= 1) {
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      const int sy = 64 * q + lane;
      if (sy < nsym) { const bool it = used ? cnt[q] != 0u : sy == 0; clen[sy] = it ? 1u : 0u; code[sy] = it ? (1u << 16) : 0u; }
    }
    return true;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) tot += __shfl_xor(tot, off);
  int kraft = 0, cls[16];
#pragma unroll
  for (int l = 0; l < 16; ++l) cls[l] = 0;
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    ln[q] = 0;
    if (cnt[q]) {
      const uint32_t r = (tot + cnt[q] - 1) / cnt[q];
      int l = r <= 1u ? 0 : 32 - __clz(static_cast<int>(r - 1u));
      l = l < 1 ? 1 : (l > 15 ? 15 : l);
      ln[q] = l;
      kraft += 1 << (15 - l);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) kraft += __shfl_xor(kraft, off);
#pragma unroll
  for (int l = 1; l < 16; ++l) {
    int c = 0;
#pragma unroll
    for (int q = 0; q < 5; ++q) c += __popcll(__ballot(ln[q] == l));
    cls[l] = c;
  }
  const unsigned long long below = (1ull << lane) - 1ull;
  auto ranks_in = [&](int l, int (&rk)[5]) {
    int acc = 0;
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      const unsigned long long m = __ballot(ln[q] == l);
      rk[q] = acc + __popcll(m & below);
      acc += __popcll(m);
    }
  };
  int slack = 32768 - kraft;
  for (int round = 0; round < 16 && slack > 0; ++round) {
#pragma unroll
    for (int l = 2; l < 16; ++l) {
      const int cost = 1 << (15 - l);
      const int take = min(cls[l], slack / cost);
      if (take > 0) {
        int rk[5];
        ranks_in(l, rk);
#pragma unroll
        for (int q = 0; q < 5; ++q) if (ln[q] == l && rk[q] < take) ln[q] = l - 1;
        cls[l] -= take; cls[l - 1] += take; slack -= take * cost;
      }
    }
  }
  if (slack != 0 || tot == 0) return false;
  int first[16]; int cd = 0;
  first[0] = 0;
#pragma unroll
  for (int l = 1; l < 16; ++l) { cd = (cd + cls[l - 1]) << 1; first[l] = cd; }
  int cdq[5] = {0, 0, 0, 0, 0};
#pragma unroll
  for (int l = 1; l < 16; ++l) {
    if (cls[l] == 0) continue;
    int rk[5];
    ranks_in(l, rk);
#pragma unroll
    for (int q = 0; q < 5; ++q) if (ln[q] == l) cdq[q] = first[l] + rk[q];
  }
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    const int sy = 64 * q + lane;
    if (sy < nsym) {
      clen[sy] = static_cast<uint32_t>(ln[q]);
      code[sy] = ln[q] ? (rev_bits(static_cast<uint32_t>(cdq[q]), ln[q]) | (static_cast<uint32_t>(ln[q]) << 16)) : 0u;
    }
  }
  return true;
}

// header of a dynamic block at bit 8 lead: BFINAL 0, BTYPE 2, HLIT 29, HDIST hdist, HCLEN 15, the 19 code-length-code lengths, then
// the 286 + hdist + 1 code lengths.  Code-length alphabet: symbols 0..15 all 4 bits long (a complete code: canonical code of symbol
// s = s), 16-18 unused.  dclen: the distance code's lengths; null (hdist 0) for the run form's one distance code of 1 bit.
template <bool DIST>
__device__ __forceinline__ void block_header(uint32_t* outw, const int lead, const int hdist, const uint32_t* clen, const uint32_t* dclen, const int tid) {
  uint8_t* outb = reinterpret_cast<uint8_t*>(outw);
  const int hb = lead * 8;
  if (tid == 0) {
    if (lead) { outb[0] = 0x78; outb[1] = 0x01; }
    or_bits(outw, hb, 4u | (29u << 3) | (static_cast<uint32_t>(hdist) << 8) | (15u << 13), 17);
  }
  if (tid < 19) or_bits(outw, hb + 17 + 3 * tid, tid < 3 ? 0u : 4u, 3);       // order 16,17,18,0,8,7,...: first three are unused
  for (int s = tid; s < NSYM + hdist + 1; s += 256) {
    const uint32_t l = s < NSYM ? clen[s] : (dclen ? dclen[s - NSYM] : 1u);
    or_bits(outw, hb + 17 + 57 + 4 * s, rev_bits(l, 4), 4);
  }
}

// the end of a dynamic block whose tokens end at bit end_bit - clen[256]: the end-of-block symbol, then the empty stored block that
// re-aligns to a byte.  Returns the bytes before the alignment pads.
__device__ __forceinline__ int block_end(uint32_t* outw, const int end_bit, const uint32_t* clen, const uint32_t* code, const int tid) {
  uint8_t* outb = reinterpret_cast<uint8_t*>(outw);
  if (tid == 0) or_bits(outw, end_bit - static_cast<int>(clen[256]), code[256] & 0xFFFFu, static_cast<int>(clen[256]));
  int body_end = (end_bit + 3 + 7) / 8;               // 3 zero bits: BFINAL 0, BTYPE 00; then to the byte boundary
  __syncthreads();
  if (tid == 0) { outb[body_end + 2] = 0xFF; outb[body_end + 3] = 0xFF; }      // LEN 0000, NLEN FFFF
  return body_end + 4;
}

// the stored form of a chunk: every thread writes its span behind the 5-byte block header.  Returns the bytes before the alignment pads.
__device__ __forceinline__ int stored_form(uint8_t* outb, const int lead, const int len, const uint32_t (&sp)[16], const int n, const int base, const int tid) {
  if (tid == 0) {
    if (lead) { outb[0] = 0x78; outb[1] = 0x01; }
    uint8_t* q = outb + lead;
    q[0] = 0; q[1] = len & 0xFF; q[2] = (len >> 8) & 0xFF; q[3] = (~len) & 0xFF; q[4] = ((~len) >> 8) & 0xFF;
  }
#pragma unroll
  for (int d = 0; d < 16; ++d)
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (4 * d + k < n) outb[lead + 5 + base + 4 * d + k] = static_cast<uint8_t>(sp[d] >> (8 * k));
  return lead + 5 + len;
}

// (thread 0) pads the chunk to a multiple of 16 bytes with empty stored blocks - 00 00 00 FF FF - and reports its length
__device__ __forceinline__ void pad_chunk(const DeflArgs& P, const int64_t chunk, uint8_t* outb, const int body_end, int* out_len) {
  int total = body_end;
  while (total & 15) { outb[total + 3] = 0xFF; outb[total + 4] = 0xFF; total += 5; }
  *out_len = total;
  P.len16[chunk] = static_cast<uint32_t>(total >> 4);
}

// E. write the chunk to its slot; raw CRC of its bytes (each 16-byte unit shifted to the end of the chunk).  area: 1024 words that are
// dead by now and take the CRC tables
__device__ __forceinline__ void write_slot(const DeflArgs& P, const int64_t chunk, const uint32_t* outw, const int* s_out_len, uint32_t* area, uint32_t* wsum) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t (*const T)[256] = reinterpret_cast<uint32_t (*)[256]>(area);
  for (int i = tid; i < 1024; i += 256) area[i] = P.tables[i];
  __syncthreads();
  const int out_len = *s_out_len;
  uint8_t* slot = P.slots + static_cast<size_t>(chunk) * SLOT;
  uint32_t crc = 0;
  for (int u = tid; u < (out_len >> 4); u += 256) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(outw + 4 * u);
    *reinterpret_cast<u32x4*>(slot + 16 * static_cast<size_t>(u)) = v;
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t c = 0;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      c ^= w[d];
      c = T[3][c & 0xFF] ^ T[2][(c >> 8) & 0xFF] ^ T[1][(c >> 16) & 0xFF] ^ T[0][c >> 24];
    }
    crc ^= gf_mul(P.xpow16[(out_len >> 4) - 1 - u], c);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) crc ^= __shfl_xor(crc, off);
  __syncthreads();
  if (lane == 0) wsum[wave] = crc;
  __syncthreads();
  if (tid == 0) P.crc[chunk] = wsum[0] ^ wsum[1] ^ wsum[2] ^ wsum[3];
}

// One workgroup compresses chunk `chunk` of the canvas P describes (the body of the compressing kernels below).  BPP: bytes of a
// pixel in the filtered stream - 4 or 3; ADAPT: the row types come from ftab.  Only step A knows either; from step B on a chunk is bytes.
template <int BPP, bool ADAPT = false>
__device__ __forceinline__ void deflate_chunk(const DeflArgs& P, const int64_t chunk, const uint8_t* ftab = nullptr) {
  // ONE buffer, two lives: the filtered chunk (padded layout) until every thread has taken its span into registers, then the
  // Huffman scratch and the output bit stream
  static_assert(PADDED >= SLOT, "the output buffer aliases the filtered chunk");
  __shared__ __attribute__((aligned(16))) uint32_t buf[PADDED / 4];
  uint8_t* const filt = reinterpret_cast<uint8_t*>(buf);
  uint32_t* const outw = buf;
  // one LDS area, two lives: histogram / code lengths / codes while the block is built, then the CRC tables
  __shared__ __attribute__((aligned(16))) uint32_t area[1024];      // (>= 3 * 288)
  uint32_t* const hist = area; uint32_t* const clen = area + 288; uint32_t* const code = area + 576;
  __shared__ uint32_t wsum[8];
  __shared__ int s_out_len, s_skip;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // ---- which pixels.  (chunk_rect states this for the window body.  Sharing it here changes the pinned code objects: in each of five
  // forms the two adaptive batch kernels come out with other scalar registers, at 6214 and 6190 instructions as before.)
  int64_t y0; int nrows, x0, npr;
  if (P.rows_per_chunk > 0) {
    y0 = chunk * P.rows_per_chunk; nrows = static_cast<int>(min(static_cast<int64_t>(P.rows_per_chunk), P.h - y0)); x0 = 0; npr = static_cast<int>(P.w);
  } else {
    y0 = chunk / P.pieces_per_row; nrows = 1;
    const int piece = static_cast<int>(chunk - y0 * P.pieces_per_row);
    x0 = piece * P.piece_px; npr = static_cast<int>(min(static_cast<int64_t>(P.piece_px), P.w - x0));
  }
  const int hasf = x0 == 0 ? 1 : 0;
  const int rowlen = hasf + BPP * npr;
  const int len = rowlen * nrows;                // <= CH by construction

  for (int i = tid; i < 288; i += 256) { hist[i] = 0; clen[i] = 0; code[i] = 0; }
  if (P.dbg && tid == 0) P.dbg[chunk * 8 + 0] = wall_clock64();
  // ---- A. load + filter into LDS.  (filter_chunk states this for the window body.  Sharing it here changes the pinned code objects,
  // as a template on BPP and ADAPT too: ist_png_deflate_kernel 6147 -> 6129 instructions, the adaptive kernel 6285 -> 6303.)
  const int npix = npr * nrows;
  // (adaptive, a chunk of one row or a piece of one: its type is one scalar load for the workgroup)
  uint32_t ft_row = 4u;
  if constexpr (ADAPT) { if (nrows == 1) ft_row = ((ConstPtr<uint8_t>)ftab)[y0]; }
  // four pixels per thread and round, all sixteen loads issued before the first filter: the one-pixel-per-iteration form
  // had four loads in flight per thread and spent 15 us of a chunk's 96 waiting for them (IST_PNG_PHASES, measured)
  for (int q0 = tid; q0 < npix; q0 += 1024) {
    uint32_t cur[4], a[4], b[4], c[4]; int pos[4]; bool first[4], on[4];
    [[maybe_unused]] uint32_t ft[4] = {4u, 4u, 4u, 4u};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int q = q0 + 256 * u;
      on[u] = q < npix;
      cur[u] = a[u] = b[u] = c[u] = 0u; pos[u] = 0; first[u] = false;
      if (on[u]) {
        const int r = nrows == 1 ? 0 : q / npr, xx = q - r * npr;      // (one row per chunk - every image wider than 2047 px - needs no division)
        const int64_t y = y0 + r; const int x = x0 + xx;
        const uint8_t* row = P.canvas + static_cast<size_t>(y) * P.pitch;
        cur[u] = *reinterpret_cast<const uint32_t*>(row + 4 * static_cast<size_t>(x));
        if (x > 0) a[u] = *reinterpret_cast<const uint32_t*>(row + 4 * static_cast<size_t>(x - 1));
        if (y > 0) {
          b[u] = *reinterpret_cast<const uint32_t*>(row - P.pitch + 4 * static_cast<size_t>(x));
          if (x > 0) c[u] = *reinterpret_cast<const uint32_t*>(row - P.pitch + 4 * static_cast<size_t>(x - 1));
        }
        pos[u] = r * rowlen + hasf + BPP * xx;
        first[u] = hasf && xx == 0;
        if constexpr (ADAPT) {
          ft[u] = nrows == 1 ? ft_row : static_cast<uint32_t>(ftab[y]);
          if (first[u]) filt[padpos(r * rowlen)] = static_cast<uint8_t>(ft[u]);
        } else
        if (first[u]) filt[padpos(r * rowlen)] = 4;              // filter type of the row
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (!on[u]) continue;
      uint32_t fv;
      if constexpr (ADAPT) fv = filter4(ft[u], cur[u], a[u], b[u], c[u]);
      else fv = paeth4(cur[u], a[u], b[u], c[u]);
#pragma unroll
      for (int k = 0; k < BPP; ++k) filt[padpos(pos[u] + k)] = static_cast<uint8_t>(fv >> (8 * k));
    }
  }
  __syncthreads();

  if (P.dbg && tid == 0) P.dbg[chunk * 8 + 1] = wall_clock64();
  // ---- B. histogram (+ the end-of-block symbol), Adler partials
  const int base = tid * SPAN;
  const int n = max(0, min(SPAN, len - base));
  uint32_t sp[16];
  load_span(filt, tid, sp);
  __syncthreads();                                   // every span is in registers: the buffer is free
  walk_span<0>(sp, n, span_masks(sp, n), hist, nullptr, nullptr, nullptr);
  if (tid == 0) atomicAdd(&hist[256], 1u);
  // (adler_partials states these sums for the window body.  Sharing it here changes the pinned code objects: ist_png_deflate_kernel
  // 6147 -> 6139 instructions.)
  uint32_t a1 = 0, a2 = 0;
#pragma unroll
  for (int d = 0; d < 16; ++d)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = 4 * d + k;
      const uint32_t b = i < n ? (sp[d] >> (8 * k)) & 255u : 0u;
      a1 += b; a2 += static_cast<uint32_t>(len - (base + i)) * b;
    }
  a2 %= 65521u;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { a1 += __shfl_xor(a1, off); a2 += __shfl_xor(a2, off); }
  if (lane == 0) { wsum[wave] = a1; wsum[4 + wave] = a2; }
  __syncthreads();
  if (tid == 0) adler_report(P, chunk, wsum, len);

  if (P.dbg && tid == 0) P.dbg[chunk * 8 + 2] = wall_clock64();
  // (build_code states this rule for the window body.  Sharing it here changes the pinned code objects: ist_png_deflate_kernel
  // 6147 -> 6123 instructions and its private segment 68 -> 72 bytes; as a template or moved verbatim 6128 and 6126.)
  // ---- C. code lengths and codes: ONE WAVE, in registers.  Not Huffman's algorithm: Shannon lengths (the smallest l with
  // count * 2^l >= total, <= 15 for a 16 KiB chunk; their Kraft sum is <= 1) and then the slack handed back - symbols
  // are shortened by one bit, shortest codes first, as long as the Kraft sum allows, round after round until the code is
  // COMPLETE (inflate rejects an incomplete literal/length code).  Every shortening costs a multiple of the smallest unit
  // left, so the rounds end with the slack at exactly zero (<= 12 rounds over 3000 random histograms; photo chunks need
  // 2-4).  Which symbols of a length class go first is decided by symbol index, so the file is the same on every run.
  // Against Huffman's lengths the token bits grow by 0.5 % (photo chunks) to 1.2 % (the bench's synthetic content; 2.3 % on noise,
  // which is stored anyway) - tools/sim_code_lengths.py -
  // and the sort (36-45 barrier steps), the serial two-queue merge (n - 1 dependent LDS round trips on one thread), the
  // depth walk and the 286-long rank loops are gone: 24 us of a chunk's ~90 (IST_PNG_PHASES) become a few.
  // Lane j holds symbols j, 64 + j, ... 256 + j.  A chunk whose code does not complete in 16 rounds is stored.
  const int lead = chunk == 0 ? 2 : 0;               // the zlib header travels with the first chunk
  __syncthreads();                                   // thread 0 has read the Adler partials out of wsum[]; hist[] is final
  if (tid == 0) s_skip = 0;
  if (wave == 0) {
    uint32_t cnt[5]; int ln[5];
    uint32_t tot = 0;
#pragma unroll
    for (int q = 0; q < 5; ++q) { const int sy = 64 * q + lane; cnt[q] = sy < NSYM ? hist[sy] : 0u; tot += cnt[q]; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) tot += __shfl_xor(tot, off);
    int kraft = 0, cls[16];                          // cls[l]: symbols of length l (wave-uniform)
#pragma unroll
    for (int l = 0; l < 16; ++l) cls[l] = 0;
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      ln[q] = 0;
      if (cnt[q]) {
        const uint32_t r = (tot + cnt[q] - 1) / cnt[q];                       // ceil(total / count), 1 .. 16385
        int l = r <= 1u ? 0 : 32 - __clz(static_cast<int>(r - 1u));           // ceil(log2(r))
        l = l < 1 ? 1 : (l > 15 ? 15 : l);
        ln[q] = l;
        kraft += 1 << (15 - l);
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) kraft += __shfl_xor(kraft, off);
#pragma unroll
    for (int l = 1; l < 16; ++l) {
      int c = 0;
#pragma unroll
      for (int q = 0; q < 5; ++q) c += __popcll(__ballot(ln[q] == l));
      cls[l] = c;
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    // rank of this lane's five symbols among the symbols of length l, in symbol order (q-major, then lane)
    auto ranks_in = [&](int l, int (&rk)[5]) {
      int acc = 0;
#pragma unroll
      for (int q = 0; q < 5; ++q) {
        const unsigned long long m = __ballot(ln[q] == l);
        rk[q] = acc + __popcll(m & below);
        acc += __popcll(m);
      }
    };
    int slack = 32768 - kraft;                       // >= 0 (Shannon lengths); 0 = complete
    for (int round = 0; round < 16 && slack > 0; ++round) {
#pragma unroll
      for (int l = 2; l < 16; ++l) {                 // (ascending: a symbol moved to l - 1 is not looked at again this round)
        const int cost = 1 << (15 - l);
        const int take = min(cls[l], slack / cost);
        if (take > 0) {                              // (wave-uniform)
          int rk[5];
          ranks_in(l, rk);
#pragma unroll
          for (int q = 0; q < 5; ++q) if (ln[q] == l && rk[q] < take) ln[q] = l - 1;
          cls[l] -= take; cls[l - 1] += take; slack -= take * cost;
        }
      }
    }
    if (slack != 0 || tot == 0) { if (lane == 0) s_skip = 1; }
    else {
      // canonical codes (RFC 1951 3.2.2): first code of every length, then symbol order inside a length; stored bit-reversed
      int first[16]; int cd = 0;
      first[0] = 0;
#pragma unroll
      for (int l = 1; l < 16; ++l) { cd = (cd + cls[l - 1]) << 1; first[l] = cd; }
      int cdq[5] = {0, 0, 0, 0, 0};
#pragma unroll
      for (int l = 1; l < 16; ++l) {
        if (cls[l] == 0) continue;                   // (wave-uniform)
        int rk[5];
        ranks_in(l, rk);
#pragma unroll
        for (int q = 0; q < 5; ++q) if (ln[q] == l) cdq[q] = first[l] + rk[q];
      }
#pragma unroll
      for (int q = 0; q < 5; ++q) {
        const int sy = 64 * q + lane;
        if (sy < NSYM) {
          clen[sy] = static_cast<uint32_t>(ln[q]);
          code[sy] = ln[q] ? (rev_bits(static_cast<uint32_t>(cdq[q]), ln[q]) | (static_cast<uint32_t>(ln[q]) << 16)) : 0u;
        }
      }
    }
  }
  __syncthreads();
  const bool skip = s_skip != 0;

  if (P.dbg && tid == 0) P.dbg[chunk * 8 + 3] = wall_clock64();
  // ---- D. bits per thread, exclusive scan, choice between the Huffman and the stored form
  const SpanMasks masks = span_masks(sp, n);         // (for the bit count and the emission: kept across the scan between them)
  const int mybits = skip ? 0 : walk_span<1>(sp, n, masks, nullptr, clen, nullptr, nullptr);
  int incl = mybits;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) { const int t = __shfl_up(incl, off); if (lane >= off) incl += t; }
  __syncthreads();                                   // outw scratch (weights) no longer needed by thread 0
  if (lane == 63) wsum[wave] = static_cast<uint32_t>(incl);
  __syncthreads();
  int wave_base = 0;
  for (int k = 0; k < wave; ++k) wave_base += static_cast<int>(wsum[k]);
  const int total_tok_bits = static_cast<int>(wsum[0] + wsum[1] + wsum[2] + wsum[3]);
  const int my_start = lead * 8 + HDR_BITS + wave_base + incl - mybits;
  const int end_bit = lead * 8 + HDR_BITS + total_tok_bits + static_cast<int>(clen[256]);
  const int huff_bytes = (end_bit + 3 + 7) / 8 + 4;  // + the empty stored block that re-aligns to a byte
  const bool stored = skip || huff_bytes >= lead + 5 + len;
  for (int i = tid; i < SLOT / 4; i += 256) outw[i] = 0;
  __syncthreads();
  if (P.dbg && tid == 0) P.dbg[chunk * 8 + 4] = wall_clock64();
  uint8_t* outb = reinterpret_cast<uint8_t*>(outw);
  int body_end;                                       // bytes before the alignment pads
  if (!stored) {
    block_header<false>(outw, lead, 0, clen, nullptr, tid);
    BitWriter bw; bw.init(outw, my_start);
    walk_span<2>(sp, n, masks, nullptr, clen, code, &bw);
    bw.flush();
    // (block_end states these five lines for the window body.  Sharing it here changes the pinned code objects: ist_png_deflate_kernel
    // 6147 -> 6172 instructions, returning the length or through a reference alike.)
    if (tid == 0) or_bits(outw, end_bit - static_cast<int>(clen[256]), code[256] & 0xFFFFu, static_cast<int>(clen[256]));
    body_end = (end_bit + 3 + 7) / 8;                 // 3 zero bits: BFINAL 0, BTYPE 00; then to the byte boundary
    __syncthreads();
    if (tid == 0) { outb[body_end + 2] = 0xFF; outb[body_end + 3] = 0xFF; }      // LEN 0000, NLEN FFFF
    body_end += 4;
  } else {
    // (stored_form states this for the window body.  Sharing it here changes the pinned code objects: ist_png_deflate_kernel
    // 6147 -> 6139 instructions, whole or split into its header and its span copy.)
    if (tid == 0) {
      if (lead) { outb[0] = 0x78; outb[1] = 0x01; }
      uint8_t* q = outb + lead;
      q[0] = 0; q[1] = len & 0xFF; q[2] = (len >> 8) & 0xFF; q[3] = (~len) & 0xFF; q[4] = ((~len) >> 8) & 0xFF;
    }
#pragma unroll
    for (int d = 0; d < 16; ++d)
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (4 * d + k < n) outb[lead + 5 + base + 4 * d + k] = static_cast<uint8_t>(sp[d] >> (8 * k));
    body_end = lead + 5 + len;
  }
  __syncthreads();
  if (tid == 0) pad_chunk(P, chunk, outb, body_end, &s_out_len);
  __syncthreads();

  if (P.dbg && tid == 0) P.dbg[chunk * 8 + 5] = wall_clock64();
  // ---- E. write the chunk to its slot; raw CRC of its bytes
  write_slot(P, chunk, outw, &s_out_len, area, wsum);
  if (P.dbg && tid == 0) P.dbg[chunk * 8 + 6] = wall_clock64();
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(7))) void ist_png_deflate_kernel(const DeflArgs P) {
  deflate_chunk<4>(P, P.chunk0 + blockIdx.x);
}
// the RGB form (IST_PNG_RGB): the same body on 3 bytes per pixel.  amdgpu_waves_per_eu(5), not 7: under the 72-register cap of 7 waves
// the body spills 16 VGPRs (68 bytes of private segment per thread, the 4-byte kernels' too); at 6 waves (80 registers) still 8; at 5 it
// has 96 registers, no spill and no private segment.  The price is resident waves: measured 1.69-1.71 ms against 1.54-1.55 ms for the
// spilling build on the 4032 x 27216 bench canvas (profiles/r13_png_rgb_waves.txt) - still below the RGBA form's 1.72-1.74 ms.  A body
// that fits 72 registers would serve both forms; it is a change of steps B - E.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5))) void ist_png_deflate_rgb_kernel(const DeflArgs P) {
  deflate_chunk<3>(P, P.chunk0 + blockIdx.x);
}

// ---- batch twins: the chunks of many canvases in ONE launch (png_encode_batch_deflate).  Chunks are numbered file-major;
// chunk_begin[f] is file f's first, chunk_begin[n_files] the total.  A file's per-chunk results and slots are the arrays'
// entries [chunk_begin[f], chunk_begin[f + 1]), so the body above runs unchanged on the file's own chunk numbers.

// workgroup blockIdx.x of a batch launch: its file *f, its chunk number *chunk in that file, and the arguments the file's own launch
// would have had (the file's slice of the slots and of the per-chunk results)
__device__ __forceinline__ DeflArgs batch_chunk(const DeflBatchArgs& B, int64_t* chunk, int* file) {
  const int64_t g = blockIdx.x;
  const int f = batch_file_of(B.chunk_begin, B.n_files, g);
  const int64_t base = ((ConstPtr<int64_t>)B.chunk_begin)[f];
  const DeflJob J = *(const DeflJob*)((ConstPtr<DeflJob>)B.jobs + f);
  DeflArgs P;
  P.canvas = J.canvas; P.pitch = J.pitch; P.w = J.w; P.h = J.h;
  P.slots = B.slots + static_cast<size_t>(base) * SLOT;
  P.len16 = B.len16 + base; P.crc = B.crc + base; P.ad_a = B.ad_a + base; P.ad_b = B.ad_b + base; P.ad_n = B.ad_n + base;
  P.tables = B.tables; P.xpow16 = B.xpow16;
  P.rows_per_chunk = J.rows_per_chunk; P.pieces_per_row = J.pieces_per_row; P.piece_px = J.piece_px;
  P.chunk0 = 0; P.dbg = nullptr;
  *chunk = g - base; *file = f;
  return P;
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(7))) void ist_png_deflate_batch_kernel(const DeflBatchArgs B) {
  int64_t chunk; int f;
  const DeflArgs P = batch_chunk(B, &chunk, &f);
  deflate_chunk<4>(P, chunk);
}

// the RGB form of the batch
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5))) void ist_png_deflate_rgb_batch_kernel(const DeflBatchArgs B) {
  int64_t chunk; int f;
  const DeflArgs P = batch_chunk(B, &chunk, &f);
  deflate_chunk<3>(P, chunk);
}

// ---- adaptive row filters (IST_PNG_FILTER_ADAPTIVE): the pre-pass that chooses a type per row, and the compressing kernels' twins
// that follow it.  The rule is stated at the top of this file.
//
// The pre-pass.  A lane takes four neighbouring pixels of row y and of row y - 1 as one 16-byte load each (+ the pixel left of them,
// an overlapping dword load), forms the five residuals of two channels at a time in packed 16-bit lanes - like paeth_pred2 - and adds
// |residual as a signed byte| into five packed sums (8 terms of at most 128 per 16-bit lane and round: no carry between the lanes),
// which it unpacks into five 32-bit sums per round.  The sums are integers: wave and workgroup reduction give the same numbers
// in any launch shape.  One lane takes the argmin in the tie order 4, 1, 2, 3, 0 and writes the byte with an ordinary store.
// LDS: the 4 x 5 reduction words.
//
// Launch shape (rows_per_group): a wave covers 256 pixels per round, a workgroup 1024.  Rows of up to kRowFilterWaveW = 1024
// pixels - previews, thumbnails, the 606-pixel plans - get a WAVE each, four rows per workgroup: such a row is at most four rounds
// of one wave, and a workgroup per row would leave three waves of four idle from the second round on (all of them below 257 px).
// Wider rows get the whole workgroup.
constexpr int kRowFilterWaveW = 1024;
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t abs_res2(s16x2 d) {            // per 16-bit lane: |d mod 256 read as a signed byte| = min(r, 256 - r)
  const s16x2 t = __builtin_bit_cast(s16x2, __builtin_bit_cast(u16x2, d) << 8) >> 8;
  const s16x2 zero = {0, 0};
  return as_u32(__builtin_elementwise_max(t, zero - t));
}
__device__ __forceinline__ void cost_pair(uint32_t x, uint32_t l, uint32_t u, uint32_t ul, uint32_t (&pk)[5]) {      // two channels, 16-bit lanes holding 0..255
  const s16x2 sx = as_s16x2(x), sl = as_s16x2(l), su = as_s16x2(u);
  pk[0] += abs_res2(sx);
  pk[1] += abs_res2(sx - sl);
  pk[2] += abs_res2(sx - su);
  pk[3] += abs_res2(sx - ((sl + su) >> 1));
  pk[4] += abs_res2(sx - as_s16x2(paeth_pred2(l, u, ul)));
}

struct RowFilterArgs {
  const uint8_t* canvas; size_t pitch; int64_t w, h;      // one file (jobs == nullptr): row number = canvas row
  const DeflJob* jobs;           // batch: per file (device memory), rows numbered file-major ...
  const int64_t* row_begin;      // ... row_begin[f] is file f's first, row_begin[n_files] the total
  int32_t n_files;
  int32_t rows_per_group;        // 4: a wave per row; 1: the workgroup's four waves share one row
  int64_t row0, n_rows;          // this launch: rows [row0, row0 + n_rows)
  uint8_t* table;                // table[row] = the type
};

template <int BPP>
__device__ __forceinline__ void row_filter_body(const RowFilterArgs& A) {
  __shared__ uint32_t part[4][5];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool per_wave = A.rows_per_group == 4;
  const int64_t g = A.row0 + (per_wave ? 4 * static_cast<int64_t>(blockIdx.x) + wave : static_cast<int64_t>(blockIdx.x));
  const bool live = g < A.row0 + A.n_rows;             // (wave-uniform; with a row per workgroup the same for all four waves)
  uint32_t acc[5] = {0u, 0u, 0u, 0u, 0u};
  if (live) {
    const uint8_t* canvas = A.canvas; size_t pitch = A.pitch; int64_t w = A.w, y = g;
    if (A.jobs) {
      const int f = batch_file_of(A.row_begin, A.n_files, g);
      const DeflJob J = *(const DeflJob*)((ConstPtr<DeflJob>)A.jobs + f);
      canvas = J.canvas; pitch = J.pitch; w = J.w; y = g - ((ConstPtr<int64_t>)A.row_begin)[f];
    }
    const uint8_t* row = canvas + static_cast<size_t>(y) * pitch;
    const int64_t first = per_wave ? lane : tid, step = per_wave ? 64 : 256;
    const uint32_t me = 0x00FF00FFu, mo = BPP == 4 ? 0x00FF00FFu : 0x000000FFu;      // (RGB: the alpha lane is zero everywhere - it costs nothing)
    for (int64_t x = 4 * first; x < w; x += 4 * step) {
      // c[0] / b[0]: the pixel left of the four (zero left of the image); b: the row above (zero above the image)
      uint32_t c[5] = {0u, 0u, 0u, 0u, 0u}, b[5] = {0u, 0u, 0u, 0u, 0u};
      const int npx = static_cast<int>(min(static_cast<int64_t>(4), w - x));
      const uint8_t* p = row + 4 * static_cast<size_t>(x);
      if (npx == 4) {
        const u32x4 v = *reinterpret_cast<const u32x4_a4*>(p);
        c[1] = v.x; c[2] = v.y; c[3] = v.z; c[4] = v.w;
        if (y > 0) { const u32x4 t = *reinterpret_cast<const u32x4_a4*>(p - pitch); b[1] = t.x; b[2] = t.y; b[3] = t.z; b[4] = t.w; }
      } else {
#pragma unroll
        for (int k = 0; k < 3; ++k)
          if (k < npx) {
            c[1 + k] = *reinterpret_cast<const uint32_t*>(p + 4 * k);
            if (y > 0) b[1 + k] = *reinterpret_cast<const uint32_t*>(p - pitch + 4 * k);
          }
      }
      if (x > 0) {
        c[0] = *reinterpret_cast<const uint32_t*>(p - 4);
        if (y > 0) b[0] = *reinterpret_cast<const uint32_t*>(p - pitch - 4);
      }
      uint32_t pk[5] = {0u, 0u, 0u, 0u, 0u};
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < npx) {
          cost_pair(c[k + 1] & me, c[k] & me, b[k + 1] & me, b[k] & me, pk);
          cost_pair((c[k + 1] >> 8) & mo, (c[k] >> 8) & mo, (b[k + 1] >> 8) & mo, (b[k] >> 8) & mo, pk);
        }
#pragma unroll
      for (int f = 0; f < 5; ++f) acc[f] += (pk[f] & 0xFFFFu) + (pk[f] >> 16);
    }
  }
#pragma unroll
  for (int f = 0; f < 5; ++f) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc[f] += __shfl_xor(acc[f], off);
    if (lane == 0) part[wave][f] = acc[f];
  }
  __syncthreads();
  if (live && lane == 0 && (per_wave || wave == 0)) {
    uint32_t cost[5];
#pragma unroll
    for (int f = 0; f < 5; ++f) cost[f] = per_wave ? part[wave][f] : part[0][f] + part[1][f] + part[2][f] + part[3][f];
    uint32_t best = 4u, least = cost[4];                // ties: the first of 4, 1, 2, 3, 0
    if (cost[1] < least) { best = 1u; least = cost[1]; }
    if (cost[2] < least) { best = 2u; least = cost[2]; }
    if (cost[3] < least) { best = 3u; least = cost[3]; }
    if (cost[0] < least) { best = 0u; }
    A.table[g] = static_cast<uint8_t>(best);
  }
}

__global__ __launch_bounds__(256) void ist_png_row_filter_kernel(const RowFilterArgs A) { row_filter_body<4>(A); }
__global__ __launch_bounds__(256) void ist_png_row_filter_rgb_kernel(const RowFilterArgs A) { row_filter_body<3>(A); }

// The compressing kernels' adaptive twins: the same body, step A following the table (a separate argument: DeflArgs / DeflBatchArgs
// are what the kernels above see, unchanged).  amdgpu_waves_per_eu(5) for both colour forms: step A holds one more value per pixel
// in flight (the type) and three more predictors' worth of code, and steps B - E are the body that already spills 16 VGPRs under the
// 72-register cap of 7 waves in the RGBA kernel; at 5 waves (96 registers) nothing spills and there is no private segment, as for the
// RGB kernel above and at the price measured there.  LDS is the body's 21544 bytes.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5))) void ist_png_deflate_adapt_kernel(const DeflArgs P, const uint8_t* ftab) {
  deflate_chunk<4, true>(P, P.chunk0 + blockIdx.x, ftab);
}
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5))) void ist_png_deflate_adapt_rgb_kernel(const DeflArgs P, const uint8_t* ftab) {
  deflate_chunk<3, true>(P, P.chunk0 + blockIdx.x, ftab);
}
// batch: file f's rows are table entries [row_begin[f], row_begin[f + 1])
template <int BPP>
__device__ __forceinline__ void deflate_adapt_batch_body(const DeflBatchArgs& B, const int64_t* row_begin, const uint8_t* ftab) {
  int64_t chunk; int f;
  const DeflArgs P = batch_chunk(B, &chunk, &f);
  deflate_chunk<BPP, true>(P, chunk, ftab + ((ConstPtr<int64_t>)row_begin)[f]);
}
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5))) void ist_png_deflate_adapt_batch_kernel(const DeflBatchArgs B, const int64_t* row_begin, const uint8_t* ftab) {
  deflate_adapt_batch_body<4>(B, row_begin, ftab);
}
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5))) void ist_png_deflate_adapt_rgb_batch_kernel(const DeflBatchArgs B, const int64_t* row_begin, const uint8_t* ftab) {
  deflate_adapt_batch_body<3>(B, row_begin, ftab);
}

// ---- window matches (IST_PNG_MATCH_WINDOW): the compressing kernels' window twins.  The rule is stated at the top of this file.
//
// One body for both colour forms and both row-filter settings (bpp and the table of row types are runtime arguments: only step A reads
// them, and this body is bound by LDS, not by registers), so two kernels: single and batch.  LDS of a workgroup, 75828 bytes (two
// workgroups on a CU of 160 KiB):
//   buf    17408  the filtered chunk, 4 pad bytes after every 64 - alive until the parse is done - then the output bit stream
//   candt  33792  16-bit entry per position, 2 pad entries after every 64 (a span is 33 dwords: a thread walking its own span and a wave
//                 walking one span are both conflict free): first H(p), then cand(p); 0xFFFF = no key / no candidate
//   htab   16384  the 4096-entry hash table: the latest position of every hash (32-bit, so that an LDS max resolves a round's inserts)
//   area    4096  run form: histogram, lengths, codes (+ its one distance code); later the CRC tables
//   area2   4096  window form: the same three and the distance histogram, lengths, codes
// Steps: A filter into buf.  B every thread takes its span into registers, writes H of its 64 positions; wave 0 then walks the spans in
// order - round s: lane i looks position 64 s + i up, then inserts it; a wave's LDS operations complete in order, so all look-ups of a
// round precede its inserts and follow those of the round before - while waves 1-3 already count the run form and their Adler sums.
// B2 every thread parses its span against the table (bytes compared in buf) into three 64-bit masks - literals, match starts, which
// matches are window matches; a match ends where the next token starts - and counts the window form.  C three waves build the three
// codes side by side.  D both forms' bits, two scans, the choice: stored or run as before, window where its padded chunk is smaller.  E as before.
constexpr int NDSYM = 30;                // distance symbols
constexpr int CAND_PITCH = 66;           // 16-bit entries per span in the candidate table
constexpr uint32_t NOCAND = 0xFFFFu;

// deflate distance symbol of distance d (1 .. 16383: symbols 0 .. 27): symbol, extra-bit count, extra-bit value
__device__ __forceinline__ void dist_code(int d, int* sym, int* eb, int* ev) {
  if (d <= 4) { *sym = d - 1; *eb = 0; *ev = 0; return; }
  const int t = d - 1, e = (31 - __builtin_clz(t)) - 1;
  *sym = 2 * (e + 1) + ((t >> e) & 1); *eb = e; *ev = t & ((1 << e) - 1);
}

// the four bytes at position p .. p + 3 of the filtered chunk (padded layout; p + 3 < CH), little-endian
__device__ __forceinline__ uint32_t load4(const uint32_t* buf, int p) {
  const int a = p & ~3, sh = 8 * (p & 3);
  const uint32_t lo = buf[padpos(a) >> 2], hi = buf[padpos(min(a + 4, CH - 4)) >> 2];      // (the last dword again where there is no next one: shifted out)
  return static_cast<uint32_t>(((static_cast<unsigned long long>(hi) << 32) | lo) >> sh);
}

// The tokens of a span in either form: bit i of lit - byte i is a literal; of mstart - a match starts at byte i and runs to the next
// token (or the span's end); of win - that match's distance is i - cand(i), otherwise 1.
struct SpanTokens { unsigned long long lit, mstart, win; };

// One pass of a thread over its tokens, in order.  PASS 0: histograms (dhist may be null: the run form's distances need none);
// 1: count bits; 2: emit.  cand: this span's row of the candidate table (read at window matches only); base: the span's first position.
template <int PASS>
__device__ __forceinline__ int walk_tokens(const uint32_t (&sp)[16], int n, const SpanTokens& M, const uint16_t* cand, const int base, uint32_t* hist, uint32_t* dhist,
                                           const uint32_t* clen, const uint32_t* dclen, const uint32_t* code, const uint32_t* dcode, BitWriter* bw) {
  int bits = 0;
  const unsigned long long tok = M.lit | M.mstart;
#pragma unroll 1
  for (int d = 0; d < 16; ++d) {
    if (4 * d >= n) break;
    const uint32_t lit4 = static_cast<uint32_t>(M.lit >> (4 * d)) & 15u, ms4 = static_cast<uint32_t>(M.mstart >> (4 * d)) & 15u;
    if (!(lit4 | ms4)) continue;
    const uint32_t w = span_word(sp, d);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = 4 * d + k;
      if (lit4 & (1u << k)) {
        const uint32_t b = (w >> (8 * k)) & 255u;
        if (PASS == 0) atomicAdd(&hist[b], 1u);
        else if (PASS == 1) bits += static_cast<int>(clen[b]);
        else { const uint32_t p = code[b]; bw->put(p & 0xFFFFu, static_cast<int>(p >> 16)); }
      } else if (ms4 & (1u << k)) {
        const unsigned long long next = (tok >> i) >> 1;
        const int mlen = next ? __ffsll(static_cast<long long>(next)) : n - i;
        const int dist = ((M.win >> i) & 1ull) ? base + i - static_cast<int>(cand[i]) : 1;
        int msym, meb, mev, dsym, deb, dev;
        len_code(mlen, &msym, &meb, &mev);
        dist_code(dist, &dsym, &deb, &dev);
        if (PASS == 0) { atomicAdd(&hist[msym], 1u); if (dhist) atomicAdd(&dhist[dsym], 1u); }
        else if (PASS == 1) bits += static_cast<int>(clen[msym]) + meb + static_cast<int>(dclen[dsym]) + deb;
        else {
          const uint32_t pm = code[msym], pd = dcode[dsym];
          bw->put(pm & 0xFFFFu, static_cast<int>(pm >> 16));
          if (meb) bw->put(static_cast<uint32_t>(mev), meb);
          bw->put(pd & 0xFFFFu, static_cast<int>(pd >> 16));
          if (deb) bw->put(static_cast<uint32_t>(dev), deb);
        }
      }
    }
  }
  return bits;
}

// One workgroup compresses chunk `chunk` with window matches.  bpp: 4 or 3; ftab: the row types of the adaptive filters, or null for
// Paeth on every row.
__device__ __forceinline__ void deflate_chunk_window(const DeflArgs& P, const int64_t chunk, const uint8_t* ftab, const int bpp) {
  static_assert(PADDED >= SLOT, "the output buffer aliases the filtered chunk");
  __shared__ __attribute__((aligned(16))) uint32_t buf[PADDED / 4];
  uint8_t* const filt = reinterpret_cast<uint8_t*>(buf);
  uint32_t* const outw = buf;
  __shared__ __attribute__((aligned(16))) uint32_t area[1024];       // (>= 3 * 288 + 2 * 32)
  __shared__ __attribute__((aligned(16))) uint32_t area2[1024];      // (>= 3 * 288 + 3 * 32)
  __shared__ int htab[4096];
  __shared__ __attribute__((aligned(4))) uint16_t candt[256 * CAND_PITCH];
  uint32_t* const hist = area; uint32_t* const clen = area + 288; uint32_t* const code = area + 576;
  uint32_t* const rdclen = area + 864; uint32_t* const rdcode = area + 896;                       // the run form's one distance code
  uint32_t* const hist2 = area2; uint32_t* const clen2 = area2 + 288; uint32_t* const code2 = area2 + 576;
  uint32_t* const dhist = area2 + 864; uint32_t* const dclen = area2 + 896; uint32_t* const dcode = area2 + 928;
  __shared__ uint32_t wsum[8];
  __shared__ int s_out_len, s_skip_run, s_skip_ll, s_skip_d, s_hdist;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const ChunkRect R = chunk_rect(P, chunk, bpp);
  const int len = R.len;

  for (int i = tid; i < 1024; i += 256) { area[i] = 0; area2[i] = 0; }
  for (int i = tid; i < 4096; i += 256) htab[i] = -1;
  if (P.dbg && tid == 0) P.dbg[chunk * 8 + 0] = wall_clock64();
  // ---- A. load + filter into LDS (the type of a row is 4 without a table)
  filter_chunk(P, R, ftab, bpp, filt);
  __syncthreads();
  // (behind the barrier: other waves zeroed these words above; they are first read in step D, several barriers on)
  if (tid == 0) { rdclen[0] = 1u; rdcode[0] = 1u << 16; }

  if (P.dbg && tid == 0) P.dbg[chunk * 8 + 1] = wall_clock64();
  // ---- B. spans into registers; H of every position; the candidate table (wave 0) beside the run form's histogram and the Adler partials
  const int base = tid * SPAN;
  const int n = max(0, min(SPAN, len - base));
  uint32_t sp[16];
  load_span(filt, tid, sp);
  uint16_t* const cand = candt + tid * CAND_PITCH;
  {
    const uint32_t nextw = tid < 255 ? *reinterpret_cast<const uint32_t*>(filt + (tid + 1) * (SPAN + 4)) : 0u;
    uint32_t* const cw = reinterpret_cast<uint32_t*>(cand);
#pragma unroll
    for (int j = 0; j < 32; ++j) {
      uint32_t pair = 0;
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int i = 2 * j + e, d = i >> 2, sh = 8 * (i & 3);
        const uint32_t lo = sp[d], hi = d < 15 ? sp[d < 15 ? d + 1 : 15] : nextw;
        const uint32_t key = sh ? (lo >> sh) | (hi << (32 - sh)) : lo;
        const uint32_t hv = base + i + 4 <= len ? (key * 2654435761u) >> 20 : NOCAND;
        pair |= hv << (16 * e);
      }
      cw[j] = pair;
    }
  }
  __syncthreads();                                   // every H is written (and every span is in registers)
  if (wave == 0) {
    const int nspans = (len + SPAN - 1) / SPAN;
    uint32_t hn = candt[lane];
    for (int s = 0; s < nspans; ++s) {
      uint16_t* const e = candt + s * CAND_PITCH + lane;
      const uint32_t h = hn;
      if (s + 1 < nspans) hn = e[CAND_PITCH];          // (the next round's hash is on its way while this round's look-up returns)
      if (h != NOCAND) {
        const int c = htab[h];
        *e = static_cast<uint16_t>(c < 0 ? NOCAND : static_cast<uint32_t>(c));
        atomicMax(&htab[h], SPAN * s + lane);
      }
    }
  }
  const SpanMasks RM = span_masks(sp, n);
  const unsigned long long eq = RM.eq;
  const SpanTokens RT{RM.lit, RM.mstart, 0ull};      // the run form
  walk_tokens<0>(sp, n, RT, cand, base, hist, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  if (tid == 0) { atomicAdd(&hist[256], 1u); atomicAdd(&hist2[256], 1u); }
  adler_partials(sp, n, base, len, wsum);
  __syncthreads();                                   // the candidate table is complete
  if (tid == 0) adler_report(P, chunk, wsum, len);
  if (P.dbg && tid == 0) P.dbg[chunk * 8 + 2] = wall_clock64();
  // ---- B2. the window parse of this span: greedy from its first byte
  // First, for all 64 positions at once (independent loads: their latency overlaps), whether the candidate's four key bytes are the
  // position's own - a hash collision, the usual case on photographs, ends here; a match of fewer than 4 bytes is no match, so only
  // positions that pass (and have 4 bytes left in the span) are measured in the serial walk, 4 bytes a step.
  unsigned long long ok4 = 0ull;
  {
    const uint32_t nextw = tid < 255 ? *reinterpret_cast<const uint32_t*>(filt + (tid + 1) * (SPAN + 4)) : 0u;
#pragma unroll
    for (int i = 0; i < 64; ++i) {
      const int d = i >> 2, sh = 8 * (i & 3);
      const uint32_t lo = sp[d], hi = d < 15 ? sp[d < 15 ? d + 1 : 15] : nextw;
      const uint32_t key = sh ? (lo >> sh) | (hi << (32 - sh)) : lo;
      const uint32_t c = cand[i];                     // (no branch: position 0 stands in where there is no candidate, so every load can be issued at once)
      const uint32_t src = load4(buf, c != NOCAND ? static_cast<int>(c) : 0);
      ok4 |= static_cast<unsigned long long>(c != NOCAND && i + 4 <= n && src == key) << i;
    }
  }
  SpanTokens WT{0ull, 0ull, 0ull};
  for (int i = 0; i < n;) {
    const int run = __ffsll(static_cast<long long>(~((eq >> i) >> 1)));      // bytes from i on that equal byte i
    int m = 0;
    if ((ok4 >> i) & 1ull) {
      const int c = static_cast<int>(cand[i]), cap = min(63, n - i);
      m = 4;
      while (m + 4 <= cap) {
        const uint32_t x = load4(buf, c + m) ^ load4(buf, base + i + m);
        if (x) { m += (__ffs(static_cast<int>(x)) - 1) >> 3; break; }
        m += 4;
      }
      if (m + 4 > cap) while (m < cap && filt[padpos(c + m)] == filt[padpos(base + i + m)]) ++m;
    }
    if (m >= 4 && m >= run) { WT.mstart |= 1ull << i; WT.win |= 1ull << i; i += m; }
    else if (run >= 4) { WT.lit |= 1ull << i; WT.mstart |= 2ull << i; i += run; }
    else { WT.lit |= 1ull << i; i += 1; }
  }
  walk_tokens<0>(sp, n, WT, cand, base, hist2, dhist, nullptr, nullptr, nullptr, nullptr, nullptr);
  const int lead = chunk == 0 ? 2 : 0;               // the zlib header travels with the first chunk
  __syncthreads();                                   // both histograms are final; nobody reads buf as the filtered chunk any more

  // ---- C. three codes, a wave each
  if (wave == 0) { const bool ok = build_code(hist, clen, code, NSYM, lane, false); if (lane == 0) s_skip_run = ok ? 0 : 1; }
  else if (wave == 1) { const bool ok = build_code(hist2, clen2, code2, NSYM, lane, false); if (lane == 0) s_skip_ll = ok ? 0 : 1; }
  else if (wave == 2) {
    const unsigned long long um = __ballot(lane < NDSYM && dhist[lane < NDSYM ? lane : 0] != 0u);
    const bool ok = build_code(dhist, dclen, dcode, NDSYM, lane, true);
    if (lane == 0) { s_skip_d = ok ? 0 : 1; s_hdist = um ? 63 - __clzll(static_cast<long long>(um)) : 0; }
  }
  __syncthreads();
  const bool skip_run = s_skip_run != 0, skip_win = s_skip_ll != 0 || s_skip_d != 0;
  const int hdist = s_hdist;

  if (P.dbg && tid == 0) P.dbg[chunk * 8 + 3] = wall_clock64();
  // ---- D. bits per thread in both forms, two exclusive scans, the choice between stored, run and window form
  const int rbits = skip_run ? 0 : walk_tokens<1>(sp, n, RT, cand, base, nullptr, nullptr, clen, rdclen, nullptr, nullptr, nullptr);
  const int wbits = skip_win ? 0 : walk_tokens<1>(sp, n, WT, cand, base, nullptr, nullptr, clen2, dclen, nullptr, nullptr, nullptr);
  int rincl = rbits, wincl = wbits;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int t = __shfl_up(rincl, off), u = __shfl_up(wincl, off);
    if (lane >= off) { rincl += t; wincl += u; }
  }
  if (lane == 63) { wsum[wave] = static_cast<uint32_t>(rincl); wsum[4 + wave] = static_cast<uint32_t>(wincl); }
  __syncthreads();
  int rwave = 0, wwave = 0;
  for (int k = 0; k < wave; ++k) { rwave += static_cast<int>(wsum[k]); wwave += static_cast<int>(wsum[4 + k]); }
  const int rtotal = static_cast<int>(wsum[0] + wsum[1] + wsum[2] + wsum[3]), wtotal = static_cast<int>(wsum[4] + wsum[5] + wsum[6] + wsum[7]);
  const int rend = lead * 8 + HDR_BITS + rtotal + static_cast<int>(clen[256]);
  const int wend = lead * 8 + HDR_BITS + 4 * hdist + wtotal + static_cast<int>(clen2[256]);
  const int rbytes = (rend + 3 + 7) / 8 + 4, wbytes = (wend + 3 + 7) / 8 + 4;      // + the empty stored block that re-aligns to a byte
  // 0 stored, 1 run, 2 window.  Stored against run as deflate_chunk decides it; the window form only where its chunk WITH its pads is
  // smaller (the 5-byte pads to a multiple of 16 are not monotone in the body: k pads with 5 k = -x mod 16, k = 13 (-x mod 16) mod 16)
  int form = 0, best = lead + 5 + len;
  if (!skip_run && rbytes < best) { form = 1; best = rbytes; }
  auto padded = [](int x) { return x + 5 * ((13 * ((16 - (x & 15)) & 15)) & 15); };
  if (!skip_win && padded(wbytes) < padded(best)) { form = 2; best = wbytes; }
  for (int i = tid; i < SLOT / 4; i += 256) outw[i] = 0;
  __syncthreads();
  if (P.dbg && tid == 0) P.dbg[chunk * 8 + 4] = wall_clock64();
  uint8_t* outb = reinterpret_cast<uint8_t*>(outw);
  int body_end;                                       // bytes before the alignment pads
  if (form != 0) {
    const bool win = form == 2;
    const uint32_t* const cl = win ? clen2 : clen; const uint32_t* const co = win ? code2 : code;
    const uint32_t* const dl = win ? dclen : rdclen; const uint32_t* const dc = win ? dcode : rdcode;
    const int hd = win ? hdist : 0, end_bit = win ? wend : rend;
    const int my_start = lead * 8 + HDR_BITS + 4 * hd + (win ? wwave + wincl - wbits : rwave + rincl - rbits);
    block_header<true>(outw, lead, hd, cl, dl, tid);
    BitWriter bw; bw.init(outw, my_start);
    walk_tokens<2>(sp, n, win ? WT : RT, cand, base, nullptr, nullptr, nullptr, nullptr, co, dc, &bw);
    bw.flush();
    body_end = block_end(outw, end_bit, cl, co, tid);
  } else body_end = stored_form(outb, lead, len, sp, n, base, tid);
  __syncthreads();
  if (tid == 0) pad_chunk(P, chunk, outb, body_end, &s_out_len);
  __syncthreads();

  if (P.dbg && tid == 0) P.dbg[chunk * 8 + 5] = wall_clock64();
  // ---- E. write the chunk to its slot; raw CRC of its bytes
  write_slot(P, chunk, outw, &s_out_len, area, wsum);
  if (P.dbg && tid == 0) P.dbg[chunk * 8 + 6] = wall_clock64();
}

__global__ __launch_bounds__(256) void ist_png_deflate_window_kernel(const DeflArgs P, const uint8_t* ftab, const int bpp) {
  deflate_chunk_window(P, P.chunk0 + blockIdx.x, ftab, bpp);
}
// batch: file f's rows are table entries [row_begin[f], row_begin[f + 1]) when there is a table
__global__ __launch_bounds__(256) void ist_png_deflate_window_batch_kernel(const DeflBatchArgs B, const int64_t* row_begin, const uint8_t* ftab, const int bpp) {
  int64_t chunk; int f;
  const DeflArgs P = batch_chunk(B, &chunk, &f);
  deflate_chunk_window(P, chunk, ftab ? ftab + ((ConstPtr<int64_t>)row_begin)[f] : nullptr, bpp);
}

struct GatherArgs { const uint8_t* slots; uint8_t* out; const int64_t* dst; const uint32_t* len16; int64_t chunk0; };

__device__ __forceinline__ void gather_chunk(const uint8_t* s, uint8_t* d, const int units) {
  for (int u = threadIdx.x; u < units; u += 256)
    *reinterpret_cast<u32x4_a4*>(d + 16 * static_cast<size_t>(u)) = *reinterpret_cast<const u32x4*>(s + 16 * static_cast<size_t>(u));
}

// chunk j: len16[j] 16-byte units from its slot to file offset dst[j] (4-byte aligned)
__global__ __launch_bounds__(256) void ist_png_gather_kernel(const GatherArgs G) {
  const int64_t j = G.chunk0 + blockIdx.x;
  gather_chunk(G.slots + static_cast<size_t>(j) * SLOT, G.out + G.dst[j], static_cast<int>(G.len16[j]));
}

// batch twin: every chunk of every file of a batch; dst[j] is the chunk's ADDRESS in its file's buffer (files live in separate buffers)
struct GatherBatchArgs { const uint8_t* slots; const uint64_t* dst; const uint32_t* len16; };
__global__ __launch_bounds__(256) void ist_png_gather_batch_kernel(const GatherBatchArgs G) {
  const int64_t j = blockIdx.x;
  gather_chunk(G.slots + static_cast<size_t>(j) * SLOT, reinterpret_cast<uint8_t*>(G.dst[j]), static_cast<int>(G.len16[j]));
}

// device -> pinned host, 16-byte units, a FIXED small grid striding over the range: the slab's trip over PCIe as a kernel that
// holds a few dozen workgroup slots, instead of the runtime's device-to-host copy, which runs as a blit kernel of thousands of
// workgroups parked on PCIe writes beside the compressing kernel (PNG stage 3.5 ms with those copies, 2.4 ms without them -
// measured with IST_PNG_SKIP_D2H - against 2.6-2.75 ms of PCIe time)
__global__ __launch_bounds__(256) void ist_png_to_host_kernel(const u32x4* __restrict__ src, u32x4* __restrict__ dst, const int64_t units) {
  for (int64_t u = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; u < units; u += static_cast<int64_t>(gridDim.x) * 256)
    dst[u] = __builtin_nontemporal_load(src + u);
}

void put32(uint8_t* p, uint32_t v) { p[0] = v >> 24; p[1] = (v >> 16) & 0xFF; p[2] = (v >> 8) & 0xFF; p[3] = v & 0xFF; }

struct ChunkGrid { int64_t n_chunks; int rows_per_chunk, pieces_per_row, piece_px; };

ChunkGrid make_grid(int64_t w, int64_t h, int color) {
  ChunkGrid g{0, 0, 0, 0};
  const int bpp = color == IST_PNG_RGB ? 3 : 4;      // bytes of a pixel in the filtered stream of a colour form (IST_PNG_RGBA / IST_PNG_RGB)
  const int64_t R = bpp * w + 1;
  if (R <= CH) { g.rows_per_chunk = static_cast<int>(CH / R); g.n_chunks = (h + g.rows_per_chunk - 1) / g.rows_per_chunk; }
  else { g.piece_px = (CH - 1) / bpp; g.pieces_per_row = static_cast<int>((w + g.piece_px - 1) / g.piece_px); g.n_chunks = h * g.pieces_per_row; }
  return g;
}

int64_t idat_limit() {
  const char* e = std::getenv("IST_PNG_IDAT_LIMIT");
  const int64_t v = e ? std::atoll(e) : 0;
  return v >= 4096 ? (v & ~15ll) : (1ll << 30);
}

constexpr int kDataStart = 64;     // signature 8 + IHDR 25 + tEXt 23 + IDAT length/type 8: the stream starts 16-byte aligned

// CRC slicing tables + x^(128 i): what the kernels and the host layout share, built once
struct DeflTables { CrcTables T; std::vector<uint32_t> xpow; };
const DeflTables& defl_tables() {
  static DeflTables D;
  static std::once_flag once;
  std::call_once(once, []() {
    make_crc_tables(&D.T);
    D.xpow.resize(SLOT / 16 + 2);
    uint32_t reg = 0x80000000u;                      // the polynomial "1"
    for (size_t i = 0; i < D.xpow.size(); ++i) { D.xpow[i] = reg; for (int z = 0; z < 16; ++z) reg = crc_byte(D.T, reg, 0); }
  });
  return D;
}

// the tables into the scratch, where the kernels read them (blocking staged copies of static data)
int upload_tables(uint8_t* d_tables, uint8_t* d_xpow, hipStream_t stream) {
  const DeflTables& D = defl_tables();
  IST_HIP(hipMemcpyAsync(d_tables, &D.T, sizeof D.T, hipMemcpyHostToDevice, stream));
  IST_HIP(hipMemcpyAsync(d_xpow, D.xpow.data(), 4 * D.xpow.size(), hipMemcpyHostToDevice, stream));
  return IST_OK;
}

// The five per-chunk result arrays as the kernels write them into ONE block, [len16 | crc | ad_a | ad_b | ad_n] with `stride` entries
// each, so that a run of chunks' results are one contiguous piece of pinned memory.  Indexed with the chunk number; `first` is the
// chunk whose results are the arrays' entry 0 (a slab's first chunk; 0 in a batch).
struct ChunkResults { uint32_t *len16, *crc, *ad_a, *ad_b, *ad_n; };
ChunkResults chunk_results(void* base, size_t stride, size_t first) {
  uint32_t* const r = static_cast<uint32_t*>(base) - first;
  return ChunkResults{r, r + stride, r + 2 * stride, r + 3 * stride, r + 4 * stride};
}

// The host side of ONE file, called slab by slab (the whole file is one slab in a batch): Adler-32 of the filtered stream from
// the chunks' partials, each chunk's place in the file (a new IDAT chunk per slab, and wherever the IDAT limit is reached), the
// CRC of every IDAT, and the ~100 bytes no kernel writes - signature, IHDR, chunk headers, trailer - as patches.
struct FileLayout {
  const CrcTables& T; const std::vector<uint32_t>& xpow; const int64_t limit;
  uint64_t a = 1, b = 0;
  uint32_t reg = 0xFFFFFFFFu;
  int64_t pos = 56, idat_len_at = 0, idat_data = 0;
  std::vector<PngPatch>* patches = nullptr;
  FileLayout() : T(defl_tables().T), xpow(defl_tables().xpow), limit(idat_limit()) {}
  void feed(const uint8_t* p, int k) { for (int i = 0; i < k; ++i) reg = crc_byte(T, reg, p[i]); }
  void header(int64_t w, int64_t h, int color, std::vector<PngPatch>* out) {
    PngPatch pt; std::memset(&pt, 0, sizeof pt);
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    std::memcpy(pt.b, sig, 8);
    put32(pt.b + 8, 13); std::memcpy(pt.b + 12, "IHDR", 4);
    put32(pt.b + 16, static_cast<uint32_t>(w)); put32(pt.b + 20, static_cast<uint32_t>(h));
    pt.b[24] = 8; pt.b[25] = color == IST_PNG_RGB ? 2 : 6; pt.b[26] = 0; pt.b[27] = 0; pt.b[28] = 0;
    uint32_t c = 0xFFFFFFFFu;
    for (int i = 12; i < 29; ++i) c = crc_byte(T, c, pt.b[i]);
    put32(pt.b + 29, c ^ 0xFFFFFFFFu);
    // an 11-byte tEXt chunk: its only job is to start the IDAT data at file offset 64
    put32(pt.b + 33, 11); std::memcpy(pt.b + 37, "tEXtSoftware\0is", 15);
    c = 0xFFFFFFFFu;
    for (int i = 37; i < 52; ++i) c = crc_byte(T, c, pt.b[i]);
    put32(pt.b + 52, c ^ 0xFFFFFFFFu);
    pt.at = 0; pt.n = 56;
    out->push_back(pt);
  }
  void open_idat() {
    PngPatch pt; std::memset(&pt, 0, sizeof pt);
    pt.at = pos; idat_len_at = pos;
    std::memcpy(pt.b + 4, "IDAT", 4);
    pt.n = 8; patches->push_back(pt);
    reg = 0xFFFFFFFFu; feed(pt.b + 4, 4);
    pos += 8; idat_data = 0;
  }
  void close_idat() {
    PngPatch pt; std::memset(&pt, 0, sizeof pt);
    pt.at = pos; put32(pt.b, reg ^ 0xFFFFFFFFu); pt.n = 4; patches->push_back(pt);
    PngPatch lp; std::memset(&lp, 0, sizeof lp);
    lp.at = idat_len_at; put32(lp.b, static_cast<uint32_t>(idat_data)); lp.n = 4; patches->push_back(lp);
    pos += 4;
  }
  // chunks [c0, c0 + cn) - a slab - with the kernel's per-chunk results; dst[k] = base + the offset of chunk c0 + k in the file.
  // last: the file ends with this slab (trailer, IEND)
  int slab(const ChunkResults& R, size_t c0, size_t cn, int64_t* dst, int64_t base, bool last, std::vector<PngPatch>* out) {
    const uint64_t M = 65521;
    patches = out;
    open_idat();                                       // a slab starts its own IDAT
    for (size_t k = 0; k < cn; ++k) {
      b = (b + (R.ad_n[c0 + k] % M) * a + R.ad_b[c0 + k]) % M;
      a = (a + R.ad_a[c0 + k]) % M;
      const int64_t bytes = static_cast<int64_t>(R.len16[c0 + k]) * 16;
      if (bytes <= 0 || bytes > SLOT) return fail(IST_E_HIP, "PNG deflate kernel returned an impossible chunk length");
      if (idat_data > 0 && idat_data + bytes + 9 > limit) { close_idat(); open_idat(); }
      dst[k] = base + pos;
      reg = gf_mul(xpow[static_cast<size_t>(R.len16[c0 + k])], reg) ^ R.crc[c0 + k];
      pos += bytes; idat_data += bytes;
    }
    if (last) {
      static const uint8_t trailer_block[5] = {0x01, 0x00, 0x00, 0xFF, 0xFF};          // final, empty stored block
      const uint32_t adler = static_cast<uint32_t>((b << 16) | a);
      PngPatch pt; std::memset(&pt, 0, sizeof pt);
      pt.at = pos;
      std::memcpy(pt.b, trailer_block, 5); put32(pt.b + 5, adler);
      feed(pt.b, 9);
      pt.n = 9; patches->push_back(pt);
      pos += 9; idat_data += 9;
      close_idat();
      PngPatch ie; std::memset(&ie, 0, sizeof ie);
      ie.at = pos; put32(ie.b, 0); std::memcpy(ie.b + 4, "IEND", 4);
      uint32_t c = 0xFFFFFFFFu;
      for (int i = 4; i < 8; ++i) c = crc_byte(T, c, ie.b[i]);
      put32(ie.b + 8, c ^ 0xFFFFFFFFu);
      ie.n = 12; patches->push_back(ie);
      pos += 12;
    } else close_idat();
    return IST_OK;
  }
};

// ---- the two places that pick a kernel for a form
// the adaptive form's pre-pass over F.n_rows rows (one file: rows of `widest` pixels; a batch: the rows of all files, the widest that wide)
void launch_row_filter(const PngForm& form, RowFilterArgs F, int64_t widest, hipStream_t st) {
  F.rows_per_group = widest <= kRowFilterWaveW ? 4 : 1;
  const dim3 groups(static_cast<unsigned>((F.n_rows + F.rows_per_group - 1) / F.rows_per_group));
  hipLaunchKernelGGL((form.bpp() == 3 ? ist_png_row_filter_rgb_kernel : ist_png_row_filter_kernel), groups, dim3(256), 0, st, F);
}
// the compressing kernel of `form`, a workgroup per chunk.  ftab: the pre-pass's row types (NULL unless adaptive); rows: the batch's row_begin (likewise)
void launch_deflate(const PngForm& form, size_t n_chunks, hipStream_t st, const DeflArgs& A, const uint8_t* ftab) {
  const dim3 grid(static_cast<unsigned>(n_chunks)), wg(256);
  const bool rgb = form.bpp() == 3;
  if (form.window()) hipLaunchKernelGGL(ist_png_deflate_window_kernel, grid, wg, 0, st, A, ftab, form.bpp());
  else if (form.adaptive()) hipLaunchKernelGGL((rgb ? ist_png_deflate_adapt_rgb_kernel : ist_png_deflate_adapt_kernel), grid, wg, 0, st, A, ftab);
  else hipLaunchKernelGGL((rgb ? ist_png_deflate_rgb_kernel : ist_png_deflate_kernel), grid, wg, 0, st, A);
}
void launch_deflate(const PngForm& form, size_t n_chunks, hipStream_t st, const DeflBatchArgs& B, const int64_t* rows, const uint8_t* ftab) {
  const dim3 grid(static_cast<unsigned>(n_chunks)), wg(256);
  const bool rgb = form.bpp() == 3;
  if (form.window()) hipLaunchKernelGGL(ist_png_deflate_window_batch_kernel, grid, wg, 0, st, B, rows, ftab, form.bpp());
  else if (form.adaptive()) hipLaunchKernelGGL((rgb ? ist_png_deflate_adapt_rgb_batch_kernel : ist_png_deflate_adapt_batch_kernel), grid, wg, 0, st, B, rows, ftab);
  else hipLaunchKernelGGL((rgb ? ist_png_deflate_rgb_batch_kernel : ist_png_deflate_batch_kernel), grid, wg, 0, st, B);
}

}  // namespace

// upper bound of the compressed form: every chunk stored.  (The RGB form never has more chunks than the RGBA one: the RGBA bound
// - the one ist_png_bound reports - holds for both.)
int64_t png_deflate_bound(int64_t w, int64_t h, int color) {
  const ChunkGrid g = make_grid(w, h, color);
  const int64_t data = g.n_chunks * SLOT + 16;
  return kDataStart + data + (data / idat_limit() + 2) * 12 + 64;
}

// host_out (optional, pinned, out_cap bytes) + aux: the file is ALSO delivered to host memory, slab by slab, on the aux
// stream while later slabs are still being compressed on `stream` — the PNG's trip over PCIe (2.6 ms for the 146 MB of a
// 439 MB photo canvas) then hides behind the encoder (3.3 ms) instead of following it.  Each slab is its own IDAT chunk.
int png_encode_device_deflate(ist_ctx* ctx, const PngForm& form, const void* canvas, size_t pitch, int64_t w, int64_t h, void* out, int64_t out_cap,
                              int64_t* out_len, void* stream_, uint8_t* host_out, void* aux_,
                              const std::function<int(int64_t, void*)>& need_rows, int64_t slab_rows_hint, void* stream2_) {
  const int color = form.color;
  const bool adaptive = form.adaptive();
  const ChunkGrid g = make_grid(w, h, color);
  if (g.n_chunks > 2147483647ll) return fail(IST_E_OUTPUT_SIZE, "image too large for one PNG launch");
  if (png_deflate_bound(w, h, color) > out_cap) return fail(IST_E_INVALID, "PNG output buffer too small (see ist_png_bound)");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  hipStream_t aux = host_out ? static_cast<hipStream_t>(aux_) : stream;
  // slabs alternate between two streams (when the caller has a second one): consecutive kernels of ONE stream do not overlap,
  // so every slab paid its own tail - the last, partly filled round of workgroups - with the rest of the chip idle; on two
  // streams slab s+1 fills in as slab s drains (a slab is ~3 rounds of workgroups: measured 0.59 ms per 3024-chunk slab alone)
  hipStream_t stream2 = (host_out && stream2_) ? static_cast<hipStream_t>(stream2_) : stream;
  const DeflTables& tables = defl_tables();
  const size_t n = static_cast<size_t>(g.n_chunks);
  auto up = [](size_t v) { return (v + 255) & ~static_cast<size_t>(255); };
  // per-chunk results, five arrays interleaved per SLAB so that a slab's results are one contiguous copy:
  // [len16 | crc | ad_a | ad_b | ad_n] x slab
  // 64 MiB of filtered stream per slab - or, when the producer renders the canvas band by band (need_rows), about one band
  // (never less than a quarter of the default: a slab is a launch, a layout pass and a copy), so that slab k is complete
  // when band k is and nothing of band k+1 is waited for
  size_t slab_chunks = 4096;
  if (slab_rows_hint > 0) {
    const int64_t rows_chunks = g.pieces_per_row > 0 ? slab_rows_hint * g.pieces_per_row : (slab_rows_hint + g.rows_per_chunk - 1) / std::max(1, g.rows_per_chunk);
    slab_chunks = static_cast<size_t>(std::min<int64_t>(4096, std::max<int64_t>(1024, rows_chunks)));
  }
  // slab s = chunks [slab_at[s], slab_at[s + 1]).  The FIRST slab is short: nothing crosses PCIe before it has been compressed,
  // laid out and gathered, so its size is the fill time of the pipeline (0.66 ms with a full first slab sharing the chip with
  // the second: measured); behind it the copies are back to back
  std::vector<size_t> slab_at{0};
  if (host_out) {
    const size_t first = std::min<size_t>(n, std::min<size_t>(slab_chunks, 768));
    for (size_t c = first; c < n; c += slab_chunks) slab_at.push_back(c);
  }
  slab_at.push_back(n);
  const size_t n_slabs = slab_at.size() - 1;
  const size_t per_slab = host_out ? slab_chunks : n;          // the largest slab (sizes the per-slab result arrays)
  // the last canvas row (exclusive) chunks [0, c_end) read
  auto rows_of = [&](size_t c_end) -> int64_t {
    const int64_t r = g.pieces_per_row > 0 ? (static_cast<int64_t>(c_end) + g.pieces_per_row - 1) / g.pieces_per_row : static_cast<int64_t>(c_end) * g.rows_per_chunk;
    return std::min<int64_t>(h, r);
  };
  // (adaptive: the row types, ONE TABLE OF h BYTES PER STREAM PARITY.  Slabs alternate between two streams and a slab boundary can
  // fall inside a row; with a table per parity a slab's pre-pass writes, and its compressing kernel reads, only bytes of its own
  // stream - the cut row is evaluated by both slabs, each into its own table - so the streams need no event and no wait for it)
  const size_t o_T = 0, o_pow = o_T + up(sizeof tables.T), o_ftab = o_pow + up(4 * tables.xpow.size()),
               o_slots = o_ftab + (adaptive ? up(2 * static_cast<size_t>(h)) : 0), total_scratch = o_slots + n * SLOT;
  // the context's grow-only scratch: a 439 MB canvas needs 443 MB of slots, and allocating + freeing that per call cost
  // more than the gather kernel (and a free synchronises the device)
  uint8_t* scratch = nullptr;
  {
    void* p = nullptr;
    const int rc = ctx_png_scratch(ctx, total_scratch, &p);
    if (rc) return rc;
    scratch = static_cast<uint8_t*>(p);
  }
  { const int rc = upload_tables(scratch + o_T, scratch + o_pow, stream); if (rc) return rc; }
  if (stream2 != stream) IST_HIP(hipStreamSynchronize(stream));      // (the tables are in place for either stream)
  // ---- every slab's compression goes out now, each followed by the copy of its per-chunk results and an event
  // (pinned: a device-to-host copy into pageable memory would block this thread until the slab is compressed, and the
  // slabs' launches would no longer run ahead of the host)
  std::vector<Event> evs(n_slabs), gathered(n_slabs);   // (a slab that was never launched has an empty one)

  PoolBlock res;
  if (!res.take(20 * per_slab * n_slabs)) return fail(IST_E_NOMEM, "out of pinned host memory for the PNG encoder");
  // file offset of every chunk: pinned host memory the gather kernel reads in place (a pageable source would cost one small
  // staged copy per slab on the aux stream; those, and the header patches, were ~0.5 ms of stream time per slab)
  PoolBlock dstp;
  if (!dstp.take(8 * n)) return fail(IST_E_NOMEM, "out of pinned host memory for the PNG encoder");
  DevBuf dbg;
  // EVERY way out of this function below - the errors too - first waits for both streams: the kernels in flight write their
  // per-chunk results into `res` and read `dstp` in place, and a block given back to the pool while slab s+1 is still
  // compressing could be handed to another thread's call.  (Declared after the two blocks: destroyed before them.)
  StreamDrain drain(stream, aux, stream2);
  static const bool phases = tuning_mode() && std::getenv("IST_PNG_PHASES") != nullptr;      // (IST_TUNING=1 processes only)
  if (phases) { KeepLastError tolerated; (void)dbg.grow(64 * n); }
  // test knob (IST_TUNING=1 IST_PNG_FAIL_AT=<slab>): fail the layout of that slab the way a damaged result would, so that the
  // error path above is exercised with kernels in flight
  static const long fail_at = (tuning_mode() && std::getenv("IST_PNG_FAIL_AT")) ? std::atol(std::getenv("IST_PNG_FAIL_AT")) : -1;
  auto compress = [&](size_t s) -> int {
    const size_t c0 = slab_at[s], cn = slab_at[s + 1] - c0;
    // (the Paeth filter of a chunk's first row reads the row above it: that row belongs to an earlier slab, already asked for)
    hipStream_t st = (s & 1) ? stream2 : stream;
    if (need_rows) { const int rc = need_rows(rows_of(c0 + cn), st); if (rc) return rc; }
    // the kernel writes its per-chunk results straight into the pinned host block (visible to the host behind the event).
    // As small device-to-host COPIES on this stream they shared the copy engine's queue with the slabs' big copies on the
    // aux stream: each big copy then took 0.9 ms instead of 0.4 and the PNG phase 6.8 ms instead of 3.4 (measured)
    const ChunkResults R = chunk_results(res.at(20 * per_slab * s), per_slab, c0);      // (the kernel indexes the arrays with the global chunk number)
    DeflArgs A;
    A.canvas = static_cast<const uint8_t*>(canvas); A.pitch = pitch; A.w = w; A.h = h;
    A.slots = scratch + o_slots;
    A.len16 = R.len16; A.crc = R.crc; A.ad_a = R.ad_a; A.ad_b = R.ad_b; A.ad_n = R.ad_n;
    A.tables = reinterpret_cast<const uint32_t*>(scratch + o_T); A.xpow16 = reinterpret_cast<const uint32_t*>(scratch + o_pow);
    A.rows_per_chunk = g.rows_per_chunk; A.pieces_per_row = g.pieces_per_row; A.piece_px = g.piece_px;
    A.chunk0 = static_cast<int64_t>(c0);
    A.dbg = static_cast<unsigned long long*>(dbg.p);
    uint8_t* ftab = nullptr;
    if (adaptive) {
      // the pre-pass of every row this slab's chunks touch, on the slab's own stream, into the table of that stream (the row above
      // the first one is only read: like the Paeth filter's, it belongs to an earlier slab and has been asked for)
      const int64_t y_lo = g.pieces_per_row > 0 ? static_cast<int64_t>(c0) / g.pieces_per_row : static_cast<int64_t>(c0) * g.rows_per_chunk;
      const int64_t y_hi = rows_of(c0 + cn);
      ftab = scratch + o_ftab + (s & 1) * static_cast<size_t>(h);
      RowFilterArgs F;
      F.canvas = A.canvas; F.pitch = pitch; F.w = w; F.h = h;
      F.jobs = nullptr; F.row_begin = nullptr; F.n_files = 0;
      F.row0 = y_lo; F.n_rows = y_hi - y_lo; F.table = ftab;
      launch_row_filter(form, F, w, st);
      IST_HIP(hipGetLastError());
    }
    launch_deflate(form, cn, st, A, ftab);
    IST_HIP(hipGetLastError());
    tl_mark("png:   compression launched, slab", static_cast<long>(s));
    { const int rc = evs[s].ensure(); if (rc) return rc; }
    IST_HIP(hipEventRecord(evs[s], st));
    return IST_OK;
  };
  // one slab ahead: slab s+1 is compressing while the host lays out slab s and the aux stream carries it away
  { const int rc = compress(0); if (rc) return rc; }

  // ---- host, slab by slab: Adler-32 of the filtered stream, the layout of the chunks in the file, the CRC of every
  // IDAT; then the slab's gather (and its trip to the host) on the aux stream
  FileLayout lay;
  int64_t* const dst = dstp.at<int64_t>();
  std::vector<std::vector<PngPatch>> slab_patches(n_slabs);     // (all of them live until the final synchronisation)
  lay.header(w, h, color, &slab_patches[0]);
  for (size_t s = 0; s < n_slabs; ++s) {
    const size_t c0 = slab_at[s], cn = slab_at[s + 1] - c0;
    if (s + 1 < n_slabs) { const int rc = compress(s + 1); if (rc) return rc; tl_mark("png: submitted the compression of slab", static_cast<long>(s + 1)); }
    IST_HIP(hipEventSynchronize(evs[s]));
    tl_mark("png: compressed (event passed), slab", static_cast<long>(s));
    if (fail_at >= 0 && static_cast<size_t>(fail_at) == s) return fail(IST_E_HIP, "PNG deflate kernel returned an impossible chunk length (forced: IST_PNG_FAIL_AT)");
    const ChunkResults R = chunk_results(res.at(20 * per_slab * s), per_slab, c0);
    const int64_t slab_begin = s == 0 ? 0 : lay.pos;   // file bytes [slab_begin, pos) are final once this slab is laid out
    { const int rc = lay.slab(R, c0, cn, dst + c0, 0, s + 1 == n_slabs, &slab_patches[s]); if (rc) return rc; }
    const int64_t pos = lay.pos;
    const std::vector<PngPatch>& patches = slab_patches[s];
    if (pos > out_cap) return fail(IST_E_INVALID, "PNG output buffer too small (see ist_png_bound)");
    // The gather rides on the stream that compressed the slab (its slots and results are complete: the event above has passed;
    // the next slab is already compressing on the other stream), and the aux stream carries NOTHING but the slabs' trips over
    // PCIe, each behind its gather's event.  With gather and copy both on aux every slab cost gather + copy in series (0.1 +
    // 0.3 ms, nine times: the whole phase was that stream, 4.0 ms for 2.75 ms of PCIe - measured, rocprofv3 timeline).
    // (Tried and dropped: the gather writing straight into the pinned file image with a small grid, no device image and no
    // copy - 4-byte-aligned 16-byte stores over PCIe from 128 workgroups were slower than gather + the runtime's copy: the phase
    // went from 3.66 to 4.23 ms.)
    tl_mark("png:   host layout done, slab", static_cast<long>(s));
    hipStream_t gs = host_out ? ((s & 1) ? stream2 : stream) : aux;
    GatherArgs G{scratch + o_slots, static_cast<uint8_t*>(out), dst, R.len16, static_cast<int64_t>(c0)};
    hipLaunchKernelGGL(ist_png_gather_kernel, dim3(static_cast<unsigned>(cn)), dim3(256), 0, gs, G);
    IST_HIP(hipGetLastError());
    tl_mark("png:   gather launched, slab", static_cast<long>(s));
    if (host_out) {
      { const int rc = gathered[s].ensure(); if (rc) return rc; }
      IST_HIP(hipEventRecord(gathered[s], gs));
      IST_HIP(hipStreamWaitEvent(aux, gathered[s], 0));
      tl_mark("png:   event created + recorded + aux ordered behind it, slab", static_cast<long>(s));
    }
    if (!host_out)                                     // (with a host sink the headers are written there, below)
      for (const PngPatch& pt : patches)
        IST_HIP(hipMemcpyAsync(static_cast<uint8_t*>(out) + pt.at, pt.b, static_cast<size_t>(pt.n), hipMemcpyHostToDevice, aux));
    if (host_out) {
      // 256-byte aligned ends.  The bytes past `pos` in the last 256 are the next slab's: its own copy, ordered behind
      // this one, delivers them
      const int64_t c_lo = slab_begin & ~255ll, c_hi = std::min<int64_t>((pos + 255) & ~255ll, out_cap);
      static const bool skip_d2h = tuning_mode() && std::getenv("IST_PNG_SKIP_D2H") != nullptr;      // experiment: what the copies cost the kernel beside them (the file is then NOT delivered)
      static const int copy_grid = (tuning_mode() && std::getenv("IST_PNG_COPY_GRID")) ? std::atoi(std::getenv("IST_PNG_COPY_GRID")) : kCopyGrid;
      if (!skip_d2h && copy_grid > 0) {
        hipLaunchKernelGGL(ist_png_to_host_kernel, dim3(static_cast<unsigned>(copy_grid)), dim3(256), 0, aux, reinterpret_cast<const u32x4*>(static_cast<const uint8_t*>(out) + c_lo),
                           reinterpret_cast<u32x4*>(host_out + c_lo), (c_hi - c_lo) / 16);
        IST_HIP(hipGetLastError());
      } else if (!skip_d2h) {
        // (round 4, tools/exp_slow_call.py + the marks around this call: one call in 600 - 3000 loses 6.5 - 7.3 ms INSIDE this
        // hipMemcpyAsync - the runtime's submission of one slab's device-to-host copy, slab 4, 8 or 9, on four different boxes; the
        // only stall of the call that is neither a wait of ours nor host scheduling.  Bounding the copies queued on the aux stream to
        // four - waiting for copy s-4's event before submitting copy s - did not remove it (1 and 3 such calls in 2 x 3000, against 2
        // and 1 unbounded) and cost 0.15 - 0.2 ms of the median call: dropped.)
        IST_HIP(hipMemcpyAsync(host_out + c_lo, static_cast<const uint8_t*>(out) + c_lo, static_cast<size_t>(c_hi - c_lo), hipMemcpyDeviceToHost, aux));
      }
      tl_mark("png: laid out, gather + copy submitted, slab", static_cast<long>(s));
    }
  }
  tl_mark("png: every slab submitted; waiting for the copies (aux stream)");
  IST_HIP(hipStreamSynchronize(aux));
  tl_mark("png: aux stream idle (the file is in host memory)");
  if (aux != stream) IST_HIP(hipStreamSynchronize(stream));
  if (stream2 != stream) IST_HIP(hipStreamSynchronize(stream2));
  tl_mark("png: encoder streams idle");
  drain.disarm();                                      // the streams are idle
  if (dbg.p) {
    std::vector<unsigned long long> hdbg(8 * n);
    (void)hipMemcpy(hdbg.data(), dbg.p, 64 * n, hipMemcpyDeviceToHost);
    double sum[6] = {0, 0, 0, 0, 0, 0};
    for (size_t j = 0; j < n; ++j) for (int k = 0; k < 6; ++k) sum[k] += static_cast<double>(hdbg[8 * j + k + 1] - hdbg[8 * j + k]);
    static const char* names[6] = {"A load+filter", "B histogram+adler", "C code build", "D bit counts+scan", "body emit", "E slot write+crc"};
    for (int k = 0; k < 6; ++k) std::fprintf(stderr, "[png phases] %-18s %8.2f us per chunk (100 MHz clock)\n", names[k], sum[k] / static_cast<double>(n) / 100.0);
  }
  if (host_out)                                        // signature, chunk headers, lengths, CRCs, trailer: ~30 bytes per slab
    for (const std::vector<PngPatch>& v : slab_patches)
      for (const PngPatch& pt : v) std::memcpy(host_out + pt.at, pt.b, static_cast<size_t>(pt.n));
  *out_len = lay.pos;
  return IST_OK;
}

int64_t png_deflate_chunks(int64_t w, int64_t h, int color) { return make_grid(w, h, color).n_chunks; }
void png_deflate_grid(int64_t w, int64_t h, int color, int64_t out[4]) {
  const ChunkGrid g = make_grid(w, h, color);
  out[0] = g.n_chunks; out[1] = g.rows_per_chunk; out[2] = g.pieces_per_row; out[3] = g.piece_px;
}
int64_t png_deflate_slot_bytes() { return SLOT; }

// The compressing form of a batch: every chunk of every file in ONE ist_png_deflate_batch_kernel launch, the host layout of
// each file (FileLayout, as for one file), then every chunk of every file in ONE ist_png_gather_batch_kernel launch.
int png_encode_batch_deflate(ist_ctx* ctx, const PngForm& form, std::vector<PngBatchFile>& files, void* stream_, bool host_patches) {
  const size_t nf = files.size();
  const int color = form.color;
  const bool adaptive = form.adaptive();
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  std::vector<ChunkGrid> grid(nf);
  std::vector<int64_t> begin(nf + 1, 0), row_begin(nf + 1, 0);      // (row_begin: the rows of every file, file-major - the adaptive form's table)
  int64_t widest = 0;
  for (size_t k = 0; k < nf; ++k) {
    grid[k] = make_grid(files[k].w, files[k].h, color);
    begin[k + 1] = begin[k] + grid[k].n_chunks;
    row_begin[k + 1] = row_begin[k] + files[k].h;
    widest = std::max(widest, files[k].w);
  }
  if (begin[nf] > 2147483647ll) return fail(IST_E_OUTPUT_SIZE, "batch too large for one PNG launch");
  const size_t n = static_cast<size_t>(begin[nf]);
  const DeflTables& tables = defl_tables();
  auto up = [](size_t v) { return (v + 255) & ~static_cast<size_t>(255); };
  // device: tables | per-file jobs | chunk_begin | slots;  pinned host: per-chunk results [len16 | crc | ad_a | ad_b | ad_n] |
  // per-chunk destination addresses (read in place by the gather) | the jobs + chunk_begin image that goes up
  // (adaptive: row_begin goes up with the jobs; behind it the table of row types, which only kernels write)
  const size_t o_T = 0, o_pow = o_T + up(sizeof tables.T), o_jobs = o_pow + up(4 * tables.xpow.size()), o_begin = o_jobs + up(sizeof(DeflJob) * nf),
               o_rows = o_begin + up(8 * (nf + 1)), o_ftab = o_rows + (adaptive ? up(8 * (nf + 1)) : 0),
               o_slots = o_ftab + (adaptive ? up(static_cast<size_t>(row_begin[nf])) : 0), total_scratch = o_slots + n * SLOT;
  const size_t h_res = 0, h_dst = up(20 * n), h_jobs = h_dst + up(8 * n), h_total = h_jobs + (o_ftab - o_jobs);
  uint8_t* scratch = nullptr;
  {
    void* p = nullptr;
    const int rc = ctx_png_scratch(ctx, total_scratch, &p);
    if (rc) return rc;
    scratch = static_cast<uint8_t*>(p);
  }
  PoolBlock pin;
  if (!pin.take(h_total)) return fail(IST_E_NOMEM, "out of pinned host memory for the PNG encoder");
  // every way out below waits for the stream first: the kernels write `pin` and read it in place (declared after it: runs first)
  StreamDrain drain(stream);
  DeflJob* hj = pin.at<DeflJob>(h_jobs);
  int64_t* hb = pin.at<int64_t>(h_jobs + (o_begin - o_jobs));
  for (size_t k = 0; k < nf; ++k) {
    const PngBatchFile& f = files[k];
    hj[k] = DeflJob{static_cast<const uint8_t*>(f.canvas), f.pitch, f.w, f.h, grid[k].rows_per_chunk, grid[k].pieces_per_row, grid[k].piece_px, 0};
  }
  std::memcpy(hb, begin.data(), 8 * (nf + 1));
  if (adaptive) std::memcpy(pin.at(h_jobs + (o_rows - o_jobs)), row_begin.data(), 8 * (nf + 1));
  { const int rc = upload_tables(scratch + o_T, scratch + o_pow, stream); if (rc) return rc; }
  IST_HIP(hipMemcpyAsync(scratch + o_jobs, pin.at(h_jobs), o_ftab - o_jobs, hipMemcpyHostToDevice, stream));
  const ChunkResults R = chunk_results(pin.at(h_res), n, 0);
  DeflBatchArgs B;
  B.jobs = reinterpret_cast<const DeflJob*>(scratch + o_jobs);
  B.chunk_begin = reinterpret_cast<const int64_t*>(scratch + o_begin);
  B.n_files = static_cast<int32_t>(nf);
  B.slots = scratch + o_slots;
  B.len16 = R.len16; B.crc = R.crc; B.ad_a = R.ad_a; B.ad_b = R.ad_b; B.ad_n = R.ad_n;
  B.tables = reinterpret_cast<const uint32_t*>(scratch + o_T); B.xpow16 = reinterpret_cast<const uint32_t*>(scratch + o_pow);
  const int64_t* d_rows = nullptr;
  uint8_t* ftab = nullptr;
  if (adaptive) {
    // ONE pre-pass launch for the rows of all files (a wave per row unless some file is wider than a wave's share), then the one
    // compressing launch
    if (row_begin[nf] > 2147483647ll) return fail(IST_E_OUTPUT_SIZE, "batch too large for one PNG launch");
    d_rows = reinterpret_cast<const int64_t*>(scratch + o_rows);
    ftab = scratch + o_ftab;
    RowFilterArgs F;
    F.canvas = nullptr; F.pitch = 0; F.w = 0; F.h = 0;
    F.jobs = B.jobs; F.row_begin = d_rows; F.n_files = B.n_files;
    F.row0 = 0; F.n_rows = row_begin[nf]; F.table = ftab;
    launch_row_filter(form, F, widest, stream);
    IST_HIP(hipGetLastError());
  }
  launch_deflate(form, n, stream, B, d_rows, ftab);
  IST_HIP(hipGetLastError());
  count_png_batch_launch();
  IST_HIP(hipStreamSynchronize(stream));
  // ---- host: each file laid out as one slab
  int64_t* dst = pin.at<int64_t>(h_dst);
  for (size_t k = 0; k < nf; ++k) {
    PngBatchFile& f = files[k];
    const size_t c0 = static_cast<size_t>(begin[k]), cn = static_cast<size_t>(begin[k + 1] - begin[k]);
    FileLayout lay;
    f.patches.clear();
    lay.header(f.w, f.h, color, &f.patches);
    const int rc = lay.slab(R, c0, cn, dst + c0, static_cast<int64_t>(reinterpret_cast<uintptr_t>(f.out)), true, &f.patches);
    if (rc) { const std::string why = g_last_error; return fail(rc, "file " + std::to_string(k) + ": " + why); }
    if (lay.pos > f.cap) return fail(IST_E_INVALID, "file " + std::to_string(k) + ": PNG output buffer too small (see ist_png_bound)");
    f.len = lay.pos;
  }
  GatherBatchArgs G{scratch + o_slots, reinterpret_cast<const uint64_t*>(dst), R.len16};
  hipLaunchKernelGGL(ist_png_gather_batch_kernel, dim3(static_cast<unsigned>(n)), dim3(256), 0, stream, G);
  IST_HIP(hipGetLastError());
  if (!host_patches)
    for (const PngBatchFile& f : files)
      for (const PngPatch& pt : f.patches) IST_HIP(hipMemcpyAsync(f.out + pt.at, pt.b, static_cast<size_t>(pt.n), hipMemcpyHostToDevice, stream));
  IST_HIP(hipStreamSynchronize(stream));
  drain.disarm();
  return IST_OK;
}

}  // namespace ist
