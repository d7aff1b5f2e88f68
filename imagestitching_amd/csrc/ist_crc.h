// ist_crc.h — CRC-32 (PNG / zlib, reflected 0xEDB88320) helpers shared by the two PNG encoders (+ their batch twins' file lookup)
#ifndef IST_CRC_H_
#define IST_CRC_H_

#include <cstdint>

namespace ist {

constexpr uint32_t kCrcPoly = 0xEDB88320u;

struct CrcTables { uint32_t t[4][256]; };

// byte-at-a-time table and the three slices on top of it
inline void make_crc_tables(CrcTables* T) {
  for (uint32_t i = 0; i < 256; ++i) {
    uint32_t c = i;
    for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ kCrcPoly : c >> 1;
    T->t[0][i] = c;
  }
  for (uint32_t i = 0; i < 256; ++i)
    for (int s = 1; s < 4; ++s) T->t[s][i] = (T->t[s - 1][i] >> 8) ^ T->t[0][T->t[s - 1][i] & 0xFF];
}

inline uint32_t crc_byte(const CrcTables& T, uint32_t reg, uint8_t b) { return T.t[0][(reg ^ b) & 0xFF] ^ (reg >> 8); }

// product of two polynomials over GF(2) modulo the CRC polynomial, reflected bit order (x^0 = 0x80000000)
#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint32_t gf_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 0; i < 32; ++i) {
    if (a & (0x80000000u >> i)) p ^= b;
    b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
  }
  return p;
}

#if defined(__HIPCC__)
// The batch twins of the PNG kernels (one launch, many files): the file holding work item g is the last f with begin[f] <= g
// (begin[0] = 0, strictly increasing).  g is wave-uniform and the table is read through the constant address space, so the
// search is scalar loads and scalar branches, and the per-file table below it is too (ist_png.hip, ist_png_deflate.hip).
template <typename T> using ConstPtr = const __attribute__((address_space(4))) T*;
__device__ __forceinline__ int batch_file_of(const int64_t* begin_, int n, int64_t g) {
  ConstPtr<int64_t> begin = (ConstPtr<int64_t>)begin_;
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (begin[mid] <= g) lo = mid; else hi = mid - 1;
  }
  return __builtin_amdgcn_readfirstlane(lo);
}
#endif

}  // namespace ist

#endif  // IST_CRC_H_
