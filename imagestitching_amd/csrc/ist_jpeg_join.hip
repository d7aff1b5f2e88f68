// ist_jpeg_join.hip — the lossless JPEG join: the kernel that moves the decoder's quantised coefficient blocks into the export's
// coefficient scratch, and the entry point around it (the rule: include/imagestitch.h, "lossless JPEG joins").
//
// Reference anchor: the export seam, safeCanvasToTempFilePath (utils/canvas.js:205-221), reached from files without a canvas: the
// page's route is decode (pages/index/index.js:1441-1520), draw (:1522-1554), export (:1577-1579).
//
// Both ends exist already and meet at the same data: the decoders (FileDecoder::coefficients) leave every component's quantised
// coefficients in dense planes, blocks_y x blocks_x x 64 int16 in natural order; the export's entropy, histogram and gather kernels
// (ist_jpeg_encode.hip) read blocks in coding order, 64 int16 each in zig-zag order.  The kernel here is the move between the two,
// run per slab of MCU rows in place of the transform kernel (jpeg_encode_slabs): 2 bytes read and 2 written per coefficient.
//   * a workgroup owns 32 consecutive blocks of ONE MCU row of the joined file (grid: x = ceil(row_blocks / 32), y = the slab's MCU
//     rows); 8 lanes own a block: lane j loads row j of the natural-order block (16 bytes) and stores zig-zag positions 8j .. 8j + 7
//     (16 bytes), so a wave reads eight whole 128-byte blocks and writes 1 KiB of consecutive scratch;
//   * a block's place in coding order gives its MCU, its component, and - through a search over the at most 128 prefix sums of MCU
//     rows (vertical) or MCU columns (horizontal), held in LDS - its source image and its place in that image's plane (join_source,
//     ist_jpeg_join.h: the same function the host check walks);
//   * natural -> zig-zag order goes through LDS (a block's 8 lanes are in one wave: the hand-over is ordered by a wave-scope fence
//     and barrier, wave_lds_order, not by emission order); no 2-byte store reaches HBM;
//   * a DC outside [-1024, 1023] or an AC outside [-1023, 1023] stores 1 into the call's flag word (a plain store: every writer
//     writes the same value); the host reads it at the encoder's own synchronisation and refuses the join (IST_JOIN_RANGE).
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "ist_ctx.h"
#include "ist_decode.h"
#include "ist_jpeg_enc.h"
#include "ist_jpeg_join.h"

namespace ist {

namespace {

std::atomic<int64_t> g_join_launches{0};

constexpr int kBlockPitch = 72;                 // int16 per block in LDS: 128 bytes + 16, so that the 8 blocks of a wave start on different banks

// zig-zag position -> natural index (T.81 figure A.6)
__device__ __attribute__((aligned(8))) const uint8_t kJoinZigzag[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13,
                                            6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38,
                                            31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// what one lane wrote to LDS is visible to the other lanes of its wave behind this (ist_jpeg_scaled.hip)
__device__ __forceinline__ void wave_lds_order() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ bool out_of_range(uint32_t pair, bool first_is_dc) {
  const int lo = static_cast<int16_t>(pair & 0xFFFFu), hi = static_cast<int16_t>(pair >> 16);
  return lo > 1023 || lo < (first_is_dc ? -1024 : -1023) || hi > 1023 || hi < -1023;
}

}  // namespace

__global__ __launch_bounds__(256) void ist_jpeg_join_kernel(const JoinArgs A) {
  __shared__ int32_t sFirst[kJoinMaxImages + 1];
  __shared__ __attribute__((aligned(16))) int16_t sBlk[kJoinBlocksPerWg * kBlockPitch];
  const JoinTable* __restrict__ T = A.table;
  const int tid = static_cast<int>(threadIdx.x);
  if (tid <= kJoinMaxImages) sFirst[tid] = T->first[tid];
  __syncthreads();
  const int j = tid & 7, slot = tid >> 3;
  const int32_t block = static_cast<int32_t>(blockIdx.x) * kJoinBlocksPerWg + slot;
  const bool live = block < A.row_blocks;         // (a wave's dead lanes are whole blocks: they only skip the loads and stores)
  int16_t* const mine = sBlk + slot * kBlockPitch;
  if (live) {
    const JoinSource s = join_source(sFirst, T->n, A.horizontal, A.is420, A.mcu_row0 + static_cast<int32_t>(blockIdx.y), block);
    const JoinImage& I = T->img[s.image];
    const int16_t* src = I.coef[s.comp] + (static_cast<size_t>(s.by) * static_cast<size_t>(I.blocks_x[s.comp]) + static_cast<size_t>(s.bx)) * 64 + j * 8;
    const uint4 v = *reinterpret_cast<const uint4*>(src);
    if (out_of_range(v.x, j == 0) || out_of_range(v.y, false) || out_of_range(v.z, false) || out_of_range(v.w, false)) *A.flag = 1u;
    *reinterpret_cast<uint4*>(mine + j * 8) = v;
  }
  wave_lds_order();
  if (live) {
    const uint2 z = *reinterpret_cast<const uint2*>(kJoinZigzag + j * 8);      // this lane's eight natural indices
    auto at = [&](uint32_t w, int k) { return static_cast<uint32_t>(static_cast<uint16_t>(mine[(w >> (8 * k)) & 255u])); };
    uint4 o;
    o.x = at(z.x, 0) | (at(z.x, 1) << 16); o.y = at(z.x, 2) | (at(z.x, 3) << 16);
    o.z = at(z.y, 0) | (at(z.y, 1) << 16); o.w = at(z.y, 2) | (at(z.y, 3) << 16);
    int16_t* dst = A.coef + (static_cast<size_t>(blockIdx.y) * static_cast<size_t>(A.row_blocks) + static_cast<size_t>(block)) * 64 + j * 8;
    *reinterpret_cast<uint4*>(dst) = o;
  }
}

int jpeg_join_launch(const JoinArgs& args, int64_t rows, void* stream) {
  const unsigned gx = static_cast<unsigned>((args.row_blocks + kJoinBlocksPerWg - 1) / kJoinBlocksPerWg);
  hipLaunchKernelGGL(ist_jpeg_join_kernel, dim3(gx, static_cast<unsigned>(rows)), dim3(256), 0, static_cast<hipStream_t>(stream), args);
  IST_HIP(hipGetLastError());
  g_join_launches.fetch_add(1, std::memory_order_relaxed);
  return IST_OK;
}

namespace {

// files -> the joined file in a pooled pinned block.  Caller holds ctx->mu and has set the device; the plan is the files' own.
int join_files_locked(ist_ctx* ctx, const uint8_t* const* files, const int64_t* lens, const JoinPlan& plan, int flags, ist_jpeg_join_info* info,
                      uint8_t** out_jpeg, int64_t* out_len) {
  const int n = plan.n;
  const int subsampling = plan.subsampling | flags;
  const int64_t cap = ist_jpeg_bound(plan.width, plan.height, subsampling);
  if (cap < 0) return fail(IST_E_INVALID, "ist_jpeg_join_files: the joined file has no bound");
  Phases ph(ctx, false);                          // (the phases are those of a decode to bitmaps: nothing is recorded for a join)
  FileDecoder fd(ctx, files, lens, n, &ph, IST_COLOR_PROFILE_IGNORE);
  // (declared behind the decoder: the stream is idle before the decoder lets go of the host coefficients that uploads may still read)
  StreamDrain drain(ctx->stream);
  int rc = fd.headers();
  if (rc) return rc;
  for (int i = 0; i < n; ++i)                     // what the arena is sized from must be what the plan was made from
    if (!fd.dec(i).jpeg || fd.dec(i).w != plan.files[static_cast<size_t>(i)].w || fd.dec(i).h != plan.files[static_cast<size_t>(i)].h)
      return fail(IST_E_DECODE, "图片" + std::to_string(i) + "解码异常: JPEG frame header changed between two reads");
  size_t off = 0;
  fd.layout_coefficients(&off);
  const size_t o_table = arena_take(&off, sizeof(JoinTable));
  rc = ctx->scratch_dec.grow(off);
  if (rc) return rc;
  rc = ctx->scratch_file.grow(static_cast<size_t>(cap));
  if (rc) return rc;
  uint8_t* const arena = static_cast<uint8_t*>(ctx->scratch_dec.p);
  PoolBlock flag_block;
  if (!flag_block.take(256)) return fail(IST_E_NOMEM, "out of pinned host memory for the JPEG join");
  volatile uint32_t* const flag = flag_block.at<volatile uint32_t>();
  *flag = 0;
  rc = fd.start(arena, nullptr, nullptr);
  if (rc) return rc;
  std::vector<JpegCoefPlanes> planes;
  rc = fd.coefficients(ctx->stream, &planes);
  if (rc) return rc;
  JoinTable table;
  rc = jpeg_join_table(plan, planes.data(), &table);
  if (rc) return rc;
  IST_HIP(hipMemcpyAsync(arena + o_table, &table, sizeof table, hipMemcpyHostToDevice, ctx->stream));
  const JpegGeometry g = jpeg_geometry(plan.width, plan.height, subsampling);
  JoinArgs A;
  A.table = reinterpret_cast<const JoinTable*>(arena + o_table); A.coef = nullptr; A.flag = const_cast<uint32_t*>(flag);
  A.horizontal = plan.direction == IST_HORIZONTAL; A.is420 = jpeg_ss_420(subsampling);
  A.row_blocks = static_cast<int32_t>(g.row_blocks); A.mcu_row0 = 0;
  JpegSlabSource src;
  src.fill = [&](int64_t r0, int64_t rows, int16_t* coef, const JpegTables*, void* st) -> int {
    A.mcu_row0 = static_cast<int32_t>(r0); A.coef = coef;
    return jpeg_join_launch(A, rows, st);
  };
  src.synced = [&]() -> int {
    if (*flag == 0) return IST_OK;
    info->reason = IST_JOIN_RANGE; info->image = -1; info->width = info->height = 0;
    return fail(IST_E_UNSUPPORTED, std::string("ist_jpeg_join_files: ") + jpeg_join_reason_text(IST_JOIN_RANGE) +
                                       " (a DC outside [-1024, 1023] or an AC outside [-1023, 1023]): the join would not be lossless");
  };
  JpegTables T;
  jpeg_enc_tables_of(plan.q[0], plan.q[1], &T);
  int64_t len = 0;
  rc = jpeg_encode_slabs(ctx, plan.width, plan.height, subsampling, T, ctx->scratch_file.p, cap, &len, ctx->stream, src);
  if (rc) return rc;
  uint8_t* host = nullptr;
  rc = read_back_pooled(ctx->scratch_file.p, static_cast<size_t>(len), ctx->stream, &host);
  if (rc) return rc;
  *out_jpeg = host; *out_len = len;
  return IST_OK;
}

}  // namespace

}  // namespace ist

using namespace ist;

extern "C" {

int64_t ist_debug_jpeg_join_launches(void) { return g_join_launches.load(std::memory_order_relaxed); }

int ist_jpeg_join_files(ist_ctx* ctx, const uint8_t* const* files, const int64_t* lens, int n, int direction, int flags,
                        ist_jpeg_join_info* out_info, uint8_t** out_jpeg, int64_t* out_len) {
  if (!ctx) return fail(IST_E_NO_CONTEXT, "无法获取绘图上下文");
  if (flags != 0 && flags != IST_JPEG_OPTIMIZE) return fail(IST_E_INVALID, "ist_jpeg_join_files: unknown flags");
  if (!files || !lens || n <= 0 || (direction != IST_VERTICAL && direction != IST_HORIZONTAL)) return fail(IST_E_INVALID, "ist_jpeg_join_files: bad argument");
  if (!out_jpeg || !out_len) return fail(IST_E_INVALID, "ist_jpeg_join_files: NULL output");
  *out_jpeg = nullptr; *out_len = 0;
  ist_jpeg_join_info info;
  JoinPlan plan;
  int rc = jpeg_join_eligible(files, lens, n, direction, &info, &plan);
  if (rc == IST_OK) {
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard g(ctx->device);
    if (!g.ok) rc = fail(IST_E_NO_DEVICE, "hipSetDevice failed");
    else rc = join_files_locked(ctx, files, lens, plan, flags, &info, out_jpeg, out_len);
  }
  if (out_info) *out_info = info;
  return rc;
}

}  // extern "C"
