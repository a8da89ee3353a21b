// Counter-based Gaussian noise (openvoice_amd/noise.py): the value at (seed, stream, purpose, channel c, frame t) is a
// pure function of those five numbers, so a live stream pushed in any chunking, a windowed stream, convert_long,
// convert_many and a one-pass convert all draw the same noise for the same audio and nobody keeps a noise tensor.
//   (r0, r1, r2, r3) = Philox4x32-10(counter = (t / 4, c, stream, purpose), key = (seed & 0xffffffff, seed >> 32))
//   pair p = (t % 4) / 2 takes (ra, rb) = (r0, r1) or (r2, r3);  u1 = ((ra >> 8) + 0.5) 2^-24,  u2 = (rb >> 8) 2^-24
//   n = sqrt(-2 ln u1) cos(2 pi u2) for even t, ... sin(2 pi u2) for odd t                        (|n| <= 5.887)
// Record-driven like ov_join_segments_f32: `records` is a DEVICE int64 [R][7] of (seed, stream, purpose, f0, nf, dst_off,
// dst_ld) and  dst[dst_off + c * dst_ld + i] = n(seed, stream, purpose, c, f0 + i),  c < C, i < nf.  Nothing else is
// written.  A record the host could not check is checked here.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "openvoice_amd.h"
#include "philox_normal.h"

namespace {

using ovn::f32x4;

constexpr int kThreads = 256;
constexpr int64_t kMaxFrame = (int64_t)1 << 34;     // frames t < 2^34: the Philox block t / 4 is one 32-bit word
constexpr int kMaxChunksPerRecord = 4096;           // grid.x bound; larger slabs take further passes

// Compute-light and store-bound: one thread owns one Philox block = four consecutive frames of one channel, lanes run
// along frames (then channels, so that the few blocks of a live chunk still fill a workgroup).  The four values are
// computed in ONE place, before the thread knows how it will store them: a value depends on nothing but its five
// coordinates.  A block wholly inside [f0, f0 + nf) whose destination is 16-byte aligned is one vector store; edge
// blocks and unaligned destinations go element by element.  Grid (chunk, record).
__global__ __launch_bounds__(kThreads) void normal_philox_kernel(const int64_t* __restrict__ records, int C,
                                                                 float* __restrict__ dst, int64_t dst_elems) {
  const int64_t* rec = records + 7 * (int64_t)blockIdx.y;
  const int64_t seed = rec[0], strm = rec[1], purpose = rec[2], f0 = rec[3], nf = rec[4], dst_off = rec[5], dst_ld = rec[6];
  if (seed < 0 || strm < 0 || strm > 0xFFFFFFFFll || purpose < 0 || purpose > 0xFFFFFFFFll) return;
  if (nf <= 0 || f0 < 0 || f0 > kMaxFrame || nf > kMaxFrame - f0) return;
  // rows would overlap, or the slab would leave [0, dst_elems): write nothing (no sum below can overflow)
  if (dst_ld < nf || dst_off < 0 || nf > dst_elems || dst_off > dst_elems - nf) return;
  if (C > 1 && (dst_elems - nf - dst_off) / dst_ld < (int64_t)(C - 1)) return;
  const uint64_t q0 = (uint64_t)f0 >> 2;
  const uint64_t nblocks = (((uint64_t)(f0 + nf - 1)) >> 2) - q0 + 1;
  const uint64_t total = nblocks * (uint64_t)C;
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)((uint64_t)seed >> 32);
  for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (uint64_t)gridDim.x * kThreads) {
    const uint64_t c = i / nblocks, q = q0 + (i - c * nblocks);
    const f32x4 v = ovn::normal_block((uint32_t)q, (uint32_t)c, (uint32_t)strm, (uint32_t)purpose, k0, k1);
    const int64_t rel = (int64_t)(q << 2) - f0;                    // slab column of the block's first frame (>= -3)
    const int64_t at = dst_off + (int64_t)c * dst_ld + rel;        // element of dst; used only where rel + e is in [0, nf)
    if (rel >= 0 && rel + 4 <= nf && (((reinterpret_cast<uintptr_t>(dst) >> 2) + (uint64_t)at) & 3) == 0) {
      *reinterpret_cast<f32x4*>(dst + at) = v;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (rel + e >= 0 && rel + e < nf) dst[at + e] = v[e];
    }
  }
}

}  // namespace

extern "C" int ov_normal_philox_f32(const int64_t* records, int R, int C, float* dst, int64_t dst_elems,
                                    int64_t max_frames, ov_stream_t stream) {
  if (!records || !dst || R <= 0 || R > 65535 || C <= 0 || dst_elems <= 0 || max_frames < 0) return OV_E_BADARG;
  if (reinterpret_cast<uintptr_t>(dst) & 3) return OV_E_ALIGN;
  // max_frames sizes the grid only: a record with more frames is still filled whole, in further passes of its workgroups
  if (max_frames > kMaxFrame) max_frames = kMaxFrame;
  const int64_t blocks = max_frames / 4 + 2;           // + 2: a slab may cut a Philox block at either end
  int64_t chunks = kMaxChunksPerRecord;
  if (blocks < (int64_t)kMaxChunksPerRecord * kThreads) {                            // (the product below cannot overflow)
    chunks = (blocks * (int64_t)C + kThreads - 1) / kThreads;
    if (chunks > kMaxChunksPerRecord) chunks = kMaxChunksPerRecord;
  }
  hipLaunchKernelGGL(normal_philox_kernel, dim3((unsigned)chunks, R), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), records, C, dst, dst_elems);
  return hipGetLastError() == hipSuccess ? OV_OK : OV_E_LAUNCH;
}
