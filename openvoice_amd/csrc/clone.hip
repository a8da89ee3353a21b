// The join between the base-speaker TTS and the tone-colour converter (openvoice_amd/clone.py): the device form of
// audio_numpy_concat (reference openvoice/api.py:56-63: every synthesized sentence followed by 50 ms / speed of
// silence), for any number of utterances in one launch.  Record-driven like ov_carry_rows_f32 and the vad kernels:
// `records` is a DEVICE int64 [R][4] of (src_off, n, dst_off, gap) and
//   dst[dst_off + j] = src[src_off + j], j < n;    dst[dst_off + n + j] = 0, j < gap.
// The sources are rows of the padded TTS output [B, 1, ld] (src_off = b * ld, n = frames_b * hop): what lies beyond n in
// a row belongs to the generator's margin and is never read.  A record the host could not check is checked here.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "openvoice_amd.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
// a 16-byte load from a 4-byte aligned address (the source of a record is aligned against its destination by chance)
typedef float f32x4_u __attribute__((ext_vector_type(4), aligned(4)));

constexpr int kThreads = 256;
constexpr int kVecsPerThread = 4;                                  // 16-byte stores in flight per thread
constexpr int64_t kChunk = (int64_t)kThreads * kVecsPerThread * 4;  // samples of a record's span per workgroup pass
constexpr int kMaxChunksPerRecord = 1024;                           // grid.x bound; longer spans take further passes

// Memory-bound: lanes run along samples.  The span [0, n + gap) of a record is cut at the DESTINATION's 16-byte
// boundaries: `head` samples (0-3) up to the first boundary, then groups of four.  A group that lies wholly inside the
// segment is one (possibly unaligned) 16-byte load and one aligned 16-byte store, one wholly inside the gap one aligned
// store of zeros; the head, the group that straddles n and the last partial group go sample by sample.  Grid (chunk,
// record): a long segment is spread over as many workgroups as it has chunks.
__global__ __launch_bounds__(kThreads) void join_segments_kernel(const float* __restrict__ src, int64_t src_elems,
                                                                 const int64_t* __restrict__ records,
                                                                 float* __restrict__ dst, int64_t dst_elems) {
  const int r = blockIdx.y;
  const int64_t src_off = records[4 * r], n = records[4 * r + 1], dst_off = records[4 * r + 2], gap = records[4 * r + 3];
  // would read outside [0, src_elems) or write outside [0, dst_elems): copy nothing (no sum below can overflow)
  if (src_off < 0 || n < 0 || n > src_elems || src_off > src_elems - n) return;
  if (dst_off < 0 || gap < 0 || n > dst_elems || gap > dst_elems - n || dst_off > dst_elems - (n + gap)) return;
  const int64_t span = n + gap;
  const float* s = src + src_off;
  float* d = dst + dst_off;
  const int64_t head = (int64_t)((4 - ((reinterpret_cast<uintptr_t>(d) >> 2) & 3)) & 3);
  if (blockIdx.x == 0 && (int64_t)threadIdx.x < head && (int64_t)threadIdx.x < span)
    d[threadIdx.x] = (int64_t)threadIdx.x < n ? s[threadIdx.x] : 0.f;
  for (int64_t c0 = head + (int64_t)blockIdx.x * kChunk; c0 < span; c0 += (int64_t)gridDim.x * kChunk) {
    f32x4 v[kVecsPerThread];
#pragma unroll
    for (int k = 0; k < kVecsPerThread; ++k) {                       // every load of the pass before its first store
      const int64_t p = c0 + ((int64_t)k * kThreads + threadIdx.x) * 4;
      v[k] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (p + 4 <= n) {
        v[k] = *reinterpret_cast<const f32x4_u*>(s + p);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (p + e < n) v[k][e] = s[p + e];
      }
    }
#pragma unroll
    for (int k = 0; k < kVecsPerThread; ++k) {
      const int64_t p = c0 + ((int64_t)k * kThreads + threadIdx.x) * 4;
      if (p + 4 <= span) {
        *reinterpret_cast<f32x4*>(d + p) = v[k];
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (p + e < span) d[p + e] = v[k][e];
      }
    }
  }
}

}  // namespace

extern "C" int ov_join_segments_f32(const float* src, int64_t src_elems, const int64_t* records, int R, float* dst,
                                    int64_t dst_elems, int64_t max_span, ov_stream_t stream) {
  if (!src || !records || !dst || R <= 0 || R > 65535 || src_elems <= 0 || dst_elems <= 0 || max_span < 0)
    return OV_E_BADARG;
  if ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 3) return OV_E_ALIGN;
  // max_span sizes the grid only: a record with a longer span is still joined whole, in further passes of its workgroups
  int64_t chunks = max_span / kChunk + 1;              // + 1: the head shifts the groups by up to three samples
  if (chunks > kMaxChunksPerRecord) chunks = kMaxChunksPerRecord;
  hipLaunchKernelGGL(join_segments_kernel, dim3((unsigned)chunks, R), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), src, src_elems, records, dst, dst_elems);
  return hipGetLastError() == hipSuccess ? OV_OK : OV_E_LAUNCH;
}
