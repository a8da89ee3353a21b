// The two hand-overs of a ragged batch that runs the bf16 channels-last generator as a few dense length groups
// (openvoice_amd/bf16.py, GeneratorBf16.decode_groups): the flow leaves fp32 channels-first rows [B][C][ld] with a
// different number of valid columns per item; the generator kernels take dense [B_g][L_g][C] bf16 tensors, one per
// group, and write dense fp32 [B_g][L_g * spf] waveforms.  Record-driven like ov_join_segments_f32 and
// ov_frame_hops_multi_f32: one launch each way serves every item of every group, and a record the host could not check
// is checked here.
//
//   pack:   records [n][5] = (src_off, src_ld, dst_off, cols, L)
//             dst[dst_off + l * C + c] = bf16(src[src_off + c * src_ld + l]),  l < cols;   0,  cols <= l < L
//           the source columns >= cols are never read (in a workspace row they are stale).
//   unpack: records [n][4] = (src_off, dst_off, keep, row)
//             dst[dst_off + j] = src[src_off + j],  j < keep;   0,  keep <= j < row.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "openvoice_amd.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
// a 16-byte load from a 4-byte aligned address (a record's source is aligned against its destination by chance)
typedef float f32x4_u __attribute__((ext_vector_type(4), aligned(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int64_t kDim = int64_t(1) << 31, kOff = int64_t(1) << 61;   // every sum of products below stays < 2^63

// Round to nearest even, as torch's float -> bfloat16 conversion and ov_rows_f32_to_cl_bf16: NaN -> 0x7fc0, infinities
// and overflow exact.
__device__ inline uint32_t bf16_rne(float f) {
  const uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// ---- pack: fp32 channels-first rows -> the groups' dense bf16 channels-last tensors -----------------------------------
// The transpose of ov_rows_f32_to_cl_bf16 (csrc/live.hip) with a record per item: a workgroup moves tiles of kTC channels
// x kTL columns through LDS (fp32, [channel][column], rows padded by one float).  fp32 side, columns contiguous: lane t
// takes the float4 of columns 4v .. 4v + 3 of channel c, v = (t & 7) + 8 * ((t >> 5) & 1), c = ((t >> 3) & 3) +
// 4 * (t >> 6) (+ 16 on the second pass) when the record's rows are 16-byte aligned -- a float4 that would cross column
// `cols` moves as scalars -- and lane = column, a wave per channel, otherwise.  bf16 side, channels contiguous: lane t
// stores the 8 channels 8 q .. 8 q + 7 (16 bytes) of column l, q = t & 3, l = t >> 2; columns in [cols, L) are stored
// as zeros without touching LDS.  Grid (column tile, channel tile, record); the column tiles of a record longer than
// the grid are taken in further passes.
constexpr int kTC = 32, kTL = 64, kTLd = kTL + 1;
constexpr int kPackTilesX = 16;

__global__ __launch_bounds__(256) void pack_groups_kernel(const float* __restrict__ src, int64_t src_len,
                                                          const int64_t* __restrict__ records, int C,
                                                          uint16_t* __restrict__ dst, int64_t dst_len, int bases_aligned) {
  __shared__ float tile[kTC * kTLd];
  const int64_t* rec = records + 5 * (int64_t)blockIdx.z;
  const int64_t src_off = rec[0], src_ld = rec[1], dst_off = rec[2], cols = rec[3], L = rec[4];
  if (src_off < 0 || src_ld < 0 || dst_off < 0 || cols < 0 || L < 1 || cols > L) return;
  if (L > kDim || src_ld > kDim || src_off > kOff || dst_off > kOff) return;
  if (dst_len < L * C || dst_off > dst_len - L * C) return;                         // would write outside dst
  if (cols > 0 && (src_len < (C - 1) * src_ld + cols || src_off > src_len - ((C - 1) * src_ld + cols))) return;
  const int t = threadIdx.x, c0 = blockIdx.y * kTC;
  const int nc = min(kTC, C - c0);                                                   // a multiple of 8
  const bool src_vec = (bases_aligned & 1) && ((src_off | src_ld) & 3) == 0;
  const bool dst_vec = (bases_aligned & 2) && (dst_off & 7) == 0;
  const float* s0 = src + src_off + (int64_t)c0 * src_ld;
  for (int64_t l0 = (int64_t)blockIdx.x * kTL; l0 < L; l0 += (int64_t)gridDim.x * kTL) {
    const int nl = (int)min((int64_t)kTL, L - l0);                                  // columns stored
    const int nv = (int)max((int64_t)0, min((int64_t)kTL, cols - l0));              // columns read
    if (nv > 0) {
      const float* s = s0 + l0;
      if (src_vec) {
        const int v = (t & 7) + 8 * ((t >> 5) & 1);
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
          const int c = ((t >> 3) & 3) + 4 * (t >> 6) + 16 * pass;
          if (c < nc && 4 * v < nv) {
            const float* p = s + (int64_t)c * src_ld + 4 * v;
            float* q = tile + c * kTLd + 4 * v;
            if (4 * v + 4 <= nv) {
              const f32x4 x = *reinterpret_cast<const f32x4*>(p);
              q[0] = x[0], q[1] = x[1], q[2] = x[2], q[3] = x[3];
            } else {
              for (int j = 0; 4 * v + j < nv; ++j) q[j] = p[j];
            }
          }
        }
      } else {
        const int l = t & 63;
        if (l < nv)
          for (int c = t >> 6; c < nc; c += 4) tile[c * kTLd + l] = s[(int64_t)c * src_ld + l];
      }
    }
    __syncthreads();
    const int q = t & 3, l = t >> 2;
    if (l < nl && 8 * q < nc) {
      uint32_t h[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) h[i] = l < nv ? bf16_rne(tile[(8 * q + i) * kTLd + l]) : 0u;
      uint16_t* d = dst + dst_off + (l0 + l) * C + c0 + 8 * q;
      if (dst_vec) {
        *reinterpret_cast<u32x4*>(d) = u32x4{h[0] | h[1] << 16, h[2] | h[3] << 16, h[4] | h[5] << 16, h[6] | h[7] << 16};
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = (uint16_t)h[i];
      }
    }
    __syncthreads();                                  // the tile is filled again by the next pass
  }
}

// ---- unpack: the groups' fp32 waveforms -> the rows of the padded output ----------------------------------------------
// ov_join_segments_f32's copy (csrc/clone.hip) with the span given as (keep, row): the span [0, row) of a record is cut at
// the DESTINATION's 16-byte boundaries; a group of four wholly inside [0, keep) is one (possibly unaligned) 16-byte load
// and one aligned 16-byte store, one wholly beyond an aligned store of zeros, the head, the group that straddles `keep`
// and the last partial group go sample by sample.  Grid (chunk, record), further passes for rows longer than the grid.
constexpr int kThreads = 256;
constexpr int kVecsPerThread = 4;
constexpr int64_t kChunk = (int64_t)kThreads * kVecsPerThread * 4;
constexpr int kUnpackChunksX = 64;

__global__ __launch_bounds__(kThreads) void unpack_groups_kernel(const float* __restrict__ src, int64_t src_len,
                                                                 const int64_t* __restrict__ records,
                                                                 float* __restrict__ dst, int64_t dst_len) {
  const int64_t* rec = records + 4 * (int64_t)blockIdx.y;
  const int64_t src_off = rec[0], dst_off = rec[1], keep = rec[2], row = rec[3];
  if (src_off < 0 || dst_off < 0 || keep < 0 || row < keep) return;
  if (keep > src_len || src_off > src_len - keep) return;                  // would read outside [0, src_len)
  if (row > dst_len || dst_off > dst_len - row) return;                    // would write outside [0, dst_len)
  const float* s = src + src_off;
  float* d = dst + dst_off;
  const int64_t head = (int64_t)((4 - ((reinterpret_cast<uintptr_t>(d) >> 2) & 3)) & 3);
  if (blockIdx.x == 0 && (int64_t)threadIdx.x < head && (int64_t)threadIdx.x < row)
    d[threadIdx.x] = (int64_t)threadIdx.x < keep ? s[threadIdx.x] : 0.f;
  for (int64_t c0 = head + (int64_t)blockIdx.x * kChunk; c0 < row; c0 += (int64_t)gridDim.x * kChunk) {
    f32x4 v[kVecsPerThread];
#pragma unroll
    for (int k = 0; k < kVecsPerThread; ++k) {                             // every load of the pass before its first store
      const int64_t p = c0 + ((int64_t)k * kThreads + threadIdx.x) * 4;
      v[k] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (p + 4 <= keep) {
        v[k] = *reinterpret_cast<const f32x4_u*>(s + p);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (p + e < keep) v[k][e] = s[p + e];
      }
    }
#pragma unroll
    for (int k = 0; k < kVecsPerThread; ++k) {
      const int64_t p = c0 + ((int64_t)k * kThreads + threadIdx.x) * 4;
      if (p + 4 <= row) {
        *reinterpret_cast<f32x4*>(d + p) = v[k];
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (p + e < row) d[p + e] = v[k][e];
      }
    }
  }
}

}  // namespace

extern "C" {

int ov_pack_groups_cl_bf16(const float* src, int64_t src_len, const int64_t* records, int n, int C, uint16_t* dst,
                           int64_t dst_len, ov_stream_t stream) {
  if (!src || !records || !dst || n < 0 || n > 65535 || C <= 0 || C % 8 != 0 || (C - 1) / kTC + 1 > 65535 ||
      src_len <= 0 || dst_len <= 0)
    return OV_E_BADARG;
  if ((reinterpret_cast<uintptr_t>(src) & 3) || (reinterpret_cast<uintptr_t>(dst) & 1)) return OV_E_ALIGN;
  if (n == 0) return OV_OK;
  const int aligned = (int)!(reinterpret_cast<uintptr_t>(src) & 15) | (int)!(reinterpret_cast<uintptr_t>(dst) & 15) << 1;
  hipLaunchKernelGGL(pack_groups_kernel, dim3(kPackTilesX, (C - 1) / kTC + 1, n), dim3(256), 0,
                     static_cast<hipStream_t>(stream), src, src_len, records, C, dst, dst_len, aligned);
  return hipGetLastError() == hipSuccess ? OV_OK : OV_E_LAUNCH;
}

int ov_unpack_groups_f32(const float* src, int64_t src_len, const int64_t* records, int n, float* dst, int64_t dst_len,
                         ov_stream_t stream) {
  if (!src || !records || !dst || n < 0 || n > 65535 || src_len <= 0 || dst_len <= 0) return OV_E_BADARG;
  if ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 3) return OV_E_ALIGN;
  if (n == 0) return OV_OK;
  hipLaunchKernelGGL(unpack_groups_kernel, dim3(kUnpackChunksX, n), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                     src, src_len, records, dst, dst_len);
  return hipGetLastError() == hipSuccess ? OV_OK : OV_E_LAUNCH;
}

}  // extern "C"
