// Live streams (openvoice_amd/live.py): the record-driven copy that moves every conversion unit's carried state --
// a solo stream's history shift between ping-pong halves, a pool's gather of ready streams' state from the per-stream
// arena into batch rows, and the scatter of a unit's new output columns back into the next unit's state -- in ONE
// launch per unit and step instead of one Python-issued slice copy per unit and stream.  Memory-bound; no LDS.
//
// And the two layout hand-overs of a live generator unit that runs on the bf16 channels-last kernels: the arena and the
// carries stay fp32 channels-first, so the unit's batch rows become a dense [B, L, C] bf16 tensor on the way in and its
// output becomes fp32 channels-first rows again on the way out -- a transpose through LDS with a cast, one launch per
// direction for every row of the batch.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "openvoice_amd.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kRowsPerBlock = 4;      // one wave per row of a block; blocks stride over a record's rows

// Record r = (src_off, dst_off, rows, cols, src_ld, dst_ld), all int64, in elements:
//   dst[dst_off + i * dst_ld + j] = src[src_off + i * src_ld + j],  i < rows, j < cols.
// The table lives on the device, so each record is checked here against the two extents: a record with negative or
// overflowing fields, or one whose destination leaves [0, dst_elems), touches nothing; a record whose destination is in
// range but whose source is not writes zeros there.  Lanes run along columns; a row moves as 16-byte vectors when both
// of its row starts are 16-byte aligned (vec_ok: the bases are, and offsets / lds are multiples of 4), scalars otherwise.
__global__ __launch_bounds__(256) void carry_rows_kernel(const int64_t* __restrict__ records, const float* __restrict__ src,
                                                         int64_t src_elems, float* __restrict__ dst, int64_t dst_elems,
                                                         int bases_aligned) {
  const int64_t* rec = records + 6 * (int64_t)blockIdx.y;
  const int64_t so = rec[0], d_o = rec[1], rows = rec[2], cols = rec[3], sld = rec[4], dld = rec[5];
  const int64_t kDim = int64_t(1) << 31, kOff = int64_t(1) << 61;   // every sum of products below stays < 2^63
  if (rows <= 0 || cols <= 0 || so < 0 || d_o < 0 || sld < 0 || dld < 0 || rows > kDim || cols > kDim || sld > kDim ||
      dld > kDim || so > kOff || d_o > kOff)
    return;
  if (rows > 1 && (dld < cols)) return;                  // rows of the destination would overlap
  const int64_t d_last = d_o + (rows - 1) * dld + cols;  // one past the last destination element
  if (d_last > dst_elems) return;
  const bool src_ok = so + (rows - 1) * sld + cols <= src_elems;      // source rows may overlap (sld 0: broadcast)
  const bool vec = bases_aligned && ((so | d_o | sld | dld) & 3) == 0;
  const int lane = threadIdx.x & 63;
  for (int64_t i = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6); i < rows;
       i += (int64_t)gridDim.x * kRowsPerBlock) {
    float* d = dst + d_o + i * dld;
    const float* s = src + so + i * sld;
    int64_t j0 = 0;
    if (vec) {
      const int64_t nv = cols >> 2;
      for (int64_t v = lane; v < nv; v += 64) {
        const f32x4 x = src_ok ? *reinterpret_cast<const f32x4*>(s + 4 * v) : f32x4{0.f, 0.f, 0.f, 0.f};
        *reinterpret_cast<f32x4*>(d + 4 * v) = x;
      }
      j0 = nv << 2;
    }
    for (int64_t j = j0 + lane; j < cols; j += 64) d[j] = src_ok ? s[j] : 0.f;
  }
}

// ---- the seam of a look-ahead stream ---------------------------------------------------------------------------------
// Record r = (old_off, new_off, dst_off, n, x), all int64, in elements (old / new relative to src, dst to dst):
//   dst[dst_off + i] = fmaf(w[i], new[i] - old[i], old[i])  for i < min(x, n),   = new[i]  for the rest of i < n.
// One record is one stream's piece of a round, so one launch serves the pool.  Checked here like the carry's records: a
// record with a negative or oversized field, x > w_elems, or whose old / new / dst span leaves its buffer touches
// nothing.  Lanes run along samples; a record moves as 16-byte vectors when the four bases are 16-byte aligned and its
// three offsets are multiples of 4 (the vector straddling x and the tail go element by element), as scalars otherwise.
// Both forms apply the same two operations per element, so the bits do not depend on the form.
constexpr int kFadeBlocks = 4;        // blocks per record; a piece is chunk x hop samples (3840 at the smallest chunk)

__device__ inline float fade_one(float w, float o, float n) { return __builtin_fmaf(w, n - o, o); }

__global__ __launch_bounds__(256) void crossfade_rows_kernel(const int64_t* __restrict__ records, const float* __restrict__ w,
                                                             int64_t w_elems, const float* __restrict__ src,
                                                             int64_t src_elems, float* __restrict__ dst, int64_t dst_elems,
                                                             int bases_aligned) {
  const int64_t* rec = records + 5 * (int64_t)blockIdx.y;
  const int64_t oo = rec[0], no = rec[1], d_o = rec[2], n = rec[3], x = rec[4];
  const int64_t kDim = int64_t(1) << 31, kOff = int64_t(1) << 61;
  if (n <= 0 || x < 0 || oo < 0 || no < 0 || d_o < 0 || n > kDim || x > kDim || oo > kOff || no > kOff || d_o > kOff) return;
  const int64_t xb = x < n ? x : n;                       // blended samples
  if (x > w_elems || oo + xb > src_elems || no + n > src_elems || d_o + n > dst_elems) return;
  const float* o = src + oo;
  const float* p = src + no;
  float* d = dst + d_o;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (int64_t)gridDim.x * blockDim.x;
  int64_t j0 = 0;
  if (bases_aligned && ((oo | no | d_o) & 3) == 0) {
    const int64_t nv = n >> 2;
    for (int64_t v = t; v < nv; v += nt) {
      const int64_t i = 4 * v;
      f32x4 y = *reinterpret_cast<const f32x4*>(p + i);
      if (i + 4 <= xb) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(o + i), c = *reinterpret_cast<const f32x4*>(w + i);
        y = f32x4{fade_one(c[0], a[0], y[0]), fade_one(c[1], a[1], y[1]), fade_one(c[2], a[2], y[2]),
                  fade_one(c[3], a[3], y[3])};
      } else if (i < xb) {
        for (int e = 0; e < 4; ++e)
          if (i + e < xb) y[e] = fade_one(w[i + e], o[i + e], y[e]);
      }
      *reinterpret_cast<f32x4*>(d + i) = y;
    }
    j0 = nv << 2;
  }
  for (int64_t j = j0 + t; j < n; j += nt) d[j] = j < xb ? fade_one(w[j], o[j], p[j]) : p[j];
}

// ---- fp32 channels-first rows <-> dense bf16 channels-last ----------------------------------------------------------
// One workgroup moves a tile of kTC channels x kTL columns of one batch row through LDS (fp32, [channel][column], rows
// padded by one float).  Two lane maps, each coalesced on its side of the transpose:
//  * fp32 side, columns contiguous.  Vector form: lane t takes the float4 of columns 4v .. 4v + 3 of channel c with
//    v = (t & 7) + 8 * ((t >> 5) & 1), c = ((t >> 3) & 3) + 4 * (t >> 6) (+ 16 on the second pass): 8 lanes cover 128
//    contiguous bytes, and a 32-lane LDS group touches banks (65 c + 4 v + j) % 32 = 4 consecutive channels x 8 v = all
//    32 banks once.  Scalar form (a base, ld or row stride that is not 16-byte aligned): lane = column, a wave per
//    channel.  A float4 that would cross column L falls back to scalars, so any L works in both forms.
//  * bf16 side, channels contiguous: lane t takes the 8 channels 8 q .. 8 q + 7 (16 bytes) of column l, q = t & 3,
//    l = t >> 2: 4 lanes cover the tile's 64 contiguous bytes of a column; in LDS a 32-lane group touches banks
//    (65 (8 q + i) + l) % 32 = (8 q + i + l) % 32 over q < 4, 8 consecutive l: all 32 banks once.
constexpr int kTC = 32, kTL = 64, kTLd = kTL + 1;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// Round to nearest even, as torch's float -> bfloat16 conversion: NaN -> 0x7fc0, infinities and overflow exact.
__device__ inline uint32_t bf16_rne(float f) {
  const uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// The fp32 side's lane map: calls f(channel, first column, columns) for this lane's pieces of the tile.
template <bool kVec, typename F> __device__ inline void for_f32_pieces(int t, int nl, F f) {
  if (kVec) {
    const int v = (t & 7) + 8 * ((t >> 5) & 1), c = ((t >> 3) & 3) + 4 * (t >> 6);
    if (4 * v < nl) {
      f(c, 4 * v, min(4, nl - 4 * v));
      f(c + 16, 4 * v, min(4, nl - 4 * v));
    }
  } else {
    const int l = t & 63;
    if (l < nl)
      for (int c = t >> 6; c < kTC; c += 4) f(c, l, 1);
  }
}

template <bool kVec>
__global__ __launch_bounds__(256) void rows_f32_to_cl_bf16_kernel(const float* __restrict__ src, int64_t src_bs, int src_ld,
                                                                  uint16_t* __restrict__ dst, int C, int L, int dst_vec) {
  __shared__ float tile[kTC * kTLd];
  const int t = threadIdx.x, l0 = blockIdx.x * kTL, c0 = blockIdx.y * kTC;
  const int nl = min(kTL, L - l0);
  const float* s = src + (int64_t)blockIdx.z * src_bs + (int64_t)c0 * src_ld + l0;
  for_f32_pieces<kVec>(t, nl, [&](int c, int l, int n) {
    const float* p = s + (int64_t)c * src_ld + l;
    float* q = tile + c * kTLd + l;
    if (n == 4) {
      const f32x4 x = *reinterpret_cast<const f32x4*>(p);
      q[0] = x[0], q[1] = x[1], q[2] = x[2], q[3] = x[3];
    } else {
      for (int j = 0; j < n; ++j) q[j] = p[j];
    }
  });
  __syncthreads();
  const int q = t & 3, l = t >> 2;
  if (l >= nl) return;
  uint32_t h[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) h[i] = bf16_rne(tile[(8 * q + i) * kTLd + l]);
  uint16_t* d = dst + ((int64_t)blockIdx.z * L + l0 + l) * C + c0 + 8 * q;
  if (dst_vec) {
    *reinterpret_cast<u32x4*>(d) = u32x4{h[0] | h[1] << 16, h[2] | h[3] << 16, h[4] | h[5] << 16, h[6] | h[7] << 16};
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = (uint16_t)h[i];
  }
}

template <bool kVec>
__global__ __launch_bounds__(256) void cl_bf16_to_rows_f32_kernel(const uint16_t* __restrict__ src, float* __restrict__ dst,
                                                                  int64_t dst_bs, int dst_ld, int C, int L, int src_vec) {
  __shared__ float tile[kTC * kTLd];
  const int t = threadIdx.x, l0 = blockIdx.x * kTL, c0 = blockIdx.y * kTC;
  const int nl = min(kTL, L - l0);
  const int q = t & 3, l = t >> 2;
  if (l < nl) {
    const uint16_t* p = src + ((int64_t)blockIdx.z * L + l0 + l) * C + c0 + 8 * q;
    uint32_t h[8];
    if (src_vec) {
      const u32x4 x = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
      for (int i = 0; i < 4; ++i) h[2 * i] = x[i] & 0xffffu, h[2 * i + 1] = x[i] >> 16;
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) h[i] = p[i];
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) tile[(8 * q + i) * kTLd + l] = __uint_as_float(h[i] << 16);
  }
  __syncthreads();
  float* d0 = dst + (int64_t)blockIdx.z * dst_bs + (int64_t)c0 * dst_ld + l0;
  for_f32_pieces<kVec>(t, nl, [&](int c, int lc, int n) {
    float* d = d0 + (int64_t)c * dst_ld + lc;
    const float* x = tile + c * kTLd + lc;
    if (n == 4) {
      *reinterpret_cast<f32x4*>(d) = f32x4{x[0], x[1], x[2], x[3]};
    } else {
      for (int j = 0; j < n; ++j) d[j] = x[j];
    }
  });
}

// Shared host checks of the two hand-overs: rows = the fp32 side (B rows of bs elements, C channels of ld columns).
bool handover_args_ok(const void* rows, const void* cl, int64_t bs, int ld, int B, int C, int L) {
  return rows && cl && B >= 1 && B <= 65535 && C >= kTC && C % kTC == 0 && C / kTC <= 65535 && L >= 1 && ld >= L &&
         bs >= (int64_t)C * ld;
}

bool aligned16(const void* p) { return !(reinterpret_cast<uintptr_t>(p) & 15); }

}  // namespace

extern "C" {

int ov_rows_f32_to_cl_bf16(const float* src, int64_t src_bs, int src_ld, uint16_t* dst, int B, int C, int L,
                           ov_stream_t stream) {
  if (!handover_args_ok(src, dst, src_bs, src_ld, B, C, L)) return OV_E_BADARG;
  const bool vec = aligned16(src) && !(src_ld & 3) && !(src_bs & 3);
  dim3 grid((L - 1) / kTL + 1, C / kTC, B);
  hipLaunchKernelGGL(vec ? rows_f32_to_cl_bf16_kernel<true> : rows_f32_to_cl_bf16_kernel<false>, grid, dim3(256), 0,
                     static_cast<hipStream_t>(stream), src, src_bs, src_ld, dst, C, L, (int)aligned16(dst));
  return hipGetLastError() == hipSuccess ? OV_OK : OV_E_LAUNCH;
}

int ov_cl_bf16_to_rows_f32(const uint16_t* src, float* dst, int64_t dst_bs, int dst_ld, int B, int C, int L,
                           ov_stream_t stream) {
  if (!handover_args_ok(dst, src, dst_bs, dst_ld, B, C, L)) return OV_E_BADARG;
  const bool vec = aligned16(dst) && !(dst_ld & 3) && !(dst_bs & 3);
  dim3 grid((L - 1) / kTL + 1, C / kTC, B);
  hipLaunchKernelGGL(vec ? cl_bf16_to_rows_f32_kernel<true> : cl_bf16_to_rows_f32_kernel<false>, grid, dim3(256), 0,
                     static_cast<hipStream_t>(stream), src, dst, dst_bs, dst_ld, C, L, (int)aligned16(src));
  return hipGetLastError() == hipSuccess ? OV_OK : OV_E_LAUNCH;
}

int ov_carry_rows_f32(const int64_t* records, int n_records, const float* src_base, int64_t src_elems, float* dst_base,
                      int64_t dst_elems, ov_stream_t stream) {
  if (!records || !src_base || !dst_base || n_records <= 0 || n_records > 65535 || src_elems <= 0 || dst_elems <= 0)
    return OV_E_BADARG;
  const int aligned = !(reinterpret_cast<uintptr_t>(src_base) & 15) && !(reinterpret_cast<uintptr_t>(dst_base) & 15);
  // 16 blocks x 4 rows per record: 64 rows in flight per record, the rest strided (state rows are 32 - 705 per record)
  dim3 grid(16, n_records);
  hipLaunchKernelGGL(carry_rows_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), records, src_base,
                     src_elems, dst_base, dst_elems, aligned);
  return hipGetLastError() == hipSuccess ? OV_OK : OV_E_LAUNCH;
}

int ov_crossfade_rows_f32(const int64_t* records, int n_records, const float* w, int64_t w_elems, const float* src_base,
                          int64_t src_elems, float* dst_base, int64_t dst_elems, ov_stream_t stream) {
  if (!records || !w || !src_base || !dst_base || n_records <= 0 || n_records > 65535 || w_elems <= 0 || src_elems <= 0 ||
      dst_elems <= 0)
    return OV_E_BADARG;
  const int aligned = aligned16(w) && aligned16(src_base) && aligned16(dst_base);
  dim3 grid(kFadeBlocks, n_records);
  hipLaunchKernelGGL(crossfade_rows_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), records, w, w_elems,
                     src_base, src_elems, dst_base, dst_elems, aligned);
  return hipGetLastError() == hipSuccess ? OV_OK : OV_E_LAUNCH;
}

}  // extern "C"
