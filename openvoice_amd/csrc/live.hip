// Live streams (openvoice_amd/live.py): the record-driven copy that moves every conversion unit's carried state --
// a solo stream's history shift between ping-pong halves, a pool's gather of ready streams' state from the per-stream
// arena into batch rows, and the scatter of a unit's new output columns back into the next unit's state -- in ONE
// launch per unit and step instead of one Python-issued slice copy per unit and stream.  Memory-bound; no LDS.
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

}  // namespace

extern "C" {

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

}  // extern "C"
