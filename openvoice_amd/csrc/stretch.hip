// speed= / duration= of a conversion (openvoice_amd/stretch.py holds the definition and its mirror): the masked latent
// z_hat, in its fp32 rows layout, resampled along time between the reverse flow and the generator.  The project's own
// definition; nothing in the reference stretches a conversion.
//
// Record-driven like ov_carry_rows_f32 and ov_wm_embed_windows_f32: one int64 record per item or window,
//   (src_off, dst_off, rows, src_ld, dst_ld, t_in, i0, j0, n_out, step)
// For jj < n_out, with the GLOBAL output frame j = j0 + jj:  pos = j * step,  i = pos >> 32,
//   f = ((pos & 0xffffffff) >> 8) * 2^-24,   a = src[r][i - i0],   b = src[r][min(i + 1 - i0, t_in - 1)],
//   dst[r][jj] = a + f * (b - a)          fp32: subtract, multiply, add -- three roundings, never contracted to an fma.
// The weights depend on j alone, so a window (a slice whose column 0 is global frame i0) holds the bits of the whole-row
// stretch; nothing depends on the launch: item b of a launch holds the bits of its solo launch.
//
// Plain VALU, memory-bound, no LDS, no atomics.  Threads run along j within a row: the 64 lanes of a wave read 64
// consecutive j, whose i span at most 64 * speed + 1 <= 129 consecutive floats at speed <= 2 -- both gathers of a wave
// fall into at most two contiguous 256-byte spans per row (three when the span is not aligned) -- and write one
// coalesced 256-byte span.  i and f are computed once per thread and reused down the rows.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "openvoice_amd.h"

// a + f * (b - a) keeps its three roundings: the mirror and the kernel agree on what is rounded
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kRowBlocks = 32;                        // blocks striding over a record's rows
constexpr int kFields = 10;
constexpr int64_t kMaxDim = int64_t(1) << 31, kMaxOff = int64_t(1) << 61;
constexpr int64_t kMaxJ = int64_t(1) << 29;           // j * step < 2^29 * 2^33 = 2^62
constexpr int64_t kOne = int64_t(1) << 32;

// The one record check, run by the host on its copy of the table and by every workgroup on the device table: sane
// fields (every sum of products below stays < 2^63), both extents, and 0 <= i - i0 <= t_in - 1 for every j the record
// covers (i is monotone in j: the first and the last j decide).  The neighbour i + 1 is clamped to the slice's last
// column: a caller hands over a slice that holds column i + 1 of its last j, or one that ends at the recording's true end.
__host__ __device__ inline bool record_ok(const int64_t* rec, int64_t src_elems, int64_t dst_elems) {
  const int64_t so = rec[0], d_o = rec[1], rows = rec[2], sld = rec[3], dld = rec[4], t_in = rec[5], i0 = rec[6],
                j0 = rec[7], n_out = rec[8], step = rec[9];
  if (rows < 1 || rows > kMaxDim || t_in < 1 || t_in > kMaxDim || n_out < 1 || n_out > kMaxDim) return false;
  if (sld < t_in || sld > kMaxDim || dld < n_out || dld > kMaxDim || so < 0 || so > kMaxOff || d_o < 0 || d_o > kMaxOff)
    return false;
  // (n_out <= 2^31 is established: kMaxJ - n_out cannot wrap, whatever j0 holds)
  if (i0 < 0 || i0 > kMaxDim || j0 < 0 || j0 > kMaxJ - n_out || step < kOne / 2 || step > 2 * kOne) return false;
  if (so + (rows - 1) * sld + t_in > src_elems || d_o + (rows - 1) * dld + n_out > dst_elems) return false;
  const int64_t first = (j0 * step) >> 32, last = ((j0 + n_out - 1) * step) >> 32;
  return first >= i0 && last - i0 <= t_in - 1;
}

__global__ __launch_bounds__(kThreads) void stretch_rows_kernel(const int64_t* __restrict__ records,
                                                                const float* __restrict__ src, int64_t src_elems,
                                                                float* __restrict__ dst, int64_t dst_elems) {
  const int64_t* rec = records + kFields * (int64_t)blockIdx.z;
  if (!record_ok(rec, src_elems, dst_elems)) return;                    // (block-uniform) a bad record writes nothing
  const int64_t so = rec[0], d_o = rec[1], rows = rec[2], sld = rec[3], dld = rec[4], t_in = rec[5], i0 = rec[6],
                j0 = rec[7], n_out = rec[8], step = rec[9];
  const int64_t jj = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (jj >= n_out) return;
  const int64_t pos = (j0 + jj) * step;
  const int64_t li = (pos >> 32) - i0;                                  // in [0, t_in - 1]: record_ok
  const int64_t li1 = li + 1 < t_in ? li + 1 : t_in - 1;
  const float f = (float)(uint32_t)((pos & 0xffffffff) >> 8) * 5.9604644775390625e-08f;      // 24 bits x 2^-24: exact
  for (int64_t r = blockIdx.y; r < rows; r += gridDim.y) {
    const float* s = src + so + r * sld;
    const float a = s[li], b = s[li1];
    const float d = b - a;
    const float m = f * d;
    dst[d_o + r * dld + jj] = a + m;
  }
}

}  // namespace

extern "C" {

int ov_stretch_rows_f32(const int64_t* records, const int64_t* records_host, int n_records, const float* src,
                        int64_t src_elems, float* dst, int64_t dst_elems, ov_stream_t stream) {
  if (!records || !records_host || !src || !dst || n_records <= 0 || n_records > 65535 || src_elems <= 0 || dst_elems <= 0)
    return OV_E_BADARG;
  if ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 3) return OV_E_ALIGN;
  if (reinterpret_cast<uintptr_t>(records) & 7) return OV_E_ALIGN;
  int64_t max_n = 0, max_rows = 0;
  for (int r = 0; r < n_records; ++r) {
    const int64_t* rec = records_host + kFields * (int64_t)r;
    if (!record_ok(rec, src_elems, dst_elems)) return OV_E_BADARG;       // nothing is launched
    max_rows = rec[2] > max_rows ? rec[2] : max_rows;
    max_n = rec[8] > max_n ? rec[8] : max_n;
  }
  const int64_t col_blocks = (max_n + kThreads - 1) / kThreads;
  if (col_blocks > 0x7fffffff) return OV_E_BADARG;
  dim3 grid((unsigned)col_blocks, (unsigned)(max_rows < kRowBlocks ? max_rows : kRowBlocks), (unsigned)n_records);
  hipLaunchKernelGGL(stretch_rows_kernel, grid, dim3(kThreads), 0, static_cast<hipStream_t>(stream), records, src,
                     src_elems, dst, dst_elems);
  return hipGetLastError() == hipSuccess ? OV_OK : OV_E_LAUNCH;
}

}  // extern "C"
