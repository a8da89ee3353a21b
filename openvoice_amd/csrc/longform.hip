// Windowed long-form conversion (openvoice_amd/longform.py): the framing of W fixed-length windows straight out of one
// long waveform (or out of one span per window, for many streams / recordings in one launch), and the copy of each
// window's core samples into the long output.  Both are memory-bound gathers / copies with 64-bit sample indices; neither
// uses LDS.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "openvoice_amd.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// hops[w][c][u] = ypad[hop * (first_frame[w] + u) + c] for u < U, ypad = wave reflect-padded by `pad` samples at the
// two TRUE ends of the file (zero beyond them): the (hop, U) plane of ov_frame_hops_f32 for the frames
// [f0, f0 + U - 3) of the whole file.  A workgroup covers 64 hop phases x 64 u; lane c reads sample hop * u + c, so a
// wave's 64 reads of one u are consecutive samples (coalesced), and every thread stores 4 consecutive u as one 16-byte
// vector.  Columns [U, U rounded up to 4) are written as 0.
__global__ __launch_bounds__(256) void frame_hops_windows_kernel(const float* __restrict__ wave, int64_t n,
                                                                 const int64_t* __restrict__ first_frame,
                                                                 int hop, int pad, int U, int ld,
                                                                 float* __restrict__ hops) {
  const int w = blockIdx.z;
  const int c = blockIdx.y * 64 + (threadIdx.x & 63);
  if (c >= hop) return;
  const int64_t f0 = first_frame[w];
  float* row = hops + ((int64_t)w * hop + c) * ld;
  for (int g = threadIdx.x >> 6; g < 16; g += 4) {
    const int u0 = blockIdx.x * 64 + 4 * g;
    if (u0 >= U) break;
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t i = (f0 + u0 + j) * hop + c - pad;     // index into the un-padded waveform
      float x = 0.f;
      if (u0 + j < U && i >= -(int64_t)pad && i < n + pad) {
        const int64_t k = i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i);   // in [0, n) because pad < n
        x = wave[k];
      }
      v[j] = x;
    }
    *reinterpret_cast<f32x4*>(row + u0) = v;
  }
}

// ov_frame_hops_multi_f32: frame_hops_windows_kernel with one source per window.  Window w frames the span
// pool[base, base + n) of its record (base, n, f0) as its own waveform, reflect-padded at the span's two ends.  The
// records live on the device, so a record the host could not check is checked here: base < 0, n <= pad (reflection
// undefined) or base + n > pool_len make the window all zeros, and nothing outside `pool` is read.
__global__ __launch_bounds__(256) void frame_hops_multi_kernel(const float* __restrict__ pool, int64_t pool_len,
                                                               const int64_t* __restrict__ records, int hop, int pad,
                                                               int U, int ld, float* __restrict__ hops) {
  const int w = blockIdx.z;
  const int c = blockIdx.y * 64 + (threadIdx.x & 63);
  if (c >= hop) return;
  const int64_t base = records[3 * w], n = records[3 * w + 1], f0 = records[3 * w + 2];
  const bool ok = base >= 0 && n > pad && base <= pool_len - n;
  const float* wave = pool + (ok ? base : 0);
  float* row = hops + ((int64_t)w * hop + c) * ld;
  for (int g = threadIdx.x >> 6; g < 16; g += 4) {
    const int u0 = blockIdx.x * 64 + 4 * g;
    if (u0 >= U) break;
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t i = (f0 + u0 + j) * hop + c - pad;     // index into the un-padded span
      float x = 0.f;
      if (ok && u0 + j < U && i >= -(int64_t)pad && i < n + pad) {
        const int64_t k = i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i);   // in [0, n) because pad < n
        x = wave[k];
      }
      v[j] = x;
    }
    *reinterpret_cast<f32x4*>(row + u0) = v;
  }
}

// out[(core_lo - out_frame0) * spf + s] = o_hat[w][(core_lo - f0) * spf + s] for s < (core_hi - core_lo) * spf, with
// (f0, core_lo, core_hi) = windows[w].  A record that is not inside its window, or whose core would land outside
// [0, out_len), copies nothing.
template <bool VEC>
__global__ __launch_bounds__(256) void stitch_window_cores_kernel(const float* __restrict__ o_hat,
                                                                  const int64_t* __restrict__ windows, int Tw, int spf,
                                                                  float* __restrict__ out, int64_t out_len,
                                                                  int64_t out_frame0) {
  const int w = blockIdx.y;
  const int64_t f0 = windows[3 * w], lo = windows[3 * w + 1], hi = windows[3 * w + 2];
  if (lo < f0 || hi < lo || hi > f0 + Tw || lo < out_frame0 || (hi - out_frame0) * spf > out_len) return;
  const int64_t count = (hi - lo) * spf;
  const float* src = o_hat + (int64_t)w * Tw * spf + (lo - f0) * spf;
  float* dst = out + (lo - out_frame0) * spf;
  const int64_t s = ((int64_t)blockIdx.x * 256 + threadIdx.x) * (VEC ? 4 : 1);
  if (s >= count) return;
  if (VEC)
    *reinterpret_cast<f32x4*>(dst + s) = *reinterpret_cast<const f32x4*>(src + s);
  else
    dst[s] = src[s];
}

}  // namespace

extern "C" {

int ov_frame_hops_windows_f32(const float* wave, int64_t n_samples, const int64_t* first_frame, int W, int hop, int pad,
                              int U, int ld, float* hops, ov_stream_t stream) {
  if (!wave || !first_frame || !hops || n_samples <= 0 || W <= 0 || W > 65535 || hop <= 0 || hop > 1024 || pad < 0 ||
      pad >= n_samples || U <= 0 || ld < U)
    return OV_E_BADARG;
  if (ld % 4 != 0 || (reinterpret_cast<uintptr_t>(hops) & 15)) return OV_E_ALIGN;
  dim3 grid((U + 63) / 64, (hop + 63) / 64, W);
  hipLaunchKernelGGL(frame_hops_windows_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), wave, n_samples,
                     first_frame, hop, pad, U, ld, hops);
  return hipGetLastError() == hipSuccess ? OV_OK : OV_E_LAUNCH;
}

int ov_frame_hops_multi_f32(const float* pool, int64_t pool_len, const int64_t* records, int W, int hop, int pad, int U,
                            int ld, float* hops, ov_stream_t stream) {
  if (!pool || !records || !hops || pool_len <= 0 || W <= 0 || W > 65535 || hop <= 0 || hop > 1024 || pad < 0 ||
      U <= 0 || ld < U)
    return OV_E_BADARG;
  if (ld % 4 != 0 || (reinterpret_cast<uintptr_t>(hops) & 15)) return OV_E_ALIGN;
  dim3 grid((U + 63) / 64, (hop + 63) / 64, W);
  hipLaunchKernelGGL(frame_hops_multi_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), pool, pool_len,
                     records, hop, pad, U, ld, hops);
  return hipGetLastError() == hipSuccess ? OV_OK : OV_E_LAUNCH;
}

int ov_stitch_window_cores_f32(const float* o_hat, const int64_t* windows, int W, int Tw, int spf, float* out,
                               int64_t out_len, int64_t out_frame0, ov_stream_t stream) {
  if (!o_hat || !windows || !out || W <= 0 || W > 65535 || Tw <= 0 || spf <= 0 || out_len <= 0 || out_frame0 < 0)
    return OV_E_BADARG;
  const int64_t per_window = (int64_t)Tw * spf;
  const bool vec = spf % 4 == 0 && !(reinterpret_cast<uintptr_t>(o_hat) & 15) && !(reinterpret_cast<uintptr_t>(out) & 15);
  const int64_t blocks = (per_window / (vec ? 4 : 1) + 255) / 256;
  if (blocks > INT32_MAX) return OV_E_BADARG;
  dim3 grid((unsigned)blocks, W);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (vec)
    hipLaunchKernelGGL(stitch_window_cores_kernel<true>, grid, dim3(256), 0, st, o_hat, windows, Tw, spf, out, out_len,
                       out_frame0);
  else
    hipLaunchKernelGGL(stitch_window_cores_kernel<false>, grid, dim3(256), 0, st, o_hat, windows, Tw, spf, out, out_len,
                       out_frame0);
  return hipGetLastError() == hipSuccess ? OV_OK : OV_E_LAUNCH;
}

}  // extern "C"
