// Ragged twins of the ReferenceEncoder kernels of ref_enc.hip (reference: openvoice/models.py:339-359): the same
// LayerNorm over frequency, 3x3 stride-2 conv + ReLU and GRU recurrence for a batch whose items have DIFFERENT numbers
// of frames.  Layout as in ref_enc.hip, [N][C][F][ld] with time contiguous; `ld` is the row stride of the whole batch
// (the longest item's length or more) and lens[n] (device int32) the frames item n really has.
//
// The contract of each kernel is stated against its dense twin: over an item's own columns it performs the twin's
// floating-point operations in the twin's order, so item n of a ragged batch gets, bit for bit, what the dense kernel
// gives for that item alone -- the conv's zero padding sits at the ITEM's end, and the GRU stops after the item's last
// step.  Every kernel writes 0 to the columns between an item's end and the row stride, so no later stage reads memory
// that nothing wrote.  A length outside [0, ld] is clamped in the kernel (the host wrapper refuses it first): a bad
// table cannot make a kernel read or write outside the rows it was given.
//
// Plain VALU kernels like their twins (1.09 GFLOP per 10 s clip): lanes along t for coalesced rows, weight indices
// wave-uniform so the compiler fetches them with scalar loads.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "openvoice_amd.h"

namespace ovk {

__device__ __forceinline__ int clamp_len(int len, int ld) { return len < 0 ? 0 : (len > ld ? ld : len); }

// layernorm_freq_kernel for columns t < lens[n] (the same s += loop, the same fmaf(d, d, v) loop, the same final
// expression); columns lens[n] <= t < ld are written as 0 without reading x there.
__global__ __launch_bounds__(256) void layernorm_freq_ragged_kernel(const float* __restrict__ x,
                                                                    const float* __restrict__ gamma,
                                                                    const float* __restrict__ beta,
                                                                    const int32_t* __restrict__ lens,
                                                                    float* __restrict__ y, int F, int ld, float eps) {
  const int n = blockIdx.y;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= ld) return;
  const int T = clamp_len(lens[n], ld);
  const float* xr = x + (int64_t)n * F * ld + t;
  float* yr = y + (int64_t)n * F * ld + t;
  if (t >= T) {
    for (int f = 0; f < F; ++f) yr[(int64_t)f * ld] = 0.f;
    return;
  }
  float s = 0.f;
  for (int f = 0; f < F; ++f) s += xr[(int64_t)f * ld];
  const float mean = s / F;
  float v = 0.f;
  for (int f = 0; f < F; ++f) {
    const float d = xr[(int64_t)f * ld] - mean;
    v = fmaf(d, d, v);
  }
  const float rstd = 1.f / sqrtf(v / F + eps);
  for (int f = 0; f < F; ++f) yr[(int64_t)f * ld] = (xr[(int64_t)f * ld] - mean) * rstd * gamma[f] + beta[f];
}

// conv2d_s2_relu_kernel<COB> with the item's own Ti = lens_in[n]: bias first, ci ascending, taps k = 0..8, fmaf.  A tap
// is valid iff 0 <= ti < Ti and 0 <= fi < Fi; rows are ld_in / ld_out floats apart.  One thread = one (fo, to) of the
// PADDED output plane x COB channels (p = fo * ld_out + to, so lanes still run along t); a thread at or beyond the item's
// (Ti - 1) / 2 + 1 output columns stores 0 and loads nothing.
template <int COB>
__global__ __launch_bounds__(256) void conv2d_s2_relu_ragged_kernel(const float* __restrict__ x,
                                                                    const float* __restrict__ w,
                                                                    const float* __restrict__ bias,
                                                                    const int32_t* __restrict__ lens_in,
                                                                    float* __restrict__ y, int Cin, int Cout, int Fi,
                                                                    int ld_in, int Fo, int ld_out) {
  const int n = blockIdx.z;
  const int co0 = blockIdx.y * COB;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= Fo * ld_out) return;
  const int fo = p / ld_out, to = p - fo * ld_out;
  const int Ti = clamp_len(lens_in[n], ld_in);
  const int To = Ti > 0 ? (Ti - 1) / 2 + 1 : 0;
  float* yn = y + ((int64_t)n * Cout + co0) * Fo * ld_out + p;
  if (to >= To) {
#pragma unroll
    for (int c = 0; c < COB; ++c) yn[(int64_t)c * Fo * ld_out] = 0.f;
    return;
  }
  int64_t off[9];
  bool ok[9];
#pragma unroll
  for (int kh = 0; kh < 3; ++kh)
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const int ti = 2 * to + kh - 1, fi = 2 * fo + kw - 1;
      ok[kh * 3 + kw] = ti >= 0 && ti < Ti && fi >= 0 && fi < Fi;
      off[kh * 3 + kw] = (int64_t)fi * ld_in + ti;
    }
  float acc[COB];
#pragma unroll
  for (int c = 0; c < COB; ++c) acc[c] = bias[co0 + c];
  const float* xn = x + (int64_t)n * Cin * Fi * ld_in;
  for (int ci = 0; ci < Cin; ++ci) {
    const float* xc = xn + (int64_t)ci * Fi * ld_in;
    float v[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) v[k] = ok[k] ? xc[off[k]] : 0.f;
    const float* wc = w + ((int64_t)co0 * Cin + ci) * 9;
#pragma unroll
    for (int c = 0; c < COB; ++c)
#pragma unroll
      for (int k = 0; k < 9; ++k) acc[c] = fmaf(wc[(int64_t)c * Cin * 9 + k], v[k], acc[c]);
  }
#pragma unroll
  for (int c = 0; c < COB; ++c) yn[(int64_t)c * Fo * ld_out] = fmaxf(acc[c], 0.f);
}

// gru_kernel<H> with the loop bound lens[n] and rows ld floats apart.  The bound is read once per workgroup and is the
// same for all of its threads, so both __syncthreads() of a step are reached by every thread: no lane leaves the loop
// early.
template <int H>
__global__ __launch_bounds__(3 * H) void gru_ragged_kernel(const float* __restrict__ gi,
                                                           const float* __restrict__ whh_t,
                                                           const float* __restrict__ bhh,
                                                           const int32_t* __restrict__ lens,
                                                           float* __restrict__ h_out, int ld) {
  __shared__ float h[H];
  __shared__ float gh[3 * H];
  const int n = blockIdx.x, j = threadIdx.x;
  if (j < H) h[j] = 0.f;
  __syncthreads();
  const int T = clamp_len(lens[n], ld);
  const float* gin = gi + (int64_t)n * 3 * H * ld;
  const float bj = bhh[j];
  for (int t = 0; t < T; ++t) {
    float acc = bj;
#pragma unroll 8
    for (int k = 0; k < H; ++k) acc = fmaf(whh_t[k * 3 * H + j], h[k], acc);
    gh[j] = acc;
    __syncthreads();
    if (j < H) {
      const float r = 1.f / (1.f + expf(-(gin[(int64_t)j * ld + t] + gh[j])));
      const float z = 1.f / (1.f + expf(-(gin[(int64_t)(H + j) * ld + t] + gh[H + j])));
      const float c = tanhf(gin[(int64_t)(2 * H + j) * ld + t] + r * gh[2 * H + j]);
      h[j] = (1.f - z) * c + z * h[j];
    }
    __syncthreads();
  }
  if (j < H) h_out[(int64_t)n * H + j] = h[j];
}

}  // namespace ovk

using namespace ovk;

extern "C" {

int ov_layernorm_freq_ragged_f32(const float* x, const float* gamma, const float* beta, const int32_t* lens, float* y,
                                 int N, int F, int ld, float eps, ov_stream_t stream) {
  if (!x || !gamma || !beta || !lens || !y || N <= 0 || F <= 0 || ld <= 0 || N > 65535) return OV_E_BADARG;
  dim3 grid((ld + 255) / 256, N);
  hipLaunchKernelGGL(layernorm_freq_ragged_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), x, gamma,
                     beta, lens, y, F, ld, eps);
  return hipGetLastError() == hipSuccess ? OV_OK : OV_E_LAUNCH;
}

int ov_conv2d_s2_relu_ragged_f32(const float* x, const float* w, const float* bias, const int32_t* lens_in, float* y,
                                 int N, int Cin, int Cout, int Fi, int ld_in, int ld_out, ov_stream_t stream) {
  if (!x || !w || !bias || !lens_in || !y || N <= 0 || Cin <= 0 || Cout <= 0 || Fi <= 0 || ld_in <= 0 || N > 65535)
    return OV_E_BADARG;
  // the longest item (ld_in frames) has (ld_in - 1) / 2 + 1 output columns: a narrower output row cannot hold it
  if (ld_out < (ld_in - 1) / 2 + 1) return OV_E_BADARG;
  if (Cout % 16 != 0) return OV_E_UNSUPPORTED;
  const int Fo = (Fi - 1) / 2 + 1;
  if ((int64_t)Fo * ld_out > INT32_MAX) return OV_E_BADARG;
  dim3 grid((Fo * ld_out + 255) / 256, Cout / 16, N);
  hipLaunchKernelGGL(conv2d_s2_relu_ragged_kernel<16>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), x, w,
                     bias, lens_in, y, Cin, Cout, Fi, ld_in, Fo, ld_out);
  return hipGetLastError() == hipSuccess ? OV_OK : OV_E_LAUNCH;
}

int ov_gru_ragged_f32(const float* gi, const float* whh_t, const float* bhh, const int32_t* lens, float* h_out, int N,
                      int H, int ld, ov_stream_t stream) {
  if (!gi || !whh_t || !bhh || !lens || !h_out || N <= 0 || ld <= 0 || N > 65535) return OV_E_BADARG;
  if (H != 128) return OV_E_UNSUPPORTED;
  hipLaunchKernelGGL(gru_ragged_kernel<128>, dim3(N), dim3(384), 0, static_cast<hipStream_t>(stream), gi, whh_t, bhh,
                     lens, h_out, ld);
  return hipGetLastError() == hipSuccess ? OV_OK : OV_E_LAUNCH;
}

}  // extern "C"
