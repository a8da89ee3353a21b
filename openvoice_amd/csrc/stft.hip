// General linear-magnitude STFT and log-mel projection (openvoice_amd/mel_processing.py: stft_magnitude, spec_to_mel_torch,
// mel_spectrogram_torch), replacing the reference's openvoice/mel_processing.py:40-75 (spectrogram_torch), :122-133
// (spec_to_mel_torch) and :136-183 (mel_spectrogram_torch) at any n_fft / hop / win / center, not only 1024 / 256 / 1024.
// Both are GEMMs on the fp32 matrix pipe (v_mfma_f32_32x32x2_f32: lane l holds A[row l & 31][k = l >> 5] and
// B[k = l >> 5][col l & 31]; C/D col = l & 31, row = (r & 3) + 8 (r >> 2) + 4 (l >> 5)) with the frames on the N side.
//
// ov_stft_mag_f32: out[b][f][t] = sqrt(re^2 + im^2 + 1e-6), (re, im)[f][t] = sum_n W(re, im)[f][n] * ypad[t * hop + n].
//   * W = zero-padded periodic Hann * (cos, -sin), built by the host in float64, rounded once to fp32 and packed in
//     A-fragment order: record ((bt * 2 + c) * G + g), lane l, element u = W_c[32 bt + (l & 31)][8 g + 2 u + (l >> 5)],
//     G = ceil(n_fft / 8); rows >= bins and k >= n_fft are zero.  A wave reads one 16-byte vector per record: a whole
//     1 KiB request, prefetched one record ahead of the eight MFMAs that use it.
//   * ypad is never materialised: the sample at padded index i is y[reflect_N(reflect_N1(i - pad2) - pad1)], the two
//     reflections of the definition in sequence (pad1 = (n_fft - hop) / 2 always, pad2 = n_fft / 2 when centred,
//     N1 = N + 2 pad1).  Near the ends this differs from one reflection by pad1 + pad2.
//   * A workgroup owns kTileT = 32 frames and up to four 32-bin tiles (one per wave, re and im accumulators paired in the
//     wave).  Per fill it stages k in [k0, k0 + 256) of its frames as ROWS, bs[frame][k] with a row stride of 257
//     floats.  The B operand of k-step s is bs[l & 31][2 s + (l >> 5)]: 32 lanes of a half read 32 consecutive banks
//     whatever the hop -- a hop that is a multiple of 32 would put the 32 frames of a contiguous span on ONE bank -- and
//     the tile costs 32.9 KB for every shape, where the span (frames - 1) * hop + n_fft is 256 KiB at hop = n_fft = 2048
//     and does not fit.  What the rows cost is n_fft / hop reads of a sample from L2 instead of one.
//   * Frames >= T and k >= n_fft are staged as zeros and never stored; the padded columns [T, ld) are stored as zeros.
//
// ov_mel_log_f32: out[b][m][t] = logf(max(sum_f mel[m][f] * spec[b][f][t], clip)).  One workgroup owns 32 frames and
//   every mel row (<= 8 tiles of 32, two per wave), stages mel[.., k0 .. k0 + 32) as rows of 33 floats and
//   spec[k0 .. k0 + 32)[32 frames] as it lies in memory; rows >= num_mels, k >= bins and frames >= T are zeros.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "openvoice_amd.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kTileT = 32;               // frames per workgroup: the N of one MFMA
constexpr int kThreads = 256;            // four waves
constexpr int kStftKC = 256;             // k per LDS fill of the STFT
constexpr int kStftLD = kStftKC + 1;     // odd row stride: conflict-free B reads for every hop
constexpr int kMelKC = 32;
constexpr int kMelLD = kMelKC + 1;
constexpr int kMaxMels = 256;
constexpr int kMaxBins = 1025;

__device__ inline int reflect(int j, int n) {     // index j of a reflect-padded signal of n samples, |overhang| < n
  j = j < 0 ? -j : j;
  return j >= n ? 2 * (n - 1) - j : j;
}

__global__ __launch_bounds__(kThreads) void stft_mag_kernel(const float* __restrict__ y, const float4* __restrict__ wpack,
                                                            float* __restrict__ out, int N, int n_fft, int hop, int pad1,
                                                            int pad2, int T, int ld, int bins, int G) {
  __shared__ float bs[kTileT * kStftLD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, col = lane & 31;
  const int t0 = blockIdx.x * kTileT;
  const int bt = blockIdx.y * 4 + wave;                         // this wave's 32-bin tile
  const bool active = bt * 32 < bins;                           // wave-uniform
  const float* yb = y + (int64_t)blockIdx.z * N;
  const int N1 = N + 2 * pad1;
  const float4* wre = wpack + ((int64_t)(bt * 2) * G) * 64 + lane;
  const float4* wim = wre + (int64_t)G * 64;
  f32x16 are = {}, aim = {};
  float4 nre = {0.f, 0.f, 0.f, 0.f}, nim = nre;
  if (active) { nre = wre[0]; nim = wim[0]; }
  for (int k0 = 0; k0 < 8 * G; k0 += kStftKC) {
    const int kc = min(kStftKC, 8 * G - k0);
    __syncthreads();                                            // the previous fill has been read
    if (tid < kc) {
      const int n = k0 + tid;
      for (int r = 0; r < kTileT; ++r) {
        const int t = t0 + r;
        float v = 0.f;
        if (t < T && n < n_fft) {
          int j = t * hop + n;                                  // < N + 2 pad1 + 2 pad2 < 2^31 (checked by the host)
          if (pad2) j = reflect(j - pad2, N1);
          j = reflect(j - pad1, N);
          j = min(max(j, 0), N - 1);
          v = yb[j];
        }
        bs[r * kStftLD + tid] = v;
      }
    }
    __syncthreads();
    if (active) {
      const float* bp = bs + col * kStftLD + half;
      for (int g = 0; g < kc / 8; ++g) {
        const float4 cre = nre, cim = nim;
        const int gn = min(k0 / 8 + g + 1, G - 1);              // one record ahead (the last one is read twice)
        nre = wre[(int64_t)gn * 64];
        nim = wim[(int64_t)gn * 64];
        const float b0 = bp[8 * g], b1 = bp[8 * g + 2], b2 = bp[8 * g + 4], b3 = bp[8 * g + 6];
        are = __builtin_amdgcn_mfma_f32_32x32x2f32(cre.x, b0, are, 0, 0, 0);
        aim = __builtin_amdgcn_mfma_f32_32x32x2f32(cim.x, b0, aim, 0, 0, 0);
        are = __builtin_amdgcn_mfma_f32_32x32x2f32(cre.y, b1, are, 0, 0, 0);
        aim = __builtin_amdgcn_mfma_f32_32x32x2f32(cim.y, b1, aim, 0, 0, 0);
        are = __builtin_amdgcn_mfma_f32_32x32x2f32(cre.z, b2, are, 0, 0, 0);
        aim = __builtin_amdgcn_mfma_f32_32x32x2f32(cim.z, b2, aim, 0, 0, 0);
        are = __builtin_amdgcn_mfma_f32_32x32x2f32(cre.w, b3, are, 0, 0, 0);
        aim = __builtin_amdgcn_mfma_f32_32x32x2f32(cim.w, b3, aim, 0, 0, 0);
      }
    }
  }
  if (!active) return;
  const int t = t0 + col;
  if (t >= ld) return;
  float* ob = out + (int64_t)blockIdx.z * bins * ld + t;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int f = bt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
    if (f < bins) ob[(int64_t)f * ld] = t < T ? sqrtf(are[r] * are[r] + aim[r] * aim[r] + 1e-6f) : 0.f;
  }
}

__global__ __launch_bounds__(kThreads) void mel_log_kernel(const float* __restrict__ spec, const float* __restrict__ mel,
                                                           float* __restrict__ out, int num_mels, int bins, int T,
                                                           int spec_ld, int64_t spec_bstride, int out_ld, float clip) {
  __shared__ float as[kMaxMels * kMelLD];
  __shared__ float bs[kMelKC * kTileT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, col = lane & 31;
  const int t0 = blockIdx.x * kTileT;
  const int ntiles = (num_mels + 31) / 32;
  const bool on0 = wave < ntiles, on1 = wave + 4 < ntiles;      // wave-uniform
  const float* sb = spec + (int64_t)blockIdx.z * spec_bstride;
  f32x16 acc0 = {}, acc1 = {};
  for (int k0 = 0; k0 < bins; k0 += kMelKC) {
    __syncthreads();
    for (int i = tid; i < ntiles * 32 * kMelKC; i += kThreads) {
      const int r = i >> 5, k = i & 31;
      as[r * kMelLD + k] = (r < num_mels && k0 + k < bins) ? mel[(int64_t)r * bins + k0 + k] : 0.f;
    }
    for (int i = tid; i < kMelKC * kTileT; i += kThreads) {
      const int k = i >> 5, t = t0 + (i & 31);
      bs[i] = (k0 + k < bins && t < T) ? sb[(int64_t)(k0 + k) * spec_ld + t] : 0.f;
    }
    __syncthreads();
    const float* a0 = as + (wave * 32 + col) * kMelLD + half;
    const float* a1 = a0 + 4 * 32 * kMelLD;
    const float* bp = bs + half * kTileT + col;
#pragma unroll 4
    for (int s = 0; s < kMelKC / 2; ++s) {
      const float b = bp[2 * s * kTileT];
      if (on0) acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[2 * s], b, acc0, 0, 0, 0);
      if (on1) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[2 * s], b, acc1, 0, 0, 0);
    }
  }
  const int t = t0 + col;
  if (t >= out_ld) return;
  float* ob = out + (int64_t)blockIdx.z * num_mels * out_ld + t;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
    if (on0 && m < num_mels) ob[(int64_t)m * out_ld] = t < T ? logf(fmaxf(acc0[r], clip)) : 0.f;
    if (on1 && m + 128 < num_mels) ob[(int64_t)(m + 128) * out_ld] = t < T ? logf(fmaxf(acc1[r], clip)) : 0.f;
  }
}

// Frames of the definition, or a negative OV_E_* code when the shape is outside the supported range.
int64_t stft_frames(int64_t N, int n_fft, int hop, int win, int center) {
  if (n_fft < 16 || n_fft > 2048 || (n_fft & 1) || hop < 1 || hop > n_fft || win < 1 || win > n_fft) return OV_E_UNSUPPORTED;
  if (N < 1 || N > ((int64_t)1 << 30)) return OV_E_BADARG;
  const int64_t pad1 = (n_fft - hop) / 2, pad2 = center ? n_fft / 2 : 0;
  const int64_t N1 = N + 2 * pad1, Np = N1 + 2 * pad2;
  if (N <= pad1 || N1 <= pad2 || Np < n_fft) return OV_E_BADARG;   // a reflection needs more samples than it pads
  return (Np - n_fft) / hop + 1;
}

}  // namespace

extern "C" {

int ov_stft_tile_frames(void) { return kTileT; }

int ov_stft_mag_f32(const float* y, const float* wpack, float* out, int B, int N, int n_fft, int hop, int win, int center,
                    int ld, ov_stream_t stream) {
  if (!y || !wpack || !out || B < 1 || B > 65535) return OV_E_BADARG;
  const int64_t T = stft_frames(N, n_fft, hop, win, center);
  if (T < 0) return (int)T;
  if (ld != (T + 3) / 4 * 4) return OV_E_BADARG;
  if ((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(out)) & 3) return OV_E_ALIGN;
  if (reinterpret_cast<uintptr_t>(wpack) & 15) return OV_E_ALIGN;
  const int bins = n_fft / 2 + 1, tiles = (bins + 31) / 32, G = (n_fft + 7) / 8;
  const dim3 grid((unsigned)((T + kTileT - 1) / kTileT), (unsigned)((tiles + 3) / 4), (unsigned)B);
  hipLaunchKernelGGL(stft_mag_kernel, grid, dim3(kThreads), 0, static_cast<hipStream_t>(stream), y,
                     reinterpret_cast<const float4*>(wpack), out, N, n_fft, hop, (n_fft - hop) / 2, center ? n_fft / 2 : 0,
                     (int)T, ld, bins, G);
  return hipGetLastError() == hipSuccess ? OV_OK : OV_E_LAUNCH;
}

int ov_mel_log_f32(const float* spec, const float* mel, float* out, int B, int num_mels, int bins, int T, int spec_ld,
                   int64_t spec_bstride, int out_ld, float clip, ov_stream_t stream) {
  if (!spec || !mel || !out || B < 1 || B > 65535 || T < 1 || num_mels < 1 || bins < 1 || !(clip > 0.f)) return OV_E_BADARG;
  if (num_mels > kMaxMels || bins > kMaxBins) return OV_E_UNSUPPORTED;
  if (spec_ld < T || out_ld != (T + 3) / 4 * 4) return OV_E_BADARG;
  if (B > 1 && spec_bstride < (int64_t)(bins - 1) * spec_ld + T) return OV_E_BADARG;
  if ((reinterpret_cast<uintptr_t>(spec) | reinterpret_cast<uintptr_t>(mel) | reinterpret_cast<uintptr_t>(out)) & 3)
    return OV_E_ALIGN;
  const dim3 grid((unsigned)((T + kTileT - 1) / kTileT), 1u, (unsigned)B);
  hipLaunchKernelGGL(mel_log_kernel, grid, dim3(kThreads), 0, static_cast<hipStream_t>(stream), spec, mel, out, num_mels, bins,
                     T, spec_ld, spec_bstride, out_ld, clip);
  return hipGetLastError() == hipSuccess ? OV_OK : OV_E_LAUNCH;
}

}  // extern "C"
