// Per-item synthesis controls of the V1 TTS path: ov_duration_f32 and ov_expand_prior_f32 (csrc/tts.hip) with
// sdp_ratio, length_scale and noise_scale read from [B] device vectors instead of kernel arguments, so that sentences
// of different speeds and noise scales share one launch sequence (reference: openvoice/models.py:474-487 applies the
// three numbers element-wise; nothing in the model ties the items of a batch together).
//
// Contract: with vectors whose every entry is the scalar, each output bit is what the scalar kernel writes; row b of
// a mixed launch is row b of the scalar kernel run with item b's numbers.  The floating-point expressions are therefore
// those of tts.hip, token for token (same contraction); what differs is who computes them: the prefix sum of the
// durations is a workgroup scan instead of one lane's loop (integers: exact in any order), and the expansion maps a
// workgroup to 64 frames x a channel slice, with the alignment rows written as one contiguous span.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "openvoice_amd.h"
#include "prior_expand.h"

namespace ovk {

// One workgroup per utterance.  Tokens go through in chunks of 256: lane-level inclusive scan by shuffles inside each
// of the 4 waves, the waves' totals meet in LDS, the chunk's total carries into the next chunk.  The sums are taken in
// uint32_t: two's-complement addition is associative, so any grouping gives the serial loop's int32 bits.
__global__ __launch_bounds__(256) void duration_items_kernel(const float* __restrict__ z_sdp, int64_t z_bstride,
                                                             float ea_m, float ea_logs, const float* __restrict__ dp,
                                                             int64_t dp_bstride, const float* __restrict__ mask,
                                                             float* __restrict__ logw, int32_t* __restrict__ cum,
                                                             int64_t* __restrict__ y_len, int T, int ld,
                                                             const float* __restrict__ sdp_ratio_b,
                                                             const float* __restrict__ length_scale_b) {
  __shared__ uint32_t wave_total[4];
  const int b = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float sdp_ratio = sdp_ratio_b[b];
  const float length_scale = length_scale_b[b];
  const float* mr = mask + (int64_t)b * ld;
  const float einv = expf(-ea_logs);
  // duration_kernel's loop, statement for statement: hipcc contracts `a * r + d * (1 - r)` differently in the unrolled
  // pairs and in the remainder iteration of this loop, so only the same loop gives every token the same bits.
  for (int t = threadIdx.x; t < T; t += 256) {
    const float mk = mr[t];
    const float ls = (z_sdp[(int64_t)b * z_bstride + t] - ea_m) * einv * mk;
    logw[(int64_t)b * ld + t] = ls * sdp_ratio + dp[(int64_t)b * dp_bstride + t] * (1.f - sdp_ratio);
  }
  __syncthreads();
  uint32_t carry = 0;
  for (int t0 = 0; t0 < T; t0 += 256) {          // T is uniform: every thread takes every barrier
    const int t = t0 + threadIdx.x;               // the token whose logw this thread stored above
    uint32_t run = 0;
    if (t < T) {
      const float w = expf(logw[(int64_t)b * ld + t]) * mr[t] * length_scale;
      run = (uint32_t)(int32_t)ceilf(w);
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t up = __shfl_up(run, off, 64);
      if (lane >= off) run += up;
    }
    if (lane == 63) wave_total[wave] = run;
    __syncthreads();
    uint32_t before = carry, all = carry;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const uint32_t tot = wave_total[w];
      if (w < wave) before += tot;
      all += tot;
    }
    if (t < T) cum[(int64_t)b * ld + t] = (int32_t)(before + run);
    carry = all;
    __syncthreads();                             // wave_total is rewritten by the next chunk
  }
  if (threadIdx.x == 0) {
    const int32_t total = (int32_t)carry;
    y_len[b] = total < 1 ? 1 : total;
  }
}

// Workgroup = 64 consecutive frames of one utterance x the channels c = 4 * blockIdx.z + wave (+ 4 * gridDim.z ...):
// lanes run along the frames, so every z_p / m_p / logs_p / noise access is one contiguous 256-byte row segment, and
// the C-long serial loop of the scalar kernel becomes C / (4 * gridDim.z) iterations per wave.  The 64 alignment rows
// of the tile are contiguous in attn ([B][Ty][Tx]): the z = 0 workgroup writes them as one flat span, a frame's token
// coming from LDS, instead of one Tx-strided row per lane.
__global__ __launch_bounds__(256) void expand_prior_items_kernel(const float* __restrict__ m_tok,
                                                                 const float* __restrict__ logs_tok,
                                                                 int64_t tok_bstride, int ldx,
                                                                 const int32_t* __restrict__ cum,
                                                                 const int64_t* __restrict__ x_len,
                                                                 const int64_t* __restrict__ y_len,
                                                                 const float* __restrict__ noise,
                                                                 int64_t noise_bstride, int ldn,
                                                                 float* __restrict__ z_p, float* __restrict__ m_p,
                                                                 float* __restrict__ logs_p, float* __restrict__ attn,
                                                                 int C, int Tx, int Ty, int ldy,
                                                                 const float* __restrict__ noise_scale_b) {
  __shared__ int token_of[64];
  const int b = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int t0 = blockIdx.x * 64;
  const int t = t0 + lane;
  const float noise_scale = noise_scale_b[b];
  const int32_t* cb = cum + (int64_t)b * ldx;
  const int xl = (int)min((int64_t)Tx, x_len[b]);
  const int j = t < Ty && t < y_len[b] ? ovp::token_of_frame(cb, xl, t) : -1;
  if (attn && blockIdx.z == 0) {        // uniform per workgroup
    if (wave == 0) token_of[lane] = j;
    __syncthreads();
    const int rows = min(64, Ty - t0);
    float* at = attn + ((int64_t)b * Ty + t0) * Tx;
    for (int idx = threadIdx.x; idx < rows * Tx; idx += 256) {
      const int r = idx / Tx, i = idx - r * Tx;
      at[idx] = i == token_of[r] ? 1.f : 0.f;
    }
  }
  if (t >= Ty) return;
  for (int c = 4 * blockIdx.z + wave; c < C; c += 4 * gridDim.z) {
    const int64_t o = ((int64_t)b * C + c) * ldy + t;
    const float m = j >= 0 ? m_tok[(int64_t)b * tok_bstride + (int64_t)c * ldx + j] : 0.f;
    const float lg = j >= 0 ? logs_tok[(int64_t)b * tok_bstride + (int64_t)c * ldx + j] : 0.f;
    if (m_p) m_p[o] = m;
    if (logs_p) logs_p[o] = lg;
    z_p[o] = ovp::prior_sample(m, noise[(int64_t)b * noise_bstride + (int64_t)c * ldn + t], lg, noise_scale);
  }
}

}  // namespace ovk

using namespace ovk;

#define OV_LAUNCH_OK() (hipGetLastError() == hipSuccess ? OV_OK : OV_E_LAUNCH)

extern "C" {

int ov_duration_items_f32(const float* z_sdp, int64_t z_bstride, float ea_m, float ea_logs, const float* dp,
                          int64_t dp_bstride, const float* mask, float* logw, int32_t* cum, int64_t* y_len, int B,
                          int T, int ld, const float* sdp_ratio_b, const float* length_scale_b, ov_stream_t stream) {
  if (!z_sdp || !dp || !mask || !logw || !cum || !y_len || !sdp_ratio_b || !length_scale_b || B <= 0 || T <= 0 ||
      ld < T)
    return OV_E_BADARG;
  hipLaunchKernelGGL(duration_items_kernel, dim3(B), dim3(256), 0, static_cast<hipStream_t>(stream), z_sdp, z_bstride,
                     ea_m, ea_logs, dp, dp_bstride, mask, logw, cum, y_len, T, ld, sdp_ratio_b, length_scale_b);
  return OV_LAUNCH_OK();
}

int ov_expand_prior_items_f32(const float* m_tok, const float* logs_tok, int64_t tok_bstride, int ldx,
                              const int32_t* cum, const int64_t* x_len, const int64_t* y_len, const float* noise,
                              int64_t noise_bstride, int ldn, float* z_p, float* m_p, float* logs_p, float* attn,
                              int B, int C, int Tx, int Ty, int ldy, const float* noise_scale_b, ov_stream_t stream) {
  if (!m_tok || !logs_tok || !cum || !x_len || !y_len || !noise || !z_p || !noise_scale_b || B <= 0 || C <= 0 ||
      Tx <= 0 || Ty <= 0 || ldx < Tx || ldy < Ty || ldn < Ty || B > 65535 || tok_bstride < (int64_t)C * ldx)
    return OV_E_BADARG;
  // 64 alignment rows of Tx floats are addressed with an int inside the kernel
  if ((int64_t)Tx * 64 > INT32_MAX) return OV_E_BADARG;
  const int slices = C >= 32 ? 4 : 1;             // inter_channels = 192: 4 slices of 48 channels, 12 per wave
  dim3 grid((Ty + 63) / 64, B, slices);
  hipLaunchKernelGGL(expand_prior_items_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), m_tok, logs_tok,
                     tok_bstride, ldx, cum, x_len, y_len, noise, noise_bstride, ldn, z_p, m_p, logs_p, attn, C, Tx, Ty,
                     ldy, noise_scale_b);
  return OV_LAUNCH_OK();
}

}  // extern "C"
