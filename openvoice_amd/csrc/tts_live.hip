// Streaming TTS (openvoice_amd/tts_live.py): the producer of the live cascade.  One record-driven launch gives every
// stream that is ready in a round its next piece of the prior sample z_p, straight into the state row of the stream's
// first unit (the flow in reverse) inside the live arena -- what ov_normal_philox_f32 (noise fill), ov_expand_prior*_f32
// (expansion into a workspace) and ov_carry_rows_f32 (move into the state) do in three launches for a whole utterance.
//
// `records` is a DEVICE int64 [R][13] of
//   (seed, stream, f0, nf, x_len, y_len, m_off, m_ld, logs_off, logs_ld, cum_off, dst_off, dst_ld)
// and for c < C, i < nf, t = f0 + i, j the token with cum[j - 1] <= t < cum[j] (m = logs = 0 when there is none):
//   dst[dst_off + c * dst_ld + i] = m[c][j] + n(seed, stream, purpose 2, c, t) * exp(logs[c][j]) * noise_scale[r]
// with m[c][j] = tok[m_off + c * m_ld + j], logs[c][j] = tok[logs_off + c * logs_ld + j], cum = cum_base + cum_off.
// The noise is philox_normal.h's, the arithmetic prior_expand.h's: each value has the bits ov_normal_philox_f32 followed
// by ov_expand_prior_items_f32 writes to z_p[c][t].  Plain VALU: no LDS, no barrier; nothing outside the pieces is
// written.  A record the host could not check is checked here.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "openvoice_amd.h"
#include "philox_normal.h"
#include "prior_expand.h"

namespace {

using ovn::f32x4;

constexpr int kThreads = 256;
constexpr int kFields = 13;
constexpr int kPurposeTtsZ = 2;                     // noise.py: PURPOSE_TTS_Z
constexpr int kMaxChunksPerRecord = 4096;           // grid.x bound; larger pieces take further passes
constexpr int64_t kDim = int64_t(1) << 31;          // frames, tokens and row strides: cum is int32
constexpr int64_t kOff = int64_t(1) << 61;          // offsets: every sum of products below stays < 2^63

// rows x cols at off with row stride ld inside [0, elems)?  (rows >= 1, cols >= 1, ld >= 0, off >= 0 already known)
__device__ inline bool slab_inside(int64_t off, int64_t rows, int64_t cols, int64_t ld, int64_t elems) {
  if (cols > elems || off > elems - cols) return false;
  return rows == 1 || ld == 0 || (elems - cols - off) / ld >= rows - 1;
}

// The noise kernel's ownership rule: one thread owns one Philox block = four consecutive frames of one channel, lanes
// run along frames, then channels.  The four noise values are computed before the thread knows which of them lie inside
// the piece or how they are stored, and each frame's token is found from (cum, t) alone, so a value depends on nothing
// but (seed, stream, c, t) and the sentence: not on f0's phase, on alignment, on R or on its neighbours.  A block wholly
// inside the piece at a 16-byte aligned destination is one vector store; everything else goes element by element.
// Grid (chunk, record).
__global__ __launch_bounds__(kThreads) void expand_prior_rows_kernel(const int64_t* __restrict__ records, int C,
                                                                     const float* __restrict__ tok, int64_t tok_elems,
                                                                     const int32_t* __restrict__ cum_base,
                                                                     int64_t cum_elems,
                                                                     const float* __restrict__ noise_scale_r,
                                                                     float* __restrict__ dst, int64_t dst_elems) {
  const int64_t* rec = records + kFields * (int64_t)blockIdx.y;
  const int64_t seed = rec[0], strm = rec[1], f0 = rec[2], nf = rec[3], x_len = rec[4], y_len = rec[5];
  const int64_t m_off = rec[6], m_ld = rec[7], logs_off = rec[8], logs_ld = rec[9], cum_off = rec[10];
  const int64_t dst_off = rec[11], dst_ld = rec[12];
  if (seed < 0 || strm < 0 || strm > 0xFFFFFFFFll) return;
  if (nf <= 0 || f0 < 0 || x_len <= 0 || y_len <= 0 || x_len >= kDim || y_len >= kDim) return;
  if (f0 > y_len || nf > y_len - f0) return;                               // the piece leaves the sentence
  if (m_off < 0 || logs_off < 0 || cum_off < 0 || dst_off < 0 || m_ld < 0 || logs_ld < 0 || dst_ld < 0) return;
  if (m_off > kOff || logs_off > kOff || cum_off > kOff || dst_off > kOff || m_ld > kDim || logs_ld > kDim ||
      dst_ld > kDim)
    return;
  if (nf > dst_ld) return;                                                 // rows of the destination would overlap
  if (!slab_inside(dst_off, C, nf, dst_ld, dst_elems)) return;
  if (!slab_inside(m_off, C, x_len, m_ld, tok_elems) || !slab_inside(logs_off, C, x_len, logs_ld, tok_elems)) return;
  if (!slab_inside(cum_off, 1, x_len, 0, cum_elems)) return;
  const int32_t* cb = cum_base + cum_off;
  const float* m_tok = tok + m_off;
  const float* logs_tok = tok + logs_off;
  const int xl = (int)x_len;
  const float noise_scale = noise_scale_r[blockIdx.y];
  const uint64_t q0 = (uint64_t)f0 >> 2;
  const uint64_t nblocks = (((uint64_t)(f0 + nf - 1)) >> 2) - q0 + 1;
  const uint64_t total = nblocks * (uint64_t)C;
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)((uint64_t)seed >> 32);
  for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (uint64_t)gridDim.x * kThreads) {
    const uint64_t c = i / nblocks, q = q0 + (i - c * nblocks);
    const f32x4 n = ovn::normal_block((uint32_t)q, (uint32_t)c, (uint32_t)strm, kPurposeTtsZ, k0, k1);
    const int64_t rel = (int64_t)(q << 2) - f0;                    // piece column of the block's first frame (>= -3)
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float z = 0.f;
      if (rel + e >= 0 && rel + e < nf) {                          // t = f0 + rel + e < y_len < 2^31
        const int j = ovp::token_of_frame(cb, xl, (int)(f0 + rel + e));
        const float m = j >= 0 ? m_tok[(int64_t)c * m_ld + j] : 0.f;
        const float lg = j >= 0 ? logs_tok[(int64_t)c * logs_ld + j] : 0.f;
        z = ovp::prior_sample(m, n[e], lg, noise_scale);
      }
      v[e] = z;
    }
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

extern "C" int ov_expand_prior_rows_f32(const int64_t* records, int R, int C, const float* tok, int64_t tok_elems,
                                        const int32_t* cum, int64_t cum_elems, const float* noise_scale_r, float* dst,
                                        int64_t dst_elems, int64_t max_frames, ov_stream_t stream) {
  if (!records || !tok || !cum || !noise_scale_r || !dst || R <= 0 || R > 65535 || C <= 0 || tok_elems <= 0 ||
      cum_elems <= 0 || dst_elems <= 0 || max_frames < 0)
    return OV_E_BADARG;
  if ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(tok) | reinterpret_cast<uintptr_t>(cum) |
       reinterpret_cast<uintptr_t>(noise_scale_r)) & 3)
    return OV_E_ALIGN;
  // max_frames sizes the grid only: a record with more frames is still written whole, in further passes of its workgroups
  if (max_frames > kDim) max_frames = kDim;
  const int64_t blocks = max_frames / 4 + 2;           // + 2: a piece may cut a Philox block at either end
  int64_t chunks = (blocks * (int64_t)C + kThreads - 1) / kThreads;      // < 2^29 * 2^31: no overflow
  if (chunks > kMaxChunksPerRecord) chunks = kMaxChunksPerRecord;
  hipLaunchKernelGGL(expand_prior_rows_kernel, dim3((unsigned)chunks, R), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), records, C, tok, tok_elems, cum, cum_elems, noise_scale_r, dst,
                     dst_elems);
  return hipGetLastError() == hipSuccess ? OV_OK : OV_E_LAUNCH;
}
