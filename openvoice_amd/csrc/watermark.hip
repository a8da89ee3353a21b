// The project's own keyed watermark (openvoice_amd/watermark.py): informed spread spectrum in the time domain.  A window
// x[0 .. L) carries 32 bits; bit j owns the samples S_j = {i : i % 32 == j}, so every bit is spread over the whole window.
//   chips       c[i] = +1 / -1 for a set / clear bit (i % 32) of word (i % 128) / 32 of
//               Philox4x32-10(counter = (i / 128, 0, 0, 3), key = (key & 0xffffffff, key >> 32))
//   projection  p_j = (1 / |S_j|) sum_{i in S_j} c[i] x[i]
//   level       a = max(strength * sqrt(mean x^2), floor)
//   embed       d_j = b_j max(a - b_j p_j, 0)  (b_j = +1 / -1 for payload bit 1 / 0),   y[i] = x[i] + d_{i % 32} c[i]
//   read        q_j = p_j(y), level a_y of y; the host turns them into scores 0.5 + 0.5 tanh(q_j / a_y)
// Record-driven like ov_carry_rows_f32: `records` is a DEVICE int64 [W][4] of (src_off, dst_off, L, bits), one 256-thread
// workgroup per window.  A record the host could not check is checked here; a bad one writes nothing.
//
// Thread t takes the samples i = t + 256 k, k ascending -- one coalesced dword per lane and step whatever the window's
// offset, and, since 256 % 32 == 0, samples of bit t % 32 only.  It keeps one partial sum for p and one for the energy;
// the eight partials of a bit and the 256 of the energy are then added in a fixed order through LDS.  So the bits a
// window gets depend on its samples, payload, key, strength and floor and on nothing else: not on W, on its place in
// the launch or on the alignment of its offsets.  (A 16-byte path would hand a thread the samples of four bits and add
// them in another order than the dword path next to it; a wave's dword access is a whole 256-byte request already.)
// Two passes over the window, the second one (embed only) reads x again: 64 KB per window, from L2.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "openvoice_amd.h"
#include "philox_normal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kBits = 32;
constexpr int64_t kMinL = 32 * 16;                  // every bit owns at least 16 samples
constexpr int64_t kMaxL = (int64_t)1 << 31;         // the Philox block i / 128 stays one 32-bit word with room to spare
constexpr int64_t kMaxOff = (int64_t)1 << 61;
constexpr uint32_t kPurposeWatermark = 3;           // noise.py: purposes 0 .. 2 are the Gaussian draws

// Calls f(i, negative) for this thread's samples i = t + 256 k < L, k ascending; negative: c[i] = -1.  Chips are made in
// registers, one Philox block = 128 signs: a 256-sample step k needs the blocks 2 k and 2 k + 1, threads 0 .. 127 the
// first and 128 .. 255 the second, and a wave reads two of a block's four words.  Lane l of a wave therefore computes
// the block of step kc + l, and the 64 steps kc .. kc + 63 each fetch their two words from that lane (v_readlane: the
// step is wave-uniform).  Every lane runs every step; only the call of f is predicated.
template <typename F> __device__ inline void for_chips(int64_t L, uint32_t k0, uint32_t k1, F f) {
  const int t = threadIdx.x, lane = t & 63;
  const int64_t steps = (L + kThreads - 1) / kThreads;
  const uint32_t half = (uint32_t)(t >> 7);
  const bool upper_words = (t & 64) != 0;            // wave-uniform: this wave reads words 2, 3 (else 0, 1)
  for (int64_t kc = 0; kc < steps; kc += 64) {
    uint32_t r[4];
    ovn::philox4x32_10((uint32_t)(2 * (kc + lane)) + half, 0u, 0u, kPurposeWatermark, k0, k1, r);
    const int w_lo = (int)(upper_words ? r[2] : r[0]), w_hi = (int)(upper_words ? r[3] : r[1]);
    const int n = (int)(steps - kc < 64 ? steps - kc : 64);
    for (int kk = 0; kk < n; ++kk) {
      const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane(w_lo, kk), hi = (uint32_t)__builtin_amdgcn_readlane(w_hi, kk);
      const uint32_t word = (lane & 32) ? hi : lo;
      const bool negative = ((word >> (lane & 31)) & 1u) == 0u;
      const int64_t i = (kc + kk) * kThreads + t;
      if (i < L) f(i, negative);
    }
  }
}

struct Stats {
  float p;        // threads 0 .. 31: the projection of bit t
  float level;    // every thread: a
};

// Pass 1 and the fixed-order reduction.  sp / se: 256 floats of LDS each.
__device__ inline Stats window_stats(const float* x, int64_t L, uint32_t k0, uint32_t k1, float strength,
                                     float floor_level, float* sp, float* se) {
  const int t = threadIdx.x;
  float p = 0.f, e = 0.f;
  for_chips(L, k0, k1, [&](int64_t i, bool negative) {
    const float v = x[i];
    p += negative ? -v : v;
    e = __builtin_fmaf(v, v, e);
  });
  sp[t] = p;
  se[t] = e;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (t < s) se[t] += se[t + s];
    __syncthreads();
  }
  Stats st;
  st.level = fmaxf(strength * sqrtf(se[0] / (float)L), floor_level);
  st.p = 0.f;
  if (t < kBits) {
    const float sum = ((sp[t] + sp[t + 32]) + (sp[t + 64] + sp[t + 96])) + ((sp[t + 128] + sp[t + 160]) + (sp[t + 192] + sp[t + 224]));
    st.p = sum / (float)((L - t + kBits - 1) / kBits);            // |S_t|
  }
  return st;
}

__device__ inline bool span_ok(int64_t off, int64_t L, int64_t elems) { return off >= 0 && off <= kMaxOff && L <= elems && off <= elems - L; }

__global__ __launch_bounds__(kThreads) void wm_embed_kernel(const float* src, int64_t src_elems, float* dst,
                                                            int64_t dst_elems, const int64_t* __restrict__ records,
                                                            uint32_t k0, uint32_t k1, float strength, float floor_level) {
  __shared__ float sp[kThreads], se[kThreads], sd[kBits];
  const int64_t* rec = records + 4 * (int64_t)blockIdx.x;
  const int64_t so = rec[0], d_o = rec[1], L = rec[2], bits = rec[3];
  if (L < kMinL || L > kMaxL || !span_ok(so, L, src_elems) || !span_ok(d_o, L, dst_elems)) return;     // (block-uniform)
  const float* x = src + so;            // (src and dst carry no __restrict__: a window may be marked in place)
  const Stats st = window_stats(x, L, k0, k1, strength, floor_level, sp, se);
  const int t = threadIdx.x;
  if (t < kBits) {
    const float b = ((uint64_t)bits >> t) & 1u ? 1.f : -1.f;
    sd[t] = b * fmaxf(st.level - b * st.p, 0.f);
  }
  __syncthreads();
  const float d = sd[t & (kBits - 1)];
  float* y = dst + d_o;
  for_chips(L, k0, k1, [&](int64_t i, bool negative) {
    const float v = x[i];
    y[i] = negative ? v - d : v + d;
  });
}

__global__ __launch_bounds__(kThreads) void wm_detect_kernel(const float* __restrict__ src, int64_t src_elems,
                                                             const int64_t* __restrict__ records, uint32_t k0, uint32_t k1,
                                                             float strength, float floor_level, float* __restrict__ q_out,
                                                             float* __restrict__ level_out) {
  __shared__ float sp[kThreads], se[kThreads];
  const int64_t* rec = records + 4 * (int64_t)blockIdx.x;
  const int64_t so = rec[0], L = rec[2];
  if (L < kMinL || L > kMaxL || !span_ok(so, L, src_elems)) return;
  const Stats st = window_stats(src + so, L, k0, k1, strength, floor_level, sp, se);
  const int t = threadIdx.x;
  if (t < kBits) q_out[(int64_t)blockIdx.x * kBits + t] = st.p;
  if (t == 0) level_out[blockIdx.x] = st.level;
}

bool launch_args_ok(const void* src, int64_t src_elems, const void* records, int W, int64_t key, float strength,
                    float floor_level) {
  // (a NaN fails every comparison)
  return src && records && src_elems > 0 && W >= 1 && W <= 65535 && key >= 0 && strength >= 0.f && strength <= 1.f &&
         floor_level > 0.f && floor_level <= 1.f;
}

}  // namespace

extern "C" {

int ov_wm_embed_windows_f32(const float* src, int64_t src_elems, float* dst, int64_t dst_elems, const int64_t* records,
                            int W, int64_t key, float strength, float floor_level, ov_stream_t stream) {
  if (!launch_args_ok(src, src_elems, records, W, key, strength, floor_level) || !dst || dst_elems <= 0) return OV_E_BADARG;
  if ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 3) return OV_E_ALIGN;
  hipLaunchKernelGGL(wm_embed_kernel, dim3((unsigned)W), dim3(kThreads), 0, static_cast<hipStream_t>(stream), src, src_elems,
                     dst, dst_elems, records, (uint32_t)key, (uint32_t)((uint64_t)key >> 32), strength, floor_level);
  return hipGetLastError() == hipSuccess ? OV_OK : OV_E_LAUNCH;
}

int ov_wm_detect_windows_f32(const float* src, int64_t src_elems, const int64_t* records, int W, int64_t key, float strength,
                             float floor_level, float* q_out, float* level_out, ov_stream_t stream) {
  if (!launch_args_ok(src, src_elems, records, W, key, strength, floor_level) || !q_out || !level_out) return OV_E_BADARG;
  if ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(q_out) | reinterpret_cast<uintptr_t>(level_out)) & 3)
    return OV_E_ALIGN;
  hipLaunchKernelGGL(wm_detect_kernel, dim3((unsigned)W), dim3(kThreads), 0, static_cast<hipStream_t>(stream), src, src_elems,
                     records, (uint32_t)key, (uint32_t)((uint64_t)key >> 32), strength, floor_level, q_out, level_out);
  return hipGetLastError() == hipSuccess ? OV_OK : OV_E_LAUNCH;
}

}  // extern "C"
