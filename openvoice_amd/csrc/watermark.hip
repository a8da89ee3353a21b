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

// Calls f(i, negative) for this thread's samples i = t + 256 k < L, k ascending; negative: c[base + i] = -1.  `base` is the
// chip index of sample 0: 0 for a whole window, a multiple of 32 for a block inside one (so that sample i still belongs
// to bit t % 32).  Chips are made in registers, one Philox block = 128 signs = four 32-sample groups.  In step k a wave
// (threads 64 w .. 64 w + 63) needs the two groups G = base / 32 + 2 w + 8 k and G + 1: words G % 4 and (G + 1) % 4 of
// the blocks G / 4 and (G + 1) / 4, which differ only when G % 4 == 3 (an odd base / 32; wave-uniform).  Lane l of a wave
// therefore computes the block(s) of step kc + l, and the 64 steps kc .. kc + 63 each fetch their two words from that
// lane (v_readlane: the step is wave-uniform).  Every lane runs every step; only the call of f is predicated.
template <typename F> __device__ inline void for_chips(int64_t L, int64_t base, uint32_t k0, uint32_t k1, F f) {
  const int t = threadIdx.x, lane = t & 63;
  const int64_t steps = (L + kThreads - 1) / kThreads;
  const int64_t g0 = base / kBits + 2 * (t >> 6);    // this wave's first group in step 0
  const int word0 = (int)(g0 & 3);                   // wave-uniform
  for (int64_t kc = 0; kc < steps; kc += 64) {
    uint32_t r[4], r2[4] = {0u, 0u, 0u, 0u};
    const uint32_t block = (uint32_t)(g0 / 4 + 2 * (kc + lane));
    ovn::philox4x32_10(block, 0u, 0u, kPurposeWatermark, k0, k1, r);
    if (word0 == 3) ovn::philox4x32_10(block + 1u, 0u, 0u, kPurposeWatermark, k0, k1, r2);
    const int w_lo = (int)(word0 == 0 ? r[0] : word0 == 1 ? r[1] : word0 == 2 ? r[2] : r[3]);
    const int w_hi = (int)(word0 == 0 ? r[1] : word0 == 1 ? r[2] : word0 == 2 ? r[3] : r2[0]);
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
__device__ inline Stats window_stats(const float* x, int64_t L, int64_t base, uint32_t k0, uint32_t k1, float strength,
                                     float floor_level, float* sp, float* se) {
  const int t = threadIdx.x;
  float p = 0.f, e = 0.f;
  for_chips(L, base, k0, k1, [&](int64_t i, bool negative) {
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
  const Stats st = window_stats(x, L, 0, k0, k1, strength, floor_level, sp, se);
  const int t = threadIdx.x;
  if (t < kBits) {
    const float b = ((uint64_t)bits >> t) & 1u ? 1.f : -1.f;
    sd[t] = b * fmaxf(st.level - b * st.p, 0.f);
  }
  __syncthreads();
  const float d = sd[t & (kBits - 1)];
  float* y = dst + d_o;
  for_chips(L, 0, k0, k1, [&](int64_t i, bool negative) {
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
  const Stats st = window_stats(src + so, L, 0, k0, k1, strength, floor_level, sp, se);
  const int t = threadIdx.x;
  if (t < kBits) q_out[(int64_t)blockIdx.x * kBits + t] = st.p;
  if (t == 0) level_out[blockIdx.x] = st.level;
}

// The block-wise form for streams (watermark.py, "streams"): a carrier window of 16 000 samples is cut into blocks of H
// samples, and per window and bit one float R_j >= 0 -- the surplus of the blocks so far -- is carried in a state row:
//   u_j = b_j p_j + R_j,   d_j = b_j max(a_m - u_j, 0),   R_j <- max(u_j - a_m, 0)       (p_j, a_m: of the block alone)
// A record is one run of consecutive blocks of one window of one stream; its workgroup walks the blocks in order with
// R_j in a register of thread j, reads the state row first unless `reset` and writes it last.  A block is reduced by
// window_stats, so with H = 16 000 (R = 0, u = b p exactly) the samples are ov_wm_embed_windows_f32's bit for bit.
constexpr int64_t kWindow = 16000;
constexpr int kBlockFields = 8;                     // (src_off, dst_off, H, blocks, bits, chip_off, state_row, reset)

__device__ inline bool hold_ok(int64_t H) {
  return H == 16000 || H == 8000 || H == 4000 || H == 3200 || H == 1600 || H == 800 || H == 640;
}

__global__ __launch_bounds__(kThreads) void wm_embed_blocks_kernel(const float* src, int64_t src_elems, float* dst,
                                                                   int64_t dst_elems, const int64_t* __restrict__ records,
                                                                   float* state, int64_t state_rows, uint32_t k0,
                                                                   uint32_t k1, float strength, float floor_level) {
  __shared__ float sp[kThreads], se[kThreads], sd[kBits];
  const int64_t* rec = records + kBlockFields * (int64_t)blockIdx.x;
  const int64_t so = rec[0], d_o = rec[1], H = rec[2], blocks = rec[3], bits = rec[4], chip_off = rec[5], row = rec[6],
                reset = rec[7];
  // (block-uniform; hold_ok bounds H, so blocks * H cannot overflow once blocks <= 25)
  if (!hold_ok(H) || blocks < 1 || blocks > kWindow / H || chip_off < 0 || chip_off % H != 0 ||
      chip_off + blocks * H > kWindow || row < 0 || row >= state_rows || (reset != 0 && reset != 1) ||
      !span_ok(so, blocks * H, src_elems) || !span_ok(d_o, blocks * H, dst_elems))
    return;
  const int t = threadIdx.x;
  float* srow = state + row * kBits;
  const float b = ((uint64_t)bits >> (t & (kBits - 1))) & 1u ? 1.f : -1.f;
  float surplus = 0.f;                                // R_t, threads 0 .. 31
  if (t < kBits && !reset) surplus = srow[t];
  for (int64_t m = 0; m < blocks; ++m) {
    const float* x = src + so + m * H;                // (no __restrict__: a block may be marked in place)
    float* y = dst + d_o + m * H;
    const int64_t base = chip_off + m * H;
    const Stats st = window_stats(x, H, base, k0, k1, strength, floor_level, sp, se);
    if (t < kBits) {
      const float u = b * st.p + surplus;
      sd[t] = b * fmaxf(st.level - u, 0.f);
      surplus = fmaxf(u - st.level, 0.f);
    }
    __syncthreads();
    const float d = sd[t & (kBits - 1)];
    for_chips(H, base, k0, k1, [&](int64_t i, bool negative) {
      const float v = x[i];
      y[i] = negative ? v - d : v + d;
    });
    // (the next block's window_stats passes a barrier between this read of sd and the next write of it)
  }
  if (t < kBits) srow[t] = surplus;
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

int ov_wm_embed_blocks_f32(const float* src, int64_t src_elems, float* dst, int64_t dst_elems, const int64_t* records, int R,
                           float* state, int64_t state_rows, int64_t key, float strength, float floor_level,
                           ov_stream_t stream) {
  if (!launch_args_ok(src, src_elems, records, R, key, strength, floor_level) || !dst || dst_elems <= 0 || !state ||
      state_rows <= 0 || state_rows > kMaxOff / kBits)
    return OV_E_BADARG;
  if ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(state)) & 3)
    return OV_E_ALIGN;
  hipLaunchKernelGGL(wm_embed_blocks_kernel, dim3((unsigned)R), dim3(kThreads), 0, static_cast<hipStream_t>(stream), src,
                     src_elems, dst, dst_elems, records, state, state_rows, (uint32_t)key, (uint32_t)((uint64_t)key >> 32),
                     strength, floor_level);
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
