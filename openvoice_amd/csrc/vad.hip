// Silence removal ahead of get_se (openvoice_amd/vad.py; the procedure of reference openvoice/se_extractor.py:77-97 with
// a deterministic energy detector in the place of the third-party network): frame energies, the keep / drop decision per
// frame, and the compaction of the kept samples.  All three kernels are record-driven: R recordings lie in one float32
// pool, described by a DEVICE int64 table [R][2] of (base, n_samples), and one launch serves all of them.  A record the
// host could not check is checked here: base < 0, n_samples < 0, base + n_samples > pool_len or more frames than the
// tables hold make the recording empty (energies 0, nothing kept, nothing copied); nothing outside the pool is read.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "openvoice_amd.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// frames of a record; 0 for a record that does not fit the pool or the tables
__device__ __forceinline__ int64_t record_frames(int64_t base, int64_t n, int64_t pool_len, int H, int ldT) {
  if (base < 0 || n <= 0 || n > pool_len || base > pool_len - n) return 0;
  const int64_t T = (n + H - 1) / H;
  return T <= ldT ? T : 0;
}

// ---- frame energy ----------------------------------------------------------------------------------------------------
// e[t] = mean of x^2 over [tH, min(N, tH + 2H)).  A frame is two hops, so a block sums kFramesPerBlock + 1 hops once (one
// wave per hop at a time) and then adds neighbours.  Lane l of the wave holds samples 4l .. 4l + 3 (+ 256 k) of the hop
// and squares and adds them in that order whether they arrived as one 16-byte load or as four bounds-checked scalars
// (a sample beyond N counts as 0), then the 64 lanes are added by a fixed butterfly: a hop's sum depends on the hop's
// samples alone -- not on R, the base, its alignment or the block that computed it.
constexpr int kFramesPerBlock = 16;

__global__ __launch_bounds__(256) void vad_frame_energy_kernel(const float* __restrict__ pool, int64_t pool_len,
                                                               const int64_t* __restrict__ records, int H, int ldT,
                                                               float* __restrict__ energy, int pool_aligned) {
  __shared__ float hop_sum[kFramesPerBlock + 1];
  const int r = blockIdx.y;
  const int64_t base = records[2 * r], n = records[2 * r + 1];
  const int64_t T = record_frames(base, n, pool_len, H, ldT);
  const int64_t t0 = (int64_t)blockIdx.x * kFramesPerBlock;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool vec_ok = pool_aligned && (base & 3) == 0;
  const float* x = pool + (T > 0 ? base : 0);
  for (int h = wave; h <= kFramesPerBlock; h += 4) {
    const int64_t s0 = (t0 + h) * H;                       // first sample of hop t0 + h
    float acc = 0.f;
    if (T > 0 && s0 < n) {                                  // (a hop beyond the end sums to 0)
      for (int j = 4 * lane; j < H; j += 256) {
        const int64_t s = s0 + j;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (s + 4 <= n && vec_ok) {
          v = *reinterpret_cast<const f32x4*>(x + s);
        } else {
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (s + c < n) v[c] = x[s + c];
        }
        // explicit fused multiply-adds: the compiler has no contraction left to decide per code path
        acc += fmaf(v[1], v[1], v[0] * v[0]) + fmaf(v[3], v[3], v[2] * v[2]);
      }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);
    if (lane == 0) hop_sum[h] = acc;
  }
  __syncthreads();
  if (threadIdx.x < kFramesPerBlock) {
    const int64_t t = t0 + threadIdx.x;
    if (t < ldT) {
      float e = 0.f;
      if (t < T) {
        const int64_t end = (t + 2) * H < n ? (t + 2) * H : n;
        e = (hop_sum[threadIdx.x] + hop_sum[threadIdx.x + 1]) / (float)(end - t * H);
      }
      energy[(int64_t)r * ldT + t] = e;
    }
  }
}

// ---- segments --------------------------------------------------------------------------------------------------------
// One workgroup per recording walks the frame axis in chunks of kSegThreads * kSegItems frames, forwards or backwards,
// with an inclusive block scan per chunk and the scan's running value carried from chunk to chunk, so a recording of any
// length is handled.  The two tables this kernel outputs double as its scratch between passes.
constexpr int kSegThreads = 1024;
constexpr int kSegItems = 4;
constexpr int kSegChunk = kSegThreads * kSegItems;

struct OpMax { __device__ static int64_t op(int64_t a, int64_t b) { return a > b ? a : b; } };
struct OpMin { __device__ static int64_t op(int64_t a, int64_t b) { return a < b ? a : b; } };
struct OpSum { __device__ static int64_t op(int64_t a, int64_t b) { return a + b; } };

// v[0 .. kSegItems) of thread i are the chunk's elements i * kSegItems + k in scan order.  On return v holds the
// inclusive scan seeded with `carry`, and `carry` the scan over everything up to the chunk's end.
template <typename Op>
__device__ __forceinline__ void block_scan(int64_t (&v)[kSegItems], int64_t& carry, int64_t* wave_tot) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 1; k < kSegItems; ++k) v[k] = Op::op(v[k - 1], v[k]);
  int64_t tot = v[kSegItems - 1];
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int64_t o = __shfl_up(tot, d);
    if (lane >= d) tot = Op::op(o, tot);
  }
  if (lane == 63) wave_tot[wave] = tot;
  const int64_t before = __shfl_up(tot, 1);                 // scan of the lanes before this one
  __syncthreads();
  int64_t pre = carry, all = carry;
  for (int w = 0; w < kSegThreads / 64; ++w) {
    const int64_t x = wave_tot[w];
    if (w < wave) pre = Op::op(pre, x);
    all = Op::op(all, x);
  }
  if (lane > 0) pre = Op::op(pre, before);
#pragma unroll
  for (int k = 0; k < kSegItems; ++k) v[k] = Op::op(pre, v[k]);
  carry = all;
  __syncthreads();                                          // wave_tot is reused by the next chunk
}

// The passes.  `flag(t)` is a 0/1 property of frame t; a forward pass computes L[t] = the last u <= t with flag(u) (-1:
// none), a backward pass F[t] = the first u >= t with flag(u) (T: none); `emit(t, value)` consumes it.  Backward passes
// run the same scan over the reversed axis.
template <bool kBackward, typename Flag, typename Emit>
__device__ __forceinline__ void scan_pass(int64_t T, int64_t* wave_tot, Flag flag, Emit emit) {
  int64_t carry = kBackward ? T : -1;
  for (int64_t c0 = 0; c0 < T; c0 += kSegChunk) {
    int64_t v[kSegItems];
#pragma unroll
    for (int k = 0; k < kSegItems; ++k) {
      const int64_t j = c0 + (int64_t)threadIdx.x * kSegItems + k;
      const int64_t t = kBackward ? T - 1 - j : j;
      v[k] = (j < T && flag(t)) ? t : (kBackward ? T : -1);
    }
    if (kBackward) block_scan<OpMin>(v, carry, wave_tot); else block_scan<OpMax>(v, carry, wave_tot);
#pragma unroll
    for (int k = 0; k < kSegItems; ++k) {
      const int64_t j = c0 + (int64_t)threadIdx.x * kSegItems + k;
      if (j < T) emit(kBackward ? T - 1 - j : j, v[k]);
    }
  }
  __syncthreads();               // what this pass stored is read by other threads in the next one
}

__global__ __launch_bounds__(kSegThreads) void vad_segments_kernel(const float* __restrict__ energy,
                                                                  const int64_t* __restrict__ records, int H, int ldT,
                                                                  float floor_lin, float range_lin, int min_silence,
                                                                  int min_speech, int pad, int32_t* mask_out,
                                                                  int64_t* offsets_out,
                                                                  int64_t* __restrict__ n_active) {
  __shared__ int64_t wave_tot[kSegThreads / 64];
  __shared__ float wave_max[kSegThreads / 64];
  const int r = blockIdx.x;
  const int64_t n = records[2 * r + 1];
  int64_t T = n > 0 ? (n + H - 1) / H : 0;
  if (T > ldT) T = 0;
  const float* e = energy + (int64_t)r * ldT;
  int32_t* m = mask_out + (int64_t)r * ldT;                 // also scratch: a 32-bit frame index or a 0/1 flag
  int64_t* o = offsets_out + (int64_t)r * ldT;              // also scratch: a frame index
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

  // the threshold: max(floor, peak * 10^(-range_db / 10)), linear domain
  float peak = 0.f;
  for (int64_t t = threadIdx.x; t < T; t += kSegThreads) peak = fmaxf(peak, e[t]);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) peak = fmaxf(peak, __shfl_xor(peak, d));
  if (lane == 0) wave_max[wave] = peak;
  __syncthreads();
  for (int w = 0; w < kSegThreads / 64; ++w) peak = fmaxf(peak, wave_max[w]);
  const float thr = fmaxf(floor_lin, peak * range_lin);
  auto raw = [&](int64_t t) { return e[t] > thr; };

  // step 3, close gaps: a silent frame between raw-active frames L < t < F with F - L - 1 < min_silence becomes active
  scan_pass<false>(T, wave_tot, raw, [&](int64_t t, int64_t L) { o[t] = L; });
  scan_pass<true>(T, wave_tot, raw, [&](int64_t t, int64_t F) {
    const int64_t L = o[t];
    m[t] = raw(t) || (L >= 0 && F < T && F - L - 1 < min_silence);
  });
  // step 4, drop blips: a closed run [L + 1, F - 1] between silent frames L and F shorter than min_speech goes
  auto silent = [&](int64_t t) { return m[t] == 0; };
  scan_pass<false>(T, wave_tot, silent, [&](int64_t t, int64_t L) { o[t] = L; });
  scan_pass<true>(T, wave_tot, silent, [&](int64_t t, int64_t F) { m[t] = m[t] != 0 && F - o[t] - 1 >= min_speech; });
  // step 5, pad: a frame within `pad` frames of a remaining active frame is kept
  auto active = [&](int64_t t) { return m[t] != 0; };
  scan_pass<false>(T, wave_tot, active, [&](int64_t t, int64_t L) { o[t] = L; });
  scan_pass<true>(T, wave_tot, active, [&](int64_t t, int64_t F) {
    const int64_t L = o[t];
    m[t] = (L >= 0 && t - L <= pad) || (F < T && F - t <= pad);
  });
  // step 6: exclusive prefix sum of the kept samples per frame
  int64_t carry = 0;
  for (int64_t c0 = 0; c0 < T; c0 += kSegChunk) {
    int64_t v[kSegItems], own[kSegItems];
#pragma unroll
    for (int k = 0; k < kSegItems; ++k) {
      const int64_t t = c0 + (int64_t)threadIdx.x * kSegItems + k;
      const int64_t left = n - t * H;
      own[k] = (t < T && m[t] != 0) ? (left < H ? left : (int64_t)H) : 0;
      v[k] = own[k];
    }
    block_scan<OpSum>(v, carry, wave_tot);
#pragma unroll
    for (int k = 0; k < kSegItems; ++k) {
      const int64_t t = c0 + (int64_t)threadIdx.x * kSegItems + k;
      if (t < T) o[t] = v[k] - own[k];
    }
  }
  if (threadIdx.x == 0) n_active[r] = carry;
  // the tables' tails beyond the recording: nothing kept
  for (int64_t t = T + threadIdx.x; t < ldT; t += kSegThreads) { m[t] = 0; o[t] = carry; }
}

// ---- compaction ------------------------------------------------------------------------------------------------------
// One wave per kept frame: its up to H samples go to out[out_base + offsets[t]].  Offsets are multiples of H, so with
// aligned bases both sides of a whole frame move as 16-byte vectors; the one partial frame is a recording's last.
constexpr int kCompactFramesPerBlock = 16;

__global__ __launch_bounds__(256) void vad_compact_kernel(const float* __restrict__ pool, int64_t pool_len,
                                                          const int64_t* __restrict__ records, int H, int ldT,
                                                          const int32_t* __restrict__ mask, const int64_t* __restrict__ offsets,
                                                          const int64_t* __restrict__ out_bases, float* __restrict__ out,
                                                          int64_t out_len, int bases_aligned) {
  const int r = blockIdx.y;
  const int64_t base = records[2 * r], n = records[2 * r + 1], ob = out_bases[r];
  const int64_t T = record_frames(base, n, pool_len, H, ldT);
  if (ob < 0 || ob > out_len) return;
  const bool vec_ok = bases_aligned && ((base | ob) & 3) == 0;
  const int lane = threadIdx.x & 63;
  const int64_t t_end = ((int64_t)blockIdx.x + 1) * kCompactFramesPerBlock;
  for (int64_t t = (int64_t)blockIdx.x * kCompactFramesPerBlock + (threadIdx.x >> 6); t < t_end && t < T; t += 4) {
    if (mask[(int64_t)r * ldT + t] == 0) continue;
    const int64_t off = offsets[(int64_t)r * ldT + t];
    const int64_t left = n - t * H, cnt = left < H ? left : (int64_t)H;
    if (off < 0 || off > out_len - ob - cnt) continue;       // would leave the output: copy nothing
    const float* s = pool + base + t * H;
    float* d = out + ob + off;
    int64_t j0 = 0;
    if (vec_ok && (off & 3) == 0) {
      const int64_t nv = cnt >> 2;
      for (int64_t v = lane; v < nv; v += 64)
        *reinterpret_cast<f32x4*>(d + 4 * v) = *reinterpret_cast<const f32x4*>(s + 4 * v);
      j0 = nv << 2;
    }
    for (int64_t j = j0 + lane; j < cnt; j += 64) d[j] = s[j];
  }
}

bool bad_common(const void* a, const void* b, int R, int H, int ldT) {
  return !a || !b || R <= 0 || R > 65535 || H <= 0 || H % 4 != 0 || ldT <= 0;
}

}  // namespace

extern "C" {

int ov_vad_frame_energy_f32(const float* pool, int64_t pool_len, const int64_t* records, int R, int H, int ldT,
                            float* energy, ov_stream_t stream) {
  if (bad_common(pool, records, R, H, ldT) || !energy || pool_len <= 0) return OV_E_BADARG;
  const int aligned = !(reinterpret_cast<uintptr_t>(pool) & 15);
  dim3 grid((ldT + kFramesPerBlock - 1) / kFramesPerBlock, R);
  hipLaunchKernelGGL(vad_frame_energy_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), pool, pool_len,
                     records, H, ldT, energy, aligned);
  return hipGetLastError() == hipSuccess ? OV_OK : OV_E_LAUNCH;
}

int ov_vad_segments_i32(const float* energy, const int64_t* records, int R, int H, int ldT, float floor_lin,
                        float range_lin, int min_silence_frames, int min_speech_frames, int pad_frames, int32_t* mask,
                        int64_t* offsets, int64_t* n_active, ov_stream_t stream) {
  if (bad_common(energy, records, R, H, ldT) || !mask || !offsets || !n_active || min_silence_frames <= 0 ||
      min_speech_frames <= 0 || pad_frames < 0 || !(floor_lin >= 0.f) || !(range_lin >= 0.f))
    return OV_E_BADARG;
  hipLaunchKernelGGL(vad_segments_kernel, dim3(R), dim3(kSegThreads), 0, static_cast<hipStream_t>(stream), energy,
                     records, H, ldT, floor_lin, range_lin, min_silence_frames, min_speech_frames, pad_frames, mask,
                     offsets, n_active);
  return hipGetLastError() == hipSuccess ? OV_OK : OV_E_LAUNCH;
}

int ov_vad_compact_f32(const float* pool, int64_t pool_len, const int64_t* records, int R, int H, int ldT,
                       const int32_t* mask, const int64_t* offsets, const int64_t* out_bases, float* out,
                       int64_t out_len, ov_stream_t stream) {
  if (bad_common(pool, records, R, H, ldT) || !mask || !offsets || !out_bases || !out || pool_len <= 0 || out_len <= 0)
    return OV_E_BADARG;
  const int aligned = !(reinterpret_cast<uintptr_t>(pool) & 15) && !(reinterpret_cast<uintptr_t>(out) & 15);
  dim3 grid((ldT + kCompactFramesPerBlock - 1) / kCompactFramesPerBlock, R);
  hipLaunchKernelGGL(vad_compact_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), pool, pool_len, records,
                     H, ldT, mask, offsets, out_bases, out, out_len, aligned);
  return hipGetLastError() == hipSuccess ? OV_OK : OV_E_LAUNCH;
}

}  // extern "C"
