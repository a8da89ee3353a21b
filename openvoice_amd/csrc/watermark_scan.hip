// The native watermark's reader at EVERY offset (openvoice_amd/watermark.py, "the scan"): where csrc/watermark.hip reads
// the window that starts at a sample the caller names, ov_wm_scan_f32 reads the 16 000-sample window that starts at every
// sample s of a waveform, so that a mark is found in audio whose start was cut, shifted or is unknown.
//
// The decomposition.  With i = 32 m + j (m < 500 the chip row, j < 32 the bit),
//   p_j(s) = (1/500) sum_m c[32 m + j] x[s + 32 m + j]
// and with t = s + j, C[m][j] = c[32 m + j]:
//   Q[t][j] = sum_m x[t + 32 m] C[m][j],        p_j(s) = Q[s + j][j] / 500
// For the 32 consecutive t = 32 n + r (r < 32) that is one 32 x 32 product with K = 500,
//   Q[32 n + r][j] = sum_m X[n + m][r] C[m][j],          X[a][r] = x[32 a + r]
// whose A operand is rows n + m of the waveform read as a [.][32] matrix: v_mfma_f32_32x32x2_f32 takes A[r][k = lane >> 5]
// from lane (r, k), so a fragment is 64 CONSECUTIVE floats of a linear copy of x in LDS -- the rows of the fragment are
// the residues, and no stride-32 read occurs.  B[k][j] is +-1.0 made in the lane from bit j of chip word m = 2 ks + k (the
// words of 125 Philox blocks, 2 KB of LDS, computed by the workgroup; there is no chip table in global memory), two VALU
// operations that serve the eight MFMAs of a k-step.  Every Q element belongs to exactly one (s, j) = (t - j, j).
//
// The tile.  A workgroup of four waves owns 896 offsets.  Wave w holds the eight accumulator tiles n = 7 w .. 7 w + 7
// (128 registers) and runs the whole K loop, 250 steps of two chip rows, for all of them: 2000 MFMAs against one chip
// fragment per step.  The offsets of block b (32 of them, s = 32 (7 w + b) + sigma) need rows sigma + j of tiles b and
// b + 1, so a wave finishes seven blocks from eight tiles; neighbouring waves compute their shared tile twice (1/8 of
// the matrix work) and no Q element ever leaves the wave.  The staged waveform is 32 (29 + 499) floats = 67 584 B, and
// after the K loop (one barrier) each wave's ring of two transposed tiles, 64 x 33 floats, aliases it: 69.6 KB per
// workgroup, two workgroups per CU.  Column 32 of a ring row carries W[t] = sum_m x[t + 32 m]^2, which the lane that
// loaded A[r][k] summed as it went (one FMA beside each MFMA), and the energy of window s is sum_j W[s + j] -- the same
// skewed read as the projections.
//
// Determinism.  Q[t][j] is one MFMA chain over m = 0 .. 499 in ascending pairs, W[t] two FMA chains over the even and the
// odd m added once, and the skewed read adds and compares in a fixed order of j; none of it depends on where t falls in a
// fragment, a wave, a tile or a record.  words / pmin / level of offset s are functions of x[s .. s + 16 000), the key,
// strength and floor alone.  No atomics.
//
// ov_wm_scan_pick then turns the three arrays into an ordered hit list, one workgroup per record, plain VALU.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "openvoice_amd.h"
#include "philox_normal.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kThreads = 256;
constexpr int kWaves = 4;
constexpr int kBits = 32;
constexpr int kWindow = 16000;
constexpr int kChipRows = kWindow / kBits;                       // 500: m
constexpr int kSteps = kChipRows / 2;                            // 250 k-steps of two chip rows
constexpr int kWaveTiles = 8;                                    // accumulator tiles of a wave
constexpr int kWaveBlocks = kWaveTiles - 1;                      // 32-offset blocks it finishes
constexpr int kTileOffsets = kWaves * kWaveBlocks * kBits;       // 896 offsets per workgroup
constexpr int kStageRows = kWaves * kWaveBlocks + 1 + kChipRows - 1;     // 528 rows of 32 samples
constexpr int kStage = kStageRows * kBits;                       // 16 896 floats
constexpr int kRingLd = kBits + 1;                               // 32 Q columns and W
constexpr int kRing = 2 * kBits * kRingLd;                       // two transposed tiles of a wave
constexpr int64_t kMaxN = (int64_t)1 << 31;
constexpr int64_t kMaxOff = (int64_t)1 << 61;
constexpr uint32_t kPurposeWatermark = 3;                        // noise.py: the chips' Philox purpose
constexpr int kMaxGroups = 8;

static_assert(kWaves * kRing <= kStage, "the rings alias the staged waveform");

__device__ inline bool span_ok(int64_t off, int64_t n, int64_t elems) { return off >= 0 && off <= kMaxOff && n <= elems && off <= elems - n; }

__global__ __launch_bounds__(kThreads) void wm_scan_kernel(const float* __restrict__ src, int64_t src_elems,
                                                           const int64_t* __restrict__ records, int64_t max_n, uint32_t k0,
                                                           uint32_t k1, float strength, float floor_level,
                                                           int32_t* __restrict__ words, float* __restrict__ pmin,
                                                           float* __restrict__ level, float* __restrict__ p_out,
                                                           int64_t out_elems) {
  __shared__ float xs[kStage];
  __shared__ uint32_t cw[kChipRows];                  // chip words, inverted: a set bit is a chip of -1
  const int64_t* rec = records + 3 * (int64_t)blockIdx.y;
  const int64_t so = rec[0], n = rec[1], oo = rec[2];
  // (block-uniform)
  if (n < kWindow || n > max_n || n > kMaxN || !span_ok(so, n, src_elems)) return;
  const int64_t S = n - kWindow + 1;
  if (!span_ok(oo, S, out_elems)) return;
  const int64_t s0 = (int64_t)blockIdx.x * kTileOffsets;
  if (s0 >= S) return;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, r = lane & 31, h = lane >> 5;

  if (t < kChipRows / 4) {
    uint32_t q[4];
    ovn::philox4x32_10((uint32_t)t, 0u, 0u, kPurposeWatermark, k0, k1, q);
#pragma unroll
    for (int i = 0; i < 4; ++i) cw[4 * t + i] = ~q[i];
  }
  // every sample a valid offset of this tile needs lies below n (s + j + 32 m <= S - 1 + 31 + 15 968 = n - 1); rows past
  // the record are zeros and reach only Q rows no valid offset reads
  const float* x = src + so;
  for (int i = t; i < kStage; i += kThreads) {
    const int64_t idx = s0 + i;
    xs[i] = idx < n ? x[idx] : 0.f;
  }
  __syncthreads();

  const bool active = s0 + (int64_t)w * (kWaveBlocks * kBits) < S;       // (wave-uniform) the wave owns a valid offset
  f32x16 acc[kWaveTiles];
  float e[kWaveTiles];
#pragma unroll
  for (int i = 0; i < kWaveTiles; ++i) {
    e[i] = 0.f;
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[i][v] = 0.f;
  }
  if (active) {
    const float* xa = xs + kBits * (kWaveBlocks * w + h) + r;            // tile i, step ks: row 7 w + i + 2 ks + h
    const int shift = 31 - r;
#pragma unroll 2
    for (int ks = 0; ks < kSteps; ++ks) {
      const uint32_t wd = cw[2 * ks + h];
      const float b = __uint_as_float(((wd << shift) & 0x80000000u) | 0x3F800000u);
#pragma unroll
      for (int i = 0; i < kWaveTiles; ++i) {
        const float a = xa[kBits * (i + 2 * ks)];
        e[i] = __builtin_fmaf(a, a, e[i]);
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[i], 0, 0, 0);
      }
    }
  }
  __syncthreads();                                    // every wave is done with xs: the rings alias it

  float* ring = xs + w * kRing;
  // tile i -> ring slot i & 1, transposed to [t][j]; C/D map: column j = lane & 31, row (v & 3) + 8 (v >> 2) + 4 h
  auto put = [&](const f32x16& c, float ei, int slot) {
    float* qt = ring + slot * kBits * kRingLd;
#pragma unroll
    for (int v = 0; v < 16; ++v) qt[((v & 3) + 8 * (v >> 2) + 4 * h) * kRingLd + r] = c[v];
    const float wt = ei + __shfl_xor(ei, 32);         // W[t]: the even and the odd chip rows
    if (h == 0) qt[r * kRingLd + kBits] = wt;
  };
  put(acc[0], e[0], 0);
#pragma unroll
  for (int b = 0; b < kWaveBlocks; ++b) {
    put(acc[b + 1], e[b + 1], (b + 1) & 1);
    __syncthreads();
    // offset s = s0 + 32 (7 w + b) + r: lane half h takes bits 16 h .. 16 h + 15, row r + j of the two tiles
    const int64_t s = s0 + (int64_t)kBits * (kWaveBlocks * w + b) + r;
    const bool valid = active && s < S;
    uint32_t word = 0u;
    float mn = __builtin_inff(), en = 0.f;
#pragma unroll
    for (int jj = 0; jj < kBits / 2; ++jj) {
      const int j = 16 * h + jj;
      const float* row = ring + (((b & 1) * kBits + r + j) & 63) * kRingLd;
      const float v = row[j];
      word |= (v >= 0.f ? 1u : 0u) << j;
      mn = fminf(mn, fabsf(v));
      en += row[kBits];
      if (p_out && valid) p_out[(oo + s) * kBits + j] = v / (float)kChipRows;
    }
    word |= (uint32_t)__shfl_xor((int)word, 32);
    mn = fminf(mn, __shfl_xor(mn, 32));
    en += __shfl_xor(en, 32);
    if (valid && h == 0) {
      words[oo + s] = (int32_t)word;
      pmin[oo + s] = mn / (float)kChipRows;           // min and a division by 500 commute: == min_j |p_j|
      level[oo + s] = fmaxf(strength * sqrtf(en / (float)kWindow), floor_level);
    }
    __syncthreads();                                  // before tile b + 2 takes the slot of tile b
  }
}

// One workgroup per record (scan_off, S): the offsets whose word is within max_errors bits of a group (G > 0), or whose
// weakest projection reaches margin * level (G == 0), as rows (s, word, k or -1, errors) in ascending s.  256 offsets a
// step: a ballot and a popcount order the hits inside a wave, four wave totals through LDS order the waves, and a
// running base orders the steps -- the same list whatever the launch.
__global__ __launch_bounds__(kThreads) void wm_pick_kernel(const int32_t* __restrict__ words, const float* __restrict__ pmin,
                                                           const float* __restrict__ level, int64_t scan_elems,
                                                           const int64_t* __restrict__ records,
                                                           const int32_t* __restrict__ groups, int G, int max_errors,
                                                           float margin, int32_t* __restrict__ hits, int cap,
                                                           int32_t* __restrict__ counts) {
  __shared__ int wave_total[kWaves];
  const int64_t off = records[2 * (int64_t)blockIdx.x], S = records[2 * (int64_t)blockIdx.x + 1];
  if (S < 0 || S >= kMaxN || !span_ok(off, S, scan_elems)) return;       // (block-uniform)
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  uint32_t g[kMaxGroups];
#pragma unroll
  for (int k = 0; k < kMaxGroups; ++k) g[k] = k < G ? (uint32_t)groups[k] : 0u;
  int32_t* out = hits + (int64_t)blockIdx.x * cap * 4;
  int base = 0;
  for (int64_t c = 0; c < S; c += kThreads) {
    const int64_t s = c + t;
    bool hit = false;
    uint32_t wd = 0u;
    int best_k = -1, best_e = 0;
    if (s < S) {
      wd = (uint32_t)words[off + s];
      if (G > 0) {
        best_e = kBits + 1;
#pragma unroll
        for (int k = 0; k < kMaxGroups; ++k) {
          const int err = __popc(wd ^ g[k]);
          if (k < G && err < best_e) best_e = err, best_k = k;
        }
        hit = best_e <= max_errors;
      } else {
        hit = pmin[off + s] >= margin * level[off + s];
      }
    }
    const unsigned long long m = __ballot(hit);
    if (lane == 0) wave_total[w] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int ww = 0; ww < kWaves; ++ww) {
      before += ww < w ? wave_total[ww] : 0;
      total += wave_total[ww];
    }
    if (hit) {
      const int pos = base + before + __popcll(m & ((1ull << lane) - 1ull));
      if (pos < cap) {
        int32_t* row = out + 4 * (int64_t)pos;
        row[0] = (int32_t)s, row[1] = (int32_t)wd, row[2] = best_k, row[3] = best_e;
      }
    }
    base += total;
    __syncthreads();
  }
  if (t == 0) counts[blockIdx.x] = base;
}

}  // namespace

extern "C" {

int ov_wm_scan_tile(void) { return kTileOffsets; }

int ov_wm_scan_f32(const float* src, int64_t src_elems, const int64_t* records, int R, int64_t max_n, int64_t key,
                   float strength, float floor_level, int32_t* words, float* pmin, float* level, float* p_out,
                   int64_t out_elems, ov_stream_t stream) {
  // (a NaN fails every comparison)
  if (!src || !records || !words || !pmin || !level || src_elems <= 0 || out_elems <= 0 || R < 1 || R > 65535 ||
      max_n < kWindow || max_n > kMaxN || key < 0 || !(strength >= 0.f && strength <= 1.f) ||
      !(floor_level > 0.f && floor_level <= 1.f))
    return OV_E_BADARG;
  if ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(words) | reinterpret_cast<uintptr_t>(pmin) |
       reinterpret_cast<uintptr_t>(level) | reinterpret_cast<uintptr_t>(p_out)) & 3)
    return OV_E_ALIGN;
  if (reinterpret_cast<uintptr_t>(records) & 7) return OV_E_ALIGN;
  const int64_t tiles = (max_n - kWindow + 1 + kTileOffsets - 1) / kTileOffsets;
  hipLaunchKernelGGL(wm_scan_kernel, dim3((unsigned)tiles, (unsigned)R), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                     src, src_elems, records, max_n, (uint32_t)key, (uint32_t)((uint64_t)key >> 32), strength, floor_level,
                     words, pmin, level, p_out, out_elems);
  return hipGetLastError() == hipSuccess ? OV_OK : OV_E_LAUNCH;
}

int ov_wm_scan_pick(const int32_t* words, const float* pmin, const float* level, int64_t scan_elems, const int64_t* records,
                    int R, const int32_t* groups, int G, int max_errors, float margin, int32_t* hits, int cap,
                    int32_t* counts, ov_stream_t stream) {
  if (!words || !pmin || !level || !records || !counts || scan_elems <= 0 || R < 1 || R > 65535 || G < 0 || G > kMaxGroups ||
      (G > 0 && !groups) || max_errors < 0 || max_errors > kBits || !(margin >= 0.f) || cap < 0 || (cap > 0 && !hits))
    return OV_E_BADARG;
  if ((reinterpret_cast<uintptr_t>(words) | reinterpret_cast<uintptr_t>(pmin) | reinterpret_cast<uintptr_t>(level) |
       reinterpret_cast<uintptr_t>(groups) | reinterpret_cast<uintptr_t>(hits) | reinterpret_cast<uintptr_t>(counts)) & 3)
    return OV_E_ALIGN;
  if (reinterpret_cast<uintptr_t>(records) & 7) return OV_E_ALIGN;
  hipLaunchKernelGGL(wm_pick_kernel, dim3((unsigned)R), dim3(kThreads), 0, static_cast<hipStream_t>(stream), words, pmin,
                     level, scan_elems, records, groups, G, max_errors, margin, hits, cap, counts);
  return hipGetLastError() == hipSuccess ? OV_OK : OV_E_LAUNCH;
}

}  // extern "C"
