// The per-element arithmetic of the duration-driven prior expansion (reference: openvoice/models.py:480-487,
// commons.py:128-142), shared by ov_expand_prior_f32 (tts.hip), ov_expand_prior_items_f32 (tts_items.hip) and
// ov_expand_prior_rows_f32 (tts_live.hip): one definition of "which token owns frame t" and of the prior sample, so the
// three kernels give a frame the same bits.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace ovp {

// The token j < xl with cum[j - 1] <= t < cum[j] (cum: the inclusive prefix sums of the durations, non-decreasing), or
// -1 when t lies at or beyond cum[xl - 1].
__device__ inline int token_of_frame(const int32_t* __restrict__ cb, int xl, int t) {
  if (xl <= 0 || t >= cb[xl - 1]) return -1;
  int lo = 0, hi = xl - 1;              // first j with cum[j] > t
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (cb[mid] > t) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// z_p = m_p + noise * exp(logs_p) * noise_scale (models.py:486-487).
__device__ inline float prior_sample(float m, float noise, float lg, float noise_scale) {
  return m + noise * expf(lg) * noise_scale;
}

}  // namespace ovp
