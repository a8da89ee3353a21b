// The counter-based Gaussian of openvoice_amd/noise.py as device functions, shared by every kernel that draws it
// (noise.hip fills slabs with it, tts_live.hip samples the TTS prior with it): one definition, so the value at (seed,
// stream, purpose, channel, frame) has the same bits wherever it is computed.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace ovn {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ inline void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                     uint32_t r[4]) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  r[0] = c0, r[1] = c1, r[2] = c2, r[3] = c3;
}

// Box-Muller on one pair of words.  u1 = (x + 0.5) 2^-24 with x = ra >> 8 is exact in fp32 for x < 2^23; for the upper
// half 1 - u1 = ((2^24 - 1 - x) + 0.5) 2^-24 is, so the logarithm goes through log1p there (near u1 = 1, where the
// radius is small, rounding u1 itself would lose all of it).  The angle is taken in half turns: 2 u2 is exact.
__device__ inline void box_muller(uint32_t ra, uint32_t rb, float& even, float& odd) {
  const uint32_t x = ra >> 8;
  float ln;
  if (x < (1u << 23))
    ln = logf(((float)x + 0.5f) * 0x1p-24f);
  else
    ln = log1pf(-(((float)(0xFFFFFFu - x) + 0.5f) * 0x1p-24f));
  const float radius = sqrtf(-2.f * ln);
  float s, c;
  sincospif((float)(rb >> 8) * 0x1p-23f, &s, &c);
  even = radius * c;
  odd = radius * s;
}

// One Philox block: the four values of frames 4 q .. 4 q + 3 of channel c, computed before the caller knows how it will
// store them.
__device__ inline f32x4 normal_block(uint32_t q, uint32_t c, uint32_t strm, uint32_t purpose, uint32_t k0, uint32_t k1) {
  uint32_t r[4];
  philox4x32_10(q, c, strm, purpose, k0, k1, r);
  f32x4 v;
  float a, b;
  box_muller(r[0], r[1], a, b);
  v[0] = a, v[1] = b;
  box_muller(r[2], r[3], a, b);
  v[2] = a, v[3] = b;
  return v;
}

}  // namespace ovn
