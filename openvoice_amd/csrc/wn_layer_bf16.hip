// One WaveNet layer in ONE launch on the bf16 matrix pipe (reference: openvoice/modules.py:192-209, commons.py:100-107):
//
//   x_in = conv_k5(bf16(W_in), bf16(h)) + b_in + cond        fp32 accumulation, v_mfma_f32_16x16x32_bf16
//   acts = bf16(tanh(x_in[:H]) * sigmoid(x_in[H:]))          gate in fp32, ONE round to nearest even, stays in LDS
//   rs   = conv_1x1(bf16(W_rs), acts) + b_rs                 fp32 accumulation
//   out  = (h + rs[:H]) * mask     skip = (first ? 0 : skip) + rs[H:]      with the UNROUNDED fp32 h
//
// The state (h, skip) stays fp32 in the [B][H][ld] row layout of ov_wn_layer_f32: only the MFMA operands are rounded, so
// a layer's error is one rounding of its operands and is not compounded through the state.
//
// Workgroup = 8 waves, one (utterance, tile of W = 16 .. 128 columns).  All waves stage, all waves multiply:
//   * staging: the tile's h columns t0 - 4 .. t0 + W + 4 are read as 16-byte vectors of fp32 rows (coalesced along T, the
//     vector rule of ov_wn_layer_f32: a vector is read iff its first column lies in [0, T)), rounded, and columns
//     t0 - 2 .. t0 + W + 2 are written to LDS CHANNEL-contiguous, xt[column][channel] with a 400-byte row pitch: the 8
//     consecutive k a lane feeds to the MFMA are one ds_read_b128, and 16 lanes on 16 consecutive columns fall into 16
//     disjoint groups of four banks (100 dwords = 36 mod 64).  Columns < 0 and >= T are zero: the conv's own padding.
//   * phase 1: wave w owns gate-row fragments 3w .. 3w + 2 (16 rows each, rows in the gate order of wn_fused_row_order) x
//     all W columns.  k order, the same for every output element: 32-channel chunk, then tap -- 30 MFMAs of k = 32.  A
//     operands (weights) stream from L2 in fragment order, one 3 KiB record per wave and k-step, requested one step ahead;
//     B operands are one ds_read_b128 per column fragment and k-step, shared by the wave's three row fragments.
//   * gate in registers (a lane's four accumulator rows are tanh a, tanh b, sigmoid a, sigmoid b of two channels), rounded
//     once, written to the acts LDS tile [column][channel] of the same pitch.
//   * phase 2 runs transposed like the fp32 kernel (D = acts^T W_rs^T): a lane holds 4 consecutive time columns of one row,
//     so h / skip / out are touched with 16-byte accesses.  6 MFMAs of k = 32 per fragment.
// Every output element is the result of the same instruction sequence on the same operands whatever the tile width, the
// tile index, the batch size or the item's row: results are bit-identical across all of them.
// LDS at W = 128: (132 + 128) x 400 B = 104 KB.  Weights: 737 KB per layer, read once per workgroup from L2.
#include <hip/hip_runtime.h>

#include <cstring>

#include "openvoice_amd.h"

namespace ovkwb {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int NW = 8;          // waves per workgroup
constexpr int CH = 32;         // k of one MFMA: input channels per k-step
constexpr int PITCH = 200;     // LDS row pitch in bf16 elements: H + 8 (400 bytes = 100 dwords = 36 mod 64 banks)
constexpr int PADA = 4;        // staged halo on each side (16-byte aligned global vectors; >= (K-1)/2)

// two floats -> packed bf16 pair (lo | hi << 16), round to nearest even: one v_cvt_pk_bf16_f32
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
  typedef float f2 __attribute__((ext_vector_type(2)));
  typedef __bf16 b2 __attribute__((ext_vector_type(2)));
  const b2 r = __builtin_convertvector(f2{lo, hi}, b2);
  uint32_t u;
  __builtin_memcpy(&u, &r, 4);
  return u;
}

// tanh(t) * sigmoid(s), the form of wn_layer.hip: two v_exp_f32 and one v_rcp_f32
__device__ __forceinline__ float wn_gate(float t, float s) {
  const float a = __builtin_amdgcn_exp2f(fabsf(t) * -2.8853900817779268f);   // e^-2|t|
  const float e = __builtin_amdgcn_exp2f(s * -1.4426950408889634f);          // e^-s  (inf for s << 0: result 0)
  const float r = __builtin_amdgcn_rcpf((1.f + a) * (1.f + e));
  return copysignf((1.f - a) * r, t);
}

__device__ __forceinline__ bf16x8 as_bf16x8(u32x4 v) {
  bf16x8 r;
  __builtin_memcpy(&r, &v, 16);
  return r;
}

template <int K, int H, int NB>
__global__ __launch_bounds__(64 * NW) void wn_layer_bf16_kernel(const ov_wn_layer_params p) {
  static_assert((2 * H) % (16 * NW) == 0 && H % CH == 0 && H + 8 <= PITCH, "H a multiple of 64, at most 192");
  static_assert(K % 2 == 1 && (K - 1) / 2 <= PADA, "odd K <= 9");
  static_assert(NB >= 1 && NB <= 8, "tile width 16 .. 128 columns");
  constexpr int RB = 2 * H / (16 * NW);        // 16-row fragments per wave, both phases
  constexpr int PAD = (K - 1) / 2;
  constexpr int W = 16 * NB;
  constexpr int NCOL = W + 2 * PAD;            // staged columns t0 - PAD .. t0 + W + PAD
  constexpr int ROWV = (W + 2 * PADA) / 4;     // 16-byte global vectors per row
  constexpr int NS1 = (H / CH) * K, NS2 = H / CH;

  __shared__ __attribute__((aligned(16))) uint16_t xt[NCOL * PITCH];
  __shared__ __attribute__((aligned(16))) uint16_t acts[W * PITCH];
  __shared__ __attribute__((aligned(16))) float msk[128];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int T = p.T;
  const uint32_t ld = (uint32_t)p.ld;
  const int b = (int)blockIdx.x / p.ntile;
  const int t0 = ((int)blockIdx.x - b * p.ntile) * W;
  const int64_t boff = (int64_t)b * p.bstride;

  // ---- staging: h tile -> bf16, channel-contiguous -------------------------------------------------------------------
  {
    const float* __restrict__ xb = p.x + boff;
    if (tid < W / 4) {
      const int t = t0 + 4 * tid;
      f32x4 m = {0.f, 0.f, 0.f, 0.f};
      if (t < T) m = *reinterpret_cast<const f32x4*>(p.mask + (int64_t)b * p.mask_bstride + t);
#pragma unroll
      for (int r = 0; r < 4; ++r) m[r] = t + r < T ? m[r] : 0.f;
      *reinterpret_cast<f32x4*>(msk + 4 * tid) = m;
    }
    // a wave covers 16 row pairs x 4 vectors: 64-byte runs of a row in global memory, 64 distinct banks in LDS
    constexpr int VG = (ROWV + 3) / 4;         // groups of 4 vectors per row
    constexpr int NGRP = (H / 32) * VG;        // (16 row pairs, 4 vectors) groups
#pragma unroll 2
    for (int grp = wave; grp < NGRP; grp += NW) {
      const int rg = grp / VG, vg = grp - rg * VG;
      const int rp = 16 * rg + (lane & 15);    // row pair: channels 2 rp, 2 rp + 1
      const int c4 = 4 * vg + (lane >> 4);
      if (c4 < ROWV) {
        const int t = t0 - PADA + 4 * c4;      // multiple of 4: a vector is wholly < 0 or >= 0
        f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = {0.f, 0.f, 0.f, 0.f};
        if (t >= 0 && t < T) {
          const float* src = xb + (uint32_t)(2 * rp) * ld + (uint32_t)t;
          v0 = *reinterpret_cast<const f32x4*>(src);
          v1 = *reinterpret_cast<const f32x4*>(src + ld);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int col = 4 * c4 + e - (PADA - PAD);         // LDS column: global column t0 - PAD + col
          if (col >= 0 && col < NCOL) {
            const bool ok = t + e < T;                       // ragged T: a vector may straddle the row end
            const uint32_t w = ok ? pack_bf16x2(v0[e], v1[e]) : 0u;
            *reinterpret_cast<uint32_t*>(xt + col * PITCH + 2 * rp) = w;
          }
        }
      }
    }
  }

  const int g = lane >> 4, c = lane & 15;      // k group (8 consecutive k) / index inside the fragment
  const int frag0 = wave * RB;
  const int row0 = 16 * frag0;

  // ---- phase 1: gate rows = W_in * h ---------------------------------------------------------------------------------
  f32x4 acc[RB][NB];
  {
    const float* __restrict__ cb = p.cond ? p.cond + (int64_t)b * p.cond_bstride : nullptr;
#pragma unroll
    for (int i = 0; i < RB; ++i) {
      f32x4 bv = *reinterpret_cast<const f32x4*>(p.b_in + row0 + 16 * i + 4 * g);
      if (cb) bv += *reinterpret_cast<const f32x4*>(cb + row0 + 16 * i + 4 * g);
#pragma unroll
      for (int j = 0; j < NB; ++j) acc[i][j] = bv;
    }
  }
  // packing: [wave][k-step][row fragment][lane] x 8 bf16, one zero k-step closing every wave's stream
  const u32x4* __restrict__ w1 = reinterpret_cast<const u32x4*>(p.w_in) + (size_t)wave * ((NS1 + 1) * RB * 64) + lane;
  u32x4 a_cur[RB], a_nxt[RB];
#pragma unroll
  for (int i = 0; i < RB; ++i) a_cur[i] = w1[i * 64];
  __syncthreads();   // (h tile in LDS)
  {
    const uint16_t* xl = xt + c * PITCH + 8 * g;
#pragma unroll 1
    for (int chunk = 0; chunk < H / CH; ++chunk) {
#pragma unroll
      for (int tap = 0; tap < K; ++tap) {
        const int s = chunk * K + tap;
#pragma unroll
        for (int i = 0; i < RB; ++i) a_nxt[i] = w1[(size_t)(s + 1) * (RB * 64) + i * 64];
        u32x4 bv[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j)
          bv[j] = *reinterpret_cast<const u32x4*>(xl + (16 * j + tap) * PITCH + chunk * CH);
#pragma unroll
        for (int i = 0; i < RB; ++i)
#pragma unroll
          for (int j = 0; j < NB; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(a_cur[i]), as_bf16x8(bv[j]), acc[i][j], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < RB; ++i) a_cur[i] = a_nxt[i];
      }
    }
  }

  // ---- gate: rows 4g + {0, 1, 2, 3} of fragment q = tanh rows of channels 8q+g, 8q+g+4, then their sigmoid rows ------
  const u32x4* __restrict__ w2 = reinterpret_cast<const u32x4*>(p.w_rs) + (size_t)wave * ((NS2 + 1) * RB * 64) + lane;
  const bool skip_rows = row0 >= H;                 // rows >= H of the res/skip conv
  const bool idle2 = p.last && !skip_rows;          // last layer: no residual rows (modules.py:203-207)
  if (!idle2) {
#pragma unroll
    for (int i = 0; i < RB; ++i) a_cur[i] = w2[i * 64];   // first res/skip record in flight during the gate
  }
  const float* __restrict__ src =
      (skip_rows ? p.skip + boff + (size_t)(row0 - H) * ld : p.x + boff + (size_t)row0 * ld) + (size_t)c * ld;
  const bool zero_src = skip_rows && p.first;       // first layer initialises the skip accumulator
#pragma unroll
  for (int i = 0; i < RB; ++i) {
    const int ch = 8 * (frag0 + i) + g;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const f32x4 v = acc[i][j];
      const uint32_t pr = pack_bf16x2(wn_gate(v[0], v[2]), wn_gate(v[1], v[3]));
      acts[(16 * j + c) * PITCH + ch] = (uint16_t)pr;
      acts[(16 * j + c) * PITCH + ch + 4] = (uint16_t)(pr >> 16);
      if (!idle2) {
        // phase 2's accumulators start at h (residual rows) / skip (skip rows): the UNROUNDED fp32 state
        const int col = t0 + 16 * j + 4 * g;          // multiple of 4; col < T => col + 3 < ld (ld % 4 == 0)
        const uint32_t voff = (uint32_t)(16 * i) * ld + (uint32_t)(col < T ? col : 0);
        if (zero_src) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        else acc[i][j] = *reinterpret_cast<const f32x4*>(src + voff);
      }
    }
  }
  __syncthreads();   // (acts in LDS)
  if (idle2) return;
#pragma unroll
  for (int i = 0; i < RB; ++i) {
    const float bv = p.b_rs[row0 + 16 * i + c];
#pragma unroll
    for (int j = 0; j < NB; ++j) acc[i][j] += bv;
  }

  // ---- phase 2: res/skip rows = W_rs * acts, transposed (M = time, N = rows) -----------------------------------------
  {
    const uint16_t* al = acts + c * PITCH + 8 * g;
#pragma unroll
    for (int s = 0; s < NS2; ++s) {
#pragma unroll
      for (int i = 0; i < RB; ++i) a_nxt[i] = w2[(size_t)(s + 1) * (RB * 64) + i * 64];
      u32x4 bv[NB];
#pragma unroll
      for (int j = 0; j < NB; ++j) bv[j] = *reinterpret_cast<const u32x4*>(al + (16 * j) * PITCH + s * CH);
#pragma unroll
      for (int i = 0; i < RB; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(bv[j]), as_bf16x8(a_cur[i]), acc[i][j], 0, 0, 0);
#pragma unroll
      for (int i = 0; i < RB; ++i) a_cur[i] = a_nxt[i];
    }
  }

  // ---- epilogue: h' = (h + res) * mask -> out;  skip + rs -> skip ----------------------------------------------------
  {
    float* __restrict__ dst =
        (skip_rows ? p.skip + boff + (size_t)(row0 - H) * ld : p.out + boff + (size_t)row0 * ld) + (size_t)c * ld;
    if (t0 + W <= T) {                               // whole tile inside the utterance: straight-line 16-byte stores
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        f32x4 mk = {1.f, 1.f, 1.f, 1.f};
        if (!skip_rows) mk = *reinterpret_cast<const f32x4*>(msk + 16 * j + 4 * g);
#pragma unroll
        for (int i = 0; i < RB; ++i)
          *reinterpret_cast<f32x4*>(dst + (uint32_t)(16 * i) * ld + (uint32_t)(t0 + 16 * j + 4 * g)) = acc[i][j] * mk;
      }
    } else {                                         // ragged last tile: columns >= T are never written
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const int col = t0 + 16 * j + 4 * g;
        if (col >= T) continue;
        f32x4 mk = {1.f, 1.f, 1.f, 1.f};
        if (!skip_rows) mk = *reinterpret_cast<const f32x4*>(msk + 16 * j + 4 * g);
#pragma unroll
        for (int i = 0; i < RB; ++i) {
          const f32x4 v = acc[i][j] * mk;
          float* o = dst + (uint32_t)(16 * i) * ld + (uint32_t)col;
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (col + r < T) o[r] = v[r];
        }
      }
    }
  }
}

typedef void (*wn_kernel_fn)(const ov_wn_layer_params);

static wn_kernel_fn kernel_for(int nb) {
  switch (nb) {
    case 1: return wn_layer_bf16_kernel<5, 192, 1>;
    case 2: return wn_layer_bf16_kernel<5, 192, 2>;
    case 3: return wn_layer_bf16_kernel<5, 192, 3>;
    case 4: return wn_layer_bf16_kernel<5, 192, 4>;
    case 5: return wn_layer_bf16_kernel<5, 192, 5>;
    case 6: return wn_layer_bf16_kernel<5, 192, 6>;
    case 7: return wn_layer_bf16_kernel<5, 192, 7>;
    case 8: return wn_layer_bf16_kernel<5, 192, 8>;
  }
  return nullptr;
}

}  // namespace ovkwb

using namespace ovkwb;

#if !defined(__HIP_DEVICE_COMPILE__)
#include <atomic>

// Compute units of the current device (cached per ordinal).
static int wnb_compute_units() {
  static std::atomic<int> cache[16];
  int dev = 0;
  const bool known = hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 16;
  if (known) {
    const int v = cache[dev].load(std::memory_order_relaxed);
    if (v > 0) return v;
  }
  int cus = 256;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
  if (known) cache[dev].store(cus, std::memory_order_relaxed);
  return cus;
}

extern "C" {

int ov_wn_layer_bf16_supported(int H, int K) { return (H == 192 && K == 5) ? 1 : 0; }

size_t ov_wn_bf16_pack_size(int rows, int cin, int K) {
  if (rows <= 0 || cin <= 0 || K <= 0 || rows % (16 * NW) || cin % CH) return 0;
  const size_t rb = rows / (16 * NW), ns = (size_t)(cin / CH) * K;
  return (size_t)NW * (ns + 1) * rb * 64 * 8;
}

// [wave][k-step][row fragment][lane] x 8 bf16; wave w = rows 16*rb*w ..; k-step s = (chunk s / K, tap s % K); a lane
// holds row (lane & 15) of its fragment and channels 32 chunk + 8 (lane >> 4) .. + 7 of that tap.
int ov_wn_bf16_pack(const float* w, int rows, int cin, int K, uint16_t* dst) {
  const size_t n = ov_wn_bf16_pack_size(rows, cin, K);
  if (!w || !dst || n == 0) return OV_E_BADARG;
  const int rb = rows / (16 * NW), ns = (cin / CH) * K;
  std::memset(dst, 0, n * sizeof(uint16_t));
  auto to_bf16 = [](float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);   // NaN
    u += 0x7fffu + ((u >> 16) & 1u);                                            // round to nearest even
    return (uint16_t)(u >> 16);
  };
  for (int wv = 0; wv < NW; ++wv)
    for (int s = 0; s < ns; ++s)
      for (int i = 0; i < rb; ++i)
        for (int l = 0; l < 64; ++l)
          for (int e = 0; e < 8; ++e) {
            const int chunk = s / K, tap = s % K;
            const int ci = chunk * CH + 8 * (l >> 4) + e;
            const int row = (wv * rb + i) * 16 + (l & 15);
            dst[((((size_t)wv * (ns + 1) + s) * rb + i) * 64 + l) * 8 + e] = to_bf16(w[((size_t)row * cin + ci) * K + tap]);
          }
  return OV_OK;
}

int ov_wn_layer_bf16_tile(int B, int T, int width) {
  if (width > 0) return (width % 16 == 0 && width <= 128) ? width : 0;
  if (width < 0 || B <= 0 || T <= 0) return 0;
  // Equal tiles of 16*nb columns per utterance; the launch runs ceil(tiles / CUs) rounds of one tile per CU, a tile
  // costing its width plus a fixed part (the 737 KB weight stream, staging, gate, epilogue: ~32 columns' worth).
  const int cus = wnb_compute_units();
  long best = -1;
  int best_nb = 8;
  for (int nb = 8; nb >= 1; --nb) {
    const long tiles = (long)B * ((T + 16 * nb - 1) / (16 * nb));
    const long cost = ((tiles + cus - 1) / cus) * (16 * nb + 32);
    if (best < 0 || cost < best) { best = cost; best_nb = nb; }
  }
  return 16 * best_nb;
}

int ov_wn_layer_bf16(const ov_wn_layer_params* pin, ov_stream_t stream) {
  if (!pin || !pin->x || !pin->out || !pin->skip || !pin->w_in || !pin->b_in || !pin->w_rs || !pin->b_rs || !pin->mask)
    return OV_E_BADARG;
  ov_wn_layer_params q = *pin;
  if (q.B <= 0 || q.T <= 0 || q.H <= 0 || q.K <= 0) return OV_E_BADARG;
  if (!ov_wn_layer_bf16_supported(q.H, q.K)) return OV_E_UNSUPPORTED;
  if (q.ld == 0) q.ld = q.T;
  if (q.ld < q.T || q.out == q.x || q.dbg) return OV_E_BADARG;
  if (q.mask_bstride == 0) q.mask_bstride = q.ld;
  if ((int64_t)q.H * q.ld > UINT32_MAX / 2) return OV_E_BADARG;   // per-utterance offsets are 32-bit in the kernel
  if ((q.ld % 4) || (q.bstride % 4) || (q.cond_bstride % 4) || (reinterpret_cast<uintptr_t>(q.x) & 15) ||
      (reinterpret_cast<uintptr_t>(q.w_in) & 15) || (reinterpret_cast<uintptr_t>(q.w_rs) & 15) ||
      (reinterpret_cast<uintptr_t>(q.b_in) & 15) || (reinterpret_cast<uintptr_t>(q.b_rs) & 15) ||
      (q.cond && (reinterpret_cast<uintptr_t>(q.cond) & 15)) || (reinterpret_cast<uintptr_t>(q.out) & 15) ||
      (reinterpret_cast<uintptr_t>(q.skip) & 15))
    return OV_E_ALIGN;
  // the mask is read as 16-byte vectors of 4 columns starting at multiples of 4, as by ov_wn_layer_f32
  if ((reinterpret_cast<uintptr_t>(q.mask) & 15) || (q.mask_bstride % 4)) return OV_E_ALIGN;
  if (q.mask_bstride < (int64_t)((q.T + 3) / 4) * 4) return OV_E_BADARG;
  const int width = ov_wn_layer_bf16_tile(q.B, q.T, q.width);
  if (width == 0) return OV_E_BADARG;
  q.width = width;
  q.ntile = (q.T + width - 1) / width;
  if ((int64_t)q.B * q.ntile > INT32_MAX) return OV_E_BADARG;
  q.acts = nullptr;
  q.row_split = 0;
  hipLaunchKernelGGL(kernel_for(width / 16), dim3((unsigned)(q.B * q.ntile)), dim3(64 * NW), 0,
                     static_cast<hipStream_t>(stream), q);
  return hipGetLastError() == hipSuccess ? OV_OK : OV_E_LAUNCH;
}

}  // extern "C"
#endif
