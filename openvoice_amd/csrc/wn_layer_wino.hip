// One WaveNet layer in ONE launch with the k = 5 gate conv in the WINOGRAD domain (reference: openvoice/modules.py:192-209,
// commons.py:100-107) -- the semantics of ov_wn_layer_f32 (wn_layer.hip), 0.55 of its gate-conv multiplies:
//
//   x_in = in_layer(h) + cond;  acts = tanh(x_in[:H]) * sigmoid(x_in[H:]);  rs = res_skip(acts)
//   h'   = (h + rs[:H]) * mask;  skip += rs[H:]                              (last layer: H rows, all skip)
//
// Phase 1.  The 5 taps are laid out as two F(4, 3) groups (w0 w1 w2)(w3 w4 0) (conv1d_wino.h: wino_lead / wino_trail); the
// trailing zero tap makes the point-infinity weight of group 1 identically zero (wino_zero_product), so a tile of 4 output
// columns costs 11 products per (row, input channel) where the direct form needs 20.  The products of both groups and all
// input channels accumulate in the transform domain, one accumulator per interpolation point (0, 1, -1, 2, -2, infinity):
//
//   x_in[co][4j + i] = sum_p At[i][p] Y_p[co][j],   Y_p[co][j] = sum_{g, ci} U_p[co][g][ci] V_p[g][ci][j]
//   U_p[co][g][ci]   = sum_k G[p][k] w[co][ci][3g + k]          (float64 at pack time: ov_wn_wino_pack_f32)
//   V_p[g][ci][j]    = sum_m Bt[p][m] h[ci][4j + 3g + m - 2]    (VALU, from global memory into LDS)
//
// bias + cond is constant along time and enters through the point-1 accumulator (At column (1, 1, 1, 1)).
//
// One workgroup = 8 waves (two per SIMD) = one tile of 32 F(4, 3) tiles = 128 columns x ALL 2H gate rows, so `acts` stays
// in LDS.  The point GEMMs run on v_mfma_f32_16x16x4_f32: wave w owns gate rows 48 w .. 48 w + 47 as 3 row fragments x 2
// tile fragments x 6 points x 4 registers = 144 accumulator registers -- with the 32x32x2 form the 12 row fragments of 32
// would have to sit three to a wave to load the four SIMDs evenly (288 registers: one wave per SIMD, nobody to cover its
// waits), or one to a wave on 12 waves (no registers left for operands at four waves per SIMD).  Same rate, 64
// flop/cycle/SIMD.  The gate row order is that of ov_wn_layer_f32 (a lane's 4 accumulator rows are both halves of two
// gates), so b_in / cond are shared with the direct kernel.
//
// There are NO helper waves: the input transform of a (channel, tile) is shared by all 24 row fragments -- 23 VALU
// instructions per 264 MFMAs' worth of work -- so every wave transforms one (channel, tile) per 16-channel chunk between
// its MFMA streams.  Per chunk: transform chunk c + 1 (requested from global memory a chunk earlier, straight into
// registers: 8 floats per lane, no raw LDS tile) into V[(c + 1) & 1], request chunk c + 2, run the 4 x 66 MFMAs of chunk c
// from V[c & 1], ONE s_barrier.  A operands (U) stream from L2 in fragment order and are refilled in place, a row fragment
// at a time, a whole super-step (4 channels x 11 products) ahead; B operands come from LDS (conflict-free ds_read_b32: odd
// channel rows are stored with their tile halves swapped) and are refilled in place behind the last row fragment.
//
// Phase 2 is the direct 1x1 res/skip GEMM out of the `acts` LDS tile, transposed so that h / skip are touched 16 bytes at a
// time -- the form and the weight packing (ov_wn_pack_f32) of wn_layer.hip at a 128-column tile.
#include <hip/hip_runtime.h>

#include "conv1d_wino.h"
#include "openvoice_amd.h"

namespace ovkwn {

using ovk::f32x2;
using ovk::f32x4;
using ovkw::lds_barrier;
using ovkw::wino_products;
using ovkw::wino_zero_product;

constexpr int K = 5, H = 192;
static_assert(ovkw::wino_lead(K) == 0 && ovkw::wino_trail(K) == 1 && wino_products(K) == 11, "(w0 w1 w2)(w3 w4 0)");
constexpr int NWAVE = 8;
constexpr int RB = 2 * H / (16 * NWAVE);   // 16-row fragments per wave (both phases): 3
constexpr int NF = 2;                      // 16-tile fragments per wave in phase 1
constexpr int NT = 16 * NF;                // F(4, 3) tiles per workgroup
constexpr int W = 4 * NT;                  // columns per workgroup: 128
constexpr int NB = W / 16;                 // 16-column fragments of phase 2
constexpr int CI = 16;                     // input channels per chunk = per s_barrier
constexpr int NCH = H / CI;
constexpr int NSLOT = wino_products(K);    // V slots: group 0 points 0..5, group 1 points 0..4
constexpr int SLOT = CI * NT;              // floats per slot
constexpr int VBUF = NSLOT * SLOT;
constexpr int NU = H / 4;                  // super-steps (4 input channels x both groups) of the k-loop
constexpr int XS = 144;                    // acts row stride in floats (wn_layer.hip WNL_XS)
constexpr int NR2 = H / 16;                // res/skip weight records (4 k-steps each)
static_assert(NWAVE * 64 == CI * NT, "one (channel, tile) per lane and chunk");

// tanh(t) * sigmoid(s) as in wn_layer.hip: two v_exp_f32 and one v_rcp_f32
__device__ __forceinline__ float gate(float t, float s) {
  const float a = __builtin_amdgcn_exp2f(fabsf(t) * -2.8853900817779268f);
  const float e = __builtin_amdgcn_exp2f(s * -1.4426950408889634f);
  const float r = __builtin_amdgcn_rcpf((1.f + a) * (1.f + e));
  return copysignf((1.f - a) * r, t);
}

__global__ __launch_bounds__(64 * NWAVE, 2) void wn_layer_wino_kernel(const ov_wn_layer_params p) {
  __shared__ __attribute__((aligned(16))) float Vs[2 * VBUF];
  __shared__ __attribute__((aligned(16))) float acts[H * XS];
  __shared__ __attribute__((aligned(16))) float msk[W];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int T = p.T;
  const uint32_t ld = (uint32_t)p.ld;
  const int b = (int)blockIdx.x / p.ntile;
  const int t0 = ((int)blockIdx.x - b * p.ntile) * W;
  const int g = lane >> 4, c = lane & 15;   // operand k-row / fragment column; accumulator rows 4g .. 4g + 3
  const int64_t boff = (int64_t)b * p.bstride;

  if (tid < W / 4) {                        // visible after the first chunk barrier
    const int t = t0 + 4 * tid;
    f32x4 m = {0.f, 0.f, 0.f, 0.f};
    if (t < T) m = *reinterpret_cast<const f32x4*>(p.mask + (int64_t)b * p.mask_bstride + t);
#pragma unroll
    for (int r = 0; r < 4; ++r) m[r] = t + r < T ? m[r] : 0.f;
    *reinterpret_cast<f32x4*>(msk + 4 * tid) = m;
  }

  // ---- input transform: this lane's (channel of the chunk, tile) ------------------------------------------------------
  const int tt = tid & (NT - 1), cil = tid / NT;
  const int tc = t0 + 4 * tt;               // the tile's first output column; its inputs are columns tc - 2 .. tc + 5
  const float* __restrict__ xrow = p.x + boff + (size_t)cil * ld;
  // columns outside [0, T) are zeros ('same' padding; beyond T the rows hold whatever the caller's buffer holds)
  uint32_t okm = 0;
#pragma unroll
  for (int m = 0; m < 8; ++m) okm |= (tc - 2 + m >= 0 && tc - 2 + m < T ? 1u : 0u) << m;
  const uint32_t offa = (okm & 1u) ? (uint32_t)(tc - 2) : 0u;            // (a vector starts inside the row or is not used)
  const uint32_t offb = (okm & 4u) ? (uint32_t)tc : 0u;
  const uint32_t offc = (okm & 64u) ? (uint32_t)(tc + 4) : 0u;
  f32x2 sa, sc;
  f32x4 sb;
  auto request = [&](int chunk) {
    const float* r = xrow + (size_t)(chunk * CI) * ld;
    sa = *reinterpret_cast<const f32x2*>(r + offa);
    sb = *reinterpret_cast<const f32x4*>(r + offb);
    sc = *reinterpret_cast<const f32x2*>(r + offc);
  };
  // V[slot][channel][tile ^ 16 (channel & 1)]: the two k-rows a half-wave reads as B operands fall into disjoint banks
  const int vdst = cil * NT + (tt ^ ((cil & 1) << 4));
  auto transform = [&](int buf) {
    float* v = Vs + buf * VBUF + vdst;
    float d[9];
    d[0] = sa[0]; d[1] = sa[1]; d[2] = sb[0]; d[3] = sb[1]; d[4] = sb[2]; d[5] = sb[3]; d[6] = sc[0]; d[7] = sc[1];
#pragma unroll
    for (int m = 0; m < 8; ++m) d[m] = ((okm >> m) & 1u) ? d[m] : 0.f;
    d[8] = 0.f;                             // read by the dropped product only
    ovkw::static_for<0, 2>([&](auto gc) {
      constexpr int gg = decltype(gc)::value;
      const float d0 = d[3 * gg], d1 = d[3 * gg + 1], d2 = d[3 * gg + 2], d3 = d[3 * gg + 3], d4 = d[3 * gg + 4],
                  d5 = d[3 * gg + 5];
      // Bt d, points 0, 1, -1, 2, -2, infinity (the operation order of conv1d_wino.h)
      const float t1 = __builtin_fmaf(-4.f, d2, d4), t2 = __builtin_fmaf(-4.f, d1, d3), t3 = d4 - d2, t4 = d3 - d1;
      v[(6 * gg + 0) * SLOT] = __builtin_fmaf(4.f, d0, __builtin_fmaf(-5.f, d2, d4));
      v[(6 * gg + 1) * SLOT] = t1 + t2;
      v[(6 * gg + 2) * SLOT] = t1 - t2;
      v[(6 * gg + 3) * SLOT] = __builtin_fmaf(2.f, t4, t3);
      v[(6 * gg + 4) * SLOT] = __builtin_fmaf(-2.f, t4, t3);
      if constexpr (!wino_zero_product(K, gg, 5)) v[(6 * gg + 5) * SLOT] = __builtin_fmaf(4.f, d1, __builtin_fmaf(-5.f, d3, d5));
    });
  };

  // ---- phase 1: Y_p = U_p V_p ------------------------------------------------------------------------------------------
  const int frag0 = wave * RB, row0 = 16 * frag0;
  f32x4 acc[RB][NF][6];
  {
    const float* __restrict__ cb = p.cond ? p.cond + (int64_t)b * p.cond_bstride : nullptr;
#pragma unroll
    for (int i = 0; i < RB; ++i) {
      f32x4 bv = *reinterpret_cast<const f32x4*>(p.b_in + row0 + 16 * i + 4 * g);
      if (cb) bv += *reinterpret_cast<const f32x4*>(cb + row0 + 16 * i + 4 * g);
#pragma unroll
      for (int f = 0; f < NF; ++f)
#pragma unroll
        for (int q = 0; q < 6; ++q) acc[i][f][q] = q == 1 ? bv : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
  // weight stream: [wave][super-step][row fragment][3][lane] x 4 floats = the 11 (+ 1 zero) U values of (row, channel
  // 4u + g); one zero super-step closes the stream
  const f32x4* __restrict__ w1 = reinterpret_cast<const f32x4*>(p.w_in) + (size_t)wave * (NU * RB * 3 * 64) + lane;
  f32x4 a_cur[RB][3];
#pragma unroll
  for (int i = 0; i < RB; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) a_cur[i][j] = w1[(i * 3 + j) * 64];
  int voff[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) voff[f] = g * NT + 16 * (f ^ (g & 1)) + c;

  request(0);
  transform(0);
  request(1);
  lds_barrier();
#pragma unroll 1
  for (int chunk = 0; chunk < NCH; ++chunk) {
    if (chunk + 1 < NCH) transform((chunk + 1) & 1);
    if (chunk + 2 < NCH) request(chunk + 2);
    const float* vb = Vs + (chunk & 1) * VBUF;
    float bq[NF][NSLOT];
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
      for (int s = 0; s < NSLOT; ++s) bq[f][s] = vb[s * SLOT + voff[f]];
    const f32x4* __restrict__ wn = w1 + (size_t)(chunk * (CI / 4) + 1) * (RB * 3 * 64);   // the next super-step's records
#pragma unroll
    for (int ul = 0; ul < CI / 4; ++ul) {
#pragma unroll
      for (int i = 0; i < RB; ++i) {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < NSLOT; ++s) {
#pragma unroll
          for (int f = 0; f < NF; ++f)
            acc[i][f][s % 6] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_cur[i][s >> 2][s & 3], bq[f][s], acc[i][f][s % 6], 0, 0, 0);
          if (i == RB - 1 && ul + 1 < CI / 4) {
#pragma unroll
            for (int f = 0; f < NF; ++f) bq[f][s] = vb[s * SLOT + (ul + 1) * 4 * NT + voff[f]];
          }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 3; ++j) a_cur[i][j] = wn[(size_t)ul * (RB * 3 * 64) + (i * 3 + j) * 64];
      }
    }
    lds_barrier();   // V[(chunk + 1) & 1] complete; V[chunk & 1] free
  }

  // ---- At, gate -> acts ---------------------------------------------------------------------------------------------------
#pragma unroll
  for (int i = 0; i < RB; ++i) {
    const int ch = 8 * (frag0 + i) + g;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      f32x4 o[4];                           // o[row r of the lane][column e of the tile]
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float y0 = acc[i][f][0][r], y1 = acc[i][f][1][r], y2 = acc[i][f][2][r], y3 = acc[i][f][3][r],
                    y4 = acc[i][f][4][r], y5 = acc[i][f][5][r];
        const float s1 = y1 + y2, e1 = y1 - y2, s2 = y3 + y4, e2 = y3 - y4;
        o[r][0] = (y0 + s1) + s2;
        o[r][1] = __builtin_fmaf(2.f, e2, e1);
        o[r][2] = __builtin_fmaf(4.f, s2, s1);
        o[r][3] = __builtin_fmaf(8.f, e2, e1) + y5;
      }
      f32x4 ga, gb;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        ga[e] = gate(o[0][e], o[2][e]);
        gb[e] = gate(o[1][e], o[3][e]);
      }
      *reinterpret_cast<f32x4*>(acts + ch * XS + 64 * f + 4 * c) = ga;
      *reinterpret_cast<f32x4*>(acts + (ch + 4) * XS + 64 * f + 4 * c) = gb;
    }
  }

  // ---- phase 2: res/skip rows = W_rs acts (transposed: a lane holds 4 consecutive columns of one row) ---------------------
  const f32x4* __restrict__ w2 = reinterpret_cast<const f32x4*>(p.w_rs) + (size_t)wave * ((NR2 + 1) * RB * 64);
  const bool skip_rows = row0 >= H;
  const bool idle2 = p.last && !skip_rows;          // last layer: no residual rows (modules.py:203-207)
  f32x4 a2[RB], a2n[RB];
  f32x4 acc2[RB][NB];
  if (!idle2) {
#pragma unroll
    for (int i = 0; i < RB; ++i) a2[i] = w2[i * 64 + lane];
    const float* __restrict__ src =
        (skip_rows ? p.skip + boff + (size_t)(row0 - H) * ld : p.x + boff + (size_t)row0 * ld) + (size_t)c * ld;
    const bool zero_src = skip_rows && p.first;     // first layer initialises the skip accumulator
#pragma unroll
    for (int i = 0; i < RB; ++i)
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const int col = t0 + 16 * j + 4 * g;        // multiple of 4; col < T => col + 3 < ld (ld % 4 == 0)
        const uint32_t voff2 = (uint32_t)(16 * i) * ld + (uint32_t)(col < T ? col : 0);
        if (zero_src) acc2[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        else acc2[i][j] = *reinterpret_cast<const f32x4*>(src + voff2);
      }
  }
  __syncthreads();   // acts complete
  if (idle2) return;
#pragma unroll
  for (int i = 0; i < RB; ++i) {
    const float bv = p.b_rs[row0 + 16 * i + c];
#pragma unroll
    for (int j = 0; j < NB; ++j) acc2[i][j] += bv;
  }
  {
    const float* al = acts + g * XS + c;
    float bcur[NB], bnxt[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) bcur[j] = al[16 * j];
#pragma unroll 1
    for (int grp = 0; grp < NR2 / 4; ++grp) {       // 16 k-steps (64 channels) per iteration
      const float* ag = al + grp * 64 * XS;
      const f32x4* __restrict__ wg = w2 + (size_t)grp * (4 * RB * 64);
#pragma unroll
      for (int m = 0; m < 16; ++m) {
        const int u = m & 3;
        if (u == 0) {                               // the record after the last one is zero padding
#pragma unroll
          for (int i = 0; i < RB; ++i) a2n[i] = (wg + (size_t)(m / 4 + 1) * (RB * 64))[i * 64 + lane];
        }
        {
          const int s = (m + 1) % 16;               // past the end it re-reads row 4g of the last group
          const float* an = (m + 1 < 16) ? ag : (grp + 1 < NR2 / 4 ? ag + 64 * XS : ag);
#pragma unroll
          for (int j = 0; j < NB; ++j) bnxt[j] = an[4 * s * XS + 16 * j];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < RB; ++i)
#pragma unroll
          for (int j = 0; j < NB; ++j)
            acc2[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(bcur[j], a2[i][u], acc2[i][j], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < NB; ++j) bcur[j] = bnxt[j];
        if (u == 3) {
#pragma unroll
          for (int i = 0; i < RB; ++i) a2[i] = a2n[i];
        }
      }
    }
  }

  // ---- epilogue: h' = (h + res) * mask -> out;  skip + rs -> skip ---------------------------------------------------------
  float* __restrict__ dst =
      (skip_rows ? p.skip + boff + (size_t)(row0 - H) * ld : p.out + boff + (size_t)row0 * ld) + (size_t)c * ld;
  if (t0 + W <= T) {                                // whole tile inside the utterance: straight-line 16-byte stores
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      f32x4 mk = {1.f, 1.f, 1.f, 1.f};
      if (!skip_rows) mk = *reinterpret_cast<const f32x4*>(msk + 16 * j + 4 * g);
#pragma unroll
      for (int i = 0; i < RB; ++i)
        *reinterpret_cast<f32x4*>(dst + (uint32_t)(16 * i) * ld + (uint32_t)(t0 + 16 * j + 4 * g)) = acc2[i][j] * mk;
    }
  } else {                                          // ragged last tile: columns >= T are never written
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int col = t0 + 16 * j + 4 * g;
      if (col >= T) continue;
      f32x4 mk = {1.f, 1.f, 1.f, 1.f};
      if (!skip_rows) mk = *reinterpret_cast<const f32x4*>(msk + 16 * j + 4 * g);
#pragma unroll
      for (int i = 0; i < RB; ++i) {
        const f32x4 v = acc2[i][j] * mk;
        float* o = dst + (uint32_t)(16 * i) * ld + (uint32_t)col;
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (col + r < T) o[r] = v[r];
      }
    }
  }
}

}  // namespace ovkwn

using namespace ovkwn;

#if !defined(__HIP_DEVICE_COMPILE__)
extern "C" {

int ov_wn_layer_wino_tile(void) { return W; }

size_t ov_wn_wino_pack_size(int rows, int cin, int Kw) {
  if (rows != 2 * H || cin != H || Kw != K) return 0;
  return ((size_t)NWAVE * NU + 1) * RB * 3 * 64 * 4;
}

// [wave][super-step u][row fragment i][j][lane] x 4: element 4j + e = slot s of row 16 (3 wave + i) + (lane & 15) and input
// channel 4u + (lane >> 4); slot s < 6: group 0 point s, 6 <= s < 11: group 1 point s - 6, s = 11: zero.
int ov_wn_wino_pack_f32(const float* w, int rows, int cin, int Kw, float* dst) {
  const size_t n = ov_wn_wino_pack_size(rows, cin, Kw);
  if (!w || !dst || n == 0) return OV_E_BADARG;
  static const double Gm[6][3] = {{1.0 / 4, 0, 0},           {-1.0 / 6, -1.0 / 6, -1.0 / 6}, {-1.0 / 6, 1.0 / 6, -1.0 / 6},
                                  {1.0 / 24, 1.0 / 12, 1.0 / 6}, {1.0 / 24, -1.0 / 12, 1.0 / 6}, {0, 0, 1}};
  for (size_t i = 0; i < n; ++i) dst[i] = 0.f;
  for (int wv = 0; wv < NWAVE; ++wv)
    for (int u = 0; u < NU; ++u)
      for (int i = 0; i < RB; ++i)
        for (int l = 0; l < 64; ++l)
          for (int s = 0; s < NSLOT; ++s) {
            const int grp = s / 6, pt = s % 6;
            const int row = (wv * RB + i) * 16 + (l & 15), ci = 4 * u + (l >> 4);
            double v = 0;
            for (int k = 0; k < 3; ++k) {
              const int tap = 3 * grp + k - ovkw::wino_lead(K);
              if (tap >= 0 && tap < K) v += Gm[pt][k] * (double)w[((size_t)row * cin + ci) * K + tap];
            }
            dst[(((((size_t)wv * NU + u) * RB + i) * 3 + s / 4) * 64 + l) * 4 + s % 4] = (float)v;
          }
  return OV_OK;
}

int ov_wn_layer_wino_f32(const ov_wn_layer_params* pin, ov_stream_t stream) {
  if (!pin || !pin->x || !pin->out || !pin->skip || !pin->w_in || !pin->b_in || !pin->w_rs || !pin->b_rs || !pin->mask)
    return OV_E_BADARG;
  ov_wn_layer_params q = *pin;
  if (q.B <= 0 || q.T <= 0 || q.H <= 0 || q.K <= 0) return OV_E_BADARG;
  if (q.H != H || q.K != K) return OV_E_UNSUPPORTED;
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
  if ((reinterpret_cast<uintptr_t>(q.mask) & 15) || (q.mask_bstride % 4)) return OV_E_ALIGN;
  if (q.mask_bstride < (int64_t)((q.T + 3) / 4) * 4) return OV_E_BADARG;
  if (q.width != 0 && q.width != W) return OV_E_BADARG;
  q.width = W;
  q.ntile = (q.T + W - 1) / W;
  if ((int64_t)q.B * q.ntile > INT32_MAX) return OV_E_BADARG;
  hipLaunchKernelGGL(wn_layer_wino_kernel, dim3((unsigned)(q.B * q.ntile)), dim3(64 * NWAVE), 0,
                     static_cast<hipStream_t>(stream), q);
  return hipGetLastError() == hipSuccess ? OV_OK : OV_E_LAUNCH;
}

}  // extern "C"
#endif
