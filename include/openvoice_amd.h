/*
 * openvoice_amd.h -- C ABI of the MI355X (gfx950) tone-colour-converter kernels.
 *
 * The reference (myshell-ai/OpenVoice) is pure Python/PyTorch and has no FFI of its own; the
 * seam these entry points replace is the ATen calls issued by
 * SynthesizerTrn.voice_conversion (reference: openvoice/models.py:492-499) and
 * SynthesizerTrn.ref_enc (openvoice/models.py:339-359).  Each function below names the
 * reference lines whose arithmetic it implements.  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *  - All tensors are fp32, contiguous along time, layout (B, C, T); pointers are DEVICE
 *    pointers unless the parameter says "host".  Caller owns every buffer; nothing here
 *    allocates, frees or synchronises.  Launches go to `stream` and return immediately.
 *  - Return value: 0 = OV_OK, negative = OV_E_* (nothing was launched).
 *  - Weights are consumed in a packed, MFMA-fragment-ordered layout produced once at load
 *    time by ov_conv1d_pack_f32 (host function).
 */
#ifndef OPENVOICE_AMD_H
#define OPENVOICE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* ov_stream_t; /* hipStream_t */

enum {
  OV_OK = 0,
  OV_E_BADARG = -1,      /* null pointer / non-positive size / inconsistent params */
  OV_E_UNSUPPORTED = -2, /* (kernel size, dilation, tile) combination not instantiated */
  OV_E_ALIGN = -3,       /* pointer/stride alignment the kernel needs is not met */
  OV_E_LAUNCH = -4       /* hipGetLastError() != hipSuccess after the launch */
};

/* Epilogues of the implicit-GEMM Conv1d kernel (v = acc + bias[row] + bias_b[b][row]). */
enum {
  /* out[b][row][t] = ((v [*mask]) [+ res] [+ add]) * scale                                   */
  OV_EPI_LINEAR = 0,
  /* WaveNet gate, reference openvoice/commons.py:100-107 via modules.py:200:
   * out[b][c][t] = tanh(v[2 tiles paired: row c]) * sigmoid(v[row c + H]); rows are packed so
   * that 32-row tile 2q holds tanh rows 32q.. and tile 2q+1 holds sigmoid rows H+32q..        */
  OV_EPI_GATE = 1,
  /* WaveNet res/skip, reference openvoice/modules.py:203-209:
   * row < split : out[b][row][t]  = (out[b][row][t] + v) * mask[b][t]      (residual, in place)
   * row >= split: out2[b][row-split][t] (+)= v     ('=' when OV_F_OUT2_INIT, else '+=')      */
  OV_EPI_RESSKIP = 2,
  /* mean-only coupling combine, reference openvoice/modules.py:441-455; x1 = res when res != NULL (indexed like
   * out), else out itself (in place):
   * forward (scale > 0): out = v*mask + x1*mask ;  reverse (scale < 0): out = (x1 - v*mask)*mask */
  OV_EPI_COUPLE = 3,
  /* posterior sample, reference openvoice/models.py:218-220 (rows paired like OV_EPI_GATE:
   * m = tile 2q, logs = tile 2q+1): out = (m*mask + res*scale*exp(logs*mask))*mask,
   * res = noise, scale = tau (or, per batch item, scale_b[b])                                  */
  OV_EPI_POSTERIOR = 4,
  /* ConvTranspose1d (k = 2*phase_s, padding phase_s/2) written as a 3-tap conv over stride-many output phases,
   * reference openvoice/models.py:279 (weights packed with row = cout*phase_s + phase):
   * out[b][cout][phase_s*t + phase] = v.
   * Every phase has exactly two non-zero taps: x[t-1], x[t] for phase < phase_s/2 and x[t], x[t+1] above.  With
   * OV_F_CONVT_GROUPED (phase_s 8 or 2 only) the rows are packed by phase group instead -- 32-row tile 2q = the
   * phases < phase_s/2, tile 2q+1 the phases >= phase_s/2 of the same output channels (phase_s 8: row-in-tile =
   * 4*(cout % 8) + phase % 4 for channels 8q..8q+7; phase_s 2: row-in-tile = cout % 32 for channels 32q..32q+31)
   * -- and the kernel skips the all-zero tap of each tile: 2/3 of the matrix work.                          */
  OV_EPI_CONVT = 5,
  /* Spectrogram magnitude, reference openvoice/mel_processing.py:61-74: rows paired like OV_EPI_GATE
   * (tile 2q = real parts of bins 32q.., tile 2q+1 = imaginary parts): out[b][f][t] = sqrt(re^2 + im^2 + scale)
   * for f < Cout (Cout need not be a multiple of 32); no bias.  Used with the even-K framing conv.           */
  OV_EPI_MAGNITUDE = 6
};

enum {
  OV_F_MASK_V = 1,    /* LINEAR: multiply v by mask[b][t] before the residual add */
  OV_F_OUT2_INIT = 2, /* RESSKIP: out2 = v instead of out2 += v (first WaveNet layer) */
  OV_F_CONVT_GROUPED = 4, /* CONVT, phase_s 8 / 2: rows packed by phase group (see OV_EPI_CONVT); M % 64 == 0 */
  OV_F_NO_XCD_MAP = 8,/* measurement knob: walk the tile list round-robin over the workgroups instead of giving each
                       * XCD (workgroup id % 8) a contiguous eighth of it; results are identical either way */
  OV_F_SCALE_B = 16   /* the struct has the trailing field scale_b (ov_conv1d_params): without this bit the library
                       * does not read it, so a caller compiled against the struct that ended at reserved0 is safe */
};

/* One Conv1d launch.  Input length == output length L ('same' padding, stride 1), as every conv
 * on the converter path (reference: openvoice/modules.py:163-171, :228-283, models.py:238,266).
 * Rows may be padded: x rows are x_ld floats apart, out/res/add/out2 rows out_ld floats apart (both
 * >= L; columns >= L are never read as data and never written).  The forward-aligned even-K conv reads
 * L + (K-1)*dil input columns (x_ld must cover them) and writes L.  16-byte staging loads are used
 * when x, x_bstride and x_ld are 16-byte aligned -- L itself may be ragged. */
typedef struct ov_conv1d_params {
  const float* x;        /* [B][>=Cin][L]; channel offset already applied to the pointer        */
  const float* w;        /* packed weights from ov_conv1d_pack_f32                              */
  const float* bias;     /* [M rounded up to 128] in packed row order; required (zeros if none) */
  const float* bias_b;   /* per-batch bias [B or 1][M] in packed row order, or NULL             */
  float* out;            /* primary output, indexed [b][row][t] with out_bstride                */
  const float* res;      /* LINEAR: residual; POSTERIOR: noise; COUPLE: x1 source; indexed like out; or NULL */
  const float* add;      /* LINEAR: second addend (MRF running sum), indexed like out; or NULL  */
  float* out2;           /* RESSKIP: skip accumulator [b][row-split][t]                         */
  const float* mask;     /* [B][>=L] sequence mask (1/0), rows mask_bstride apart, or NULL      */
  int64_t x_bstride;     /* elements between consecutive batches of x                           */
  int64_t out_bstride;
  int64_t res_bstride;
  int64_t add_bstride;
  int64_t out2_bstride;
  int64_t bias_b_bstride;/* 0 broadcasts one row to every batch item                            */
  int64_t mask_bstride;  /* 0 = L                                                               */
  int32_t B, Cin, L;
  int32_t x_ld;          /* row stride of x in floats; 0 = L                                    */
  int32_t out_ld;        /* row stride of out/res/add/out2; 0 = L (CONVT: L * phase_s)          */
  int32_t M;             /* packed rows = 32 * m_tiles, as passed to ov_conv1d_pack_f32          */
  int32_t Cout;          /* rows >= Cout (LINEAR/COUPLE/RESSKIP) are padding and never stored    */
  int32_t K, dil;        /* taps, dilation; odd K: 'same' padding (K-1)*dil/2; even K: taps t .. t+(K-1)*dil,
                          * no left padding (the framing conv of the spectrogram)                   */
  int32_t epi, flags, split, phase_s;
  int32_t tiles_per_wg;  /* 0 = the dispatcher's launch rule (persistent -- one workgroup per resident slot, striding
                          * over the tiles -- for large launches, else one tile per workgroup);
                          * n > 0 = ceil(tiles / n) workgroups; n < 0 = persistent, forced -- tests / measurement */
  int32_t tile;          /* 0 = chosen by the dispatcher; else 1 + tile id (128x128, 64x256,
                          * 32x512, 32x256) -- tuning / measurement knob                         */
  int32_t loaders;       /* loader waves per workgroup: 0 = chosen by the dispatcher, else 1/2/4            */
  int32_t chunk;         /* input channels per LDS fill: 0 = default (32 for 1x1, else 16), or 16/32 */
  float in_slope;        /* leaky-ReLU slope applied to x while staging (1.0f = identity)        */
  float scale;
  /* Length-aware work list (padded batches: ragged convert_batch, batched TTS -- reference openvoice/models.py:477-489
   * pads every utterance to the longest).  col_limit[b] * col_limit_scale = the output columns of utterance b that
   * matter (clamped to [0, L]); time tiles wholly beyond it are dropped from the work list -- their columns of out
   * are NOT written -- and the remaining tiles are dealt evenly over the workgroups.  Every computed value is
   * bit-identical to the full launch.  NULL = the whole tensor.  DEVICE pointer, int32 [B]; ignored (whole tensor)
   * when B > 256.  The caller owns the margin: the generator's receptive field is 13.3 frames, so a limit of
   * length + 16 frames leaves every valid sample unchanged (ov_frame_limits_i32). */
  const int32_t* col_limit;
  int32_t col_limit_scale; /* columns of this launch per unit of col_limit (e.g. the stage's upsampling factor) */
  int32_t reserved0;
  /* OV_EPI_POSTERIOR only, and read only when flags has OV_F_SCALE_B: one scale (tau) per batch item.  DEVICE
   * pointer, fp32 [B], 4-byte aligned, or NULL.  Non-NULL: item b computes with scale_b[b] in place of `scale` -- the
   * same expression in the same order, so item b holds the bits of a launch whose scalar `scale` is scale_b[b];
   * `scale` is then ignored.  NULL (or no OV_F_SCALE_B): `scale`, as before the field existed.  Dense like col_limit,
   * the other one-value-per-item vector (no stride: a launch over the items [b0, b1) of a larger batch passes
   * scale_b + b0).  Every other epilogue ignores the field. */
  const float* scale_b;
} ov_conv1d_params;

/* ---- host-side helpers -------------------------------------------------------------------- */

/* Number of floats ov_conv1d_pack_f32 writes for a dense [Cout][Cin][K] weight. */
size_t ov_conv1d_pack_size(int Cout, int Cin, int K);
/* Rows of the packed weight (Cout rounded up to the packing granule, 128). */
int ov_conv1d_pack_rows(int Cout);
/* Re-lay a dense row-major HOST weight w[Cout][Cin][K] into MFMA A-fragment order (HOST dst).
 * Replaces nothing in the reference; it is the load-time transform that lets the kernel read
 * every weight fragment as one coalesced 1 KiB record.  Layout: DESIGN.md "Packed weights". */
int ov_conv1d_pack_f32(const float* w, int Cout, int Cin, int K, float* dst);

/* ---- device entry points ------------------------------------------------------------------ */

/* Implicit-GEMM Conv1d on fp32 MFMA with fused prologue/epilogue.  Replaces F.conv1d /
 * F.conv_transpose1d + the surrounding elementwise ops at: openvoice/modules.py:194-209 (WN),
 * :296-306 (ResBlock1), :439-455 (coupling), openvoice/models.py:216-220 (posterior encoder),
 * :273-286 (generator conv_pre, ups, MRF). */
int ov_conv1d_f32(const ov_conv1d_params* p, ov_stream_t stream);

/* One ResBlock1 iteration in ONE launch, reference openvoice/modules.py:296-306 (the loop body of
 * ResBlock1.forward with x_mask = None, as the generator calls it at models.py:280-286):
 *   out = ( c2( lrelu( c1( lrelu(x, slope) ), slope ) ) + x [+ add] ) * scale
 * c1 = Conv1d(C, C, K, dilation dil), c2 = Conv1d(C, C, K, dilation 1), both 'same'-padded; w1 / w2 packed by
 * ov_conv1d_pack_f32(C, C, K), b1 / b2 [128] in packed row order.  `add` / `scale` carry the MRF running sum and
 * the final 1/num_kernels of models.py:282-286.  The intermediate tensor stays in LDS (sliding window along time,
 * openvoice_amd/csrc/conv1d_pair.h); results are bit-identical to the two ov_conv1d_f32 launches it replaces.
 * x / out / add are [B][C][L] with rows `ld` floats apart (0 = L), 16-byte aligned rows (ld % 4 == 0);
 * out must not alias x or add.  Instantiated for the HBM-bound stages only: ov_resblock_pair_supported(). */
typedef struct ov_respair_params {
  const float* x;
  const float* w1;
  const float* b1;
  const float* w2;
  const float* b2;
  float* out;
  const float* add;      /* or NULL */
  int64_t x_bstride, out_bstride, add_bstride;
  int32_t B, C, L;
  int32_t ld;            /* row stride of x / out / add in floats; 0 = L */
  int32_t K, dil;
  int32_t nwg;           /* 0 = one workgroup per resident slot; n > 0 forces n workgroups (tests) */
  float slope;           /* leaky-ReLU slope of both activations (modules.py:14: 0.1) */
  float scale;
  unsigned long long* dbg; /* measurement only, NULL in production: [workgroups][4 waves][8] shader-clock ticks per
                          * phase (residual issue, chunk wait, c1, h store, h barrier, c2, epilogue, tail) */
  const int32_t* col_limit; /* length-aware work list, as ov_conv1d_params.col_limit: utterance b is walked only up
                          * to column col_limit[b] * col_limit_scale (steps beyond are neither computed nor written;
                          * what is computed is bit-identical to the full launch); NULL = whole tensor; DEVICE int32 [B],
                          * B <= 256 */
  int32_t col_limit_scale;
  int32_t reserved0;
} ov_respair_params;
int ov_resblock_pair_f32(const ov_respair_params* p, ov_stream_t stream);
/* 1 when (C, K, dil) has a fused instance, else 0 (callers then issue the two ov_conv1d_f32 launches). */
int ov_resblock_pair_supported(int C, int K, int dil);

/* One WaveNet layer in ONE launch, reference openvoice/modules.py:192-209 (the loop body of WN.forward) with
 * commons.py:100-107 (fused_add_tanh_sigmoid_multiply):
 *   x_in = in_layer(x) + cond;  acts = tanh(x_in[:H]) * sigmoid(x_in[H:]);  rs = res_skip_layer(acts)
 *   out  = (x + rs[:H]) * mask;  skip = (first ? 0 : skip) + rs[H:]       (last layer: rs has H rows, all skip)
 * x / out / skip are [B][H][T] with rows ld floats apart and batch items bstride apart; out must not alias x (tiles
 * read a (K-1)/2-column halo of x from their neighbours: the caller ping-pongs two buffers).  `acts` never leaves
 * the CU (openvoice_amd/csrc/wn_layer.hip).
 * Weights: w_in = ov_wn_pack_f32 of the dense [2H][H][K] in_layer weight with its ROWS in gate order -- 16-row
 * block q holds, at row 4j + {0, 1, 2, 3}, the tanh rows of channels 8q + j and 8q + j + 4 followed by their
 * sigmoid rows (j = 0..3); b_in [2H] and cond [B or 1][2H] (cond_bstride 0 broadcasts) in the same row order.
 * w_rs = ov_wn_pack_f32 of the dense [2H][H][1] res_skip weight in natural row order (last layer: rows 0..H-1 zero,
 * the H skip rows at H..2H-1), b_rs [2H] likewise.
 * Replaces two ov_conv1d_f32 launches (OV_EPI_GATE, OV_EPI_RESSKIP); results agree with them to fp32 rounding
 * (different summation order; the gate uses v_exp_f32 / v_rcp_f32 instead of libm tanhf / expf: <= 4e-7 absolute). */
typedef struct ov_wn_layer_params {
  const float* x;
  float* out;
  float* skip;
  const float* w_in;
  const float* b_in;
  const float* cond;     /* or NULL */
  const float* w_rs;
  const float* b_rs;
  const float* mask;     /* [B][T] 0/1, rows mask_bstride apart (0 = ld); 16-byte aligned, mask_bstride a multiple
                          * of 4 and >= T rounded up to 4 (read as 16-byte vectors: OV_E_ALIGN / OV_E_BADARG otherwise) */
  int64_t bstride;       /* batch stride of x / out / skip */
  int64_t cond_bstride;
  int64_t mask_bstride;
  int32_t B, H, T;
  int32_t ld;            /* row stride in floats, multiple of 4; 0 = T */
  int32_t K;
  int32_t first;         /* 1: skip is initialised, not accumulated (layer 0) */
  int32_t last;          /* 1: the layer has no residual rows; out is not written */
  int32_t width;         /* tile width in columns: 0 = chosen by the launcher (ov_wn_layer_tile), else 16 .. 128 step 16 */
  int32_t ntile;         /* filled in by the launcher */
  int32_t row_split;     /* 0: the launcher decides; 1: always the fused launch; 3: always the row-split pair (needs acts,
                          * dbg must be NULL) */
  unsigned long long* dbg; /* measurement only, NULL in production: [workgroups][8 matrix waves][8] shader-clock ticks
                          * per phase (first chunk wait, gate-conv k-steps, chunk waits, gate, operand issue + acts
                          * barrier, res/skip k-steps, epilogue) and the wave's start tick */
  float* acts;           /* ABI 2.05; or NULL: scratch [B][H][ld] (batch stride = bstride, 16-byte aligned, not x / out /
                          * skip).  With it the launcher may run the layer as TWO launches whose workgroups each own a
                          * third of the rows -- gate rows -> acts, then res/skip rows -- when B * ceil(T / 16) tiles would
                          * leave most compute units idle (one or two utterances at frame rate); results bit-identical */
} ov_wn_layer_params;
int ov_wn_layer_f32(const ov_wn_layer_params* p, ov_stream_t stream);
/* 1 when (hidden channels, taps) has a fused instance (192, 5: every WN of the converter and of the V1 speaker). */
int ov_wn_layer_supported(int H, int K);
/* Floats written by ov_wn_pack_f32 (0 when rows % 128 or cin % 32). */
size_t ov_wn_pack_size(int rows, int cin, int K);
/* Dense HOST w[rows][cin][K] -> 16x16x4 A-fragment order, [wave][record][row block][lane][4 k-steps] (HOST dst). */
int ov_wn_pack_f32(const float* w, int rows, int cin, int K, float* dst);
/* Tile width the launcher uses for (B, T) on the current device: equal tiles per utterance, a multiple of 16
 * columns, that fill the compute units in whole rounds (width > 0: validated and returned; 0 = invalid). */
int ov_wn_layer_tile(int B, int T, int width);

/* The same layer (reference openvoice/modules.py:192-209, commons.py:100-107) with the k = 5 gate conv computed in the
 * Winograd domain: two F(4, 3) groups (w0 w1 w2)(w3 w4 0), 11 products per 4 output columns where the direct form needs
 * 20 (openvoice_amd/csrc/wn_layer_wino.hip); the 1x1 res/skip conv and the updates of h / skip as in ov_wn_layer_f32.
 * Same parameter struct and argument rules, except: w_in = ov_wn_wino_pack_f32 of the dense [2H][H][5] in_layer weight
 * with its rows in the gate order described above (b_in, cond, w_rs, b_rs as for ov_wn_layer_f32); one workgroup per
 * (utterance, tile of ov_wn_layer_wino_tile() = 128 columns), `width` 0 or 128; row_split / acts are ignored (one launch
 * always) and dbg must be NULL.  H = 192, K = 5 only (OV_E_UNSUPPORTED otherwise).  Results agree with ov_wn_layer_f32
 * to fp32 rounding: the transforms round where the direct form does not (~3-5x its error against float64, measured). */
int ov_wn_layer_wino_f32(const ov_wn_layer_params* p, ov_stream_t stream);
/* Columns of one workgroup tile of ov_wn_layer_wino_f32. */
int ov_wn_layer_wino_tile(void);
/* Floats written by ov_wn_wino_pack_f32 (0 unless rows = 384, cin = 192, K = 5). */
size_t ov_wn_wino_pack_size(int rows, int cin, int K);
/* Dense HOST w[rows][cin][5] -> U_p[row][g][ci] = sum_k G[p][k] w[row][ci][3g + k] (float64, rounded once to fp32) in
 * 16x16x4 A-fragment order, [wave][4 input channels][row fragment][3][lane][4]: a lane's 12 floats are group 0 points
 * 0..5, group 1 points 0..4 and a zero; one zero record group closes the stream (HOST dst). */
int ov_wn_wino_pack_f32(const float* w, int rows, int cin, int K, float* dst);

/* The same layer (reference openvoice/modules.py:192-209, commons.py:100-107) on the bf16 matrix pipe
 * (openvoice_amd/csrc/wn_layer_bf16.hip): the STATE stays fp32, only the matrix operands are rounded, each once, to the
 * nearest even bf16:
 *   x_in = in_layer_bf16(bf16(x)) + b_in + cond;  acts = bf16(tanh(x_in[:H]) * sigmoid(x_in[H:]))      fp32 sums and gate
 *   rs   = res_skip_layer_bf16(acts) + b_rs;      out = (x + rs[:H]) * mask with the UNROUNDED x;  skip (+)= rs[H:]
 * Same parameter struct, layouts, argument rules, alignment rules, error codes and reads beyond column T as
 * ov_wn_layer_f32 (a 16-byte vector of x / skip / mask is read iff its first column, a multiple of 4, is < T), except:
 * w_in / w_rs point to BF16 data, ov_wn_bf16_pack of the dense fp32 weights described there (gate row order for w_in;
 * the last layer's w_rs padded to 2H rows); dbg must be NULL (OV_E_BADARG); row_split / acts are ignored: always one
 * launch, `acts` stays in LDS.  One workgroup per (utterance, tile of `width` = 16 .. 128 columns, 0 = chosen by
 * ov_wn_layer_bf16_tile).  The value of an output element does not depend on the tile width, the tile index, B or the
 * item's row (one fixed summation order: 32-channel chunk, then tap): bit-identical across all of them.  H = 192, K = 5
 * only (OV_E_UNSUPPORTED otherwise).  (Added within 2.12: additive symbols.) */
int ov_wn_layer_bf16(const ov_wn_layer_params* p, ov_stream_t stream);
/* 1 for (hidden channels, taps) = (192, 5), else 0. */
int ov_wn_layer_bf16_supported(int H, int K);
/* bf16 elements written by ov_wn_bf16_pack (0 when rows % 128 or cin % 32). */
size_t ov_wn_bf16_pack_size(int rows, int cin, int K);
/* Dense HOST fp32 w[rows][cin][K] -> bf16 (nearest even, once) in 16x16x32 A-fragment order, [wave = rows / 8][k-step =
 * (32-channel chunk, tap)][row fragment][lane][8 channels], one zero k-step closing each wave's stream (HOST dst). */
int ov_wn_bf16_pack(const float* w, int rows, int cin, int K, uint16_t* dst);
/* Tile width the launcher of ov_wn_layer_bf16 uses for (B, T) on the current device (width > 0: validated and returned;
 * 0 = invalid). */
int ov_wn_layer_bf16_tile(int B, int T, int width);

/* Framing for the linear spectrogram, reference openvoice/mel_processing.py:54-58 (reflect pad) and the framing
 * step of torch.stft at :61-72: hops[b][c][u] = ypad[hop*u + c] for u < U, with ypad the waveform [B][N]
 * reflect-padded by `pad` samples on each side (zero beyond that).  hops is (B, hop, U) with rows ld apart.
 * With n_fft = 4*hop the windowed DFT + magnitude is then ov_conv1d_f32 with K = 4, Cin = hop and
 * OV_EPI_MAGNITUDE (weights = window * cos / -sin, rows paired re/im). */
int ov_frame_hops_f32(const float* wave, float* hops, int B, int N, int hop, int pad, int U, int ld,
                      ov_stream_t stream);

/* General linear-magnitude STFT, the reference's spectrogram_torch (openvoice/mel_processing.py:40-75) at any supported
 * shape -- ov_frame_hops_f32 + the framing conv cover n_fft == 4 * hop only:
 *   out[b][f][t] = sqrt(re^2 + im^2 + 1e-6),  (re, im)[f][t] = sum_n hann_pad[n] (cos, -sin)(2 pi f n / n_fft) ypad[t * hop + n]
 * for f <= n_fft / 2 and t < T = (Np - n_fft) / hop + 1.  ypad (Np samples) is y [B][N] reflect-padded by
 * (n_fft - hop) / 2 (:54-58) and, when `center`, that result reflect-padded AGAIN by n_fft / 2 (torch.stft at :61-72): two
 * reflections in sequence, indexed in place.  hann_pad is the periodic Hann window of `win` samples with (n_fft - win) / 2
 * zeros to its left, as torch.stft pads it; it reaches the kernel only through `wpack`, which the host builds in float64
 * and rounds once to fp32 (openvoice_amd/mel_processing.py stft_weights): float4 record ((bt * 2 + c) * G + g), lane l,
 * element u = W_c[32 bt + (l & 31)][8 g + 2 u + (l >> 5)], c = 0 re / 1 im, G = ceil(n_fft / 8), zeros beyond bins and n_fft;
 * 16-byte aligned.  out is [B][n_fft / 2 + 1][ld] with ld == T rounded up to 4; columns [T, ld) are written as 0.
 * Supported: 16 <= n_fft <= 2048 and even, 1 <= hop <= n_fft, 1 <= win <= n_fft (else OV_E_UNSUPPORTED); N larger than
 * each pad it reflects, N <= 2^30, B <= 65535 (else OV_E_BADARG).  Nothing is launched when a check fails.  (Added within
 * 2.12: an additive symbol.) */
int ov_stft_mag_f32(const float* y, const float* wpack, float* out, int B, int N, int n_fft, int hop, int win, int center,
                    int ld, ov_stream_t stream);
/* Frames one workgroup of ov_stft_mag_f32 and ov_mel_log_f32 owns (tests size their shapes by it). */
int ov_stft_tile_frames(void);
/* Mel projection with dynamic-range compression, the reference's spec_to_mel_torch (openvoice/mel_processing.py:122-133:
 * torch.matmul(mel_basis, spec) at :131, spectral_normalize_torch at :132 = log(clamp(x, min = 1e-5)), :8-14), and with
 * ov_stft_mag_f32 in front of it mel_spectrogram_torch (:136-183):
 *   out[b][m][t] = logf(max(sum_f mel[m][f] * spec[b][f][t], clip))
 * spec rows are spec_ld >= T apart and items spec_bstride apart; mel is DEVICE [num_mels][bins] fp32; out is
 * [B][num_mels][out_ld] with out_ld == T rounded up to 4, columns [T, out_ld) written as 0.  num_mels <= 256 and
 * bins <= 1025 (else OV_E_UNSUPPORTED); clip > 0.  (Added within 2.12: an additive symbol.) */
int ov_mel_log_f32(const float* spec, const float* mel, float* out, int B, int num_mels, int bins, int T, int spec_ld,
                   int64_t spec_bstride, int out_ld, float clip, ov_stream_t stream);

/* Windowed framing for long recordings (openvoice_amd/longform.py), replacing for each window the reflect pad + framing of
 * the reference's one-pass spectrogram_torch (openvoice/mel_processing.py:54-72, called at openvoice/api.py:145):
 *   hops[w][c][u] = ypad[hop * (first_frame[w] + u) + c],  u < U,
 * ypad = the ONE long waveform wave[n_samples] reflect-padded by `pad` samples at its two true ends (zero beyond), so
 * that window w's plane is the slice [first_frame[w], first_frame[w] + U) of ov_frame_hops_f32's whole-file plane and
 * the K = 4 framing conv with OV_EPI_MAGNITUDE yields spectrogram(whole)[:, :, f0 : f0 + U - 3] bit for bit without
 * the whole-file spectrogram.  first_frame is a DEVICE int64 [W]; hops is [W][hop][ld], ld % 4 == 0 and 16-byte
 * aligned (stored as 16-byte vectors; columns [U, U rounded up to 4) are written as 0).  Sample indices are 64-bit.
 * ABI 2.10. */
int ov_frame_hops_windows_f32(const float* wave, int64_t n_samples, const int64_t* first_frame, int W, int hop, int pad,
                              int U, int ld, float* hops, ov_stream_t stream);
/* ov_frame_hops_windows_f32 with one source per window (many streams / recordings in one launch,
 * openvoice_amd/longform.py StreamPool / convert_many): records is a DEVICE int64 [W][3] of (base, n_samples,
 * first_frame); window w frames pool[base, base + n_samples) as its own waveform,
 *   hops[w][c][u] = ypad_w[hop * (first_frame + u) + c],  u < U,
 * ypad_w = that span reflect-padded by `pad` samples at both of its ends (zero beyond).  Same host checks and error
 * codes as ov_frame_hops_windows_f32 (pool_len plays n_samples' part, pad < n_samples is checked per record).  The
 * kernel checks every record itself: base < 0, n_samples <= pad or base + n_samples > pool_len writes zeros for that
 * window and reads nothing.  64-bit sample indices.  ABI 2.11. */
int ov_frame_hops_multi_f32(const float* pool, int64_t pool_len, const int64_t* records, int W, int hop, int pad, int U,
                            int ld, float* hops, ov_stream_t stream);
/* The cores of W windows into the long output (the reference writes the one-pass o_hat, openvoice/api.py:146-156):
 * windows is a DEVICE int64 [W][3] of (first_frame, core_lo, core_hi) in frames, o_hat [W][Tw * spf] the windows'
 * generator outputs (spf samples per frame);
 *   out[(core_lo - out_frame0) * spf + s] = o_hat[w][(core_lo - first_frame) * spf + s],  s < (core_hi - core_lo) * spf.
 * A record whose core is not inside its window or whose samples would land outside [0, out_len) copies nothing.
 * 64-bit output offsets.  ABI 2.10. */
int ov_stitch_window_cores_f32(const float* o_hat, const int64_t* windows, int W, int Tw, int spf, float* out,
                               int64_t out_len, int64_t out_frame0, ov_stream_t stream);
/* Record-driven row copy of live streams' carried state (openvoice_amd/live.py): records is a DEVICE int64
 * [n_records][6] of (src_off, dst_off, rows, cols, src_ld, dst_ld), in elements relative to src_base / dst_base;
 *   dst_base[dst_off + i * dst_ld + j] = src_base[src_off + i * src_ld + j],  i < rows, j < cols.
 * One launch serves every unit and stream of a step: a stream's history shift between ping-pong halves, a pool's gather
 * of ready streams' state from its per-stream arena into batch rows, and the scatter of new columns back; it replaces
 * the units x streams Python-issued slice copies (torch `dst[...].copy_(src[...])`) a step would otherwise cost.
 * Source and destination regions of one launch must not overlap.  Host checks: null pointers, n_records in
 * [1, 65535], extents > 0 (OV_E_BADARG).  The kernel checks every record against src_elems / dst_elems: a record with a
 * negative, oversized (rows, cols, ld > 2^31) or overlapping-row (rows > 1 and dst_ld < cols) destination, or whose
 * destination leaves [0, dst_elems), touches nothing; one whose destination is in range but whose source is not writes
 * zeros there.  Rows move as 16-byte vectors when both bases are 16-byte aligned and the record's offsets and lds are
 * multiples of 4, as scalars otherwise; 64-bit offsets.  ABI 2.12. */
int ov_carry_rows_f32(const int64_t* records, int n_records, const float* src_base, int64_t src_elems, float* dst_base,
                      int64_t dst_elems, ov_stream_t stream);
/* The seam of a live stream with bounded look-ahead (openvoice_amd/live.py, lookahead_frames=): successive pieces come
 * from different truncations of the input, so the first x samples of a piece are blended with the samples the previous
 * round's preview computed for the same positions.  records is a DEVICE int64 [n_records][5] of
 * (old_off, new_off, dst_off, n, x), in elements, old / new relative to src_base and dst relative to dst_base; w an
 * fp32 DEVICE vector of w_elems fade-in weights (the host builds 0.5 - 0.5 cos(pi (i + 1) / (X + 1)) in float64 and
 * rounds once).  For i < n:
 *   dst[dst_off + i] = fmaf(w[i], src[new_off + i] - src[old_off + i], src[old_off + i])   for i < min(x, n),
 *   dst[dst_off + i] = src[new_off + i]                                                      otherwise.
 * One launch serves every stream of a pool's round; it replaces, per stream and round, torch's
 * `torch.addcmul(old, w, new - old)` on the first x samples plus a slice copy of the rest (three launches and two
 * temporaries each).  Source and destination regions of one launch must not overlap.  Host checks: null pointers,
 * n_records in [1, 65535], extents > 0 (OV_E_BADARG).  The kernel checks every record: one with a negative or oversized
 * (n, x > 2^31) field, n < 1, x > w_elems, or whose old span [old_off, old_off + min(x, n)), new span or destination
 * leaves its buffer touches nothing.  A record moves as 16-byte vectors when all four bases are 16-byte aligned and its
 * three offsets are multiples of 4, as scalars otherwise, with the same bits either way; 64-bit offsets.  Additive to
 * ABI 2.12: found by name, like ov_normal_philox_f32. */
int ov_crossfade_rows_f32(const int64_t* records, int n_records, const float* w, int64_t w_elems, const float* src_base,
                          int64_t src_elems, float* dst_base, int64_t dst_elems, ov_stream_t stream);
/* The two layout hand-overs of a live generator unit that runs the bf16 channels-last kernels (openvoice_amd/live.py,
 * generator="bf16"): the live arena and the carries stay fp32 channels-first, the bf16 generator reads and writes dense
 * channels-last bf16.  The fp32 side is B rows of `bs` elements, each [C][ld] with L valid columns; the bf16 side is a
 * dense [B][L][C] tensor.  One launch per direction serves every row of a unit's batch.
 *   ov_rows_f32_to_cl_bf16:  dst[(b * L + l) * C + c] = bf16(src[b * src_bs + c * src_ld + l]),  round to nearest
 *     even with NaN -> 0x7fc0 and the infinities kept: the same bits as torch's
 *     `x[..., :L].transpose(1, 2).to(torch.bfloat16).contiguous()` on a strided view, which it replaces
 *     (GeneratorBf16.decode does that on a dense tensor, two torch launches);
 *   ov_cl_bf16_to_rows_f32:  dst[b * dst_bs + c * dst_ld + l] = f32(src[(b * L + l) * C + c]),  exact; columns >= L and
 *     everything between the rows are left as they were.  Replaces `dst[:, :, :L].copy_(src.transpose(1, 2))`.
 * Both are transposes tiled through LDS (32 channels x 64 columns, rows padded by one float: no bank conflicts on either
 * side), with 64-bit offsets.  The fp32 side moves as 16-byte vectors when its base is 16-byte aligned and ld and bs
 * are multiples of 4 (a vector that would cross column L moves as scalars: any L >= 1), as scalars otherwise; the bf16
 * side as 16-byte vectors when its base is 16-byte aligned.  Host checks (OV_E_BADARG): null pointers, B outside
 * [1, 65535], C not a positive multiple of 32 (or > 32 * 65535), L < 1, ld < L, bs < C * ld.
 * Additive symbols of ABI 2.12 (no version change). */
int ov_rows_f32_to_cl_bf16(const float* src, int64_t src_bs, int src_ld, uint16_t* dst, int B, int C, int L,
                           ov_stream_t stream);
int ov_cl_bf16_to_rows_f32(const uint16_t* src, float* dst, int64_t dst_bs, int dst_ld, int B, int C, int L,
                           ov_stream_t stream);

/* Silence removal ahead of the tone-colour embedding (openvoice_amd/vad.py, se_extractor.split_audio_vad): the
 * procedure of reference openvoice/se_extractor.py:77-97 -- voice-activity segments, concatenated active audio -- with
 * a deterministic energy detector standing in for the third-party network the reference calls (se_extractor.py:80-86:
 * get_vad_segments(..., min_speech_duration=0.1, min_silence_duration=1)).  Three record-driven launches serve R
 * recordings that lie in one float32 pool: records is a DEVICE int64 [R][2] of (base, n_samples); recording r is
 * pool[base, base + n_samples) and has T_r = ceil(n_samples / H) frames; the per-frame tables have ldT >= max T_r
 * columns.  Host checks of all three (OV_E_BADARG): null pointers, R outside [1, 65535], H not a positive multiple of 4,
 * ldT <= 0, pool_len / out_len <= 0.  The kernels check every record: base < 0, n_samples <= 0, base + n_samples >
 * pool_len or T_r > ldT make the recording empty (energies 0, nothing kept, nothing copied).  64-bit pool offsets.
 * Additive symbols of ABI 2.12 (no version change).
 *
 * Frame energy (stands in for the detector's per-window speech probability, se_extractor.py:80-86):
 *   energy[r][t] = mean of x[n]^2 over the samples n in [t H, min(n_samples, t H + 2 H)),  t < T_r  (0 for t >= T_r).
 * 16-byte loads when the pool is 16-byte aligned and base % 4 == 0, scalars otherwise; a frame's sum is formed in one
 * fixed order either way, so it does not depend on R or on where the recording lies in the pool. */
int ov_vad_frame_energy_f32(const float* pool, int64_t pool_len, const int64_t* records, int R, int H, int ldT,
                            float* energy, ov_stream_t stream);
/* The keep / drop decision per frame (stands in for the segment rules of get_vad_segments, se_extractor.py:80-88), one
 * workgroup per recording, prefix / suffix scans over the frame axis, any T_r:
 *   raw-active  e[t] > max(floor_lin, max_t e[t] * range_lin);
 *   a silent run between two raw-active frames shorter than min_silence_frames becomes active;
 *   then an active run shorter than min_speech_frames becomes silent;
 *   then every remaining run grows by pad_frames on each side, clipped to [0, T_r).
 * mask [R][ldT] (1 = kept), offsets [R][ldT] = the kept samples before frame t (a frame holds min(H, n_samples - t H)),
 * n_active [R] = the kept samples of the recording.  Additional host checks: min_silence_frames <= 0,
 * min_speech_frames <= 0, pad_frames < 0, a negative or NaN floor_lin / range_lin (OV_E_BADARG). */
int ov_vad_segments_i32(const float* energy, const int64_t* records, int R, int H, int ldT, float floor_lin,
                        float range_lin, int min_silence_frames, int min_speech_frames, int pad_frames, int32_t* mask,
                        int64_t* offsets, int64_t* n_active, ov_stream_t stream);
/* The concatenation of the kept audio (se_extractor.py:90-94: audio_active += audio[start:end]):
 *   out[out_bases[r] + offsets[r][t] + j] = pool[base_r + t H + j],  j < min(H, n_samples - t H), for every kept frame.
 * out_bases is a DEVICE int64 [R].  16-byte copies when both buffers are 16-byte aligned and base and out_base are
 * multiples of 4.  A frame whose destination would leave [0, out_len) copies nothing. */
int ov_vad_compact_f32(const float* pool, int64_t pool_len, const int64_t* records, int R, int H, int ldT,
                       const int32_t* mask, const int64_t* offsets, const int64_t* out_bases, float* out,
                       int64_t out_len, ov_stream_t stream);

/* ---- the join between the base-speaker TTS and the converter (csrc/clone.hip, openvoice_amd/clone.py) ---------------
 * The device form of audio_numpy_concat (reference openvoice/api.py:56-63: `audio_segments += segment_data.reshape(-1)
 * .tolist()` then `audio_segments += [0] * int((sr * 0.05) / speed)` per sentence, `np.array(...).astype(np.float32)`),
 * for any number of utterances in one launch.  records is a DEVICE int64 [R][4] of (src_off, n, dst_off, gap), in
 * elements relative to src / dst:
 *   dst[dst_off + j] = src[src_off + j],  j < n;      dst[dst_off + n + j] = 0,  j < gap.
 * The sources are rows of the padded TTS output [B, 1, ld] (src_off = b * ld, n = frames_b * hop); what lies beyond n
 * in a row is never read.  n = 0 and gap = 0 are legal.  Records must not overlap in dst (the host plan,
 * clone.join_plan, guarantees it); nothing outside the records' spans is written.  The kernel checks every record: one
 * with a negative field, or that would read outside [0, src_elems) or write outside [0, dst_elems), copies nothing.
 * Grid (chunk, record): 16-byte stores on the destination's own 16-byte grid, whatever dst_off is (the kernel peels up
 * to three samples), 16-byte loads at the source's alignment, scalars at the edges; 64-bit indices.  max_span = the
 * largest n + gap of the launch sizes the grid (a record with a longer span is still joined whole).  Host checks: null
 * pointers, R in [1, 65535], extents > 0, max_span >= 0 (OV_E_BADARG); src and dst 4-byte aligned (OV_E_ALIGN).
 * Additive to ABI 2.12: found by name, like the vad kernels. */
int ov_join_segments_f32(const float* src, int64_t src_elems, const int64_t* records, int R, float* dst,
                         int64_t dst_elems, int64_t max_span, ov_stream_t stream);

/* ---- a ragged batch on the bf16 generator as dense length groups (csrc/ragged_bf16.hip, openvoice_amd/bf16.py) --------
 * Stand in for the generator of reference openvoice/models.py:272-291 applied to a PADDED batch (models.py:488:
 * `self.dec((z * y_mask)[:, :, :max_len], g=g)` computes every item at the longest item's length): GeneratorBf16.
 * decode_groups sorts the items by length, cuts them into a few groups and runs each group as a dense [B_g][L_g][C]
 * bf16 tensor of its own length.  These two record-driven launches are the hand-over between the fp32 channels-first
 * rows the flow leaves (item b: [C][ld], cols_b valid columns) and the groups' dense tensors; one launch each way serves
 * every item of every group.  Offsets are in elements relative to src / dst, 64-bit.
 *   ov_pack_groups_cl_bf16: records is a DEVICE int64 [n][5] of (src_off, src_ld, dst_off, cols, L);
 *       dst[dst_off + l * C + c] = bf16(src[src_off + c * src_ld + l]),  l < cols, c < C;      0,  cols <= l < L:
 *     round to nearest even with NaN -> 0x7fc0, the bits of torch's `.to(torch.bfloat16)` and of
 *     ov_rows_f32_to_cl_bf16.  The source columns >= cols are NOT read (in a workspace row they are stale, possibly
 *     NaN).  Any cols >= 0 and L >= 1.  A transpose tiled through LDS: the fp32 side moves as 16-byte vectors when src
 *     is 16-byte aligned and src_off and src_ld are multiples of 4 (a vector that would cross column `cols` moves as
 *     scalars), the bf16 side as 16-byte vectors when dst is 16-byte aligned and dst_off a multiple of 8.
 *   ov_unpack_groups_f32: records is a DEVICE int64 [n][4] of (src_off, dst_off, keep, row);
 *       dst[dst_off + j] = src[src_off + j],  j < keep;      dst[dst_off + j] = 0,  keep <= j < row.
 *     16-byte stores on the destination's own 16-byte grid, loads at the source's alignment, scalars at the edges.
 * Records must not overlap in dst; nothing outside the records' spans is written.  Host checks (OV_E_BADARG): null
 * pointers, n outside [0, 65535] (n = 0 launches nothing), src_len / dst_len <= 0, C not a positive multiple of 8;
 * src / dst not aligned to their element size (OV_E_ALIGN).  The kernels check every record: one with a negative
 * field, L < 1, cols > L or keep > row, or that would read outside [0, src_len) or write outside [0, dst_len), reads
 * nothing and writes nothing.  Additive to ABI 2.12: found by name, like ov_join_segments_f32. */
int ov_pack_groups_cl_bf16(const float* src, int64_t src_len, const int64_t* records, int n, int C, uint16_t* dst,
                           int64_t dst_len, ov_stream_t stream);
int ov_unpack_groups_f32(const float* src, int64_t src_len, const int64_t* records, int n, float* dst, int64_t dst_len,
                         ov_stream_t stream);

/* ---- counter-based Gaussian noise (csrc/noise.hip, openvoice_amd/noise.py) -------------------------------------------
 * Stands in for the reference's torch.randn / randn_like draws (openvoice/models.py:220, :476, :486) where a caller
 * asks for `seed=`: the value at (seed, stream, purpose, channel c, frame t) is a pure function of those five numbers,
 * 0 <= seed < 2^63, 0 <= stream, purpose, c < 2^32, 0 <= t < 2^34:
 *   (r0, r1, r2, r3) = Philox4x32-10(counter = (t / 4, c, stream, purpose), key = (seed & 0xffffffff, seed >> 32)),
 *     the standard function: multipliers 0xD2511F53 (on word 0) and 0xCD9E8D57 (on word 2), key increments 0x9E3779B9
 *     and 0xBB67AE85, one round (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), ten rounds;
 *   j = t % 4: pair j / 2 takes (ra, rb) = (r0, r1) or (r2, r3);  u1 = ((ra >> 8) + 0.5) 2^-24,  u2 = (rb >> 8) 2^-24;
 *   n = sqrt(-2 ln u1) cos(2 pi u2) for even j, sqrt(-2 ln u1) sin(2 pi u2) for odd j;  |n| <= sqrt(50 ln 2) = 5.887.
 * Purposes in use: 0 the converter's posterior noise, 1 the TTS noise_w (frames = token positions), 2 the TTS noise_z.
 * records is a DEVICE int64 [R][7] of (seed, stream, purpose, f0, nf, dst_off, dst_ld), offsets in elements of dst:
 *   dst[dst_off + c * dst_ld + i] = n(seed, stream, purpose, c, f0 + i),  c < C, i < nf;
 * nothing else is written (pad columns and what lies between slabs keep their contents).  One thread owns one Philox
 * block (four consecutive frames of one channel) and computes its four values before it knows how they are stored: a
 * block wholly inside the slab at a 16-byte aligned destination is one vector store, everything else goes element by
 * element, so a value does not depend on f0's phase, on alignment, on R or on its neighbours.  The logarithm of
 * u1 >= 1/2 is taken as log1p(-(1 - u1)) (1 - u1 is exact in fp32 there, u1 is not) and the angle as sin / cos of 2 u2
 * half turns (exact argument).  max_frames = the largest nf of the launch sizes the grid only.  Host checks: null
 * pointers, R outside [1, 65535], C <= 0, dst_elems <= 0, max_frames < 0 (OV_E_BADARG); dst 4-byte aligned
 * (OV_E_ALIGN).  The kernel checks every record: one with a negative field, stream or purpose >= 2^32, f0 + nf > 2^34,
 * nf > dst_ld, or a slab that leaves [0, dst_elems) writes nothing.  Additive to ABI 2.12: found by name, like the vad
 * and join kernels. */
int ov_normal_philox_f32(const int64_t* records, int R, int C, float* dst, int64_t dst_elems, int64_t max_frames,
                         ov_stream_t stream);

/* The project's own keyed watermark (openvoice_amd/watermark.py) behind the converter's provenance hook, reference
 * openvoice/api.py:162-201 (add_watermark / detect_watermark, which call the third-party wavmark network once per
 * 16 000-sample window).  NOT wavmark-compatible: informed spread spectrum in the time domain.  A window x[0 .. L)
 * carries 32 bits; bit j owns the samples S_j = {i : i % 32 == j}:
 *   c[i]  = +1 / -1 for a set / clear bit (i % 32) of word (i % 128) / 32 of
 *           Philox4x32-10(counter = (i / 128, 0, 0, 3), key = (key & 0xffffffff, key >> 32))   (ov_normal_philox_f32's core)
 *   p_j   = (1 / |S_j|) sum_{i in S_j} c[i] x[i],      a = max(strength * sqrt(mean x^2), floor_level)
 *   embed:  d_j = b_j max(a - b_j p_j, 0), b_j = +1 / -1 for payload bit j set / clear;  y[i] = x[i] + d_{i % 32} c[i]
 *   detect: q_out[w][j] = p_j and level_out[w] = a of the window as it is; bit j reads as q_j >= 0.
 * records is a DEVICE int64 [W][4] of (src_off, dst_off, L, bits), offsets in elements relative to src / dst, the payload
 * in the low 32 bits of `bits` (bit j = (bits >> j) & 1); detect reads src_off and L only.  One launch serves every
 * window, one 256-thread workgroup each.  dst may be src: a window's source and destination coincide or do not overlap,
 * and the windows of one launch do not overlap each other.  Sums are added in a fixed order that depends on L alone, so
 * what a window gets does not depend on W, on its place in the launch or on the alignment of its offsets.  Host checks
 * (OV_E_BADARG): null pointers, extents <= 0, W outside [1, 65535], key < 0, strength outside [0, 1], floor_level outside
 * (0, 1]; pointers 4-byte aligned (OV_E_ALIGN).  The kernel checks every record: one with L outside [512, 2^31], a
 * negative offset, or whose window leaves [0, src_elems) (embed: or [0, dst_elems)) writes nothing.  Additive to ABI
 * 2.12: found by name, like ov_normal_philox_f32. */
int ov_wm_embed_windows_f32(const float* src, int64_t src_elems, float* dst, int64_t dst_elems, const int64_t* records,
                            int W, int64_t key, float strength, float floor_level, ov_stream_t stream);
int ov_wm_detect_windows_f32(const float* src, int64_t src_elems, const int64_t* records, int W, int64_t key,
                             float strength, float floor_level, float* q_out, float* level_out, ov_stream_t stream);
/* The block-wise form of the same mark, for streams (openvoice_amd/watermark.py, "streams"): a carrier window of 16 000
 * samples is cut into 16 000 / H blocks of H samples, H (the hold) one of 16000, 8000, 4000, 3200, 1600, 800, 640, and
 * per window and bit one float R_j >= 0, the surplus of the blocks so far, is carried.  For a block x with p_j and
 * a_m = max(strength * sqrt(mean_block x^2), floor_level) of the block alone, chips counted from the window's start:
 *   u_j = b_j p_j + R_j,   d_j = b_j max(a_m - u_j, 0),   y[i] = x[i] + d_{i % 32} c[i],   R_j <- max(u_j - a_m, 0)
 * so that b_j p_j(y) >= mean_m a_m >= floor_level over the whole window: ov_wm_detect_windows_f32 reads every bit.
 * records is a DEVICE int64 [R][8] of (src_off, dst_off, H, blocks, bits, chip_off, state_row, reset): a run of `blocks`
 * consecutive blocks of one window, the first one chip_off samples (a multiple of H) after the window's start, source
 * and destination offsets in elements of src / dst (dst may be src), the payload in the low 32 bits of `bits`.  state
 * is DEVICE float [state_rows][32]: the record's workgroup (256 threads, one per record) starts from row state_row, or
 * from zero when reset = 1, walks its blocks in order and writes the row back at the end.  No two records of one launch
 * may name the same row, and their destinations must not overlap.  A block is reduced in the order
 * ov_wm_embed_windows_f32 reduces a window, so H = 16 000 gives that entry point's samples bit for bit, and what a run
 * gets depends on its samples, payload, parameters and incoming row alone.  Host checks (OV_E_BADARG): null pointers,
 * extents <= 0, R outside [1, 65535], state_rows <= 0, key < 0, strength outside [0, 1], floor_level outside (0, 1];
 * pointers 4-byte aligned (OV_E_ALIGN).  The kernel checks every record: one whose H is not in the list, with blocks
 * < 1, chip_off negative or no multiple of H, chip_off + blocks H > 16 000, state_row outside [0, state_rows), reset
 * other than 0 / 1, a negative offset, or whose run leaves [0, src_elems) or [0, dst_elems) writes nothing, neither
 * samples nor state.  Additive to ABI 2.12: found by name. */
int ov_wm_embed_blocks_f32(const float* src, int64_t src_elems, float* dst, int64_t dst_elems, const int64_t* records,
                           int R, float* state, int64_t state_rows, int64_t key, float strength, float floor_level,
                           ov_stream_t stream);
/* The same reader at EVERY offset of a waveform, for audio whose start was cut, shifted or is unknown
 * (openvoice_amd/watermark.py, "the scan").  records is a DEVICE int64 [R][3] of (src_off, n, out_off): for every
 * s in [0, n - 16 000] of the waveform src[src_off .. src_off + n), with p_j(s) and a(s) the projections and the level
 * of the window x[s .. s + 16 000) as defined above, at index out_off + s
 *   words[.] = the 32 bits (bit j set iff p_j(s) >= 0),   pmin[.] = min_j |p_j(s)|,   level[.] = a(s)
 * and, when p_out is not NULL (a [out_elems][32] array: tests and soft decisions), p_out[.][j] = p_j(s).  The
 * projections run on the fp32 matrix pipe: with C[m][j] = c[32 m + j] (500 x 32) and t = s + j,
 *   Q[t][j] = sum_{m < 500} x[t + 32 m] C[m][j],   p_j(s) = Q[s + j][j] / 500
 * 32 consecutive t at a time, the chips made from their Philox words on the device.  The energy is sum_j W[s + j] with
 * W[t] = sum_m x[t + 32 m]^2.  Every sum runs in an order that does not depend on s, on the tile or on the record:
 * what offset s gets is a function of its 16 000 samples, key, strength and floor_level alone.  One launch serves every
 * record: ov_wm_scan_tile() = 896 offsets per 256-thread workgroup, a grid of ceil((max_n - 15 999) / 896) x R with
 * max_n the largest n of the call.  The output ranges of the records must not overlap.  Host checks (OV_E_BADARG): null
 * pointers (p_out excepted), extents <= 0, R outside [1, 65535], max_n outside [16 000, 2^31], key < 0, strength outside
 * [0, 1], floor_level outside (0, 1]; pointers 4-byte aligned, records 8-byte (OV_E_ALIGN).  The kernel checks every
 * record: one with n < 16 000 or n > max_n, a negative offset, a waveform that leaves [0, src_elems) or an output range
 * that leaves [0, out_elems) writes nothing.  Additive to ABI 2.12: found by name. */
int ov_wm_scan_f32(const float* src, int64_t src_elems, const int64_t* records, int R, int64_t max_n, int64_t key,
                   float strength, float floor_level, int32_t* words, float* pmin, float* level, float* p_out,
                   int64_t out_elems, ov_stream_t stream);
/* Offsets one workgroup of ov_wm_scan_f32 owns (tests size their shapes by it). */
int ov_wm_scan_tile(void);
/* The hits of a scan, one 256-thread workgroup per record, in ascending offset.  records is a DEVICE int64 [R][2] of
 * (scan_off, S): offsets s in [0, S) at index scan_off + s of words / pmin / level (scan_elems elements each).  With
 * G > 0 (groups: DEVICE int32 [G], G <= 8) offset s is a hit when e = min_k popcount(words[s] ^ groups[k]) <=
 * max_errors (k the lowest such); with G == 0 when pmin[s] >= margin * level[s] (fp32 product), k = -1, e = 0.  The
 * first `cap` hits of record i are the rows hits[i * cap + .] = (s, words[s], k, e) (DEVICE int32 [R * cap][4]; cap = 0:
 * count only, hits may be NULL), counts[i] is the number of hits whether they fitted or not.  The compaction is ordered
 * (ballot, popcount, a running base): the list does not depend on the launch.  Host checks (OV_E_BADARG): null pointers,
 * scan_elems <= 0, R outside [1, 65535], G outside [0, 8], max_errors outside [0, 32], margin < 0, cap < 0; alignment as
 * above.  A record with a negative field, S >= 2^31 or a range that leaves [0, scan_elems) writes nothing, counts[i]
 * included.  Additive to ABI 2.12: found by name. */
int ov_wm_scan_pick(const int32_t* words, const float* pmin, const float* level, int64_t scan_elems, const int64_t* records,
                    int R, const int32_t* groups, int G, int max_errors, float margin, int32_t* hits, int cap,
                    int32_t* counts, ov_stream_t stream);

/* speed= / duration= of a conversion (openvoice_amd/stretch.py: the definition and its float64 / integer mirror; the
 * project's own -- nothing in the reference stretches a conversion): the masked latent z_hat, fp32 rows, resampled along
 * time between the reverse flow and the generator.  records is a DEVICE int64 [n_records][10] of
 *   (src_off, dst_off, rows, src_ld, dst_ld, t_in, i0, j0, n_out, step)
 * offsets and lds in elements relative to src / dst; i0 the GLOBAL frame index of the source's column 0, j0 the global
 * index of the first output frame written, step = round(speed * 2^32) in [2^31, 2^33].  For jj < n_out, j = j0 + jj:
 *   pos = j * step (int64),  i = pos >> 32,  f = ((pos & 0xffffffff) >> 8) * 2^-24   (exact in fp32)
 *   dst[dst_off + r * dst_ld + jj] = a + f * (b - a),   a = src[src_off + r * src_ld + i - i0],
 *                                                       b = src[src_off + r * src_ld + min(i + 1 - i0, t_in - 1)]
 * in fp32, in that order -- subtract, multiply, add, never contracted to an fma.  The weights depend on the global j
 * alone: a window of a long recording computes the bits of the whole-file stretch, and nothing depends on the launch's
 * shape.  step = 2^32 copies.  Source and destination must not overlap.  records_host is a HOST copy of the same
 * table: the call checks every record of it before it launches anything, and one bad record makes it return
 * OV_E_BADARG with nothing launched; it also sizes the grid (the largest n_out and rows).  The kernel checks every
 * record of the DEVICE table again, with the same function, so a record that is out of range there is never executed
 * and writes nothing.  A record is good when rows, t_in and n_out lie in [1, 2^31], t_in <= src_ld <= 2^31,
 * n_out <= dst_ld <= 2^31, the offsets in [0, 2^61], 0 <= i0 <= 2^31, j0 >= 0, j0 + n_out <= 2^29, both spans lie inside
 * [0, src_elems) / [0, dst_elems), and 0 <= i - i0 <= t_in - 1 for every j it covers.  The neighbour i + 1 is clamped to
 * the slice's last column: the caller gives a slice that holds column i + 1 of its last j or that ends at the
 * recording's true end (openvoice_amd/stretch.py: plan_windows).  Other host checks: null pointers, n_records outside
 * [1, 65535], extents <= 0 (OV_E_BADARG); src / dst 4-byte, records 8-byte aligned (OV_E_ALIGN).  Plain VALU, threads
 * along j, no LDS, no atomics.  Additive to ABI 2.12: found by name. */
int ov_stretch_rows_f32(const int64_t* records, const int64_t* records_host, int n_records, const float* src,
                        int64_t src_elems, float* dst, int64_t dst_elems, ov_stream_t stream);

/* Rate conversion at the audio boundary, reference openvoice/api.py:123,144 (``librosa.load(path, sr=...)`` = resampy's
 * kaiser_best band-limited sinc interpolation): a polyphase FIR over a mono waveform,
 *   y[t] = sum_{j < 2 taps} h[t % P][j] * x[(t * Q) / P - taps + 1 + j]        (x = 0 outside [0, n_in))
 * with P / Q = output rate / input rate in lowest terms and h the [P][2 taps] float64 weights of the interpolation
 * filter at each of the P fractional positions (openvoice_amd/audio_io.py: kaiser_best_phases, the same weights its host
 * restatement applies); float64 accumulation.  All pointers DEVICE.  ABI 2.06. */
int ov_polyphase_fir_f32(const float* x, const double* h, float* y, int64_t n_in, int64_t n_out, int P, int Q, int taps,
                         ov_stream_t stream);

/* The same polyphase FIR for many streams in ONE launch (openvoice_amd/rates.py: the per-stream resamplers of live and
 * windowed streams, and the whole-recording rate conversion of convert_many).  records is a DEVICE int64 [n_records][11]
 * with one record per stream and direction, each with its own rate pair:
 *   [0] src_off   element of src_base that holds input sample src_base_index ([1])
 *   [1] src_base_index, [2] src_end: global input indices [src_base_index, src_end) are valid in the arena
 *   [3] n_total   the input's total length once it has ended, -1 while it is still arriving
 *   [4] t0, [5] n_out: the record computes outputs t0 .. t0 + n_out - 1 (global output indices)
 *   [6] dst_off   dst_base[dst_off + k] receives output t0 + k
 *   [7] h_off     element of h_base where the record's [P][2 taps] float64 phase table starts (kaiser_best_phases)
 *   [8] P, [9] Q, [10] taps   as in ov_polyphase_fir_f32
 * Output t equals ov_polyphase_fir_f32's output t of the whole input x[0 .. n_total) bit for bit (one __device__
 * function computes both: the same n = (t Q) / P, j order, float64 accumulation, indices < 0 or >= n_total skipped, one
 * rounding); while n_total is -1 no index is skipped on the right, so a record must only ask for outputs whose taps
 * have all arrived.  Outputs t >= n_total * P / Q (resampy's count) are written as 0: librosa's fix=True padding.
 * Host checks: null pointers, n_records in [1, 65535], extents > 0, max_out > 0 (OV_E_BADARG); max_out is the largest
 * n_out of the table (the grid's width: up to 256 blocks of 256 outputs per record, longer records stride).  The kernel
 * checks every record: non-positive or oversized fields (P, Q, taps > 2^20; indices > 2^40; offsets > 2^61), a
 * destination [dst_off, dst_off + n_out) that leaves [0, dst_elems) or a phase table that leaves [0, h_elems): the
 * record writes nothing; a record whose needed input indices leave [src_base_index, src_end) or the arena writes zeros.
 * Additive symbol of ABI 2.12 (no version change). */
int ov_polyphase_fir_rows_f32(const int64_t* records, int n_records, const float* src_base, int64_t src_elems,
                              const double* h_base, int64_t h_elems, float* dst_base, int64_t dst_elems, int64_t max_out,
                              ov_stream_t stream);

/* conv_post + tanh, reference openvoice/models.py:287-289:
 * out[b][0][t] = tanh( sum_{c,j} w[c][j] * lrelu(x[b][c][t+j-(K-1)/2], in_slope) ), no bias.
 * w is the dense [C][K] DEVICE weight. */
int ov_conv_post_tanh_f32(const float* x, const float* w, float* out, int B, int C, int L, int K,
                          float in_slope, ov_stream_t stream);
/* The same with a length-aware tail: samples t >= col_limit[b] * col_limit_scale of utterance b are written as 0
 * without reading x there (the generator launches before it left those columns unwritten, see
 * ov_conv1d_params.col_limit).  col_limit NULL = ov_conv_post_tanh_f32.  (A col_limit_scale that is not a multiple
 * of 4 takes the per-sample kernel: the 16-byte path decides per 4 consecutive samples.)
 * Read reach: with n = min(L, col_limit[b] * col_limit_scale), the samples t < n are those of the unlimited launch bit
 * for bit and depend on x[b][c][0 .. n + (K - 1) / 2) only: the conv of a sample below the limit reaches (K - 1) / 2
 * (= 3 at K = 7) columns past it, which the generator must have written; nothing from column n + (K - 1) / 2 on enters a
 * result (the 16-byte path may load the rest of that 4-sample group, it never uses it). */
int ov_conv_post_tanh_limited_f32(const float* x, const float* w, float* out, int B, int C, int L, int K,
                                  float in_slope, const int32_t* col_limit, int col_limit_scale, ov_stream_t stream);
/* limits[b] = min(T, max(0, lengths[b]) + margin): the frames of utterance b the generator has to produce so that
 * every sample of its first lengths[b] frames is unaffected by what lies beyond (margin >= 14: the generator's
 * one-sided receptive field is 13.3 frames -- conv_pre 3, ups 1 + 1/8 + 1/64 + 1/128, MRF 60 samples per stage,
 * conv_post 3 samples; reference openvoice/models.py:225-291). */
int ov_frame_limits_i32(const int64_t* lengths, int32_t* limits, int B, int T, int margin, ov_stream_t stream);

/* y[b][m] = bias[m] + sum_k w[m][k] * x[b][k]  (dense row-major w, all DEVICE).  The T=1
 * conditioning convs, reference openvoice/modules.py:189-190 (cond_layer) and
 * openvoice/models.py:275 (dec.cond), and ref_enc.proj (models.py:359). */
int ov_linear_f32(const float* x, const float* w, const float* bias, float* y, int B, int M, int Kdim,
                  ov_stream_t stream);

/* mask[b][t] = t < lengths[b] ? 1 : 0 for t < T, reference openvoice/commons.py:121-125.
 * Rows of mask are ld floats apart (0 = T); columns >= T are not written. */
int ov_sequence_mask_f32(const int64_t* lengths, float* mask, int B, int T, int ld, ov_stream_t stream);
/* dst[r][t] = src[r * ld + t], t < T: the engine's 16-byte aligned rows -> the dense [.., T] tensors the model seam
 * returns (z, z_p, z_hat, y_mask of openvoice/models.py:499). */
int ov_unpad_rows_f32(const float* src, float* dst, int rows, int T, int ld, ov_stream_t stream);

/* ---- ReferenceEncoder (extract_se), reference openvoice/models.py:339-359 -----------------------
 * Layout: time is the contiguous axis everywhere, [N][C][F][T]; the spectrogram [N][F][T] is the
 * C = 1 case, and the conv-stack output [N][128][9][T'] read as [N][1152][T'] is the GRU input in
 * the (B, C, T) layout of ov_conv1d_f32 (feature index c*9 + f, as models.py:351-354 builds it). */

/* y[n][f][t] = LayerNorm over f of x[n][:, t] (nn.LayerNorm(F), reference models.py:344). */
int ov_layernorm_freq_f32(const float* x, const float* gamma, const float* beta, float* y, int N, int F, int T,
                          float eps, ov_stream_t stream);

/* y = relu(conv2d(x, w, bias, stride 2, pad 1)), 3x3; w is the reference's [Cout][Cin][kh=time][kw=freq]
 * (models.py:314-325, :346-349).  x [N][Cin][Fi][Ti] -> y [N][Cout][(Fi-1)/2+1][(Ti-1)/2+1].
 * Cout must be a multiple of 16. */
int ov_conv2d_s2_relu_f32(const float* x, const float* w, const float* bias, float* y, int N, int Cin, int Cout,
                          int Fi, int Ti, ov_stream_t stream);

/* GRU recurrence over T steps from h0 = 0, final hidden state out (nn.GRU batch_first, models.py:356-357).
 * gi [N][3H][T] = W_ih x_t + b_ih (gate order r,z,n), whh_t = W_hh transposed to [H][3H], bhh [3H],
 * h_out [N][H].  H must be 128. */
int ov_gru_f32(const float* gi, const float* whh_t, const float* bhh, float* h_out, int N, int H, int T,
               ov_stream_t stream);

/* ---- ReferenceEncoder over a RAGGED batch (csrc/ref_enc_ragged.hip), reference openvoice/models.py:339-359 --------
 * The three kernels above for items of different lengths in one launch: rows are `ld` floats apart for the whole
 * batch ([N][C][F][ld], ld >= the longest item) and lens (DEVICE int32 [N]) holds each item's own number of frames.
 * Over an item's own columns each kernel performs its dense twin's operations in the twin's order, so item n gets bit
 * for bit what the dense entry point gives for that item alone (T = lens[n]); the columns from the item's end up to the
 * row stride are written as 0.  A length outside [0, ld] is clamped in the kernel.  Host checks as for the dense twins
 * (OV_E_BADARG: null pointers -- lens included --, non-positive extents, N > 65535; OV_E_UNSUPPORTED as stated).
 * Additive to ABI 2.12: found by name, like the vad, join and noise kernels. */

/* ov_layernorm_freq_f32 for columns t < lens[n] of item n (nn.LayerNorm(F), reference models.py:344); columns
 * lens[n] <= t < ld of y are written as 0 and not read from x. */
int ov_layernorm_freq_ragged_f32(const float* x, const float* gamma, const float* beta, const int32_t* lens, float* y,
                                 int N, int F, int ld, float eps, ov_stream_t stream);

/* ov_conv2d_s2_relu_f32 with Ti = lens_in[n] per item (models.py:314-325, :346-349): the zero padding of the 3x3
 * stride-2 conv sits at the ITEM's end.  x [N][Cin][Fi][ld_in] -> y [N][Cout][(Fi-1)/2+1][ld_out]; output columns
 * to < (lens_in[n]-1)/2+1 are computed, the rest up to ld_out written as 0.  ld_out >= (ld_in-1)/2+1 (OV_E_BADARG
 * otherwise); Cout must be a multiple of 16. */
int ov_conv2d_s2_relu_ragged_f32(const float* x, const float* w, const float* bias, const int32_t* lens_in, float* y,
                                 int N, int Cin, int Cout, int Fi, int ld_in, int ld_out, ov_stream_t stream);

/* ov_gru_f32 over lens[n] steps of item n (nn.GRU batch_first, models.py:356-357): gi [N][3H][ld], h_out [N][H] the
 * state after the item's last true step (h0 = 0 for lens[n] = 0).  H must be 128. */
int ov_gru_ragged_f32(const float* gi, const float* whh_t, const float* bhh, const int32_t* lens, float* h_out, int N,
                      int H, int ld, ov_stream_t stream);

/* ---- V1 base-speaker TTS front end (SynthesizerTrn.infer, reference openvoice/models.py:467-490) ----
 * Token-rate tensors are (B, C, T) fp32 with rows `ld` floats apart (ld >= T), like the frame-rate
 * tensors of the converter.  The dense 1x1 / k3 convs of this path go through ov_conv1d_f32. */

/* out[b][h][t] = t < lengths[b] ? emb[tokens[b][t]][h] * scale : 0 -- nn.Embedding * sqrt(H), transposed and
 * masked (models.py:49-54).  tokens [B][T] int64 (ids outside [0, V) are clamped; check them on the host). */
int ov_embed_f32(const int64_t* tokens, const float* emb, const int64_t* lengths, float* out, int B, int T, int H,
                 int V, int ld, float scale, ov_stream_t stream);

enum {
  OV_LN_PRE_RELU = 1, /* relu before the statistics: DurationPredictor conv -> relu -> norm (models.py:91-97) */
  OV_LN_POST_GELU = 2 /* exact (erf) GELU after the affine: DDSConv (modules.py:122-126)                      */
};
/* Channel LayerNorm of modules.py:17-29 / attentions.py:12-24 with the surrounding elementwise ops fused:
 * v = x (+ res) [relu]; y = (v - mean_c) * rstd_c * gamma + beta [gelu]; y += res2; y *= mask[b][t].
 * res, res2, mask may be NULL; out may alias x or res2. */
int ov_layernorm_ch_f32(const float* x, const float* res, const float* gamma, const float* beta, const float* res2,
                        const float* mask, float* out, int B, int C, int T, int ld, float eps, int flags,
                        ov_stream_t stream);

/* Multi-head self-attention with windowed relative-position keys and values (attentions.py:264-329):
 * q, k, v, out are (B, n_heads*dk, T); emb_k / emb_v are the shared [2*window+1][dk] tables; scores of masked
 * (query, key) pairs are set to -1e4 before the softmax as in the reference.  q, k, v share the batch stride
 * qkv_bstride (they may be row blocks of one fused projection output).  dk must be 96; T <= 1172. */
int ov_rel_attention_f32(const float* q, const float* k, const float* v, const float* emb_k, const float* emb_v,
                         const float* mask, float* out, int64_t qkv_bstride, int64_t out_bstride, int B, int n_heads,
                         int dk, int T, int ld, int window, ov_stream_t stream);

/* Depthwise dilated conv on the masked input, DDSConv.convs_sep (modules.py:102-112, :121):
 * out[b][c][t] = bias[c] + sum_j w[c][j] * (x*mask)[b][c][t + (j - (K-1)/2) * dil];  w is [C][K], K odd. */
int ov_dwconv1d_f32(const float* x, const float* w, const float* bias, const float* mask, float* out, int B, int C,
                    int T, int ld, int K, int dil, ov_stream_t stream);

/* ConvFlow.pre (1 -> C pointwise conv) + DDSConv's `x + g` (modules.py:487-488, :118-119):
 * out[b][c][t] = w[c] * x0[b][t] + bias[c] + g[b][c][t]   (g may be NULL); x0 rows are x0_bstride apart. */
int ov_expand1_f32(const float* x0, int64_t x0_bstride, const float* w, const float* bias, const float* g, float* out,
                   int B, int C, int T, int ld, ov_stream_t stream);

/* out[b][c][t] = (x[b][c][t] + bias_b[b][c]) * mask[b][t]: DurationPredictor's `x + cond(g)` and the `x * x_mask`
 * in front of its first conv (models.py:88-90). */
int ov_add_bias_mask_f32(const float* x, const float* bias_b, const float* mask, float* out, int B, int C, int T,
                         int ld, ov_stream_t stream);

/* ConvFlow.forward(reverse=True) after its projection (modules.py:493-511, transforms.py:50-188): channel c1
 * of z (B, 2, T) goes through the inverse rational-quadratic spline with linear tails whose 3*num_bins-1
 * unnormalised parameters are the first rows of h (B, >= 3*num_bins-1, T); both channels are then masked.
 * c0, c1 in {0, 1} select the physical channels (the Flips between flows are not materialised).  num_bins = 10. */
int ov_rq_spline_inverse_f32(float* z, int64_t z_bstride, int c0, int c1, const float* h, int64_t h_bstride,
                             const float* mask, int B, int T, int ld, int num_bins, int filter_channels,
                             float tail_bound, ov_stream_t stream);

/* Durations (models.py:474-479; ElementwiseAffine reverse modules.py:397-399 for the one channel that is used):
 * logw = ((z_sdp - ea_m) * exp(-ea_logs) * mask) * sdp_ratio + dp * (1 - sdp_ratio);
 * cum[b][t] = inclusive prefix sum of ceil(exp(logw) * mask * length_scale) (int32); y_len[b] = max(1, total). */
int ov_duration_f32(const float* z_sdp, int64_t z_bstride, float ea_m, float ea_logs, const float* dp,
                    int64_t dp_bstride, const float* mask, float* logw, int32_t* cum, int64_t* y_len, int B, int T,
                    int ld, float sdp_ratio, float length_scale, ov_stream_t stream);

/* generate_path + the two attn matmuls + the prior sample (models.py:480-487, commons.py:128-142): frame t' of
 * utterance b takes token j with cum[j-1] <= t' < cum[j];  z_p = m_p + noise * exp(logs_p) * noise_scale with
 * m_p = logs_p = 0 for t' >= y_len[b].  m_tok / logs_tok are (B, C, Tx) with batch stride tok_bstride (the two
 * halves of the encoder's projection).  m_p, logs_p (B, C, Ty rows ldy) and attn [B][Ty][Tx] are optional outputs. */
int ov_expand_prior_f32(const float* m_tok, const float* logs_tok, int64_t tok_bstride, int ldx, const int32_t* cum,
                        const int64_t* x_len, const int64_t* y_len, const float* noise, int64_t noise_bstride, int ldn, float* z_p,
                        float* m_p, float* logs_p, float* attn, int B, int C, int Tx, int Ty, int ldy,
                        float noise_scale, ov_stream_t stream);

/* Per-item synthesis controls (additive: same ABI version).  The reference applies sdp_ratio, length_scale and
 * noise_scale element-wise (models.py:474-487), so the items of a batch may each have their own.
 *
 * ov_duration_items_f32 replaces the same lines as ov_duration_f32 (models.py:474-479) with sdp_ratio_b[b] and
 * length_scale_b[b], two [B] fp32 device vectors, in place of the two scalars.  Row b of logw, cum and y_len holds the
 * bits ov_duration_f32 writes there when called with item b's pair; the prefix sum is a workgroup scan. */
int ov_duration_items_f32(const float* z_sdp, int64_t z_bstride, float ea_m, float ea_logs, const float* dp,
                          int64_t dp_bstride, const float* mask, float* logw, int32_t* cum, int64_t* y_len, int B,
                          int T, int ld, const float* sdp_ratio_b, const float* length_scale_b, ov_stream_t stream);

/* ov_expand_prior_f32 (models.py:480-487, commons.py:128-142) with noise_scale_b[b], a [B] fp32 device vector, in
 * place of the scalar: z_p = m_p + noise * exp(logs_p) * noise_scale_b[b].  Every output of item b holds the bits
 * ov_expand_prior_f32 writes when called with noise_scale_b[b]; Tx <= 2^25. */
int ov_expand_prior_items_f32(const float* m_tok, const float* logs_tok, int64_t tok_bstride, int ldx,
                              const int32_t* cum, const int64_t* x_len, const int64_t* y_len, const float* noise,
                              int64_t noise_bstride, int ldn, float* z_p, float* m_p, float* logs_p, float* attn,
                              int B, int C, int Tx, int Ty, int ldy, const float* noise_scale_b, ov_stream_t stream);

/* The streaming form of the same prior sample (csrc/tts_live.hip, openvoice_amd/tts_live.py): ONE launch gives every
 * stream that is ready its next piece of z_p, written straight into the state row of its first live unit.  records is a
 * DEVICE int64 [R][13], record r one stream's piece:
 *   [0] seed, [1] stream   the (seed, stream) pair of its noise_z (purpose 2), as for ov_normal_philox_f32
 *   [2] f0, [3] nf         the frames [f0, f0 + nf) of the sentence
 *   [4] x_len, [5] y_len   the sentence's tokens and frames
 *   [6] m_off, [7] m_ld, [8] logs_off, [9] logs_ld   its token-rate m / logs rows (the two halves of the encoder's
 *                          projection) in tok: m[c][j] = tok[m_off + c * m_ld + j], logs likewise
 *   [10] cum_off           its row of inclusive duration prefix sums: cum[j] = cum_base[cum_off + j]
 *   [11] dst_off, [12] dst_ld   where the piece goes
 * all offsets in elements.  For c < C, i < nf, t = f0 + i and j the token with cum[j-1] <= t < cum[j] (m = logs = 0
 * when no token owns t):
 *   dst[dst_off + c * dst_ld + i] = m[c][j] + n(seed, stream, 2, c, t) * exp(logs[c][j]) * noise_scale_r[r]
 * and nothing else is written.  Each value holds the bits ov_normal_philox_f32 followed by ov_expand_prior_items_f32
 * writes to z_p[c][t] (the three kernels share the Philox / Box-Muller and the expansion arithmetic as device
 * functions).  One thread owns one Philox block, as in ov_normal_philox_f32, so a value does not depend on f0's phase,
 * on alignment, on R or on its neighbours; a block wholly inside the piece at a 16-byte aligned address is one vector
 * store.  noise_scale_r: an fp32 DEVICE vector of R values.  max_frames = the largest nf of the launch sizes the grid
 * only.  Host checks: null pointers, R outside [1, 65535], C <= 0, tok_elems / cum_elems / dst_elems <= 0,
 * max_frames < 0 (OV_E_BADARG); pointers 4-byte aligned (OV_E_ALIGN).  The kernel checks every record: one with a
 * negative field, stream >= 2^32, x_len or y_len outside [1, 2^31), nf < 1, f0 + nf > y_len, nf > dst_ld, or whose
 * m / logs / cum rows leave [0, tok_elems) / [0, cum_elems) or whose piece leaves [0, dst_elems) writes nothing.
 * Additive to ABI 2.12: found by name, like ov_normal_philox_f32. */
int ov_expand_prior_rows_f32(const int64_t* records, int R, int C, const float* tok, int64_t tok_elems,
                             const int32_t* cum, int64_t cum_elems, const float* noise_scale_r, float* dst,
                             int64_t dst_elems, int64_t max_frames, ov_stream_t stream);

/* ---- bf16 generator (BASELINE.json configs[4]; reference openvoice/models.py:272-291, modules.py:296-306) ------
 * Channels-last bf16 activations (B, L, C): C contiguous, rows dense.  bf16 values are passed as uint16_t bit
 * patterns.  Accumulation and bias are fp32; outputs are rounded to nearest even. */
typedef struct ov_conv1d_bf16_params {
  const uint16_t* x;    /* [B][L][Cin] bf16                                                              */
  const uint16_t* w;    /* packed by ov_conv1d_bf16_pack                                                  */
  const float* bias;    /* [Cout] fp32 or NULL                                                            */
  uint16_t* out;        /* [B][L][Cout] bf16                                                              */
  const uint16_t* res;  /* residual, like out, or NULL                                                    */
  const uint16_t* add;  /* second addend (MRF running sum), like out, or NULL                             */
  int32_t B, L, Cin, Cout, K, dil;   /* 'same' padding (K-1)*dil/2; Cin % 32 == 0, Cout % 32 == 0         */
  int32_t phase_s;      /* > 1: ConvTranspose as a phase conv -- Cout = phase_s * C columns ordered
                         * (phase, c); column (ph, c) of row t is written to out[b][t * phase_s + ph][c]    */
  int32_t bias_bstride; /* elements between the bias vectors of consecutive batch items (0 = shared)     */
  int32_t layout;       /* 0 = dispatcher's choice; measurement knobs: 2 = weight fragments requested one k-step
                         * ahead (round-1 scheme) instead of three; otherwise 0                     */
  float in_slope;       /* leaky-ReLU slope applied to x while staging (1.0f = identity)                  */
  float scale;          /* out = (conv + bias + res + add) * scale                                        */
  float out_slope;      /* leaky-ReLU applied to the result before rounding (0 or 1.0f = none): a tensor whose only
                         * consumer activates it (conv1 of a ResBlock pair) is stored activated, and that consumer
                         * stages it with in_slope = 1 -- no unpack / activate / repack pass in its loaders */
  unsigned long long* dbg; /* measurement only, NULL in production: [workgroups][4 matrix waves][8] ticks per phase */
} ov_conv1d_bf16_params;

/* Number of bf16 elements ov_conv1d_bf16_pack writes for a dense fp32 [Cout][Cin][K] weight (0 if unsupported). */
size_t ov_conv1d_bf16_pack_size(int Cout, int Cin, int K);
/* Round a dense HOST fp32 weight to bf16 and lay it out in MFMA B-fragment order (HOST dst). */
int ov_conv1d_bf16_pack(const float* w, int Cout, int Cin, int K, uint16_t* dst);
/* Generator convs in bf16: out = (conv1d(lrelu(x)) + bias [+ res] [+ add]) * scale -- the ResBlock convs
 * (reference openvoice/modules.py:296-306, models.py:280-286; k in {3,7,11}, dilation in {1,3,5}), conv_pre (k7,
 * per-utterance bias = dec.cond, models.py:273-275) and, with phase_s, the ConvTranspose ups (models.py:278-279). */
int ov_conv1d_bf16cl(const ov_conv1d_bf16_params* p, ov_stream_t stream);
/* leaky_relu + conv_post (C -> 1, no bias) + tanh on the bf16 channels-last tensor, fp32 output [B][L]
 * (reference openvoice/models.py:287-289); w is the dense [C][K] fp32 DEVICE weight.  C = 32, K = 7. */
int ov_conv_post_tanh_bf16(const uint16_t* x, const float* w, float* out, int B, int C, int L, int K, float in_slope,
                           ov_stream_t stream);

/* One ResBlock1 iteration in ONE launch on the bf16 channels-last tensors (the fp32 twin: ov_resblock_pair_f32):
 *   out = bf16( (c2(lrelu(bf16(c1(lrelu(x)) + b1))) + b2 + x [+ add]) * scale ),  reference openvoice/modules.py:296-306.
 * The intermediate is rounded to bf16 exactly where the two ov_conv1d_bf16cl launches round it and stays in LDS;
 * results are bit-identical to that path.  w1 / w2 from ov_conv1d_bf16_pack(C, C, K), b1 / b2 fp32 [C].
 * C in {32, 64}; out must not alias x (add may alias out). */
typedef struct ov_respair_bf16_params {
  const uint16_t* x;    /* [B][L][C] bf16 */
  const uint16_t* w1;
  const float* b1;
  const uint16_t* w2;
  const float* b2;
  uint16_t* out;        /* [B][L][C] bf16 */
  const uint16_t* add;  /* MRF running sum, like out, or NULL */
  int32_t B, L, C, K, dil;
  int32_t nwg;          /* 0 = one workgroup per resident slot; n > 0 forces n workgroups (tests) */
  float slope, scale;
  unsigned long long* dbg; /* measurement only, NULL in production: [workgroups][4 waves][9] ticks per phase */
} ov_respair_bf16_params;
int ov_resblock_pair_bf16cl(const ov_respair_bf16_params* p, ov_stream_t stream);
int ov_resblock_pair_bf16_supported(int C, int K, int dil);

/* One ResBlock1 iteration in ONE launch (C in {32, 64, 128}), second generation
 * (csrc/conv1d_bf16_pair2.hip).  Tensors between these launches are stored ACTIVATED:
 *   x   = bf16(lrelu(x_raw, slope))  [B][L][C]            (the producer applied the leaky ReLU before rounding)
 *   t   = bf16(lrelu(c1(x) + b1, slope))                   (never leaves the CU)
 *   out = bf16(act((c2(t) + b2 + x~) * scale)),            x~ = x >= 0 ? x : x / slope  (exact inverse in fp32),
 *         act = leaky ReLU with out_slope (1.0f: the raw sum, for a tensor that is consumed as `add` or by a kernel
 *         that activates on load);
 *   with `add` (a RAW tensor, the MRF running sum):
 *   out = bf16(act((bf16(c2(t) + b2 + x~) + add) * scale)).
 * reference openvoice/modules.py:296-306, models.py:280-286.  w1 / w2 from ov_conv1d_bf16_pack16(C, C, K), b1 / b2
 * fp32 [C].  out must not alias x; add may alias out. */
typedef struct ov_respair2_bf16_params {
  const uint16_t* x;    /* [B][L][C] bf16, activated */
  const uint16_t* w1;
  const float* b1;
  const uint16_t* w2;
  const float* b2;
  uint16_t* out;        /* [B][L][C] bf16 */
  const uint16_t* add;  /* MRF running sum (raw), like out, or NULL */
  int32_t B, L, C, K, dil;
  int32_t nwg;          /* 0 = one workgroup per CU; n > 0 forces n workgroups (tests) */
  float slope;          /* leaky-ReLU slope of x and t, 0 < slope <= 1 */
  float scale;
  float out_slope;      /* 0 or 1.0f = store the raw sum */
  int32_t exp_flags;    /* 0 in production.  MEASUREMENT ONLY: bit 0 = the loader waves idle after the first tile (wrong
                         * results); value 8 = ~500 VALU instructions of busy work per step on the loader waves */
  unsigned long long* dbg; /* measurement only, NULL in production: [workgroups][4 matrix + 4 loader waves][8] ticks per phase */
} ov_respair2_bf16_params;
int ov_resblock_pair2_bf16cl(const ov_respair2_bf16_params* p, ov_stream_t stream);
/* Weights for ov_resblock_pair2_bf16cl (v_mfma_f32_16x16x32_bf16 fragment order; HOST w and dst; dst holds
 * ov_conv1d_bf16_pack_size(Cout, Cin, K) elements, the last 512 an all-zero record). */
int ov_conv1d_bf16_pack16(const float* w, int Cout, int Cin, int K, uint16_t* dst);
int ov_resblock_pair2_bf16_supported(int C, int K, int dil);

/* ---- split-precision Conv1d: fp32-level products on the bf16 matrix pipe (opt-in; csrc/conv1d_split3.h) -----------
 * An fp32 tensor is carried as THREE bf16 planes, v = hi + mid + lo with hi = bf16(v), mid = bf16(v - hi),
 * lo = bf16(v - hi - mid) (round to nearest even; lossless for fp32), channels-last and plane-major: [3][B][L][C].
 * A product x * w is the six plane products of weight >= 2^-18 (hi*hi, hi*mid, mid*hi, hi*lo, lo*hi, mid*mid) on
 * v_mfma_f32_16x16x32_bf16 with fp32 accumulation (`products` = 6), or the three of weight >= 2^-9 on the hi / mid
 * planes only (`products` = 3: 16-bit operands).
 *   out = split3( lrelu( (conv1d(x, w) + bias [+ res~]) * scale, out_slope ) )
 * x is read as stored (the producer stores it activated); res~ = res for res_slope = 1, else the inverse leaky ReLU of
 * res (res >= 0 ? res : res / res_slope: the residual tensor is the conv input of the pair, stored activated).
 * reference: openvoice/modules.py:296-306 (xt = c1(lrelu(x)); xt = c2(lrelu(xt)); x = xt + x).
 * Cin = Cout in {64, 128, 256}, K in {3, 7, 11}, dil in {1, 3, 5} (with res: dil = 1); out must alias neither x nor res.
 * What a launch computes is bit-identical with and without col_limit. */
typedef struct ov_conv1d_split3_params {
  const uint16_t* x;     /* [3][B][L][Cin] bf16 planes */
  const uint16_t* w;     /* ov_conv1d_split3_pack(Cout, Cin, K) */
  const float* bias;     /* [Cout] fp32 */
  uint16_t* out;         /* [3][B][L][Cout] bf16 planes */
  const uint16_t* res;   /* planes like out, or NULL */
  int64_t x_plane, out_plane, res_plane;   /* elements between consecutive planes (>= B * L * C, multiples of 8) */
  int32_t B, L, Cin, Cout, K, dil;
  int32_t nwg;           /* 0 = one workgroup per CU; n > 0 forces n workgroups (tests) */
  int32_t products;      /* 6 or 3 */
  float res_slope;       /* 0 < res_slope <= 1 */
  float out_slope;       /* 0 < out_slope <= 1; 1 = store the raw result */
  float scale;
  int32_t col_limit_scale; /* with col_limit: output columns per unit of col_limit (>= 1) */
  unsigned long long* dbg; /* measurement only, NULL in production: [workgroups][4 matrix waves][8] ticks per phase */
  const int32_t* col_limit; /* DEVICE int32 [B] or NULL: columns of each utterance that matter = col_limit[b] *
                             * col_limit_scale; 128-row time tiles that start at or beyond them are neither computed nor
                             * written (length-aware work lists, as ov_conv1d_params.col_limit; B <= 256, else ignored) */
} ov_conv1d_split3_params;
int ov_conv1d_split3(const ov_conv1d_split3_params* p, ov_stream_t stream);
/* Elements (uint16) of the packed three-plane weight stream; 0 when Cout or Cin is not a multiple of 32. */
size_t ov_conv1d_split3_pack_size(int Cout, int Cin, int K);
/* HOST w [Cout][Cin][K] fp32 -> 16x16x32 A-fragment order, record (((ct * Cin/32 + c) * K + tap) * 3 + plane) * 2 + f,
 * one trailing all-zero record. */
int ov_conv1d_split3_pack(const float* w, int Cout, int Cin, int K, uint16_t* dst);
int ov_conv1d_split3_supported(int Cin, int Cout, int K, int dil);
/* Layout kernels around an MRF stage that runs on ov_conv1d_split3 (the fp32 engine keeps [B][C][L], time contiguous):
 * planes [3][B][L][C] = split3(lrelu(x, slope)) of x [B][C][L] fp32 (reference: the leaky_relu of modules.py:298 moved
 * to the producer), and out [B][C][L] fp32 = (a~ [+ b~] [+ c~]) * scale, each operand de-activated with in_slope (the
 * MRF sum / mean, models.py:280-286).  C even, <= 512. */
int ov_split3_from_f32(const float* x, uint16_t* planes, int64_t plane_stride, int B, int C, int L, float slope,
                       ov_stream_t stream);
int ov_split3_to_f32(const uint16_t* a, const uint16_t* b, const uint16_t* c, int64_t plane_stride, float* out, int B,
                     int C, int L, float in_slope, float scale, ov_stream_t stream);

/* ---- Winograd-domain fp32 Conv1d (round 6; openvoice_amd/csrc/conv1d_wino.h) --------------------------------------
 * The stride-1 'same' convs of ResBlock1, reference openvoice/modules.py:296-306 -- xt = c1(lrelu(x)), xt = c2(lrelu(xt)),
 * x = xt + x -- and the MRF sum / mean of models.py:280-286, with fewer executed multiplies than the direct form:
 *   out = lrelu((conv1d(lrelu(x, in_slope), w, dilation dil) + bias [+ res] [+ add]) * scale, out_slope)
 * evaluated as ceil(K/3) shifted 3-tap groups by the minimal-filtering algorithm F(4, 3) (interpolation points 0, +-1, +-2,
 * infinity): weights transformed once in float64 at pack time, input tiles transformed in fp32 on the way into LDS, the
 * products of all groups and input channels accumulated in the transform domain on v_mfma_f32_32x32x2_f32 (six GEMMs,
 * one per point), the inverse transform + operands in the epilogue.  fp32 arithmetic throughout; executed MACs per
 * output and (co, ci): 1.5 (K = 3), 4 (K = 7), 5.75 (K = 11) instead of K (the products of a group's zero padding taps at
 * points 0 / infinity are identically zero and never issued: K = 7 is laid out with one zero tap at each end).  The transforms round where the direct conv
 * does not: against float64 the result carries ~4x the rounding error of ov_conv1d_f32 (tests/test_gpu_wino.py).
 * Tensors are fp32 [B][C][L], rows x_ld / out_ld floats apart (0 = L); L, x_ld, out_ld multiples of 4 and every
 * pointer 16-byte aligned; Cin % ov_conv1d_wino_chunk(K, Cout) == 0, Cout <= 512 and a multiple of 64 (K = 3 / 7 / 11) or
 * of 32 (K = 11); out must not alias x
 * (it may be the very tensor passed as res or add -- the MRF running sum is accumulated in place). */
typedef struct ov_conv1d_wino_params {
  const float* x;        /* [B][Cin][L] */
  const float* w;        /* ov_conv1d_wino_pack_f32(Cout, Cin, K) */
  const float* bias;     /* [Cout] natural row order; required (zeros if none) */
  float* out;            /* [B][Cout][L] */
  const float* res;      /* residual, indexed like out, or NULL */
  const float* add;      /* second addend (MRF running sum), indexed like out, or NULL */
  int64_t x_bstride, out_bstride, res_bstride, add_bstride;   /* elements between consecutive utterances */
  int32_t B, Cin, Cout, L;
  int32_t x_ld, out_ld;  /* row strides in floats; 0 = L */
  int32_t K, dil;
  int32_t nwg;           /* 0 = one workgroup per resident slot; n > 0 forces n workgroups (tests) */
  int32_t frags;         /* 128-column fragments per matrix wave: 0 = chosen by the dispatcher, else 1 or 2 (tuning knob) */
  float in_slope;        /* leaky-ReLU slope applied to x while staging (1.0f = identity) */
  float scale;
  unsigned long long* dbg; /* measurement only, NULL in production: [workgroups][8 waves][8] shader-clock ticks per phase
                          * (matrix waves: k-step loops, chunk barriers, epilogue, item set-up; helper waves: staging
                          * issue, transform, raw write, barriers); [7] = chunks */
  const int32_t* col_limit; /* DEVICE int32 [B] or NULL: length-aware work list exactly as ov_conv1d_params.col_limit --
                          * column blocks that start at or beyond col_limit[b] * col_limit_scale are neither computed
                          * nor written, what is computed is bit-identical to the full launch; B <= 256, else ignored */
  int32_t col_limit_scale;
  float out_slope;       /* leaky-ReLU slope applied to the RESULT before it is stored (the first conv of a ResBlock pair hands
                          * its consumer an activated tensor, which then stages it with in_slope = 1); 0 or 1 = none; only
                          * without res / add.  (2.09: this field was `reserved0`.) */
} ov_conv1d_wino_params;
int ov_conv1d_wino_f32(const ov_conv1d_wino_params* p, ov_stream_t stream);
/* n = 1 .. 3 INDEPENDENT convs (no conv reads or writes a tensor another one writes) as ONE persistent launch: the three
 * ResBlocks of an MRF step (K = 3, 7, 11 on the same shape).  Every workgroup walks its share of the K = 11 conv, then of
 * the K = 7 conv, then of the K = 3 conv, with no device-wide synchronisation in between; the shares are cut by cost so
 * that the launch ends with K = 3 items.  Every output element is computed by the instruction sequence of the single
 * launch: the results are bit-identical to n calls of ov_conv1d_wino_f32, in any order of `convs`.  Each conv passes the
 * checks of ov_conv1d_wino_f32; beyond them the convs must agree on B, L, Cin, Cout, dil, col_limit, col_limit_scale
 * (OV_E_BADARG) and have pairwise different K, Cout % 64 == 0, frags 0 or 2, dbg NULL (OV_E_UNSUPPORTED); nothing is launched
 * when a check fails.  nwg is read from convs[0]; n = 1 is ov_conv1d_wino_f32(convs).  (Added within 2.12: an additive
 * symbol.) */
int ov_conv1d_wino_multi_f32(const ov_conv1d_wino_params* convs, int n, ov_stream_t stream);
/* 1 when (Cin, Cout, K, dil) has an instance, else 0 (callers then use ov_conv1d_f32). */
int ov_conv1d_wino_supported(int Cin, int Cout, int K, int dil);
/* Input channels per LDS fill of the instance for K taps and Cout rows (Cout % 128 == 0: four 32-row fragments per
 * workgroup; Cout % 64 == 0: two; Cout % 32 == 0: one, K = 11 only); the packed stream is ordered by it; 0 = no instance. */
int ov_conv1d_wino_chunk(int K, int Cout);
/* Floats of the packed transform-domain weights; 0 when the shape has no instance. */
size_t ov_conv1d_wino_pack_size(int Cout, int Cin, int K);
/* HOST w [Cout][Cin][K] fp32 -> U_p[co][g][ci] = sum_k G[p][k] w[co][ci][3g + k] (float64, rounded once to fp32) in
 * 32x32x2 A-fragment order: 1 KiB sub-record ((mt * Cin/CI + c) * (CI * G / 4) + sp) * 3 + j holds for lane l elements
 * 4j .. 4j + 3 of the 12-vector [k-step 2sp: p = 0..5][k-step 2sp + 1: p = 0..5] of row 32 mt + (l & 31) and k-row
 * 2 * kstep + (l >> 5) = g * CI + ci_local of chunk c; three zero sub-records close the stream (HOST dst). */
int ov_conv1d_wino_pack_f32(const float* w, int Cout, int Cin, int K, float* dst);

/* Library/ABI version (major*100 + minor).  2.01: ov_conv1d_params.col_limit, ov_conv_post_tanh_limited_f32,
 * ov_frame_limits_i32.  2.02: ov_unpad_rows_f32, ov_conv1d_bf16_pack16, ov_resblock_pair2_bf16cl (+ _supported).
 * 2.03: ov_conv1d_split3 (+ _pack_size, _pack, _supported), ov_split3_from_f32, ov_split3_to_f32.  2.04:
 * ov_conv1d_split3_params.col_limit / col_limit_scale.  2.05: ov_wn_layer_params.acts / row_split (the field that
 * was `reserved`; the struct grew by one pointer at its end).  2.06: ov_polyphase_fir_f32.  2.07: ov_conv1d_wino_f32 (+ _supported, _chunk,
 * _pack_size, _pack_f32).  2.08: ov_conv1d_wino_f32 instances for Cout % 32 == 0 at K = 11 (one 32-row fragment per
 * workgroup; ov_conv1d_wino_chunk(11, 32) = 2 where 2.07 returned 0).  2.09: ov_conv1d_wino_params.out_slope (the field that
 * was `reserved0`: same size and offset, 0 = none).  2.10: ov_frame_hops_windows_f32, ov_stitch_window_cores_f32.  2.11: ov_frame_hops_multi_f32.  2.12: ov_carry_rows_f32 (and, added later within 2.12 without a version change, ov_polyphase_fir_rows_f32 and ov_vad_frame_energy_f32, ov_vad_segments_i32, ov_vad_compact_f32, ov_rows_f32_to_cl_bf16, ov_cl_bf16_to_rows_f32: additive symbols, which the Python binding looks up by name when it loads the library; likewise ov_wn_layer_wino_f32, ov_wn_layer_wino_tile, ov_wn_wino_pack_size and ov_wn_wino_pack_f32, and ov_join_segments_f32, and ov_pack_groups_cl_bf16 and ov_unpack_groups_f32, and ov_wn_layer_bf16, ov_wn_layer_bf16_supported,
 * ov_wn_layer_bf16_tile, ov_wn_bf16_pack_size and ov_wn_bf16_pack, and ov_wm_embed_windows_f32 and
 * ov_wm_detect_windows_f32, and ov_wm_embed_blocks_f32, and ov_wm_scan_f32, ov_wm_scan_tile and ov_wm_scan_pick,
 * and ov_stretch_rows_f32, and ov_stft_mag_f32,
 * ov_stft_tile_frames and ov_mel_log_f32; and ov_conv1d_params.scale_b, one pointer appended
 * to the struct and read only under OV_F_SCALE_B, a flag no older caller sets: the version stays 212 and a caller built
 * against the shorter struct stays binary compatible).  The Python binding
 * refuses a library older than the entry points it calls (openvoice_amd/_lib.py MIN_VERSION). */
int ov_version(void);
/* The version THIS header describes.  Parameter structs grow at their END in minor versions (2.04, 2.05, 2.07 did): a
 * caller must be compiled against the header of the library it loads -- compare ov_version() with OV_ABI_VERSION at start-up
 * and refuse a mismatch in either direction when it passes parameter structs (the Python bindings do:
 * openvoice_amd/_lib.py MIN_VERSION; the ctypes mirrors are checked field by field against this header in
 * tests/test_abi_cpu.py).  A struct is never reordered and a field never changes meaning within a major version, with
 * one exception stated here: 2.05 renamed ov_wn_layer_params.reserved to row_split AND appended `acts`, so a caller
 * built against 2.04 or older is NOT binary compatible with 2.05+ for that struct. */
#define OV_ABI_VERSION 212
/* 0 for a production build; non-zero = a measurement build with parts of the kernels compiled out (results are
 * meaningless; openvoice_amd/_lib.py refuses to load it unless OPENVOICE_AMD_ALLOW_EXPERIMENT=1). */
int ov_build_experiment(void);

#ifdef __cplusplus
}
#endif
#endif /* OPENVOICE_AMD_H */
