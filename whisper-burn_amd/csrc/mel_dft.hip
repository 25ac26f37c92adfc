// K1r: the reference recipe's log-mel frontend for gfx950 (opt-in: wb_model_set_frontend(m, 1), WB_FRONTEND_REFERENCE).
//
// K1 (mel.hip) computes the log-mel through a 20x20 FFT with exact twiddles: closer to the true log-mel than the
// reference, but not what the reference computes.  The reference's stfft (audio.rs:284-367) is a dense f32 DFT whose
// angle table b[k][n] = f32(f32(k) * f32(2 pi / 400)) * f32(n) reaches ~1250 rad, so each of its angles is off by up to
// ~6e-5 rad; that table, not the summation order, is what separates its log-mel from the exact one.  This kernel
// computes that recipe:
//   table    [416][400] f32 built once on the host (mel_dft_table_build): row 2k = cos(b[k][:]) * w, row 2k+1 =
//            sin(b[k][:]) * (-w) for k < 201 (audio.rs:359-364), rows 402..415 zero; w = the f32 Hann window.  Stored
//            on the device transposed ([400][416], n-major) so that a wave's A operand of one k step is one 128-byte row.
//   stage 0  one tile of 32 frames of one window staged in LDS as [400][33] with K1's reflect indexing at the window
//            edges (audio.rs:297-306; no padded copy)
//   stage 1  [416 x 400] x [400 x 32] on exact-f32 MFMA (v_mfma_f32_32x32x2_f32, bitwise an fmaf chain over k): wave w
//            owns table rows 32w .. 32w+31 = bins 16w .. 16w+15.  The rows of Re and Im of a bin are interleaved, so in
//            the accumulator layout (row = 4 (lane / 32) + (r & 3) + 8 (r / 4)) Re and Im of one bin and frame are the
//            registers r, r+1 of one lane: |X|^2 = re*re + im*im in registers (no contraction: the reference's two
//            squares and one add, audio.rs:39-40)
//   stage 2  sparse Slaney filterbank in ascending bin order, relu(x - 1e-10) + 1e-10, logf(x) / f32(ln 10)
//            (helper.rs:8-10, :24-27; not K1's log2 form), stored UN-normalised; per-tile (max, min) in K1's layout
//            (maxima over n_frames, minima over n_emit); zero padding frames up to pad_limit as K1 writes them
// finalize: relu(x - m8) + m8 with m8 = f32(f64(max) - 8), then (x + 4) / 4 (audio.rs:50-53), on EVERY element --
//           K1's fix-up skips tiles with nothing below m8, up to 1 ulp off this form.
// Bound: f32 MFMA, 332.8 kFLOP per frame (416 x 400 x 2); the table (666 KB) is read from L2 by every block.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "kernels.h"
#include "wave_ops.h"

namespace wb {

namespace {

constexpr int DFT_FT = 32;                        // frames per block: one MFMA column tile, = K1's tile (gmax layout)
constexpr int DFT_WAVES = MEL_DFT_ROWS_PAD / 32;  // 13: one 32-row tile of the table (16 bins) per wave
constexpr int DFT_THREADS = DFT_WAVES * 64;       // 832
constexpr int BROW = DFT_FT + 1;                  // LDS row stride of the frame tile [400][33] and the spectra [201][33]
constexpr int DFT_KU = 8;                         // k steps (of 2) whose A operands are loaded ahead of their MFMAs

typedef float f32x16 __attribute__((ext_vector_type(16)));

__global__ __launch_bounds__(DFT_THREADS) void mel_dft_kernel(
    const float* __restrict__ pcm, const MelWindow* __restrict__ wins, const MelTables* __restrict__ tabs,
    const float* __restrict__ tab_t, float* __restrict__ out, int64_t win_stride, int row_stride,
    float* __restrict__ gmax, int bmax_stride, int pad, int pad_limit) {
  // frame tile B[n][f] (stage 0-1), then the power spectra P[k][f] (stage 2) in the same words
  __shared__ float lds[MEL_N_FFT * BROW];
  __shared__ float red[2][DFT_WAVES];

  const MelWindow w = wins[blockIdx.y];
  const int f0 = blockIdx.x * DFT_FT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int zend = min(w.n_emit + pad, pad_limit);            // frames [n_emit, zend) := 0  (transcribe.rs:171-177)
  if (f0 >= w.n_frames) {
    // only zero padding frames can fall into this tile; no (max, min) pair (as K1: mel.hip)
    float* oz = out + (int64_t)blockIdx.y * win_stride;
    for (int e = tid; e < MEL_N_MELS * DFT_FT; e += DFT_THREADS) {
      const int m = e / DFT_FT, f = f0 + (e - m * DFT_FT);
      if (f >= w.n_emit && f < zend) oz[(int64_t)m * row_stride + f] = 0.f;
    }
    return;
  }
  const int N = w.n_samples;
  const float* x = pcm + w.pcm_off;

  // ---- stage 0: B[n][f] = x[reflect(f0 * 160 - 200 + f * 160 + n)]; consecutive threads read consecutive samples of a
  // frame row, the LDS stride 33 keeps their column writes on distinct banks
  const int g0 = f0 * MEL_HOP - MEL_N_FFT / 2;
  for (int e = tid; e < MEL_N_FFT * DFT_FT; e += DFT_THREADS) {
    const int f = e / MEL_N_FFT, n = e - f * MEL_N_FFT;
    int j = g0 + f * MEL_HOP + n;
    if (j < 0) j = -j;
    if (j >= N) j = 2 * (N - 1) - j;
    j = max(0, min(j, N - 1));   // frames past the window's last frame are never emitted
    lds[n * BROW + f] = x[j];
  }
  __syncthreads();

  // ---- stage 1: D[32 rows of wave w][32 frames] = sum_n T[row][n] B[n][f], n ascending in steps of 2 ----
  // lane l: A = T[32 w + (l & 31)][2 kk + (l >> 5)], B = B[2 kk + (l >> 5)][l & 31]
  const int li = lane & 31, lh = lane >> 5;
  const float* ap = tab_t + (int64_t)lh * MEL_DFT_ROWS_PAD + wave * 32 + li;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; r++) acc[r] = 0.f;
  for (int kb = 0; kb < MEL_N_FFT / 2; kb += DFT_KU) {
    float a[DFT_KU];
#pragma unroll
    for (int u = 0; u < DFT_KU; u++) a[u] = ap[(int64_t)(2 * (kb + u)) * MEL_DFT_ROWS_PAD];
#pragma unroll
    for (int u = 0; u < DFT_KU; u++) {
      const float b = lds[(2 * (kb + u) + lh) * BROW + li];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], b, acc, 0, 0, 0);
    }
  }
  static_assert((MEL_N_FFT / 2) % DFT_KU == 0, "k steps must divide into load batches");
  __syncthreads();   // every wave has consumed the frame tile: the region becomes P[k][f]
  // lane (li, lh), pair j: bin 16 w + 2 lh + (j & 1) + 4 (j >> 1), frame li; Re = acc[2j], Im = acc[2j+1]
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const int k = wave * 16 + 2 * lh + (j & 1) + 4 * (j >> 1);
    if (k < MEL_N_BINS) {
#pragma clang fp contract(off)
      const float re = acc[2 * j], im = acc[2 * j + 1];
      lds[k * BROW + li] = re * re + im * im;
    }
  }
  __syncthreads();

  // ---- stage 2: filterbank (ascending bins), log10, un-normalised store, tile (max, min) ----
  const float LN10 = 2.302585092994045684f;   // f32(ln 10) (helper.rs:24-27)
  float lmax = -INFINITY, lmin = INFINITY;
  float* o = out + (int64_t)blockIdx.y * win_stride + f0;
  for (int e = tid; e < MEL_N_MELS * DFT_FT; e += DFT_THREADS) {
    const int m = e / DFT_FT, f = e - m * DFT_FT;
    const int s0 = tabs->tap_start[m], len = tabs->tap_len[m];
    const float* tw = tabs->tap_w + m * MEL_MAX_TAPS;
    float acc_m = 0.f;
    for (int t = 0; t < len; t++) acc_m = fmaf(tw[t], lds[(s0 + t) * BROW + f], acc_m);
    const float v = __fdiv_rn(logf(fmaxf(acc_m - 1.0e-10f, 0.f) + 1.0e-10f), LN10);
    const int fr = f0 + f;
    if (fr < w.n_frames) lmax = fmaxf(lmax, v);
    if (fr < w.n_emit) { lmin = fminf(lmin, v); o[(int64_t)m * row_stride + f] = v; }
    else if (fr < zend) o[(int64_t)m * row_stride + f] = 0.f;
  }
  lmax = wave_max(lmax);
  lmin = -wave_max(-lmin);
  if (lane == 0) { red[0][wave] = lmax; red[1][wave] = lmin; }
  __syncthreads();
  if (tid == 0) {
    float bm = red[0][0], bn = red[1][0];
#pragma unroll
    for (int i = 1; i < DFT_WAVES; i++) { bm = fmaxf(bm, red[0][i]); bn = fminf(bn, red[1][i]); }
    gmax[((int64_t)blockIdx.y * bmax_stride + blockIdx.x) * 2] = bm;
    gmax[((int64_t)blockIdx.y * bmax_stride + blockIdx.x) * 2 + 1] = bn;
  }
}

// Reference-form clamp and normalisation (audio.rs:50-53) of every emitted element: one block per (tile, window).
__global__ __launch_bounds__(256) void mel_dft_finalize_kernel(const MelWindow* __restrict__ wins, float* __restrict__ out,
                                                               int64_t win_stride, int row_stride,
                                                               const float* __restrict__ bmm, int bmax_stride) {
  __shared__ float wmax;
  const int blk = blockIdx.x, w = blockIdx.y, tid = threadIdx.x;
  const int nblk = (wins[w].n_frames + DFT_FT - 1) / DFT_FT;
  if (blk >= nblk) return;
  if (tid < 64) {   // max of the window (audio.rs:50) = max over its tiles' maxima
    float v = -INFINITY;
    for (int i = tid; i < nblk; i += 64) v = fmaxf(v, bmm[((int64_t)w * bmax_stride + i) * 2]);
    v = wave_max(v);
    if (tid == 0) wmax = v;
  }
  __syncthreads();
  const float m8 = (float)((double)wmax - 8.0);   // f64 max - 8.0, handed to the f32 tensor op as f32
  const int f0 = blk * DFT_FT, nf = min(DFT_FT, wins[w].n_emit - f0);
  float* o = out + (int64_t)w * win_stride + f0;
  for (int e = tid; e < MEL_N_MELS * DFT_FT; e += 256) {
    const int m = e / DFT_FT, f = e - m * DFT_FT;
    if (f < nf) {
      float* q = o + (int64_t)m * row_stride + f;
      const float c = fmaxf(*q - m8, 0.f) + m8;   // tensor_max_scalar (helper.rs:8-10)
      *q = __fdiv_rn(c + 4.0f, 4.0f);
    }
  }
}

}  // namespace

void launch_mel_dft(hipStream_t st, const float* pcm, const MelWindow* wins_dev, int n_windows, int max_frames,
                    const MelTables* tabs_dev, const float* dft_tab_dev, float* out, int64_t win_stride, int row_stride,
                    float* bmax_dev, int pad, int pad_limit) {
  static_assert(DFT_FT == 32, "the (max, min) pairs share K1's tile of 32 frames (mel_bmax_stride)");
  dim3 grid((std::min(max_frames + pad, std::max(pad_limit, max_frames)) + DFT_FT - 1) / DFT_FT, n_windows);
  hipLaunchKernelGGL(mel_dft_kernel, grid, dim3(DFT_THREADS), 0, st, pcm, wins_dev, tabs_dev, dft_tab_dev, out,
                     win_stride, row_stride, bmax_dev, mel_bmax_stride(max_frames), pad, pad_limit);
}

void launch_mel_dft_finalize(hipStream_t st, const MelWindow* wins_dev, int n_windows, float* out, int64_t win_stride,
                             int row_stride, const float* bmax_dev, int max_frames) {
  dim3 grid((max_frames + DFT_FT - 1) / DFT_FT, n_windows);
  hipLaunchKernelGGL(mel_dft_finalize_kernel, grid, dim3(256), 0, st, wins_dev, out, win_stride, row_stride, bmax_dev,
                     mel_bmax_stride(max_frames));
}

// ---- host: the DFT table ---------------------------------------------------------------
// audio.rs:348-364: b[k][n] = (f32(k) * f32(2 pi / 400)) * f32(n) in f32; cos / sin of the f32 angle evaluated in f64 and
// rounded to f32; times w (resp. -w) in f32.  Row-major [402][400]: row 2k = Re, row 2k+1 = Im of bin k.
void mel_dft_table_build(const float* hann400, float* table_402x400) {
  const float coe = (float)(M_PI * 2.0 / 400.0);
  for (int k = 0; k < MEL_N_BINS; k++) {
    const float bk = (float)k * coe;
    for (int n = 0; n < MEL_N_FFT; n++) {
      const float ang = bk * (float)n;
      table_402x400[(2 * k) * MEL_N_FFT + n] = (float)cos((double)ang) * hann400[n];
      table_402x400[(2 * k + 1) * MEL_N_FFT + n] = (float)sin((double)ang) * (-hann400[n]);
    }
  }
}

}  // namespace wb
