// Host-callable launchers of the gfx950 kernels (defined in the .hip files).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

namespace wb {

// ---- per-kernel profiling (wb_profile_enable): the call site tags the NEXT launch of this thread with a kernel
// class and its algorithmic bytes; the launcher hands the tag's start / stop events to the dispatch itself
// (hipExtLaunchKernelGGL), so the elapsed time is that kernel's own begin -> end -- the quantity
// `rocprofv3 --kernel-trace` reports.  With profiling off a tag costs one predictable branch.
enum KernelClass {
  KC_PREPARE = 0, KC_ATTN_FUSED, KC_CROSS_ATTN, KC_GEMV_COUT, KC_MLP_FUSED, KC_LOGITS, KC_TOPK_MERGE,
  KC_GEMV_LN_QKV, KC_SELF_ATTN, KC_GEMV_OUT, KC_GEMV_LN_CQ, KC_GEMV_LN_MLP1, KC_GEMV_MLP2, KC_CROSS_FUSED,
  // batch mode (more than 8 live rows): one class per kernel of the per-layer chain
  KC_B_RESOLVE_LN, KC_B_GEMM, KC_B_SELF_ATTN, KC_B_CROSS_STREAM, KC_B_CROSS_CHUNK, KC_B_COMBINE, KC_B_GELU_FOLD,
  KC_B_LOGITS_GEMM, KC_B_TOPK_ROWS, KC_PERSIST, KC_BEAM_UPDATE, KC_FOLD_LN_ROWS,
  // token alignment (align.hip): at most two launches per decoder layer that owns an alignment head, one DTW launch
  KC_ALIGN_STATS, KC_ALIGN_ACCUM, KC_ALIGN_DTW,
  // token scoring (score.hip): one launch each per scoring call
  KC_SCORE_LOGITS, KC_SCORE_MERGE,
  // temperature sampling (sample.hip): the draw + bookkeeping launch behind a sampling step's logits tail
  KC_SAMPLE_UPDATE,
  // timestamp decoding (tsrules.hip): the filter + pick + bookkeeping launch behind a timestamp step's logits tail
  KC_TS_UPDATE,
  // beam search under the timestamp rules (tsbeam.hip): per-row candidates, per-window bookkeeping
  KC_TSBEAM_ROWS, KC_TSBEAM_UPDATE,
  // prompt prefill (prefill.hip): one launch per decoder layer of a prefill pass
  KC_PREFILL_STORE,
  KC_COUNT
};
void prof_tag(int cls, double algo_bytes);
bool prof_take_events(hipEvent_t* start, hipEvent_t* stop);
#define WB_KLAUNCH(kernel, grid, block, shmem, stream, ...)                                        \
  do {                                                                                             \
    hipEvent_t _pa, _pb;                                                                           \
    if (wb::prof_take_events(&_pa, &_pb))                                                          \
      hipExtLaunchKernelGGL(kernel, grid, block, shmem, stream, _pa, _pb, 0, __VA_ARGS__);         \
    else                                                                                           \
      hipLaunchKernelGGL(kernel, grid, block, shmem, stream, __VA_ARGS__);                         \
  } while (0)


// ---- mel frontend (mel.hip) ---------------------------------------------------------
constexpr int MEL_N_FFT = 400, MEL_HOP = 160, MEL_N_MELS = 80, MEL_N_BINS = 201, MEL_MAX_TAPS = 16;

// the 128-row geometry (large-v3 and later): at 16 kHz its Slaney rows have at most 9 taps; 12 keeps whole float4 chunks
constexpr int MEL128_N_MELS = 128, MEL128_MAX_TAPS = 12;

struct MelTables {            // device-resident constants, built once per (device, sample_rate)
  float hann[400];            // audio.rs:272-278
  float2 tw[400];             // W_400^{n2*k1}, index n2*20+k1
  int tap_start[80];          // sparse Slaney filterbank rows (audio.rs:67-143)
  int tap_len[80];
  float tap_w[80 * MEL_MAX_TAPS];
};
struct MelTables128 {         // the same for 128 mel rows
  float hann[400];
  float2 tw[400];
  int tap_start[MEL128_N_MELS];
  int tap_len[MEL128_N_MELS];
  float tap_w[MEL128_N_MELS * MEL128_MAX_TAPS];
};
// Host-side construction; returns 0 / -1 if a row has more taps than its table holds.  80 rows: the f32 op order of the
// reference.  128 rows: designed in f64 (the Slaney construction as librosa evaluates it), rounded once to f32.
int mel_tables_build(double sample_rate, MelTables* host_out);
int mel_tables_build(double sample_rate, MelTables128* host_out);

struct MelWindow {            // one window of PCM
  int64_t pcm_off;            // offset (samples) of the window start in the PCM buffer
  int32_t n_samples;          // window length in samples (>= 400)
  int32_t n_frames;           // n_samples / 160: frames that enter the max (audio.rs:41-42, :50)
  int32_t n_emit;             // frames written: min(n_frames, clip)  (transcribe.rs:171-177 clips AFTER prep_audio)
  int32_t reserved;
};

// (log10(max(mel,1e-10)) + 4) / 4 for every (window, mel row, frame), zeros for the frames [n_emit, n_emit + pad) below
// pad_limit, + per-tile (max, min) of the un-normalised values.
// out[w][m][t] at out + w*win_stride + m*row_stride + t.  bmax: n_windows * mel_bmax_stride(max_frames) * 2 floats.
int mel_bmax_stride(int max_frames);
void launch_mel_spectrogram(hipStream_t st, const float* pcm, const MelWindow* wins_dev, int n_windows,
                            int max_frames, const MelTables* tabs_dev, float* out, int64_t win_stride,
                            int row_stride, float* bmax_dev, int pad, int pad_limit);
// ... the 128-row instance: out[w] is [128][row_stride]
void launch_mel_spectrogram(hipStream_t st, const float* pcm, const MelWindow* wins_dev, int n_windows,
                            int max_frames, const MelTables128* tabs_dev, float* out, int64_t win_stride,
                            int row_stride, float* bmax_dev, int pad, int pad_limit);
// clamp fix-up: max(x, gmax - 8) (audio.rs:52) on the tiles that need it (normally none: the log-mel is written once)
void launch_mel_finalize(hipStream_t st, const MelWindow* wins_dev, int n_windows, float* out, int64_t win_stride,
                         int row_stride, const float* bmax_dev, int max_frames, int n_mels = MEL_N_MELS);
// reference-recipe frontend (mel_dft.hip): dense f32 DFT on MFMA against the reference's own f32 angle table
// (audio.rs:348-364); same window / output / bmax geometry as the two launches above, but the main kernel stores the
// un-normalised log10 and the finalize applies relu(x - m8) + m8 and (x + 4) / 4 to every emitted element.
constexpr int MEL_DFT_ROWS = 2 * MEL_N_BINS, MEL_DFT_ROWS_PAD = 416;   // Re / Im rows interleaved, padded to 13 x 32
// host: table [402][400] (row 2k = cos(b[k]) * w, row 2k+1 = sin(b[k]) * (-w)) from the f32 Hann window
void mel_dft_table_build(const float* hann400, float* table_402x400);
// dft_tab_dev: the same table transposed and padded, [400][MEL_DFT_ROWS_PAD] (rows >= 402 zero)
void launch_mel_dft(hipStream_t st, const float* pcm, const MelWindow* wins_dev, int n_windows, int max_frames,
                    const MelTables* tabs_dev, const float* dft_tab_dev, float* out, int64_t win_stride, int row_stride,
                    float* bmax_dev, int pad, int pad_limit);
void launch_mel_dft_finalize(hipStream_t st, const MelWindow* wins_dev, int n_windows, float* out, int64_t win_stride,
                             int row_stride, const float* bmax_dev, int max_frames);
void launch_fill_f32(hipStream_t st, float* p, int64_t n, float v);
// 16-bit PCM -> f32 with the reference's scale s / 32767 (bin/transcribe/main.rs:45-52), correctly rounded division
void launch_pcm_s16_to_f32(hipStream_t st, const int16_t* src, int64_t n, float* dst);

// ---- GEMM (gemm.hip): C = act(A*B + bias) (+ residual) (+ aux[aux_idx[m]]) --------------
enum { ACT_NONE = 0, ACT_GELU = 1 };
struct RowDesc {             // optional per-row A addressing (implicit-GEMM conv, packed windows)
  int32_t off;               // element offset of the row start (may be negative: masked k never read)
  int16_t klo, khi;          // A[m][k] := 0 for k outside [klo, khi)   (ROWS mode)
                             // CONV1 mode: klo = 1 if first frame of its window, khi = 1 if last
};
// Alignment: A rows are read as float4 -- A and every row start (m * lda, or desc[m].off) must be 16-byte aligned (lda % 4 == 0,
// off % 4 == 0), and a row's whole quads around [klo, khi) must be readable (the elements outside the mask are discarded, not
// used).  B is read as float4 along N up to ldb (ldb % 4 == 0, B 16-byte aligned): columns [N, ldb) are read and discarded.
struct GemmArgs {
  const float* A = nullptr; int64_t lda = 0;     // ROWS: A[m][k] = A[m*lda + k] (or A[desc[m].off + k])
  const RowDesc* a_desc = nullptr;               // per-row descriptors (device), or null
  int a_mask_align = 1;                          // the caller's guarantee: every klo / khi of a_desc is a multiple of this
                                                 // (the split-precision kernel stages whole octets: it needs a multiple of 8)
  int conv1_tstride = 0;                         // >0 selects CONV1 gather: A[m][ci*3+kk] = A[off + ci*tstride + kk - 1]
  const float* B = nullptr; int ldb = 0;         // [K][N] row-major
  float* C = nullptr; int ldc = 0;
  const float* bias = nullptr;                   // [N]
  const float* residual = nullptr; int ldr = 0;  // [M][N], added after activation.  May alias C ONLY with ksplit <= 1: every
                                                 // kernel reads residual[row][col] and writes C[row][col] from the same thread, once
  const float* aux = nullptr; const int32_t* aux_idx = nullptr; int ld_aux = 0;  // + aux[aux_idx[m]][n]
  float col_scale = 1.f; int col_scale_period = 0, col_scale_width = 0;  // out *= col_scale where (n % period) < width
  int M = 0, N = 0, K = 0;                       // K % 16 == 0
  int act = ACT_NONE;
  int ksplit = 1; int64_t c_split_stride = 0;    // split-K: raw partials of K-slice z go to C + z * c_split_stride
  // column blocks: output column n lands at C + (n / c_block_cols) * c_block_stride + row * ldc + n % c_block_cols (0: plain).
  // The cross-K/V projection of ALL decoder layers is one GEMM over [d][n_layer * 2d]; its output is laid out layer-major
  // ([layer][row][2d]) so that a decode step's pass over ONE layer's cached K/V is one dense stream (session.cpp).
  int c_block_cols = 0; int64_t c_block_stride = 0;
  int* range_flag = nullptr;                     // split-precision kernel only: set to 1 (system scope) when a result is not
                                                 // finite, i.e. an operand left fp16's range (|x| >= 65504)
  // split-precision kernel only -- activations as fp16 PIECES (hi = fp16(x), lo = fp16((x - hi) 2^11); two [M][ld] planes,
  // the same 4 bytes per element as f32), written ONCE by the producer instead of being split by every column block of every
  // consumer GEMM on its way into LDS (round 5: ~100 of the ~226 non-MFMA instructions per k-tile of that kernel):
  const uint16_t* Ah = nullptr; const uint16_t* Al = nullptr;   // A pre-split: A[m][k] pieces at [m * lda + k] (plain rows only)
  uint16_t* Ch = nullptr; uint16_t* Cl = nullptr;               // C as pieces at [row * ldc + col] INSTEAD of the f32 C
};
int launch_gemm_f32(hipStream_t st, const GemmArgs& a);   // exact-f32 MFMA (v_mfma_f32_32x32x2_f32)
// split precision (gemm_f16x3.hip): f32-grade products from three fp16 MFMAs; weight pre-split as Wh, Wl [N][ldwt] fp16
int launch_gemm_f16x3(hipStream_t st, const GemmArgs& a, const uint16_t* Wh, const uint16_t* Wl, int ldwt);
void launch_split_weight_f16(hipStream_t st, const float* W, int K, int N, uint16_t* hi, uint16_t* lo);

// ---- elementwise / normalisation (ops.hip) ----------------------------------------
// y[m] = LN(x[m]) * g + b, biased variance; eps placement per variant (see whisper_hip.h)
// Contract (LayerNorm, its pieces variant and embed): rows are dense ([M][d]) and read / written as float4 -- d % 4 == 0 and
// x, y, g, b (E, pos) 16-byte aligned, yh / yl 8-byte aligned.  The launchers do not check it: with d % 4 != 0 the tail of every
// row would be dropped silently.  Every caller's d is a model width (a multiple of 64).
void launch_layernorm(hipStream_t st, const float* x, float* y, int M, int d, const float* g, const float* b,
                      float eps, int eps_inside_sqrt);
// ... with the result as fp16 pieces (GemmArgs::Ah / Al): yh, yl [M][d]
void launch_layernorm_pieces(hipStream_t st, const float* x, uint16_t* yh, uint16_t* yl, int M, int d, const float* g,
                             const float* b, float eps, int eps_inside_sqrt);
// x[r] = E[tok[r]] + pos[r % L]    (mod.rs:141-146)
void launch_embed(hipStream_t st, const int32_t* tok, int n_rows, int L, int d, const float* E, const float* pos,
                  float* x);

// ---- attention (attention.hip) ---------------------------------------------------
// Prompt prefill (prefill.hip): K | V columns of qkv [nA n][ld] (row a n + p) -> row p S + a of Kc / Vc [Lmax S][d]; tabs
// non-null: also tabs[(n - 1) & 1][a][p] = p S + a.  Returns -1 for a shape it does not serve (nothing launched).
int launch_prefill_store(hipStream_t st, const float* qkv, int nA, int n, int d, int ld, int S, int Lmax, float* Kc, float* Vc,
                         int* tabs);

struct AttnSeg { int32_t q_row0, q_len, kv_row0, kv_len; };   // one (batch) segment of packed rows
// O[q][h*64..] = softmax((Q*s)(K*s)^T [+causal]) V per segment and head, head size 64 (mod.rs:493-533)
// causal: key kv is visible to query q iff kv <= q (positions inside the segment).  kv_len >= 1 for every segment with q_len > 0.
// Contract: rows are read / written as float4 -- ldq % 4 == 0, ldkv % 4 == 0, ldo % 4 == 0 and Q, K, V, O 16-byte aligned
// (Oh / Ol: 8-byte aligned); max_q_len >= every segment's q_len.  The launchers do not check it.
void launch_attention_f32(hipStream_t st, const float* Q, int ldq, const float* K, const float* V, int ldkv,
                          float* O, int ldo, const AttnSeg* segs_dev, int n_segs, int max_q_len, int n_head,
                          float scale, int causal);
// the same with the choice of arithmetic: split = the 16-bit matrix path (fp16 hi / lo operands, three MFMAs per product, f32
// accumulate: f32-grade; operands must stay inside fp16's range -- see attention.hip), else exact f32
// Oh / Ol non-null: the 16-bit kernel writes its output as fp16 pieces there (ldo halves per row) instead of f32 into O.
// Returns true when it did (the caller's next GEMM then reads pieces), false when O holds f32 (exact-f32 kernels).
bool launch_attention(hipStream_t st, const float* Q, int ldq, const float* K, const float* V, int ldkv,
                      float* O, int ldo, const AttnSeg* segs_dev, int n_segs, int max_q_len, int n_head,
                      float scale, int causal, bool split, uint16_t* Oh = nullptr, uint16_t* Ol = nullptr);

// ---- token alignment (align.hip): kept cross-attention weights -> z-score / median / head mean -> DTW ----------------
// Q [rows][ldq] and K [kv rows][ldkv] are the PRE-SCALED cross-attention query / key of one decoder layer (head size 64,
// float4 reads: ldq % 4 == 0, ldkv % 4 == 0, 16-byte aligned); segs as for attention (q_row0 / q_len: the token row,
// kv_row0 / kv_len: its window's encoder positions, kv_len >= 1); heads_dev: the layer's alignment heads in order.
constexpr int ALIGN_MAX_LEN = 448;
// stats[(h * n_rows + row) * ld_stats + q] = (max, sum exp(s - max)) of score row (heads_dev[h], row, q)
void launch_align_row_stats(hipStream_t st, const float* Q, int ldq, const float* K, int ldkv, const AttnSeg* segs_dev,
                            int n_rows, int max_len, const int32_t* heads_dev, int n_heads, float2* stats, int ld_stats);
// M[(row * ld_row + q) * ldm + c] (+)= median_c(zscore_q(softmax weights)) of every head of the list, in order.
// first != 0: the list starts the whole head set (M is written); n_total > 0: it ends it (M = sum / n_total).
// filter_width odd, 1 .. 15; max_len <= ALIGN_MAX_LEN.  Returns 0, or -1 for an unsupported shape (nothing launched).
int launch_align_accumulate(hipStream_t st, const float* Q, int ldq, const float* K, int ldkv, const AttnSeg* segs_dev,
                            int n_rows, int max_len, int max_C, const int32_t* heads_dev, int n_heads, const float2* stats,
                            int ld_stats, float* M, int ld_row, int ldm, int filter_width, int first, int n_total);
// DTW over x[i][j] = (negate ? -1 : 1) * X[(x_row0 + i) * ldx + j], i < n, j < c: out[out0 + i] = column of the first path
// cell of row i.  trace: n_rows * trace_stride words, trace_stride >= max_n * ldt, ldt >= ceil(max c / 4).  n <= 512.
struct DtwSeg { int32_t x_row0, n, c, out0; };
int launch_align_dtw(hipStream_t st, const float* X, int ldx, int negate, const DtwSeg* segs_dev, int n_rows, int max_n,
                     uint32_t* trace, int64_t trace_stride, int ldt, int32_t* out);

// ---- token scoring (score.hip): log-softmax statistics of h E^T without the logits --------------------------------------
// h [R][d] (the final-LayerNorm rows, d % 32 == 0, 16-byte aligned) x Et [d][ldv] (E^T, ldv % 4 == 0, ldv >= V; columns
// [V, ldv) are read and contribute nothing).  Grid: ceil(R / SCORE_BM) row tiles x vs vocabulary splits; split s owns the
// SCORE_BN-column tiles [s T / vs, (s + 1) T / vs) of the T = ceil(V / SCORE_BN) tiles.
// mask [V] (0 / -inf, may be null) is added to the rows with row_masked[r] != 0 only; target[r] in [0, V) or -1;
// probes (probe_row[p] in [0, R), probe_id[p] in [0, V)) are always scored without the mask.
constexpr int SCORE_BM = 32, SCORE_BN = 128;
struct ScoreArgs {
  const float* h = nullptr; int R = 0, d = 0;
  const float* Et = nullptr; int ldv = 0, V = 0;
  const float* mask = nullptr; const uint8_t* row_masked = nullptr;
  const int32_t* target = nullptr;
  const int32_t* probe_row = nullptr; const int32_t* probe_id = nullptr; int n_probe = 0;
  int vs = 1;
  // written by score_logits_kernel: part [vs][R] = (max, sum exp(x - max)) of the row's own statistic (masked when
  // row_masked) and of the unmasked one; target_logit [R] (rows with a target; under the row's mask); probe_logit [n_probe]
  float4* part = nullptr; float* target_logit = nullptr; float* probe_logit = nullptr;
  // written by score_merge_kernel: lse [R] (own statistic), logprob [R] = target_logit - lse (NaN without a target),
  // probe_lp [n_probe] = probe_logit - lse of the unmasked statistic
  float* lse = nullptr; float* logprob = nullptr; float* probe_lp = nullptr;
};
int score_splits(int R, int V, int requested);            // requested <= 0: enough splits to fill the machine at this R
int launch_score_logits(hipStream_t st, const ScoreArgs& a);   // 0, or -1 for an unsupported shape (nothing launched)
void launch_score_merge(hipStream_t st, const ScoreArgs& a);

}  // namespace wb
