// Encoder / decoder orchestration over the gfx950 kernels (host side).
#pragma once
#include <functional>
#include <vector>

#include "kernels.h"
#include "wb_internal.h"

namespace wb {

// Geometry of a batch of mel windows laid out [n_windows][n_mels][row_stride] (n_mels: the model's); T[w] = frames incl. padding.
struct MelBatch {
  const float* mel = nullptr;      // device
  int64_t win_stride = 0;          // floats between windows
  int row_stride = 0;              // floats between mel rows
  std::vector<int> T;              // frames per window (<= n_audio_ctx)
};

struct EncoderOut {
  std::vector<int> C;              // encoder positions per window: (T-1)/2+1  (mod.rs:244 stride-2 conv)
  std::vector<int> row0;           // first packed row of each window
  int rows = 0;                    // sum C
};

// AudioEncoder::forward (mod.rs:228-260) for a packed batch of ragged windows -> out[rows][d].
// (guarded: see split_guarded)
int run_encoder(wb_model* m, hipStream_t st, Workspace& ws, const MelBatch& mb, float* out_dev, EncoderOut* eo);
int run_encoder_unguarded(wb_model* m, hipStream_t st, Workspace& ws, const MelBatch& mb, float* out_dev, EncoderOut* eo);

// Run `body` (a pass that may use the split-precision GEMM, gemm_f16x3.hip) under the range-flag word `flag_host` /
// `flag_dev` (one mapped host word per pass owner: session or model); if the kernel raised it -- an activation outside
// fp16's range -- the model switches to the exact-f32 kernel for good and the pass runs again.  `deferred` non-null: no
// synchronisation here; the caller resolves the flag at its next one (split_guard_resolve) and repeats the work itself.
int split_guarded(wb_model* m, hipStream_t st, int* flag_host, int* flag_dev, bool* deferred,
                  const std::function<int()>& body);
bool split_guard_resolve(wb_model* m, int* flag_host);

// TextDecoder::forward (mod.rs:131-157), stateless: tokens_dev [n*L], enc_dev [n*C][d] -> logits_dev [n*L][V].
int run_decoder_stateless(wb_model* m, hipStream_t st, Workspace& ws, const int32_t* tokens_dev, int n, int L,
                          const float* enc_dev, int C, float* logits_dev);

// Token alignment (align.hip): one teacher-forced pass of the decoder over n token rows, stopped after the query projection
// of the last layer that owns an alignment head; two launches per such layer fold its heads' cross-attention weights into
// M, one DTW launch turns M into start positions.  Everything is enqueued on `st`; the caller synchronises once.
struct AlignJob {
  int n = 0, L = 0;                       // rows; row stride of tokens / M / start_pos (>= every len)
  std::vector<int32_t> tokens;            // [n][L], entries past a row's len: any valid id
  std::vector<int> len, C, kv_row0;       // per row: tokens, encoder positions, first row of its window in the K source
  const float* enc_dev = nullptr;         // non-null: project the cross K here (enc_rows x d input); else use ckv
  int enc_rows = 0;
  const float* ckv = nullptr;             // cached pre-scaled cross K|V: layer i at ckv + i * ckv_layer_stride, rows of ldkv
  int64_t ckv_layer_stride = 0; int ldkv = 0;
  std::vector<int32_t> head_layer, head_id;   // the alignment heads, layers ascending
  int n_prefix = 0, drop_last = 0, filter_width = 7, maxC = 0;
  std::vector<int> drop_rows;             // per-row drop_last (empty: drop_last for every row)
  // host arrays staged to the device by run_align: they live here so that they outlive the enqueued copies
  // (the device side is the workspace's AlignBufs)
  std::vector<AttnSeg> segs_host; std::vector<DtwSeg> dtw_host;
};
int run_align(wb_model* m, hipStream_t st, Workspace& ws, AlignJob& job);

// Token scoring (score.hip): one teacher-forced pass of the whole decoder over n token rows (ragged like AlignJob: rows
// packed with stride L, positions past a row's len carry token 0 and their results are never read), ended by the fused
// logits product that keeps only log-softmax statistics.  Row r = i * L + l is position l of token row i: its target is
// tokens[i][l + 1] (none at the row's last position), scored under `mask_dev` when l + 1 <= mask_until_len; the probes sit
// at position probe_pos of every row, always unmasked.  Everything is enqueued on `st`; the caller synchronises once and
// then reads result_host: logprob [n * L], then probe_lp [n * n_probe].
struct ScoreJob {
  int n = 0, L = 0;
  std::vector<int32_t> tokens;            // [n][L]
  std::vector<int> len, C, kv_row0;       // per row: tokens, encoder positions, first row of its window in the K/V source
  const float* enc_dev = nullptr;         // non-null: project the cross K|V here (enc_rows x d input); else use ckv
  int enc_rows = 0;
  const float* ckv = nullptr;             // cached pre-scaled cross K|V: layer i at ckv + i * ckv_layer_stride, rows of ldkv
  int64_t ckv_layer_stride = 0; int ldkv = 0;
  const float* mask_dev = nullptr;        // [V] 0 / -inf (needed when mask_until_len > 0)
  int mask_until_len = 0;
  std::vector<int32_t> probe_ids; int probe_pos = 0;
  int v_splits = 0;                       // 0: auto
  // host staging (outlives the enqueued copies) and results
  std::vector<AttnSeg> segs_host; std::vector<int32_t> i32_host;
  std::vector<float> result_host;
};
int run_score(wb_model* m, hipStream_t st, Workspace& ws, ScoreJob& job);

// Prompt prefill (prefill.hip): one teacher-forced pass over the SAME n prompt tokens for nA active windows (rows packed
// [a][p]), stopped after the last layer's QKV projection; behind every layer's QKV GEMM the K / V columns go to row p S + a of
// that layer's paged self-KV cache, and the first layer's launch writes the position tables of parity (n - 1) & 1.
// Everything is enqueued on `st`, nothing waits; the job's host arrays outlive the enqueued copies.
struct PrefillJob {
  int nA = 0, n = 0;
  std::vector<int32_t> tokens;            // [n]
  std::vector<int> C, kv_row0;            // per active window: encoder positions, first row of its window in the K/V source
  const float* ckv = nullptr;             // cached pre-scaled cross K|V: layer i at ckv + i * ckv_layer_stride, rows of ldkv
  int64_t ckv_layer_stride = 0; int ldkv = 0;
  int S = 0, Lmax = 0;                    // geometry of the cache: slots per step, positions
  float* kc = nullptr; float* vc = nullptr; int64_t kv_layer_stride = 0;   // layer i's [Lmax S][d] at kc + i * kv_layer_stride
  int* tabs = nullptr;                    // [2][S][Lmax]
  std::vector<AttnSeg> segs_host; std::vector<int32_t> tok_host;
};
int run_prefill(wb_model* m, hipStream_t st, Workspace& ws, PrefillJob& job);
extern std::mutex g_stateless_mu;      // api.cpp: serialises the stateless entry points (they share the model's scratch)

// split-precision fp16 MFMA GEMM when split copies sh / sl ([N][ldwt] fp16) are given and the shape fits, else exact-f32 MFMA
int gemm_dispatch(const wb_model* m, hipStream_t st, const GemmArgs& a, int ldwt, const uint16_t* sh = nullptr,
                  const uint16_t* sl = nullptr);

// Process-wide mel constant tables for (device, sample_rate).
int get_mel_tables(int device, double sample_rate, const MelTables** out_dev);
int get_mel_tables(int device, double sample_rate, const MelTables128** out_dev);

// The log-mel frontend of one call: K1 (mel.hip, WB_FRONTEND_FFT) or the reference recipe (mel_dft.hip,
// WB_FRONTEND_REFERENCE), with its device tables (cached per device).  Every PCM entry point launches through here.
struct MelFrontend {
  int frontend = WB_FRONTEND_FFT;
  int n_mels = MEL_N_MELS;          // 80, or 128 (K1 only: the reference has no 128-row recipe)
  const MelTables* tabs = nullptr;
  const MelTables128* tabs128 = nullptr;   // n_mels == 128
  const float* dft_tab = nullptr;   // reference recipe only: [400][MEL_DFT_ROWS_PAD]
};
// n_mels other than 80 / 128, or the reference recipe at 128 rows -> WB_ERR_ARG
int get_mel_frontend(int device, double sample_rate, int frontend, int n_mels, MelFrontend* out);
// main kernel + finalize; `between` (optional) runs after the main launch (developer trace stages)
void launch_mel_frontend(hipStream_t st, const MelFrontend& fe, const float* pcm, const MelWindow* wins_dev, int n_windows,
                         int max_frames, float* out, int64_t win_stride, int row_stride, float* bmax_dev, int pad,
                         int pad_limit, const std::function<void()>& between = {});
// developer tool (WHISPER_HIP_ENC_TRACE): a stream-ordered copy of one more stage into this thread's encoder trace
void enc_trace_stage(hipStream_t st, const char* name, const void* p, size_t bytes);

}  // namespace wb
