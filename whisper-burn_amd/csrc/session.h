// Stateful decode session: mel -> encoder -> cross-K/V once per window batch, then KV-cached steps.
#pragma once
#include <vector>

#include "decode.h"
#include "engine.h"

namespace wb {
// What a beam search under the timestamp rules leaves on the host: per window the finalized candidates in store order
// (generated tokens, f64 score, rank) and, per step, the live beams behind it (token, parent beam index, f64 score) with the
// number newly finished.  Windows that were not active have n_cand = -1 and no steps.
struct TsBeamResult {
  int W = 0, depth = 0;
  std::vector<int> n_cand, best, n_steps;                      // [W]
  std::vector<std::vector<std::vector<int32_t>>> cand_tokens;  // [W][n_cand]
  std::vector<std::vector<double>> cand_score, cand_rank;      // [W][n_cand]
  std::vector<int> tr_n, tr_fin;                               // [depth][W]
  std::vector<int32_t> tr_tok, tr_par;                         // [depth][W][MAX_BEAMS]
  std::vector<double> tr_score;                                // [depth][W][MAX_BEAMS]
};
}  // namespace wb

struct wb_session {
  wb_model* m = nullptr;
  uint64_t model_uid = 0;       // m->uid at creation: what the pool is keyed by (m may dangle once its model is freed)
  int device = 0;               // m->device, kept so that a session can be destroyed after its model
  hipStream_t st = nullptr;
  hipStream_t st2 = nullptr;       // reads the chained decode's finished flags behind ev_seg while `st` runs ahead
  hipEvent_t ev_seg = nullptr;
  int W = 0, max_beams = 0, S = 0, padding = 0;
  double sample_rate = 16000.0;   // only feeds the mel filterbank (audio.rs:44)
  int Lmax = 0;                 // capacity (positions) of the self-KV cache / tables
  std::vector<int> T, C, row0;  // per window: mel frames (padded), encoder positions, first packed row
  std::vector<wb::MelWindow> wins_host; void* wins_dev_ptr = nullptr;   // what the device window table holds
  std::vector<int> meta_host; void* meta_dev_ptr = nullptr;             // ... and the window meta table
  std::vector<uint8_t> mask_host; void* mask_dev_ptr = nullptr;         // ... and the special-token mask (set_special_mask)
  int enc_rows = 0, maxC = 0, n_chunks = 0;
  wb::Workspace ws;
  wb::DevMem pcm, mel, wins, gmax, enc_out, ckv, win_meta;
  float* pcm_stage = nullptr; size_t pcm_stage_bytes = 0;   // pinned host staging of the caller's PCM (session_encode_pcm)
  wb::DevMem kc, vc, tabs, state;
  wb::StepLayout lay;
  char* host_block = nullptr;           // mapped pinned host memory: step state | top-k ids | top-k log-probs
  char* host_block_dev = nullptr;       // its device-visible address
  size_t host_bytes = 0;
  size_t chain_flags_off = 0;           // offset of the chained decode's per-row progress flags in host_block
  int* state_host = nullptr;            // views into host_block
  int32_t* topk_id_host = nullptr;      // [S][TOPK_MAX]
  float* topk_lp_host = nullptr;
  wb::DevMem x, h, att, Pqkv, Po, Pq, P1, P2, Pa, Pc, carec, ca, logits, tstats, row_stats, mask, lp_tmp, gctl, gtok, hm;
  int sk_qkv = 0, sk_o = 0, sk_1 = 0, sk_2 = 0;                             // its K-splits per weight shape (0: shape not served)
  wb::DevMem ps_layers, ps_roles, ps_ctl, ps_dead, ps_tstats, ps_stamps;   // persistent flag-chained decode (decode_persist.hip)
  wb::DevMem ps_gx, ps_gpa, ps_gpc, ps_gp2, ps_gxn, ps_ghid;     // ... its residual streams / planes as 8-byte {tag, value} granules
  unsigned ps_launches = 0;                     // launches so far: the high half of the granule tags
  int ps_grid = -1;                                                    // co-resident blocks for this model (-1: not asked yet)
  // Launch setup of the persistent kernel (decode_chain.cpp: ps_setup_ensure): the per-layer argument blocks (ps_layers) and
  // the dealt role tables (ps_roles) stay on the device while ps_setup_key -- everything they were built from -- stands.
  // Same rule as wins_host / meta_host / mask_host: the key is voided before the contents change.
  std::vector<uint64_t> ps_setup_key;
  std::vector<wb::PsRole> ps_roles_host;        // the dealt roles (the stamps file names them)
  std::vector<int> ps_role_off_host;            // ... and their blocks
  int ps_setup_grid = 0, ps_setup_n_lg = 0, ps_setup_n_res = 0;
  // pinned host words of a greedy call: [0, ps_pin_back) the control block's seed (host -> device), then what the host reads
  // after the launch (the error word, the control block, the token rows) behind ONE synchronisation
  int* ps_pin = nullptr; size_t ps_pin_ints = 0;
  bool ps_pin_busy = false;                     // a copy out of / into ps_pin may be in flight (no synchronisation since)
  int n_tiles_v = 0, ct_v = 128;
  int ks_qkv = 1, ksl_qkv = 0, ks_o = 1, ksl_o = 0, ks_1 = 1, ksl_1 = 0, ks_2 = 1, ksl_2 = 0, ks_v = 1, ksl_v = 0;
  wb::DevMem bc_ctl, bc_topk;   // device-chained beam search (decode.h: BeamChainArgs): control block, top-k rows of the step
  wb::DevMem sc_ctl, sc_topk;   // device-chained sampling (decode.h: SampleChainArgs): control block, the steps' top-1 rows
  uint64_t sample_sig = 0;      // what the captured sampling steps bake in (session_sample_chain)
  // every sample of the last sampling call (wb_session_last_samples): generated tokens [W][best_of][depth], their counts
  // [W][best_of] (-1: the window was not active)
  std::vector<int32_t> smp_tokens, smp_len; int smp_best_of = 0, smp_depth = 0;
  // device-chained timestamp decoding (decode.h: TsChainArgs): control block, the steps' top-1 rows, and the suppress bytes
  // [2][ceil(V / 4)] words -- suppress, then suppress | suppress_first (wb_session_set_suppress; has_suppress: set on this use)
  wb::DevMem ts_ctl, ts_topk, ts_sup;
  std::vector<uint8_t> ts_sup_host; void* ts_sup_dev_ptr = nullptr;     // what ts_sup holds (same rule as mask_host)
  bool has_suppress = false;
  uint64_t ts_sig = 0;          // what the captured timestamp steps bake in (session_ts_chain)
  // beam search under the timestamp rules (decode.h: TsBeamUpdateArgs): control block, candidate rows; the finalized
  // candidates and the trace of the last call (wb_session_last_beams / wb_session_last_beam_trace)
  wb::DevMem tb_ctl, tb_topk;
  uint64_t tsbeam_sig = 0;
  wb::TsBeamResult tb_last;
  std::vector<int> prev_len, prev_win;
  int prev_n = 0, step = 0;
  bool has_mask = false, decode_ready = false;
  int last_use_mask = 0, last_had_logits = 0;
  wb::PrefillJob prefill_job;       // host staging of the last prefill pass (session_prefill does not wait for its copies)
  int prefill_mode = 0;             // wb_session_set_prefill: 0 the chains prefill a prompt step by step, 1 by one pass (prefill.cpp)
  // profiling only: which kernel classes carried the per-row cached K/V bytes of the last enqueued step, and how many
  // chained steps were enqueued since s->step was last advanced (the chained loop advances it once, at its end)
  int prof_cls_cross = -1, prof_cls_self = -1, prof_step_off = 0;
  // Range-guard words of the 16-bit matrix paths (mapped pinned host memory; the kernels raise them through guard_dev):
  // [0] the split-precision encoder-side GEMM of this session's encode pass (engine.cpp: split_guarded), [1] the
  // split-precision decoder GEMM of its batch-mode steps (dec_split_check).  Per session: sessions of one model on different
  // streams / threads never see or clear each other's flags.
  int* guard_host = nullptr; int* guard_dev = nullptr;
  bool enc_guard_pending = false;   // the encode pass was enqueued with a deferred check (session_enc_guard_resolve)
  wb::MelBatch enc_mb;              // ... its input, kept so the pass can be repeated on the exact-f32 kernel
  std::unordered_map<uint64_t, hipGraphExec_t> graphs;   // captured decode steps, keyed by launch shape
  int64_t n_captures = 0;                                // step graphs captured over the session's life (wb_session_graph_captures)
  uint64_t buf_sig = 0;                                  // signature of the buffers the graphs were captured with
  uint64_t beam_sig = 0;                                 // ... and of the constants of the last device-chained beam search
  void clear_graphs();
  ~wb_session();
};

namespace wb {
// profile accumulators (profile.cpp)
struct Profile {
  bool on = false;
  double ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};
Profile& profile();
// per-kernel-class accumulators of the tagged launches (decode.h: prof_tag / WB_KLAUNCH)
struct KernelStat { int64_t calls = 0; double ms = 0, bytes = 0; };
void prof_adjust_bytes(int cls, double delta);   // correct a class's algorithmic bytes after the fact (dead rows)
void prof_collect();          // after the stream was synchronised: fold the pending tagged launches into the stats
// Timed region helper: records two events on `st` and adds the elapsed ms to slot `i` (when profiling is on).
struct ScopedTimer {
  hipStream_t st; int slot; hipEvent_t a = nullptr, b = nullptr; bool on;
  ScopedTimer(hipStream_t s, int slot_);
  void stop();          // records the end event
  void collect();       // after the stream was synchronised: accumulate
  ~ScopedTimer();
};

void session_pool_register(wb_model* m);   // a model became alive (build_model)
void session_pool_purge(wb_model* m);
int session_create(wb_model* m, int n_windows, int max_beams, int padding, wb_session** out);
// defer_guard: do not synchronise for the encoder's range guard; the caller calls session_enc_guard_resolve after its next
// synchronisation of s->st (the decode's) and, when told so, repeats the decode.
int session_encode_pcm(wb_session* s, const float* pcm, int64_t n_pcm, const int64_t* starts, const int64_t* lens,
                       bool pcm_on_device, bool defer_guard = false);
int session_enc_guard_resolve(wb_session* s, bool* reencoded);
void session_rewind(wb_session* s);      // back to step 0 over the same (re-)encoded window batch
int session_reserve(wb_session* s, int max_len);
// Prompt prefill by ONE teacher-forced pass (prefill.cpp): leaves the session where the n steps
// wb_session_step(tokens[t], parent = t == 0 ? -1 : a, window = wa[a], k = 0), t = 0 .. n - 1, leave it (up to the rounding of
// exact-f32 MFMA GEMMs against the steps' f32 GEMVs).  Enqueues on s->st and does not wait; the session must be at step 0.
int session_prefill(wb_session* s, const int32_t* tokens, int n, const int* wa, int nA);
// the chains' prefill of prompt[0 .. P - 1) for the active windows wa: the pass when the session's mode asks for it (and
// WHISPER_HIP_PREFILL_PASS allows it) on a fresh session, else P - 1 steps
int session_prefill_prompt(wb_session* s, const int32_t* prompt, int P, const int* wa, int nA);
// beam search with the bookkeeping on the device (decode.hip: dec_beam_update_kernel): *handled = false when the shape is not
// served (the caller runs the host-driven search)
int session_beam_chain(wb_session* s, const int32_t* prompt, int prompt_len, int beam_size, int eot, int max_depth,
                       int mask_until_len, int32_t* out_tokens, int32_t row_stride, int32_t* out_lens, bool* handled);
// temperature sampling with the draw and the bookkeeping on the device (sample_chain.cpp); active / stream_ids / out_sum /
// out_best may be null
struct SampleCall { float temperature; int best_of; uint64_t seed; int attempt; };
int session_sample_chain(wb_session* s, const int32_t* prompt, int prompt_len, const SampleCall& sp, const uint8_t* active,
                         const int32_t* stream_ids, int eot, int max_depth, int mask_until_len, int32_t* out_tokens,
                         int32_t row_stride, int32_t* out_lens, double* out_sum, int32_t* out_best);
// timestamp-token decoding with the rules, the pick and the bookkeeping on the device (ts_chain.cpp); active / stream_ids /
// out_sum / out_best may be null
int session_ts_chain(wb_session* s, const wb_timestamp_params& tp, const int32_t* prompt, int prompt_len, const uint8_t* active,
                     const int32_t* stream_ids, int eot, int max_depth, int32_t* out_tokens, int32_t row_stride,
                     int32_t* out_lens, double* out_sum, int32_t* out_best);
// shared by the timestamp chains: the suppress bytes as the kernels' words, and the argument checks
void pack_suppress(const uint8_t* a, const uint8_t* b, int V, uint32_t* out);
int check_ts_params(const wb_timestamp_params& tp, int V, int eot, const char* who);
int check_beam_params(const wb_timestamp_params& tp, const wb_beam_params& bp, int max_beams, int* max_candidates);
// beam search under the timestamp rules with the candidates and the bookkeeping on the device (tsbeam_chain.cpp)
int session_tsbeam_chain(wb_session* s, const wb_timestamp_params& tp, const wb_beam_params& bp, const int32_t* prompt, int prompt_len,
                         const uint8_t* active, int eot, int max_depth, int32_t* out_tokens, int32_t row_stride, int32_t* out_lens,
                         double* out_score, int32_t* out_n_candidates);
int session_greedy_chain(wb_session* s, const int32_t* prompt, int eot, int max_depth, int mask_until_len, int prompt_len,
                         int32_t* out_tokens, int32_t row_stride, int32_t* out_lens);
// wb_session_align (align.cpp); drop_last_rows non-null: drop_last per window instead of the scalar, and a row that leaves
// no DTW row is accepted (all its positions stay -1)
int session_align(wb_session* s, const int32_t* tokens, int32_t row_stride, const int32_t* lens, const int32_t* heads,
                  int32_t n_heads, int32_t n_prefix, int32_t drop_last, int32_t filter_width, int32_t* start_pos,
                  float* matrix, const int32_t* drop_last_rows);
// wb_session_score (score.cpp); token_logprobs may be null (probes only)
int session_score(wb_session* s, const int32_t* tokens, int32_t row_stride, const int32_t* lens, int32_t mask_until_len,
                  const int32_t* probe_ids, int32_t n_probe, int32_t probe_pos, float* token_logprobs,
                  float* probe_logprobs);
}  // namespace wb
