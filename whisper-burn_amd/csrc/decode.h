// Launchers of the KV-cached decode-step kernels (decode.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "kernels.h"
#include "wb_internal.h"

namespace wb {

constexpr int MAX_BEAMS = 8;     // live beams per window (reference: beam_size 5, transcribe.rs:232)
constexpr int TOPK_MAX = 8;
constexpr int CA_STRIDE = 66;    // cross-attention chunk partial: m, l, o[64]
constexpr int CA_NCH_MAX = 12;   // most key chunks a (row, head) is split into: ceil(1500 / 128)
constexpr int TS_STRIDE = 2 + 2 * TOPK_MAX;   // logits tile partial: max, sum-exp, k x (value, id)
constexpr int GV_CT = 128;       // columns per GEMV block tile
constexpr int GV_CT_LOGITS = 128; // logits tile (64 = twice the blocks measured slower: 17.7 vs 16.3 us, merge 6.3 vs 4.4 us)
constexpr int KS_MAX = 16;       // most K-split partials any consumer folds

// Per-step state block (ints): header, per-slot arrays, per-window lists.  The host writes it into
// mapped pinned memory; dec_prepare_kernel copies it to device memory for the rest of the step.
enum { ST_N = 0, ST_STEP = 1, ST_HDR = 4 };
// Device control block of the chained greedy decode (ints): step, then cur_tok[S], done[S], out_len[S].
enum { GC_STEP = 0, GC_NDONE = 1, GC_ALLDONE = 2, GC_BAD = 3, GC_HDR = 4 };   // [1]: windows finished so far, [2]: all of them,
                                                                          // [3]: a row had no finite log-prob (top1_or_eot)
struct StepLayout {
  int S = 0, W = 0;                                  // slot capacity, windows
  int tok = 0, parent = 0, len = 0, win = 0;         // offsets of int[S] arrays
  int dead = 0;                                      // int[S]: 1 = this row's window already ended (chained greedy decode):
                                                     // its attention blocks exit at once and stream no cached K/V
  int win_nb = 0, win_slots = 0;                     // int[W], int[W][MAX_BEAMS]
  int total = 0;
};
inline StepLayout make_step_layout(int S, int W) {
  StepLayout l;
  l.S = S; l.W = W;
  l.tok = ST_HDR; l.parent = l.tok + S; l.len = l.parent + S; l.win = l.len + S; l.dead = l.win + S;
  l.win_nb = l.dead + S; l.win_slots = l.win_nb + W; l.total = l.win_slots + W * MAX_BEAMS;
  return l;
}

enum { PRO_PLAIN = 0, PRO_GELU = 1, PRO_ATTN = 2, PRO_LN = 3 };
struct GemvArgs {
  const float* W = nullptr; int ldw = 0;    // [K][ldw] row-major
  int K = 0, N = 0, KS = 1, KSL = 0;        // K-split count / slice length
  int pro = PRO_PLAIN;
  // PLAIN: src [rows][K].  GELU: src = partials [KSp][S][K] of lin1, pbias.  ATTN: src = chunk partials.
  // LN: src = residual stream x_in [S][K] (K == d); pending partials pend [KSp][S][K] + pbias are folded
  //     first (KSp = 0: none), block (0,0) writes the folded stream to x_out, then LayerNorm(g, b, eps).
  const float* src = nullptr; int ld_src = 0;
  const float* pend = nullptr; const float* pbias = nullptr; int KSp = 0;
  float* x_out = nullptr;
  const float* ln_g = nullptr; const float* ln_b = nullptr; float ln_eps = 0.f; int ln_inside = 0;
  int n_head = 0, n_chunks = 0;             // ATTN prologue
  float* P = nullptr;                       // out partials [KS][S][N]
  float* h_tmp = nullptr;                   // [S][K] scratch: LN rows of the 9 - 16-row logits pass (dec_fold_ln_rows_kernel)
  // STATS epilogue (logits): + mask, per-tile max / sum-exp / top-k -> tstats [row][n_tiles][TS_STRIDE]
  const float* mask = nullptr; int use_mask = 0, topk = 0; float* tstats = nullptr;
  const int* st = nullptr; int S = 0;
  int ct = 0;                               // columns per block (0 = 128); multiple of 4
};

void gemv_plan(int K, int N, int* KS, int* KSL);
int cross_attn_chunk();

void launch_dec_prepare(hipStream_t st, const int* state_host_mapped, int* state_dev, const StepLayout& lay, int n,
                        int* tabs, int Lmax, const float* E, const float* pos, int d, float* x, const int* gctl);
void launch_dec_resolve_ln(hipStream_t st, const int* state, int n_max, const float* x_in, float* x_out,
                           const float* P, int KS, int S, const float* bias, int d, const LayerNormW& ln,
                           int eps_inside_sqrt, float* h);
void launch_dec_gemv(hipStream_t st, const GemvArgs& a, int n_rows_hint, bool stats);
bool dec_logits_two_launches(const GemvArgs& a, int n_rows_hint);   // (a with pro = PRO_LN, KS, K, ct, h_tmp set)
void launch_dec_self_attn(hipStream_t st, const int* state, const StepLayout& lay, int n_max, int n_head,
                          const float* Pqkv, int KS, const float* bqkv, int d, float* Kc, float* Vc, const int* tab,
                          int Lmax, float scale, float* att);
// fused query projection of the cross-attention kernel (small models; see dec_cross_attn_kernel)
struct CaFuse {
  const float* x_in = nullptr;    // residual stream [S][d]
  const float* pend = nullptr; int KSp = 0; const float* pbias = nullptr;   // pending out-projection partials + bias
  float* x_out = nullptr;         // folded residual stream (written by block chunk 0 / head 0 of each window)
  const float* ln_g = nullptr; const float* ln_b = nullptr; float ln_eps = 0.f; int ln_inside = 0;
  const float* Wq = nullptr;      // [d][d] row-major
  // fused out-projection (optional): Wo [d][d]; records {m, l, P[d]} go to rec [n_head * n_chunks][S][2 + d]
  const float* Wo = nullptr;
  float* rec = nullptr;
};
bool cross_attn_can_fuse_q(int d);
void launch_dec_cross_attn(hipStream_t st, const int* state, const StepLayout& lay, int n_windows, int n_head,
                           int n_chunks, const float* Pq, int KS, const float* bq, int d, const float* ckv, int ldkv,
                           int koff, const int* win_row0, const int* win_C, float scale, float* ca, int max_nb,
                           const CaFuse* fuse = nullptr);
// batch mode, one beam per window: one block per (head, window) streams the whole cached K/V and writes the normalised
// head outputs to att [S][d] (no chunk partials, no combine launch)
// the streaming kernel with the front of the sublayer inside (fold of the pending planes, cross_attn_ln, Wq): see decode.hip
constexpr int CSF_MAX_D = 1280;
struct CaStreamFuse {
  const float* x_in = nullptr; float* x_out = nullptr;            // residual stream in / folded stream out (head 0's blocks)
  const float* pend = nullptr; int KSp = 0; const float* pbias = nullptr;   // the self-attention out-projection's planes + bias
  const float* ln_g = nullptr; const float* ln_b = nullptr; float ln_eps = 0.f; int ln_inside = 0;
  const float* Wq = nullptr;                                      // [d][d]
};
bool cross_stream_can_fuse(int d);
void launch_dec_cross_attn_stream_fused(hipStream_t st, const int* state, const StepLayout& lay, int n_windows, int n_head,
                                        const float* bq, int d, const float* ckv, int ldkv, int koff, const int* win_row0,
                                        const int* win_C, float scale, float* att, const CaStreamFuse& fz);
void launch_dec_cross_attn_stream(hipStream_t st, const int* state, const StepLayout& lay, int n_windows, int n_head,
                                  const float* Pq, int KS, const float* bq, int d, const float* ckv, int ldkv, int koff,
                                  const int* win_row0, const int* win_C, float scale, float* att);
// what the merge kernel needs to prepare the NEXT chained step (x == nullptr: it does not)
struct NextPrep {
  float* x = nullptr;        // residual-stream rows [S][d] the next step starts from
  const float* E = nullptr;  // token embedding [V][d]
  const float* pos = nullptr;   // decoder positional embedding [n_text_ctx][d]
  int* tabs = nullptr;       // position tables, double-buffered by step parity
  int d = 0;
  // mapped host memory, int[S][2] = (steps completed, finished) per row: the host polls it instead of copying the
  // control block back and synchronising the stream after every chunk of chained steps
  int* hflags = nullptr;
};
void launch_dec_topk_merge(hipStream_t st, int* state, int n_max, const float* tstats, int n_tiles, int k,
                           int32_t* out_id, float* out_lp, float* row_stats, const StepLayout& lay, int* gctl, int* gtok,
                           int Lmax, int eot, const NextPrep& nx);
void launch_dec_gelu_fold(hipStream_t st, const int* state, int n_max, const float* P, int KS, int S, int K,
                          const float* bias, float* out);
void launch_dec_attn_combine(hipStream_t st, const int* state, int n_max, const float* ca, int n_head, int n_chunks,
                             float* out);
void launch_dec_topk_rows(hipStream_t st, int* state, int n_max, const float* logits, int V, const float* mask,
                          int use_mask, int k, int32_t* out_id, float* out_lp, float* row_stats, const StepLayout& lay,
                          int* gctl, int* gtok, int Lmax, int eot);
void launch_dec_logprob_row(hipStream_t st, const float* x, int KS, int64_t plane, int V, const float* mask,
                            int use_mask, const float* stats, float* out);

// ---- device-chained beam search (src/beam.rs:9-110 + transcribe.rs:253-312 on the device) -------------------------
// The host-driven beam search (transcribe.cpp: beam_search_windows) pays a synchronisation, a PCIe read of the top-k and the
// beam bookkeeping per step (~45 us of a ~240 us step at tiny.en).  Here the bookkeeping is a one-block kernel between two
// steps: it reads the step's top-k rows, applies beam_search_step (beam.rs:39-79) window by window in f64 exactly as the host
// code does, runs the termination test of beam.rs:23-27 and writes the NEXT step's state block (token, parent slot, length,
// window of every live beam) to device memory, where dec_prepare_kernel picks it up: the host enqueues step after step
// without looking.  Sequences are a tree of (token, parent node) pairs -- one node per (step, window, beam) -- walked back
// by the host at the end.
constexpr int BEAM_KB = 2 * TOPK_MAX;     // beams a window can hold: k new + k finished (beam.rs:72-78)
enum { BC_DEPTH = 0, BC_ALLDONE = 1, BC_ERR = 2, BC_NLIVE = 3, BC_HDR = 8 };   // header ints of the control block
struct BeamChainLayout {
  int W = 0, max_depth = 0;
  // int offsets: nb[W], done[W], node / fin / prev_slot / slot_now [W][BEAM_KB]; then doubles lp[W][BEAM_KB] (8-byte aligned);
  // then the node pool int2[(max_depth + 1) * W * BEAM_KB]
  int nb = 0, done = 0, node = 0, fin = 0, prev_slot = 0, slot_now = 0, lp = 0, nodes = 0, total_ints = 0;
};
inline BeamChainLayout make_beam_layout(int W, int max_depth) {
  BeamChainLayout b;
  b.W = W; b.max_depth = max_depth;
  b.nb = BC_HDR; b.done = b.nb + W; b.node = b.done + W; b.fin = b.node + W * BEAM_KB; b.prev_slot = b.fin + W * BEAM_KB;
  b.slot_now = b.prev_slot + W * BEAM_KB;
  b.lp = (b.slot_now + W * BEAM_KB + 1) & ~1;
  b.nodes = b.lp + 2 * W * BEAM_KB;
  b.total_ints = b.nodes + 2 * (max_depth + 1) * W * BEAM_KB;
  return b;
}
struct BeamChainArgs {
  int* ctl = nullptr; BeamChainLayout bl;
  const int32_t* topk_id = nullptr; const float* topk_lp = nullptr;   // [S][TOPK_MAX] of the step just run (device memory)
  int* state_out = nullptr; StepLayout lay;                            // the next step's state block (device memory)
  int k = 0, eot = 0, first = 0;                                       // first: no step has run yet (termination test + slots only)
  int V = 0;                                                           // vocabulary: a top-k id outside [0, V) (NaN logits) ends its beam and raises BC_ERR
  int step_pos = 0;                                                    // position index (ST_STEP) of the first decode step
  int* done_flag_host = nullptr;                                       // mapped host word: set when every window has ended
  // dec_prepare_kernel's work for the next step, done here (one launch less per step): position tables + embedding rows
  int* tabs = nullptr; int Lmax = 0; const float* E = nullptr; const float* pos = nullptr; int d = 0; float* x = nullptr;
};
void launch_dec_beam_update(hipStream_t st, const BeamChainArgs& a);

// ---- device-chained temperature sampling (sample.hip, sample_chain.cpp) ------------------------------------------
// Independent rows (slot = active window ordinal * best_of + j), one Gumbel-max draw per row and step on a counter-based
// generator: the bookkeeping kernel behind the logits tail draws the row's token from the step's logits, records it and
// prepares the row for the next step.  Everything a call may vary without changing the launch sequence -- 1 / T, seed,
// attempt, the rows' stream ids -- lives in the control block, so one captured graph serves every temperature and seed.
enum { SC_NDONE = 0, SC_ALLDONE = 1, SC_ERR = 2, SC_NROWS = 3, SC_BEST_OF = 4, SC_ATTEMPT = 5, SC_SEED_LO = 6, SC_SEED_HI = 7,
       SC_INVT = 8, SC_HDR = 16 };   // header ints of the control block ([SC_INVT]: the bits of the f32 1 / T)
struct SampleChainLayout {
  int S = 0, W = 0, max_depth = 0;
  // int offsets: stream / fin / ngen [S], win_fin [W] (finished rows per window); then doubles sum [S] (8-byte aligned);
  // then the generated tokens int[S][max_depth]
  int stream = 0, fin = 0, ngen = 0, win_fin = 0, sum = 0, tokens = 0, total_ints = 0;
};
inline SampleChainLayout make_sample_layout(int S, int W, int max_depth) {
  SampleChainLayout b;
  b.S = S; b.W = W; b.max_depth = max_depth;
  b.stream = SC_HDR; b.fin = b.stream + S; b.ngen = b.fin + S; b.win_fin = b.ngen + S;
  b.sum = (b.win_fin + W + 1) & ~1;
  b.tokens = b.sum + 2 * S;
  b.total_ints = b.tokens + S * max_depth;
  return b;
}
struct SampleChainArgs {
  int* ctl = nullptr; SampleChainLayout sl;
  const float* logits = nullptr; int V = 0;                            // the step's unmasked logits [S][V]
  const float* mask = nullptr; int use_mask = 0;                       // the step's special mask (added when use_mask)
  const float* row_stats = nullptr;                                    // [S][2]: row maximum and log-sum-exp under that mask
  int* state = nullptr; StepLayout lay;                                // the step state block (device memory), updated in place
  int eot = 0;
  // the next step's position tables and embedding rows (what dec_prepare_kernel does for a host-driven step)
  int* tabs = nullptr; int Lmax = 0; const float* E = nullptr; const float* pos = nullptr; int d = 0; float* x = nullptr;
};
void launch_dec_sample_update(hipStream_t st, const SampleChainArgs& a, int n_rows);
// test hook (wb_sample_rows): the draw alone, one block per row, on caller data in device memory
struct SampleRowsArgs {
  const float* logits = nullptr; int R = 0, ld = 0, V = 0;
  const float* mask = nullptr; const uint8_t* row_masked = nullptr;    // mask [V] added to the rows with row_masked[r] != 0
  const float* row_stats = nullptr;                                    // [R][2]
  float inv_t = 1.f; uint32_t seed_lo = 0, seed_hi = 0, attempt = 0;
  const int32_t* stream = nullptr; const int32_t* position = nullptr;  // [R]
  int eot = 0;
  int32_t* out_token = nullptr; float* out_logprob = nullptr; int32_t* out_err = nullptr;   // [R], [R], one word
};
void launch_sample_rows(hipStream_t st, const SampleRowsArgs& a);

// ---- device-chained timestamp decoding (tsrules.hip, ts_chain.cpp) ------------------------------------------------
// The sampling chain's rows and launch shape under Whisper's timestamp rules: the bookkeeping kernel behind the logits tail
// filters the row by the rules (per-row state words + the static suppress bytes, no mask array), picks the token (argmax at
// 1 / T = 0, the Gumbel-max draw of sample.hip otherwise), records it with its log-prob under the filters and prepares the
// next step.  Every rule parameter, 1 / T, seed, attempt and the streams live in the control block: one captured graph serves
// every temperature, seed and rule setting.
enum { TC_NDONE = 0, TC_ALLDONE = 1, TC_ERR = 2, TC_NROWS = 3, TC_BEST_OF = 4, TC_ATTEMPT = 5, TC_SEED_LO = 6, TC_SEED_HI = 7,
       TC_INVT = 8,           // the bits of the f32 1 / T; 0: greedy (the key is the logit itself)
       TC_TB = 9, TC_NTS = 10, TC_MAX_INIT = 11, TC_MAX_TS = 12, TC_HDR = 16 };
struct TsChainLayout {
  int S = 0, W = 0, max_depth = 0;
  // int offsets: stream / fin / ngen / last_was_ts / penult_was_ts / last_ts [S], win_fin [W]; then doubles sum [S] (8-byte
  // aligned); then the generated tokens int[S][max_depth]
  int stream = 0, fin = 0, ngen = 0, last_was = 0, penult_was = 0, last_ts = 0, win_fin = 0, sum = 0, tokens = 0, total_ints = 0;
};
inline TsChainLayout make_ts_layout(int S, int W, int max_depth) {
  TsChainLayout b;
  b.S = S; b.W = W; b.max_depth = max_depth;
  b.stream = TC_HDR; b.fin = b.stream + S; b.ngen = b.fin + S; b.last_was = b.ngen + S; b.penult_was = b.last_was + S;
  b.last_ts = b.penult_was + S; b.win_fin = b.last_ts + S;
  b.sum = (b.win_fin + W + 1) & ~1;
  b.tokens = b.sum + 2 * S;
  b.total_ints = b.tokens + S * max_depth;
  return b;
}
// The rule state of one row (block-uniform): what the filter of a position needs beside the suppress bytes.
struct TsRowState {
  int n_gen = 0;                // tokens generated so far
  int last_was = 0, penult_was = 0;   // gen[-1] / gen[-2] is a timestamp (penult_was is read only when n_gen >= 2)
  int last_ts = -1;             // the last generated timestamp id, -1: none
};
struct TsRules { int tb = 0, n_ts = 0, max_init = -1, max_ts = -1, eot = 0; };
struct TsChainArgs {
  int* ctl = nullptr; TsChainLayout tl;
  const float* logits = nullptr; int V = 0;                            // the step's unmasked logits [S][V]
  const uint32_t* sup = nullptr; const uint32_t* sup_first = nullptr;  // suppress bytes [V] packed 4 per word (pad bytes 0);
                                                                       // sup_first = suppress | suppress_first; null: none
  const float* row_stats = nullptr;                                    // [S][2]: [0] the row maximum over all ids (the key's shift)
  int* state = nullptr; StepLayout lay;
  int eot = 0;
  int* tabs = nullptr; int Lmax = 0; const float* E = nullptr; const float* pos = nullptr; int d = 0; float* x = nullptr;
};
void launch_dec_ts_update(hipStream_t st, const TsChainArgs& a, int n_rows);
// test hook (wb_timestamp_rows): the filter + pick alone, one block per row, on caller data in device memory
struct TsRowsArgs {
  const float* logits = nullptr; int R = 0, ld = 0, V = 0;
  const uint32_t* sup = nullptr; const uint32_t* sup_first = nullptr;
  const float* row_max = nullptr;                                      // [R]: the row maximum over all ids
  TsRules rules;
  float inv_t = 0.f; uint32_t seed_lo = 0, seed_hi = 0, attempt = 0;
  const int32_t* n_gen = nullptr; const int32_t* prev1 = nullptr; const int32_t* prev2 = nullptr; const int32_t* last_ts = nullptr;
  const int32_t* stream = nullptr; const int32_t* position = nullptr;  // [R]
  int32_t* out_token = nullptr; float* out_logprob = nullptr; int32_t* out_forced = nullptr; float* out_stats = nullptr;
  int32_t* out_err = nullptr;                                          // [R], [R], [R], [R][2], one word
};
void launch_ts_rows(hipStream_t st, const TsRowsArgs& a);

// ---- beam search under the timestamp rules (tsbeam.hip, tsbeam_chain.cpp) ------------------------------------------
// Whisper's BeamSearchDecoder on the device, per window: dec_tsbeam_rows_kernel (one block per live row, behind the logits
// tail) leaves the row's B + 1 best allowed ids with their log-probs under the filtered log-softmax;
// dec_tsbeam_update_kernel (one wave per window) ranks the window's candidates by f64 cumulative score, walks them into the
// next live beams and the finished store, carries each child's rule state over from its parent and writes the next step's
// state block.  B, C = max_candidates and every rule parameter live in the control block: one captured graph serves every
// rule setting and patience.
enum { TB_DEPTH = 0, TB_ALLDONE = 1, TB_ERR = 2, TB_NENDED = 3, TB_NWIN = 4, TB_B = 5, TB_C = 6, TB_TB = 7, TB_NTS = 8,
       TB_MAX_INIT = 9, TB_MAX_TS = 10, TB_NLIVE = 11, TB_HDR = 16 };
struct TsBeamLayout {
  int S = 0, W = 0, max_depth = 0;
  // int offsets.  Per window: nb (live beams), ended, nfin (store entries) [W]; per live beam slot / node / last_was /
  // penult_was / last_ts [W][MAX_BEAMS]; store nodes fin_node [W][BEAM_KB] (the node the end-of-text hangs on, -1: the
  // prompt); per row (slot) its beam index row_beam [S]; the trace tr_n / tr_fin [max_depth][W].  Then doubles (8-byte
  // aligned): score [W][MAX_BEAMS], fin_score [W][BEAM_KB], tr_score [max_depth][W][MAX_BEAMS].  Then the node tree
  // int2 (token, parent node) [max_depth][W][MAX_BEAMS]: node (t W + w) MAX_BEAMS + q is live beam q of window w behind step t.
  int nb = 0, ended = 0, nfin = 0, slot = 0, node = 0, last_was = 0, penult_was = 0, last_ts = 0, fin_node = 0, row_beam = 0,
      tr_n = 0, tr_fin = 0, score = 0, fin_score = 0, tr_score = 0, nodes = 0, total_ints = 0;
};
inline TsBeamLayout make_tsbeam_layout(int S, int W, int max_depth) {
  TsBeamLayout b;
  b.S = S; b.W = W; b.max_depth = max_depth;
  const int WB = W * MAX_BEAMS, DW = max_depth * W;
  b.nb = TB_HDR; b.ended = b.nb + W; b.nfin = b.ended + W; b.slot = b.nfin + W; b.node = b.slot + WB; b.last_was = b.node + WB;
  b.penult_was = b.last_was + WB; b.last_ts = b.penult_was + WB; b.fin_node = b.last_ts + WB; b.row_beam = b.fin_node + W * BEAM_KB;
  b.tr_n = b.row_beam + S; b.tr_fin = b.tr_n + DW;
  b.score = (b.tr_fin + DW + 1) & ~1;
  b.fin_score = b.score + 2 * WB; b.tr_score = b.fin_score + 2 * W * BEAM_KB;
  b.nodes = b.tr_score + 2 * DW * MAX_BEAMS;
  b.total_ints = b.nodes + 2 * DW * MAX_BEAMS;
  return b;
}
// what the rows kernel leaves per row behind the [S][TOPK_MAX] id / log-prob arrays: int[S][4]
enum { TBR_COUNT = 0, TBR_FORCED = 1, TBR_TS_LSE = 2, TBR_MN = 3, TBR_STRIDE = 4 };   // [2], [3]: the bits of the f32 statistics
struct TsBeamRowsArgs {
  int* ctl = nullptr; TsBeamLayout bl;
  const float* logits = nullptr; int V = 0;                            // the step's unmasked logits [S][V]
  const uint32_t* sup = nullptr; const uint32_t* sup_first = nullptr;  // as TsChainArgs
  const int* state = nullptr; StepLayout lay;
  int eot = 0;
  int32_t* topk_id = nullptr; float* topk_lp = nullptr; int* row_out = nullptr;   // [S][TOPK_MAX] x 2, [S][TBR_STRIDE]
};
struct TsBeamUpdateArgs {
  int* ctl = nullptr; TsBeamLayout bl;
  const int32_t* topk_id = nullptr; const float* topk_lp = nullptr; const int* row_out = nullptr;
  int* state = nullptr; StepLayout lay;                                // the step state block (device memory), rewritten
  int eot = 0, V = 0;
  int step_pos = 0;                                                    // position index (ST_STEP) of the first decode step
  // the next step's position tables and embedding rows (x == nullptr: the scripted test hook has no model)
  int* tabs = nullptr; int Lmax = 0; const float* E = nullptr; const float* pos = nullptr; int d = 0; float* x = nullptr;
};
void launch_dec_tsbeam_rows(hipStream_t st, const TsBeamRowsArgs& a, int n_rows);
void launch_dec_tsbeam_update(hipStream_t st, const TsBeamUpdateArgs& a);
// test hook (wb_timestamp_beam_rows): the rows kernel's device function alone, one block per row, on caller data
struct TsBeamRowsHookArgs {
  const float* logits = nullptr; int R = 0, ld = 0, V = 0, k = 0;
  const uint32_t* sup = nullptr; const uint32_t* sup_first = nullptr;
  TsRules rules;
  const int32_t* n_gen = nullptr; const int32_t* prev1 = nullptr; const int32_t* prev2 = nullptr; const int32_t* last_ts = nullptr;
  int32_t* out_id = nullptr; float* out_lp = nullptr;                  // [R][k]
  int32_t* out_count = nullptr; int32_t* out_forced = nullptr; float* out_stats = nullptr; int32_t* out_err = nullptr;
};
void launch_tsbeam_rows_hook(hipStream_t st, const TsBeamRowsHookArgs& a);

// ---- fused small-batch sublayer kernels (decode_fused.hip) ----------------------------------------------
// Common prologue of both: x = x_in + (pbias + sum_s pend[s]) (KSp planes of [S][d]; KSp = 0: none), block 0
// writes x to x_out, then LayerNorm(ln_g, ln_b, ln_eps).
struct MlpFusedArgs {
  const int* st = nullptr; int S = 0, d = 0;
  const float* x_in = nullptr; const float* pend = nullptr; int KSp = 0; const float* pbias = nullptr; float* x_out = nullptr;
  // n_chunks > 0: `pend` holds cross-attention chunk records [n_head * n_chunks][S][2 + d] = {m, l, o_chunk Wo} instead of
  // plain partial planes (KSp = n_head * n_chunks): the fold weights plane (h, c) by exp(m_hc - M_h) / sum_c exp(..) l_hc
  int n_head = 0, n_chunks = 0;
  const float* ln_g = nullptr; const float* ln_b = nullptr; float ln_eps = 0.f; int ln_inside = 0;
  const float* W1 = nullptr; int ld1 = 0; const float* b1 = nullptr;     // [d][4d], [4d]
  const float* W2 = nullptr;                                             // [4d][d]
  float* P = nullptr;                                                    // out: planes [4d / 64][S][d] (lin2 bias NOT added)
  unsigned long long* stamps = nullptr;                                  // developer probe (-DWB_STAMPS): phase clock of block 0
  // row groups (9 - 16 live rows on the fused sublayer path): group g = blockIdx.y handles rows [8 g, 8 g + 8); the kernel
  // wrapper sets row0 and shifts x_in / pend / x_out / P by row0 rows (plain planes only, not the record mode)
  int row0 = 0;
  // persistent mode only: the same streams / planes as 8-byte {tag, value} granules (handoff.h)
  const void* g_x_in = nullptr; const void* g_pend = nullptr; void* g_x_out = nullptr; void* g_P = nullptr;
};
struct AttnFusedArgs {
  const int* st = nullptr; StepLayout lay; int S = 0, d = 0, n_head = 0;
  const float* x_in = nullptr; const float* pend = nullptr; int KSp = 0; const float* pbias = nullptr; float* x_out = nullptr;
  const float* ln_g = nullptr; const float* ln_b = nullptr; float ln_eps = 0.f; int ln_inside = 0;
  const float* Wqkv = nullptr; int ldqkv = 0; const float* bqkv = nullptr; float scale = 0.f;   // [d][3d], [3d]
  float* Kc = nullptr; float* Vc = nullptr; const int* tabs = nullptr; int Lmax = 0;            // this layer's cache
  const float* Wo = nullptr;                                                                    // [d][d]
  float* P = nullptr;                                                    // out: planes [n_head][S][d] (out bias NOT added)
  unsigned long long* stamps = nullptr;                                  // developer probe (-DWB_STAMPS): phase clock of block 0
  const void* g_x_in = nullptr; const void* g_pend = nullptr; void* g_x_out = nullptr; void* g_P = nullptr;   // persistent mode
};
struct CrossFusedArgs {
  const int* st = nullptr; StepLayout lay; int S = 0, d = 0, n_head = 0;
  const float* x_in = nullptr; const float* pend = nullptr; int KSp = 0; const float* pbias = nullptr; float* x_out = nullptr;
  const float* ln_g = nullptr; const float* ln_b = nullptr; float ln_eps = 0.f; int ln_inside = 0;
  const float* Wq = nullptr; const float* bq = nullptr; float scale = 0.f;         // [d][d], [d]
  const float* ckv = nullptr; int ldkv = 0, koff = 0;                             // cached cross K|V rows (K pre-scaled)
  const int* win_row0 = nullptr; const int* win_C = nullptr;
  int n_pass = 1;                                                                 // 2: some window has CROSS_FUSED_MAX_C < C <= 2 CROSS_FUSED_MAX_C keys
  const float* Wo = nullptr;                                                      // [d][d]
  float* P = nullptr;                                                             // out: planes [n_head][S][d] (out bias NOT added)
  unsigned long long* stamps = nullptr;
  const void* g_x_in = nullptr; const void* g_pend = nullptr; void* g_x_out = nullptr; void* g_P = nullptr;   // persistent mode
};
// ---- batch mode: skinny split-K weight-stream GEMM (decode_batch.hip) ---------------------------------------------
struct SkinnyArgs {
  const float* A = nullptr; int lda = 0;          // activations [M][K]
  const float* B = nullptr; int ldb = 0;          // weight [K][N] row-major (Linear: [d_in, d_out])
  int M = 0, N = 0, K = 0, ksplit = 1;            // M <= 64, N % 64 == 0, K % (32 ksplit) == 0
  float* P = nullptr; int plane = 0;              // split-K planes out: P[z * plane + r * N + n]  (plane in elements)
  // split-precision variant: the weight as fp16 hi / lo (x 2^11) pieces in MFMA tiles (LinearW::th / tl); null = exact f32
  const uint16_t* Bh = nullptr; const uint16_t* Bl = nullptr;
  int* range_flag = nullptr;                      // raised (mapped host word) when a result of a LIVE row is not finite
  const int* st = nullptr;                        // step state (st[ST_N] = live rows: rows past it hold stale activations); null: all M
};
// W [K][N] f32 -> hi, lo tiles [N / 16][K / 32][4][16][8] fp16 (K % 32 == 0, N % 16 == 0)
void launch_split_weight_f16_tiles(hipStream_t st, const float* W, int K, int N, uint16_t* hi, uint16_t* lo);
int skinny_ksplit(int K, int N, int max_ks, int max_rows);   // 0: shape not served
bool skinny_supported(int M, int K, int N);
int launch_dec_skinny_gemm(hipStream_t st, const SkinnyArgs& a);

// ---- persistent flag-chained greedy decode (decode_persist.hip) --------------------------------------------------
// ONE co-resident grid runs every sublayer of every step of the device-chained greedy loop: a block executes the
// roles i = blockIdx.x, + gridDim.x, ... of a per-step role list in dependency order (self-attention block (head, row),
// cross-attention block (head, row), MLP block (64 hidden units), logits tile (128 vocabulary columns), merge (row)),
// streams each role's weights BEFORE it waits for the arrival counter of the role's producers, and publishes its output
// planes with write-through stores (handoff.h).  No kernel boundary, no grid barrier, fixed summation orders.
struct PsLayerArgs {
  AttnFusedArgs attn; CrossFusedArgs cross; MlpFusedArgs mlp;
  const float* mlp_b2 = nullptr;              // [d]: bias of the layer's second MLP matrix (two-phase MLP roles add it themselves)
};
enum { PSR_ATTN = 0, PSR_CROSS = 1, PSR_MLP = 2, PSR_LOGITS = 3, PSR_MERGE = 4, PSR_FINLN = 5 };
struct PsRole { int kind, layer, a, b; };     // a: head / hidden slice / first tile, b: row (logits: tiles of the role; layer: its ordinal)
constexpr int PS_MAX_FORCED = 8;
struct PersistArgs {
  const PsLayerArgs* layers = nullptr;        // [n_layer] (device)
  const PsRole* roles = nullptr; int n_roles = 0;   // one step's roles, grouped by block, each block's in dependency order (device)
  const int* role_off = nullptr;              // [grid + 1]: block b runs roles [role_off[b], role_off[b + 1]) every step
  // [grid]: the index of block b's role that keeps step-invariant operands resident in LDS for the whole launch (the block's
  // only layer role, a self- or cross-attention one), -1: none.  Null: no block does (WHISPER_HIP_PERSIST_RESIDENT=0)
  const int* res_role = nullptr;
  int n_logits_roles = 0;
  int n_layer = 0, n_rows = 0, S = 0, d = 0, n_head = 0, nb_mlp = 0;
  int n_pass = 1;                             // key passes of the cross-attention roles (2: a window with > CROSS_FUSED_MAX_C keys)
  int* ctl = nullptr;                         // HX_* control words + arrival counters (device; set up by the host)
  int step0 = 0, n_steps = 0;                 // first decode step of the chain, most steps to run
  // prompt prefill inside the launch: the first n_forced steps do not choose their next token -- position step0 + e + 1 holds
  // forced[e] (the rest of the prompt, transcribe.rs:203) -- and skip the logits work
  int n_forced = 0; int forced[PS_MAX_FORCED] = {0, 0, 0, 0, 0, 0, 0, 0};
  int mask_until_len = 0;                     // special-token mask while len <= this (transcribe.rs:271-275)
  // logits role: LN(row) . E^T tile -> (best value, best id) per row and tile.  mlp2: row = x_fin, the last layer's finished rows
  // (granules), normalised by the role itself; else the final-LN role folds x_fin + b2 + sum P2 and leaves LN of it in g_xn
  const void* x_fin = nullptr; const void* P2 = nullptr; const float* b2_last = nullptr;
  void* g_xn = nullptr;                       // planes form only: [S][d] granules ln(x + last MLP), once per row by the final-LN role
  unsigned tag_base = 0;                      // granule tags of this launch: tag_base + 2 + 3 (e n_layer + l) + sublayer
  const float* ln_g = nullptr; const float* ln_b = nullptr; float ln_eps = 0.f; int ln_inside = 0;
  const float* Et = nullptr; int vocab_ld = 0, V = 0; const float* mask = nullptr;
  // tile records [2][S][n_tiles] x 16 bytes {tag, best value, tag, best id} (handoff.h: Rec), double-buffered by step parity,
  // tagged with the step's final-LN tag; zero-filled when allocated
  void* tstats = nullptr; int n_tiles = 0;
  // 1: first-layer self-attention picks the row's next token from the records itself; 0: it waits for the merge role's x row
  // (WHISPER_HIP_PERSIST_PICK=merge).  Travels by value: not part of the cached setup
  int pick = 1;
  // 1: the MLP role runs in two phases (decode_persist.hip, "the MLP edge"): its 64 hidden values per row go to g_hid, every MLP
  // block then finishes 16 columns of the residual row, and the logits roles apply the final LayerNorm to that row themselves
  // (the deal holds no final-LN role); 0: 4 d / 64 partial planes per layer and a final-LN role (WHISPER_HIP_PERSIST_MLP=planes).
  // Travels by value; the dealt roles depend on it (part of the cached setup's key)
  int mlp2 = 1;
  void* g_hid = nullptr;                      // [S][4 d] granules: GELU(hidden) of the layer whose MLP roles are running
  // merge role: argmax over the tiles, chain bookkeeping, next step's embedding
  int* gctl = nullptr; int* gtok = nullptr; int Lmax = 0, eot = 0;
  const float* E = nullptr; const float* pos = nullptr; void* x0 = nullptr; int* tabs = nullptr;   // x0: granules
  int* dead = nullptr;                        // [S]: rows whose window has ended
  unsigned long long* stamps = nullptr;       // optional timeline: [n_steps][n_roles][3] (role start, wait passed, done)
};
// One step's roles dealt to the blocks (decode_chain.cpp; no device, no session).  Layer role i sits on block i % grid; the
// policy decides where the final-LN, logits and merge roles go.  PS_DEAL_SLACK keeps merge(r) and finln(r) off the blocks
// that hold a first-layer self- or cross-attention role (they must be back at their wait, operands requested, before the
// step ends); PS_DEAL_LEGACY puts them on the least loaded blocks.  Every block's list is a subsequence of the one global
// dependency order (layer roles by layer and sublayer, finln, logits, merge).  Two-phase MLP roles (PersistArgs::mlp2) also wait
// for the other MLP roles of their own layer: that form needs nb_mlp <= grid, which puts those roles on different blocks.
enum { PS_DEAL_SLACK = 0, PS_DEAL_LEGACY = 1 };
struct PsDeal {
  std::vector<PsRole> roles;                  // grouped by block
  std::vector<int> role_off;                  // [grid + 1]
  std::vector<int> res_role;                  // [grid]: PersistArgs::res_role (all -1 with res_on false)
  int n_lg = 0, n_res = 0;
  std::vector<int> tail_block;                // [n_rows]: the block kept for row r's final-LN role (it takes no logits tiles)
};
// finln false: no final-LN roles (the logits roles normalise the rows themselves); everything else is dealt as with them
PsDeal ps_deal_roles(int n_layer, int n_head, int n_rows, int nb_mlp, int n_tiles, int grid, int policy, bool res_on,
                     bool finln = true);
int ps_ctl_ints(int S, int n_layer);
bool dec_persist_supported(int d, int n_rows, int max_keys);
int dec_persist_resident_slots(int d, int n_rows, int max_keys);   // resident float4 slots per thread; 0: nothing useful fits
bool dec_persist_resident_geometry(int d, int n_rows, int max_keys, int out[5]);   // {RS, NRND, NWO_A, NVT, NWO_X} of that instance
// grid: blocks of 512 threads that are co-resident on this device for (d, n_rows) -- 0 if the kernel cannot run
int dec_persist_max_grid(int device, int d, int n_rows, int max_keys);
int launch_dec_persist(hipStream_t st, const PersistArgs& a, int grid);
// seeds the granule copy of the first step's x rows: tag = tag_base + 1 (what the first self-attention blocks expect), and
// the control block's stop word (ctl: the HX_* words, zeroed on the stream in front of this): HX_STOP = INT_MAX, the decode goes on
void launch_ps_seed(hipStream_t st, const float* x, int n, void* gx, unsigned tag, int* ctl);
// test-only: the pick of the first-layer self-attention role in isolation (one block): the best of `n_tiles` records tagged
// `tag` -> *out_id (0x7fffffff: no record compares).  ctl: ps_ctl_ints(1, 1) zeroed ints (the sweep's stop / error words)
void launch_ps_pick_test(hipStream_t st, const void* rec, int n_tiles, unsigned tag, int* ctl, int* out_id);
// test-only: ONE layer's MLP roles of the persistent kernel in the two-phase form, alone: 4 d / 64 co-resident blocks, block j =
// hidden slice j, up to 4 rows (d = 128 or 384).  a: the role's arguments with the granule pointers set (g_x_in and g_pend carry
// tag_in; the finished rows land in g_x_out with tag_in + 1); dead [S]: != 0 masks a row; g_hid: (S + 2) x 4 d zeroed granules;
// b2 [d]; ctl: ps_ctl_ints(1, 1) zeroed ints.  -1: the shape is not served or the cooperative launch was refused
struct PsMlp2TestArgs {
  MlpFusedArgs a; int n_rows = 0; const int* dead = nullptr; void* g_hid = nullptr; const float* b2 = nullptr; unsigned tag_in = 0;
  int* ctl = nullptr;
};
int launch_ps_mlp2_test(hipStream_t st, const PsMlp2TestArgs& t);
// test-only: ONE logits role of the persistent kernel over its first n_t tiles (n_t = 1 or 2), a block of its own, up to 4 rows (d =
// 128 or 384).  a.mlp2 = 1: the role sweeps a.x_fin (rows tagged `tag`) and normalises them itself; a.mlp2 = 0: a second block runs the
// final-LN role of every row (a.nb_mlp planes of a.P2 folded onto a.x_fin + a.b2_last -> a.g_xn), then the logits role on a.g_xn.
// Records land in a.tstats [S][a.n_tiles], tagged `tag`.  a.ctl: ps_ctl_ints(1, 1) zeroed ints; a.dead [S].  -1: shape not served
int launch_ps_logits_test(hipStream_t st, const PersistArgs& a, unsigned tag, int n_t);

#if defined(HIPEMU) && !defined(HIPEMU_PROD_GEOMETRY)
// (functional-model build: three tiles per pass, so that micro models run both rings -- one pass at n_audio_ctx = 400
// (C = 200 keys), two passes for its doubled windows (C = 395) and for reference-length windows (C = 745).  The second
// functional-model library, `make prod` in tools/hipemu, compiles the PRODUCT's ring of 768 keys: tests/test_emu_functional.py
// runs the real window lengths through it)
constexpr int CROSS_FUSED_MAX_C = 384;
#else
constexpr int CROSS_FUSED_MAX_C = 768;   // keys per window one pass of the fused cross-attention block holds (n_audio_ctx / 2 = 750)
#endif
constexpr int CROSS_FUSED_MAX_PASSES = 2;   // ... and the passes it can make (C = 1500: the opt-in 30 s window)
void launch_dec_cross_fused(hipStream_t st, const CrossFusedArgs& a, int n_rows_hint);
bool dec_fused_supported(int d);
int dec_mlp_fused_planes(int d);
void launch_dec_mlp_fused(hipStream_t st, const MlpFusedArgs& a, int n_rows_hint);
void launch_dec_attn_fused(hipStream_t st, const AttnFusedArgs& a, int n_rows_hint);
// test-only: the d = 384 self-attention sublayer with n_reg (2 or 4) QKV weight rounds in registers; -1: not served
int launch_dec_attn_fused_rounds(hipStream_t st, const AttnFusedArgs& a, int n_rows_hint, int n_reg);

}  // namespace wb
