// Beam search under the timestamp rules: the host side of tsbeam.hip (control block, prompt prefill, chunks of steps as one
// graph, Whisper's finalize and ranking), its C ABI and the two test hooks (the rows kernel alone; both kernels without a
// model, driven by a caller's logits callback).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

#include "decode_step.h"

using namespace wb;

namespace wb {

int check_beam_params(const wb_timestamp_params& tp, const wb_beam_params& bp, int max_beams, int* max_candidates) {
  WB_REQUIRE(tp.temperature == 0.f, WB_ERR_ARG, "beam search: temperature %g must be 0", (double)tp.temperature);
  WB_REQUIRE(tp.best_of == 1, WB_ERR_ARG, "beam search: best_of %d must be 1", tp.best_of);
  WB_REQUIRE(bp.beam_size >= 1 && bp.beam_size <= TOPK_MAX - 1, WB_ERR_ARG, "beam search: beam_size %d outside [1, %d]", bp.beam_size,
             TOPK_MAX - 1);
  WB_REQUIRE(bp.beam_size <= max_beams, WB_ERR_ARG, "beam search: beam_size %d above max_beams %d", bp.beam_size, max_beams);
  WB_REQUIRE(std::isfinite(bp.patience) && bp.patience >= 1.f, WB_ERR_ARG, "beam search: patience %g must be finite and >= 1",
             (double)bp.patience);
  WB_REQUIRE(std::isfinite(bp.length_penalty), WB_ERR_ARG, "beam search: length_penalty is not finite");
  const double c = std::nearbyint((double)bp.beam_size * (double)bp.patience);      // round-half-even (the default rounding mode)
  WB_REQUIRE(c <= (double)BEAM_KB, WB_ERR_ARG, "beam search: max_candidates %g above %d", c, BEAM_KB);
  *max_candidates = (int)c;
  return WB_OK;
}

namespace {

// the initial control block: one live beam per active window holding the prompt, score 0, empty rule state, in row a
void tsbeam_init(std::vector<int>& ctl, const TsBeamLayout& bl, const std::vector<int>& wa, const wb_timestamp_params& tp, int B, int C) {
  ctl.assign((size_t)bl.total_ints, 0);
  ctl[TB_NWIN] = (int)wa.size(); ctl[TB_B] = B; ctl[TB_C] = C;
  ctl[TB_TB] = tp.tok_timestamp_begin; ctl[TB_NTS] = tp.n_timestamps;
  ctl[TB_MAX_INIT] = tp.max_initial_timestamp_index; ctl[TB_MAX_TS] = tp.max_timestamp_index;
  for (int w = 0; w < bl.W; w++) ctl[bl.ended + w] = 1;
  for (int i = 0; i < bl.max_depth * bl.W; i++) ctl[bl.tr_n + i] = -1;
  for (size_t a = 0; a < wa.size(); a++) {
    const int w = wa[a], o = w * MAX_BEAMS;
    ctl[bl.ended + w] = 0; ctl[bl.nb + w] = 1;
    ctl[bl.slot + o] = (int)a; ctl[bl.node + o] = -1; ctl[bl.last_ts + o] = -1;
    ctl[bl.row_beam + a] = 0;
  }
  ctl[TB_NLIVE] = (int)wa.size();
}

double beam_rank(double score, int n_text, float length_penalty) {
  if (length_penalty < 0.f) return n_text > 0 ? score / (double)n_text : -std::numeric_limits<double>::infinity();
  return score / std::pow((5.0 + (double)n_text) / 6.0, (double)length_penalty);
}

// Whisper's finalize and ranking over the control block (copied to the host), and the trace.
void tsbeam_finalize(const std::vector<int>& ctl, const TsBeamLayout& bl, const std::vector<int>& wa, int B, float length_penalty,
                     int eot, TsBeamResult& out) {
  const int W = bl.W, D = bl.max_depth;
  const double* score = reinterpret_cast<const double*>(ctl.data() + bl.score);
  const double* fin_score = reinterpret_cast<const double*>(ctl.data() + bl.fin_score);
  const double* tr_score = reinterpret_cast<const double*>(ctl.data() + bl.tr_score);
  const int* nodes = ctl.data() + bl.nodes;
  auto walk = [&](int nd) {
    std::vector<int32_t> seq;
    for (; nd >= 0; nd = nodes[2 * nd + 1]) seq.push_back(nodes[2 * nd]);
    std::reverse(seq.begin(), seq.end());
    return seq;
  };
  out = TsBeamResult();
  out.W = W; out.depth = D;
  out.n_cand.assign(W, -1); out.best.assign(W, -1); out.n_steps.assign(W, 0);
  out.cand_tokens.assign(W, {}); out.cand_score.assign(W, {}); out.cand_rank.assign(W, {});
  out.tr_n.assign((size_t)D * W, 0); out.tr_fin.assign((size_t)D * W, 0);
  out.tr_tok.assign((size_t)D * W * MAX_BEAMS, 0); out.tr_par.assign((size_t)D * W * MAX_BEAMS, 0);
  out.tr_score.assign((size_t)D * W * MAX_BEAMS, 0.0);
  for (int w : wa) {
    auto& toks = out.cand_tokens[w];
    auto& sc = out.cand_score[w];
    for (int i = 0; i < ctl[bl.nfin + w]; i++) {
      toks.push_back(walk(ctl[bl.fin_node + w * BEAM_KB + i]));
      toks.back().push_back(eot);
      sc.push_back(fin_score[w * BEAM_KB + i]);
    }
    if ((int)toks.size() < B) {                    // too few finished: the live beams by descending score (ties: lower index)
      const int nb = ctl[bl.nb + w];
      std::vector<int> order(nb);
      for (int j = 0; j < nb; j++) order[j] = j;
      std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return score[w * MAX_BEAMS + x] > score[w * MAX_BEAMS + y]; });
      for (int j : order) {
        if ((int)toks.size() >= B) break;
        toks.push_back(walk(ctl[bl.node + w * MAX_BEAMS + j]));
        sc.push_back(score[w * MAX_BEAMS + j]);
      }
    }
    out.n_cand[w] = (int)toks.size();
    double best_rank = -std::numeric_limits<double>::infinity();
    int best = 0;
    for (size_t i = 0; i < toks.size(); i++) {
      const int n_text = (int)toks[i].size() - ((!toks[i].empty() && toks[i].back() == eot) ? 1 : 0);
      const double rk = beam_rank(sc[i], n_text, length_penalty);
      out.cand_rank[w].push_back(rk);
      if (rk > best_rank) { best_rank = rk; best = (int)i; }          // (the first of equal maxima)
    }
    out.best[w] = best;
    for (int t = 0; t < D; t++) {
      const int n = ctl[bl.tr_n + t * W + w];
      if (n < 0) break;
      out.n_steps[w] = t + 1;
      out.tr_n[(size_t)t * W + w] = n; out.tr_fin[(size_t)t * W + w] = ctl[bl.tr_fin + t * W + w];
      for (int q = 0; q < n; q++) {
        const int nd = (t * W + w) * MAX_BEAMS + q, par = nodes[2 * nd + 1];
        out.tr_tok[nd] = nodes[2 * nd]; out.tr_par[nd] = par < 0 ? 0 : par % MAX_BEAMS; out.tr_score[nd] = tr_score[nd];
      }
    }
  }
}

int export_beams(const TsBeamResult& r, int32_t cap, int32_t* tokens, int32_t row_stride, int32_t* lens, double* scores, double* ranks,
                 int32_t* n) {
  for (int w = 0; w < r.W; w++) {
    n[w] = r.n_cand[w];
    for (int i = 0; i < std::min(r.n_cand[w], cap); i++) {
      const auto& t = r.cand_tokens[w][i];
      WB_REQUIRE((int)t.size() <= row_stride, WB_ERR_ARG, "row_stride %d < %d", row_stride, (int)t.size());
      std::copy(t.begin(), t.end(), tokens + ((size_t)w * cap + i) * row_stride);
      lens[(size_t)w * cap + i] = (int32_t)t.size();
      scores[(size_t)w * cap + i] = r.cand_score[w][i];
      ranks[(size_t)w * cap + i] = r.cand_rank[w][i];
    }
  }
  return WB_OK;
}

void export_trace(const TsBeamResult& r, int32_t max_steps, int32_t* n_steps, int32_t* n_live, int32_t* n_finished, int32_t* tokens,
                  int32_t* parents, double* scores) {
  const int W = r.W, T = std::min(max_steps, r.depth);
  for (int w = 0; w < W; w++) n_steps[w] = r.n_steps[w];
  for (int t = 0; t < T; t++)
    for (int w = 0; w < W; w++) {
      const size_t o = (size_t)t * W + w;
      n_live[o] = r.tr_n[o]; n_finished[o] = r.tr_fin[o];
      for (int q = 0; q < MAX_BEAMS; q++) {
        tokens[o * MAX_BEAMS + q] = r.tr_tok[o * MAX_BEAMS + q]; parents[o * MAX_BEAMS + q] = r.tr_par[o * MAX_BEAMS + q];
        scores[o * MAX_BEAMS + q] = r.tr_score[o * MAX_BEAMS + q];
      }
    }
}

}  // namespace

// session_ts_chain's structure with the beam search's two launches behind the logits tail.  Rows are dense: the update
// kernel deals the live beams of the windows that have not ended to slots 0 .. n - 1 every step.
int session_tsbeam_chain(wb_session* s, const wb_timestamp_params& tp, const wb_beam_params& bp, const int32_t* prompt, int P,
                         const uint8_t* active, int eot, int max_depth, int32_t* out_tokens, int32_t row_stride, int32_t* out_lens,
                         double* out_score, int32_t* out_n_candidates) {
  wb_model* m = s->m;
  const wb_dims& D = m->dims;
  const int W = s->W, V = D.n_vocab;
  WB_TRY(check_ts_params(tp, V, eot, "beam search"));
  int C = 0;
  WB_TRY(check_beam_params(tp, bp, s->max_beams, &C));
  const int B = bp.beam_size;
  WB_REQUIRE(W <= 64, WB_ERR_ARG, "beam search: %d windows (at most 64 per session)", W);
  WB_REQUIRE(P >= 1 && max_depth >= 0, WB_ERR_ARG, "beam search: prompt_len %d / max_depth %d", P, max_depth);
  WB_REQUIRE(row_stride >= P + max_depth, WB_ERR_ARG, "row_stride %d < %d", row_stride, P + max_depth);
  for (int i = 0; i < P; i++) WB_REQUIRE(prompt[i] >= 0 && prompt[i] < V, WB_ERR_ARG, "prompt token %d out of range", prompt[i]);
  WB_REQUIRE(s->step == 0, WB_ERR_STATE, "wb_session_decode_timestamps_beam: the session is at step %d (wb_session_rewind first)", s->step);
  WB_REQUIRE(s->has_suppress, WB_ERR_STATE, "wb_session_decode_timestamps_beam: wb_session_set_suppress was not called on this session");
  std::vector<int> wa;
  for (int w = 0; w < W; w++)
    if (!active || active[w]) wa.push_back(w);
  const int nA = (int)wa.size();
  if (nA == 0) return WB_OK;
  const int asked_depth = max_depth;
  WB_HIP(hipSetDevice(m->device));
  if (!s->decode_ready || s->Lmax < P + max_depth) WB_TRY(session_reserve(s, P + max_depth + 1));
  max_depth = std::min(max_depth, s->Lmax - (P - 1));
  hipStream_t st = s->st;
  const int S = s->S;
  const StepLayout& L = s->lay;
  // prefill: all prompt tokens but the last only feed the KV cache, one row per active window -- P - 1 steps, or one pass
  // when the session's prefill mode asks for it (prefill.cpp)
  WB_TRY(session_prefill_prompt(s, prompt, P, wa.data(), nA));
  const bool start_finished = prompt[P - 1] == eot;       // nothing is generated behind an end-of-text
  const TsBeamLayout bl = make_tsbeam_layout(S, W, (start_finished || max_depth < 0) ? 0 : max_depth);
  WB_TRY(s->tb_ctl.ensure((size_t)bl.total_ints * 4));
  // candidate ids | log-probs [S][TOPK_MAX], the rows' counts and statistics [S][TBR_STRIDE], the logits tail's own top-1 rows
  WB_TRY(s->tb_topk.ensure((size_t)S * TOPK_MAX * 16 + (size_t)S * TBR_STRIDE * 4));
  std::vector<int> ctl;
  tsbeam_init(ctl, bl, wa, tp, B, C);
  if (bl.max_depth > 0) {
    int* hs = s->state_host;
    memset(hs, 0, (size_t)L.total * 4);
    hs[ST_N] = nA; hs[ST_STEP] = P - 1;
    for (int a = 0; a < nA; a++) {
      hs[L.tok + a] = prompt[P - 1]; hs[L.parent + a] = P > 1 ? a : -1; hs[L.len + a] = P; hs[L.win + a] = wa[a];
      hs[L.win_slots + wa[a] * MAX_BEAMS] = a;
      hs[L.win_nb + wa[a]] = 1;
    }
    WB_HIP(hipMemcpyAsync(s->tb_ctl.p, ctl.data(), ctl.size() * 4, hipMemcpyHostToDevice, st));
    WB_HIP(hipStreamSynchronize(st));
    // launch shape: the bucket of the most rows a call with this beam size can have (W B), so that one graph serves every
    // set of active windows (plan.persist is not consulted: the persistent kernel has no place for the beams)
    const StepPlan plan = plan_step(s, W * B, true);
    TsBeamStepIO io;
    int32_t* base = s->tb_topk.as<int32_t>();
    int32_t* cand_id = base; float* cand_lp = reinterpret_cast<float*>(base + (size_t)S * TOPK_MAX);
    int* row_out = base + (size_t)2 * S * TOPK_MAX;
    io.topk_id = row_out + (size_t)S * TBR_STRIDE;
    io.topk_lp = reinterpret_cast<float*>(io.topk_id + (size_t)S * TOPK_MAX);
    const int G = (V + 3) >> 2;
    TsBeamRowsArgs& r = io.rows;
    r.ctl = s->tb_ctl.as<int>(); r.bl = bl; r.logits = s->logits.as<float>(); r.V = V;
    r.sup = s->ts_sup.as<uint32_t>(); r.sup_first = s->ts_sup.as<uint32_t>() + G;
    r.state = s->state.as<int>(); r.lay = L; r.eot = eot; r.topk_id = cand_id; r.topk_lp = cand_lp; r.row_out = row_out;
    TsBeamUpdateArgs& u = io.upd;
    u.ctl = s->tb_ctl.as<int>(); u.bl = bl; u.topk_id = cand_id; u.topk_lp = cand_lp; u.row_out = row_out;
    u.state = s->state.as<int>(); u.lay = L; u.eot = eot; u.V = V; u.step_pos = P - 1;
    u.tabs = s->tabs.as<int>(); u.Lmax = s->Lmax; u.E = m->tok_emb; u.pos = m->dec_pos; u.d = D.n_text_state; u.x = s->x.as<float>();
    // the captured steps bake in the control block and its layout (S, W: launch_step's buffer signature; max_depth: here),
    // the candidate rows, the suppress buffer, eot and the first step's position: drop THEM when those differ from the last
    // call -- the rule parameters, the beam size's C, patience and length penalty do not
    const uint64_t sig = ((uint64_t)(uintptr_t)s->tb_ctl.p * 1099511628211ull) ^ ((uint64_t)(uintptr_t)s->ts_sup.p * 0x9E3779B97F4A7C15ull) ^
                         ((uint64_t)(uintptr_t)s->tb_topk.p * 0xC2B2AE3D27D4EB4Full) ^ ((uint64_t)max_depth << 20) ^
                         ((uint64_t)(P - 1) << 44) ^ (uint64_t)(unsigned)eot ^ 1u;
    if (sig != s->tsbeam_sig) {
      for (auto it = s->graphs.begin(); it != s->graphs.end();)
        if (it->first & GRAPH_KEY_TSBEAM) { (void)hipGraphExecDestroy(it->second); it = s->graphs.erase(it); }
        else ++it;
      s->tsbeam_sig = sig;
    }
    ScopedTimer tm(st, 3);
    prof_tag(KC_PREPARE, 8.0 * nA * D.n_text_state);
    launch_dec_prepare(st, reinterpret_cast<const int*>(s->host_block_dev), s->state.as<int>(), L, nA, s->tabs.as<int>(), s->Lmax,
                       m->tok_emb, m->dec_pos, D.n_text_state, s->x.as<float>(), nullptr);
    const int chunk = 16;
    int depth = 0;
    int hdr[TB_HDR] = {0};
    while (depth < max_depth) {
      int enq = 0;
      while (depth + enq < max_depth && enq < chunk) {
        const int run = (max_depth - (depth + enq) >= chunk && enq == 0) ? chunk : 1;
        StepCall call;
        call.k = 1; call.use_mask = 0; call.reps = run; call.tbio = &io;
        WB_TRY(launch_step(s, plan, call));
        if (profile().on) profile().ms[4] += run;
        enq += run;
      }
      depth += enq;
      WB_HIP(hipMemcpyAsync(hdr, s->tb_ctl.p, sizeof(hdr), hipMemcpyDeviceToHost, st));
      WB_HIP(hipStreamSynchronize(st));
      if (hdr[TB_ALLDONE] || hdr[TB_ERR]) break;   // every window has ended: the kernels of further steps would exit at once
    }
    tm.stop();
    WB_HIP(hipMemcpyAsync(ctl.data(), s->tb_ctl.p, ctl.size() * 4, hipMemcpyDeviceToHost, st));
    WB_HIP(hipStreamSynchronize(st));
    tm.collect();
    if (profile().on) prof_collect();
    s->prof_step_off = 0;
  }
  s->step += ctl[TB_DEPTH];
  s->prev_n = 0; s->prev_len.clear(); s->prev_win.clear();     // (the device-side slots are not mirrored: no host-driven step may follow)
  s->last_had_logits = 0;
  WB_TRY(dec_split_check(s));
  WB_REQUIRE(ctl[TB_ERR] == 0, WB_ERR_STATE, "beam search: a logits row or a score was not finite, or the rules left a beam no id");
  tsbeam_finalize(ctl, bl, wa, B, bp.length_penalty, eot, s->tb_last);
  bool all_done = true;
  for (int w : wa) {
    const TsBeamResult& r = s->tb_last;
    const auto& seq = r.cand_tokens[w][r.best[w]];
    int32_t* row = out_tokens + (size_t)w * row_stride;
    for (int i = 0; i < P; i++) row[i] = prompt[i];
    std::copy(seq.begin(), seq.end(), row + P);
    out_lens[w] = P + (int32_t)seq.size();
    if (out_score) out_score[w] = r.cand_score[w][r.best[w]];
    if (out_n_candidates) out_n_candidates[w] = r.n_cand[w];
    all_done = all_done && (ctl[bl.ended + w] != 0 || start_finished);
  }
  if (max_depth < asked_depth && !all_done)
    WB_REQUIRE(false, WB_ERR_SHAPE, "Token sequence length %d must not exceed %d.", s->Lmax + 1, s->Lmax);
  return WB_OK;
}

}  // namespace wb

extern "C" {

void wb_beam_params_default(wb_beam_params* p) {
  if (!p) return;
  p->beam_size = 5; p->patience = 1.0f; p->length_penalty = -1.0f;
}

int wb_session_decode_timestamps_beam(wb_session* s, const wb_decode_params* p, const wb_timestamp_params* tp,
                                      const wb_beam_params* bp, const int32_t* prompt, int32_t prompt_len, const uint8_t* active,
                                      int32_t* out_tokens, int32_t row_stride, int32_t* out_lens, double* out_score,
                                      int32_t* out_n_candidates) {
  WB_REQUIRE(s && p && tp && bp && prompt && out_tokens && out_lens, WB_ERR_ARG, "wb_session_decode_timestamps_beam: null argument");
  wb::GpuTurn turn(s->device);
  return session_tsbeam_chain(s, *tp, *bp, prompt, prompt_len, active, p->tok_end_of_text, p->max_depth, out_tokens, row_stride,
                              out_lens, out_score, out_n_candidates);
}

int wb_session_last_beams(wb_session* s, int32_t cap, int32_t* tokens, int32_t row_stride, int32_t* lens, double* scores,
                          double* ranks, int32_t* n) {
  WB_REQUIRE(s && tokens && lens && scores && ranks && n && cap >= 1 && row_stride >= 1, WB_ERR_ARG, "wb_session_last_beams: bad argument");
  WB_REQUIRE(s->tb_last.W == s->W, WB_ERR_STATE, "wb_session_last_beams: no beam search has run on this session");
  return export_beams(s->tb_last, cap, tokens, row_stride, lens, scores, ranks, n);
}

int wb_session_last_beam_trace(wb_session* s, int32_t max_steps, int32_t* n_steps, int32_t* n_live, int32_t* n_finished,
                               int32_t* tokens, int32_t* parents, double* scores) {
  WB_REQUIRE(s && n_steps && n_live && n_finished && tokens && parents && scores && max_steps >= 0, WB_ERR_ARG,
             "wb_session_last_beam_trace: bad argument");
  WB_REQUIRE(s->tb_last.W == s->W, WB_ERR_STATE, "wb_session_last_beam_trace: no beam search has run on this session");
  export_trace(s->tb_last, max_steps, n_steps, n_live, n_finished, tokens, parents, scores);
  return WB_OK;
}

int wb_timestamp_beam_rows(int device, const float* logits, int32_t R, int32_t ld, int32_t V, const uint8_t* suppress,
                           const uint8_t* suppress_first, int32_t tok_timestamp_begin, int32_t n_timestamps,
                           int32_t max_initial_timestamp_index, int32_t max_timestamp_index, const int32_t* n_gen,
                           const int32_t* prev1, const int32_t* prev2, const int32_t* last_ts, int32_t eot, int32_t k,
                           int32_t* out_ids, float* out_logprobs, int32_t* out_count, int32_t* out_forced, float* out_stats,
                           int32_t* out_err) {
  WB_REQUIRE(logits && n_gen && prev1 && prev2 && last_ts && out_ids && out_logprobs && out_count && out_forced && out_stats && out_err,
             WB_ERR_ARG, "wb_timestamp_beam_rows: null argument");
  WB_REQUIRE(R >= 1 && V >= 1 && ld >= V && (int64_t)R * ld < ((int64_t)1 << 31) && k >= 1 && k <= TOPK_MAX, WB_ERR_ARG,
             "wb_timestamp_beam_rows: R %d, V %d, ld %d, k %d", R, V, ld, k);
  wb_timestamp_params tp;
  wb_timestamp_params_default(&tp);
  tp.tok_timestamp_begin = tok_timestamp_begin; tp.n_timestamps = n_timestamps;
  tp.max_initial_timestamp_index = max_initial_timestamp_index; tp.max_timestamp_index = max_timestamp_index;
  WB_TRY(check_ts_params(tp, V, eot, "wb_timestamp_beam_rows"));
  for (int r = 0; r < R; r++)
    WB_REQUIRE(n_gen[r] >= 0 && last_ts[r] >= -1 && last_ts[r] < V, WB_ERR_ARG, "wb_timestamp_beam_rows: row %d: n_gen %d / last_ts %d", r,
               n_gen[r], last_ts[r]);
  wb::GpuTurn turn(device);
  WB_HIP(hipSetDevice(device));
  const int G = (V + 3) >> 2;
  DevMem dx, dsup, di32, dout;
  WB_TRY(dx.alloc((size_t)R * ld * 4));
  WB_TRY(dsup.alloc((size_t)2 * G * 4));
  WB_TRY(di32.alloc((size_t)R * 4 * 4));
  std::vector<uint32_t> words((size_t)2 * G);
  pack_suppress(suppress, nullptr, V, words.data());
  pack_suppress(suppress, suppress_first, V, words.data() + G);
  std::vector<int32_t> rowi((size_t)R * 4);
  const int32_t* cols[4] = {n_gen, prev1, prev2, last_ts};
  for (int c = 0; c < 4; c++) memcpy(rowi.data() + (size_t)c * R, cols[c], (size_t)R * 4);
  // the outputs sit between guard bands of poisoned words, checked after the run: ids, log-probs [R][k], count, forced [R],
  // stats [R][2], the error word
  constexpr size_t GUARD = 64;
  const size_t out_words = (size_t)2 * R * k + (size_t)4 * R + 1;
  WB_TRY(dout.alloc((out_words + 2 * GUARD) * 4));
  hipStream_t st = nullptr;
  WB_HIP(hipMemsetAsync(dout.p, 0xFF, dout.bytes, st));
  WB_HIP(hipMemcpyAsync(dx.p, logits, (size_t)R * ld * 4, hipMemcpyHostToDevice, st));
  WB_HIP(hipMemcpyAsync(dsup.p, words.data(), words.size() * 4, hipMemcpyHostToDevice, st));
  WB_HIP(hipMemcpyAsync(di32.p, rowi.data(), rowi.size() * 4, hipMemcpyHostToDevice, st));
  TsBeamRowsHookArgs a;
  a.logits = dx.as<float>(); a.R = R; a.ld = ld; a.V = V; a.k = k;
  a.sup = dsup.as<uint32_t>(); a.sup_first = a.sup + G;
  a.rules.tb = tok_timestamp_begin; a.rules.n_ts = n_timestamps; a.rules.max_init = max_initial_timestamp_index;
  a.rules.max_ts = max_timestamp_index; a.rules.eot = eot;
  a.n_gen = di32.as<int32_t>(); a.prev1 = a.n_gen + R; a.prev2 = a.n_gen + 2 * R; a.last_ts = a.n_gen + 3 * R;
  a.out_id = dout.as<int32_t>() + GUARD; a.out_lp = reinterpret_cast<float*>(a.out_id + (size_t)R * k);
  a.out_count = a.out_id + (size_t)2 * R * k; a.out_forced = a.out_count + R;
  a.out_stats = reinterpret_cast<float*>(a.out_forced + R); a.out_err = a.out_forced + 3 * R;
  WB_HIP(hipMemsetAsync(a.out_err, 0, 4, st));
  prof_tag(KC_TSBEAM_ROWS, 9.0 * (double)R * V);
  launch_tsbeam_rows_hook(st, a);
  WB_HIP(hipGetLastError());
  WB_HIP(hipMemcpyAsync(out_ids, a.out_id, (size_t)R * k * 4, hipMemcpyDeviceToHost, st));
  WB_HIP(hipMemcpyAsync(out_logprobs, a.out_lp, (size_t)R * k * 4, hipMemcpyDeviceToHost, st));
  WB_HIP(hipMemcpyAsync(out_count, a.out_count, (size_t)R * 4, hipMemcpyDeviceToHost, st));
  WB_HIP(hipMemcpyAsync(out_forced, a.out_forced, (size_t)R * 4, hipMemcpyDeviceToHost, st));
  WB_HIP(hipMemcpyAsync(out_stats, a.out_stats, (size_t)R * 2 * 4, hipMemcpyDeviceToHost, st));
  WB_HIP(hipMemcpyAsync(out_err, a.out_err, 4, hipMemcpyDeviceToHost, st));
  uint32_t guards[2][GUARD];
  WB_HIP(hipMemcpyAsync(guards[0], dout.p, GUARD * 4, hipMemcpyDeviceToHost, st));
  WB_HIP(hipMemcpyAsync(guards[1], dout.as<int32_t>() + GUARD + out_words, GUARD * 4, hipMemcpyDeviceToHost, st));
  WB_HIP(hipStreamSynchronize(st));
  for (int b = 0; b < 2; b++)
    for (size_t i = 0; i < GUARD; i++)
      WB_REQUIRE(guards[b][i] == 0xFFFFFFFFu, WB_ERR_STATE, "wb_timestamp_beam_rows: guard band %d overwritten at word %zu", b, i);
  return WB_OK;
}

int wb_timestamp_beam_search_device(int device, const wb_timestamp_params* tp, const wb_beam_params* bp, int32_t n_windows,
                                    int32_t V, const uint8_t* suppress, const uint8_t* suppress_first, int32_t eot,
                                    int32_t max_depth, wb_tsbeam_logits_fn fill, void* user, int32_t* cand_tokens,
                                    int32_t row_stride, int32_t* cand_lens, double* cand_scores, double* cand_ranks,
                                    int32_t* n_cand, int32_t* best, int32_t* n_steps, int32_t* n_live, int32_t* n_finished,
                                    int32_t* tr_tokens, int32_t* tr_parents, double* tr_scores) {
  WB_REQUIRE(tp && bp && fill && cand_tokens && cand_lens && cand_scores && cand_ranks && n_cand && best && n_steps && n_live &&
                 n_finished && tr_tokens && tr_parents && tr_scores, WB_ERR_ARG, "wb_timestamp_beam_search_device: null argument");
  WB_REQUIRE(n_windows >= 1 && n_windows <= 64 && V >= 1 && max_depth >= 1 && row_stride >= max_depth, WB_ERR_ARG,
             "wb_timestamp_beam_search_device: n_windows %d, V %d, max_depth %d, row_stride %d", n_windows, V, max_depth, row_stride);
  WB_TRY(check_ts_params(*tp, V, eot, "wb_timestamp_beam_search_device"));
  int C = 0;
  WB_TRY(check_beam_params(*tp, *bp, MAX_BEAMS, &C));
  const int W = n_windows, B = bp->beam_size, S = W * MAX_BEAMS, G = (V + 3) >> 2;
  wb::GpuTurn turn(device);
  WB_HIP(hipSetDevice(device));
  const StepLayout L = make_step_layout(S, W);
  const TsBeamLayout bl = make_tsbeam_layout(S, W, max_depth);
  DevMem d_ctl, d_state, d_topk, d_x, d_sup;
  WB_TRY(d_ctl.ensure((size_t)bl.total_ints * 4));
  WB_TRY(d_state.ensure((size_t)L.total * 4));
  WB_TRY(d_topk.ensure((size_t)S * TOPK_MAX * 8 + (size_t)S * TBR_STRIDE * 4));
  WB_TRY(d_x.ensure((size_t)S * V * 4));
  WB_TRY(d_sup.ensure((size_t)2 * G * 4));
  std::vector<uint32_t> words((size_t)2 * G);
  pack_suppress(suppress, nullptr, V, words.data());
  pack_suppress(suppress, suppress_first, V, words.data() + G);
  WB_HIP(hipMemcpy(d_sup.p, words.data(), words.size() * 4, hipMemcpyHostToDevice));
  std::vector<int> wa(W);
  for (int w = 0; w < W; w++) wa[w] = w;
  std::vector<int> ctl;
  tsbeam_init(ctl, bl, wa, *tp, B, C);
  std::vector<int> hs((size_t)L.total, 0);
  hs[ST_N] = W;
  for (int w = 0; w < W; w++) { hs[L.parent + w] = -1; hs[L.len + w] = 1; hs[L.win + w] = w; hs[L.win_slots + w * MAX_BEAMS] = w; hs[L.win_nb + w] = 1; }
  WB_HIP(hipMemcpy(d_ctl.p, ctl.data(), ctl.size() * 4, hipMemcpyHostToDevice));
  WB_HIP(hipMemcpy(d_state.p, hs.data(), hs.size() * 4, hipMemcpyHostToDevice));
  TsBeamRowsArgs r;
  r.ctl = d_ctl.as<int>(); r.bl = bl; r.logits = d_x.as<float>(); r.V = V; r.sup = d_sup.as<uint32_t>(); r.sup_first = r.sup + G;
  r.state = d_state.as<int>(); r.lay = L; r.eot = eot;
  r.topk_id = d_topk.as<int32_t>(); r.topk_lp = reinterpret_cast<float*>(r.topk_id + (size_t)S * TOPK_MAX);
  r.row_out = r.topk_id + (size_t)2 * S * TOPK_MAX;
  TsBeamUpdateArgs u;
  u.ctl = r.ctl; u.bl = bl; u.topk_id = r.topk_id; u.topk_lp = r.topk_lp; u.row_out = r.row_out;
  u.state = d_state.as<int>(); u.lay = L; u.eot = eot; u.V = V; u.step_pos = 0;
  std::vector<float> x((size_t)S * V);
  std::vector<int32_t> win(S), beam(S), tok(S), par(S);
  const int* nodes = ctl.data() + bl.nodes;
  for (int depth = 0; depth < max_depth; depth++) {
    WB_HIP(hipMemcpy(hs.data(), d_state.p, hs.size() * 4, hipMemcpyDeviceToHost));
    WB_HIP(hipMemcpy(ctl.data(), d_ctl.p, ctl.size() * 4, hipMemcpyDeviceToHost));
    const int n = hs[ST_N];
    if (n == 0 || ctl[TB_ERR]) break;
    WB_REQUIRE(n <= S, WB_ERR_STATE, "wb_timestamp_beam_search_device: %d live rows", n);
    for (int i = 0; i < n; i++) {
      win[i] = hs[L.win + i]; beam[i] = ctl[bl.row_beam + i];
      const int nd = ctl[bl.node + win[i] * MAX_BEAMS + beam[i]];
      tok[i] = nd < 0 ? -1 : nodes[2 * nd];
      par[i] = nd < 0 ? -1 : (nodes[2 * nd + 1] < 0 ? 0 : nodes[2 * nd + 1] % MAX_BEAMS);
    }
    const int rc = fill(user, depth, n, win.data(), beam.data(), tok.data(), par.data(), x.data());
    WB_REQUIRE(rc == 0, rc, "wb_timestamp_beam_search_device: the logits callback failed");
    WB_HIP(hipMemcpy(d_x.p, x.data(), (size_t)n * V * 4, hipMemcpyHostToDevice));
    launch_dec_tsbeam_rows(nullptr, r, n);
    launch_dec_tsbeam_update(nullptr, u);
    WB_HIP(hipGetLastError());
  }
  WB_HIP(hipMemcpy(ctl.data(), d_ctl.p, ctl.size() * 4, hipMemcpyDeviceToHost));
  WB_REQUIRE(ctl[TB_ERR] == 0, WB_ERR_STATE, "beam search: a logits row or a score was not finite, or the rules left a beam no id");
  TsBeamResult res;
  tsbeam_finalize(ctl, bl, wa, B, bp->length_penalty, eot, res);
  WB_TRY(export_beams(res, BEAM_KB, cand_tokens, row_stride, cand_lens, cand_scores, cand_ranks, n_cand));
  for (int w = 0; w < W; w++) best[w] = res.best[w];
  export_trace(res, max_depth, n_steps, n_live, n_finished, tr_tokens, tr_parents, tr_scores);
  return WB_OK;
}

}  // extern "C"
