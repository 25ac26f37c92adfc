// Device-chained timestamp decoding: the host side of tsrules.hip's dec_ts_update_kernel (suppress bytes, control block,
// prompt prefill, chunks of steps as one graph, the best-of-n pick), its C ABI, the test hook that runs the rules alone, the
// slicing of a decoded window into segments and the seek loop over a waveform.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

#include "decode_step.h"

using namespace wb;

namespace wb {

// u8 [V] -> the kernel's words: 4 ids per word, id v in byte (v & 3) of word v >> 2, pad bytes 0
void pack_suppress(const uint8_t* a, const uint8_t* b, int V, uint32_t* out) {
  const int G = (V + 3) >> 2;
  for (int g = 0; g < G; g++) {
    uint32_t w = 0;
    for (int q = 0; q < 4; q++) {
      const int v = 4 * g + q;
      if (v < V && ((a && a[v]) || (b && b[v]))) w |= 1u << (8 * q);
    }
    out[g] = w;
  }
}

int check_ts_params(const wb_timestamp_params& tp, int V, int eot, const char* who) {
  WB_REQUIRE(tp.temperature >= 0.f && std::isfinite(tp.temperature) && (tp.temperature == 0.f || std::isfinite(1.0f / tp.temperature)),
             WB_ERR_ARG, "%s: temperature %g must be 0 or finite and > 0 with a finite 1 / temperature", who, (double)tp.temperature);
  WB_REQUIRE(tp.n_timestamps >= 0 && tp.tok_timestamp_begin >= 0 && (int64_t)tp.tok_timestamp_begin + tp.n_timestamps <= V, WB_ERR_ARG,
             "%s: timestamp range [%d, %d + %d) outside [0, %d)", who, tp.tok_timestamp_begin, tp.tok_timestamp_begin, tp.n_timestamps, V);
  WB_REQUIRE(eot >= 0 && eot < V, WB_ERR_ARG, "%s: end-of-text token out of range", who);
  WB_REQUIRE(!(eot >= tp.tok_timestamp_begin && eot < tp.tok_timestamp_begin + tp.n_timestamps), WB_ERR_ARG,
             "%s: end-of-text %d lies inside the timestamp range", who, eot);
  WB_REQUIRE(tp.max_initial_timestamp_index >= -1 && tp.max_timestamp_index >= -1 && tp.attempt >= 0, WB_ERR_ARG,
             "%s: max_initial_timestamp_index %d / max_timestamp_index %d / attempt %d", who, tp.max_initial_timestamp_index,
             tp.max_timestamp_index, tp.attempt);
  return WB_OK;
}

// session_sample_chain's structure under the timestamp rules.  Rows are a * best_of + j over the ACTIVE windows in order; the
// special mask is never applied (use_mask = 0 on every step: a three-token prompt would otherwise mask the timestamps
// themselves), so every chunk of 16 steps is one graph.
int session_ts_chain(wb_session* s, const wb_timestamp_params& tp, const int32_t* prompt, int P, const uint8_t* active,
                     const int32_t* stream_ids, int eot, int max_depth, int32_t* out_tokens, int32_t row_stride,
                     int32_t* out_lens, double* out_sum, int32_t* out_best) {
  wb_model* m = s->m;
  const wb_dims& D = m->dims;
  const int W = s->W, V = D.n_vocab, bo = tp.best_of;
  WB_TRY(check_ts_params(tp, V, eot, "timestamps"));
  WB_REQUIRE(bo >= 1 && bo <= s->max_beams, WB_ERR_ARG, "timestamps: best_of %d outside [1, %d]", bo, s->max_beams);
  WB_REQUIRE(tp.temperature > 0.f || bo == 1, WB_ERR_ARG, "timestamps: best_of %d needs temperature > 0", bo);
  WB_REQUIRE(P >= 1 && max_depth >= 0, WB_ERR_ARG, "timestamps: prompt_len %d / max_depth %d", P, max_depth);
  WB_REQUIRE(row_stride >= P + max_depth, WB_ERR_ARG, "row_stride %d < %d", row_stride, P + max_depth);
  for (int i = 0; i < P; i++) WB_REQUIRE(prompt[i] >= 0 && prompt[i] < V, WB_ERR_ARG, "prompt token %d out of range", prompt[i]);
  WB_REQUIRE(s->step == 0, WB_ERR_STATE, "wb_session_decode_timestamps: the session is at step %d (wb_session_rewind first)", s->step);
  WB_REQUIRE(s->has_suppress, WB_ERR_STATE, "wb_session_decode_timestamps: wb_session_set_suppress was not called on this session");
  std::vector<int> wa;                             // the active windows
  for (int w = 0; w < W; w++)
    if (!active || active[w]) wa.push_back(w);
  const int nA = (int)wa.size(), R = nA * bo;
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
  const TsChainLayout tl = make_ts_layout(S, W, std::max(max_depth, 0));
  WB_TRY(s->ts_ctl.ensure((size_t)tl.total_ints * 4));
  WB_TRY(s->ts_topk.ensure((size_t)S * TOPK_MAX * 8));
  std::vector<int> ctl((size_t)tl.total_ints, 0);
  const float inv_t = tp.temperature > 0.f ? 1.0f / tp.temperature : 0.f;
  ctl[TC_NROWS] = R; ctl[TC_BEST_OF] = bo; ctl[TC_ATTEMPT] = tp.attempt;
  ctl[TC_SEED_LO] = (int)(uint32_t)(tp.seed & 0xffffffffull); ctl[TC_SEED_HI] = (int)(uint32_t)(tp.seed >> 32);
  memcpy(&ctl[TC_INVT], &inv_t, 4);
  ctl[TC_TB] = tp.tok_timestamp_begin; ctl[TC_NTS] = tp.n_timestamps;
  ctl[TC_MAX_INIT] = tp.max_initial_timestamp_index; ctl[TC_MAX_TS] = tp.max_timestamp_index;
  const bool start_finished = prompt[P - 1] == eot;       // nothing is generated behind an end-of-text
  for (int a = 0; a < nA; a++)
    for (int j = 0; j < bo; j++) {
      const int r = a * bo + j;
      ctl[tl.stream + r] = (int)((uint32_t)(stream_ids ? stream_ids[wa[a]] : wa[a] * bo) + (uint32_t)j);
      ctl[tl.fin + r] = start_finished ? 1 : 0;
      ctl[tl.last_ts + r] = -1;
    }
  int steps_done = 0;
  if (!start_finished && max_depth > 0) {
    // the first step's state block, as wb_session_step writes it: every row continues its window's prefill row
    int* hs = s->state_host;
    memset(hs, 0, (size_t)L.total * 4);
    hs[ST_N] = R; hs[ST_STEP] = P - 1;
    for (int a = 0; a < nA; a++) {
      for (int j = 0; j < bo; j++) {
        const int r = a * bo + j;
        hs[L.tok + r] = prompt[P - 1]; hs[L.parent + r] = P > 1 ? a : -1; hs[L.len + r] = P; hs[L.win + r] = wa[a];
        hs[L.win_slots + wa[a] * MAX_BEAMS + j] = r;
      }
      hs[L.win_nb + wa[a]] = bo;
    }
    WB_HIP(hipMemcpyAsync(s->ts_ctl.p, ctl.data(), ctl.size() * 4, hipMemcpyHostToDevice, st));
    WB_HIP(hipStreamSynchronize(st));
    // launch shape: the bucket of the most rows a call on this session can have (W best_of), so that one graph serves every
    // set of active windows (plan.persist is not consulted: the persistent kernel has no place for the rules)
    const StepPlan plan = plan_step(s, W * bo, true);
    TsStepIO tio;
    tio.topk_id = s->ts_topk.as<int32_t>();
    tio.topk_lp = reinterpret_cast<float*>(s->ts_topk.as<int32_t>() + (size_t)S * TOPK_MAX);
    const int G = (V + 3) >> 2;
    TsChainArgs& u = tio.upd;
    u.ctl = s->ts_ctl.as<int>(); u.tl = tl; u.logits = s->logits.as<float>(); u.V = V;
    u.sup = s->ts_sup.as<uint32_t>(); u.sup_first = s->ts_sup.as<uint32_t>() + G;
    u.row_stats = s->row_stats.as<float>(); u.state = s->state.as<int>(); u.lay = L; u.eot = eot;
    u.tabs = s->tabs.as<int>(); u.Lmax = s->Lmax; u.E = m->tok_emb; u.pos = m->dec_pos; u.d = D.n_text_state; u.x = s->x.as<float>();
    // the captured timestamp steps bake in the control block, its layout (S, W: the buffer signature of launch_step;
    // max_depth: here), the suppress buffer and eot: drop THEM when those differ from the last call -- temperature, seed,
    // attempt, streams and the rule parameters do not
    const uint64_t tsig = ((uint64_t)(uintptr_t)s->ts_ctl.p * 1099511628211ull) ^ ((uint64_t)(uintptr_t)s->ts_sup.p * 0x9E3779B97F4A7C15ull) ^
                          ((uint64_t)max_depth << 20) ^ (uint64_t)(unsigned)eot ^ 1u;
    if (tsig != s->ts_sig) {
      for (auto it = s->graphs.begin(); it != s->graphs.end();)
        if (it->first & GRAPH_KEY_TS) { (void)hipGraphExecDestroy(it->second); it = s->graphs.erase(it); }
        else ++it;
      s->ts_sig = tsig;
    }
    ScopedTimer tm(st, 3);
    prof_tag(KC_PREPARE, 8.0 * R * D.n_text_state);
    launch_dec_prepare(st, reinterpret_cast<const int*>(s->host_block_dev), s->state.as<int>(), L, R, s->tabs.as<int>(), s->Lmax,
                       m->tok_emb, m->dec_pos, D.n_text_state, s->x.as<float>(), nullptr);
    const int chunk = 16;
    int depth = 0;
    int hdr[TC_HDR] = {0};
    while (depth < max_depth) {
      int enq = 0;
      while (depth + enq < max_depth && enq < chunk) {
        const int run = (max_depth - (depth + enq) >= chunk && enq == 0) ? chunk : 1;
        StepCall call;
        // (call.eot stays at its default, as in session_sample_chain: prefill and timestamp steps keep each other's graphs)
        call.k = 1; call.use_mask = 0; call.reps = run; call.tio = &tio;
        WB_TRY(launch_step(s, plan, call));
        if (profile().on) profile().ms[4] += run;
        enq += run;
      }
      depth += enq;
      WB_HIP(hipMemcpyAsync(hdr, s->ts_ctl.p, sizeof(hdr), hipMemcpyDeviceToHost, st));
      WB_HIP(hipStreamSynchronize(st));
      if (hdr[TC_ALLDONE] || hdr[TC_ERR]) break;   // every row has ended: the kernels of further steps would exit at once
    }
    tm.stop();
    WB_HIP(hipMemcpyAsync(ctl.data(), s->ts_ctl.p, ctl.size() * 4, hipMemcpyDeviceToHost, st));
    WB_HIP(hipStreamSynchronize(st));
    tm.collect();
    if (profile().on) prof_collect();
    s->prof_step_off = 0;
    for (int r = 0; r < R; r++) steps_done = std::max(steps_done, ctl[tl.ngen + r]);   // (an unfinished row picked once per step)
  }
  s->step += steps_done;
  s->prev_n = 0; s->prev_len.clear(); s->prev_win.clear();     // (the device-side slots are not mirrored: no host-driven step may follow)
  s->last_had_logits = 0;
  WB_TRY(dec_split_check(s));
  WB_REQUIRE(ctl[TC_ERR] == 0, WB_ERR_STATE, "timestamps: a logits row was not finite, or the rules left it no id");
  const double* sum = reinterpret_cast<const double*>(ctl.data() + tl.sum);
  bool all_done = true;
  s->smp_best_of = bo; s->smp_depth = tl.max_depth;
  s->smp_tokens.assign((size_t)W * bo * tl.max_depth, 0);
  s->smp_len.assign((size_t)W * bo, -1);
  for (int a = 0; a < nA; a++) {
    const int w = wa[a];
    int best = 0;
    double best_rank = -INFINITY;
    for (int j = 0; j < bo; j++) {
      const int r = a * bo + j, ng = ctl[tl.ngen + r];
      const int n_text = ng - ((ng > 0 && ctl[tl.tokens + r * tl.max_depth + ng - 1] == eot) ? 1 : 0);
      const double rank = n_text > 0 ? sum[r] / (double)n_text : -INFINITY;
      if (rank > best_rank) { best_rank = rank; best = j; }       // (the first of equal maxima)
      if (out_sum) out_sum[(size_t)w * bo + j] = sum[r];
      s->smp_len[(size_t)w * bo + j] = ng;
      for (int i = 0; i < ng; i++) s->smp_tokens[((size_t)w * bo + j) * tl.max_depth + i] = ctl[tl.tokens + r * tl.max_depth + i];
      all_done = all_done && ctl[tl.fin + r] != 0;
    }
    const int r = a * bo + best, ng = ctl[tl.ngen + r];
    int32_t* row = out_tokens + (size_t)w * row_stride;
    for (int i = 0; i < P; i++) row[i] = prompt[i];
    for (int i = 0; i < ng; i++) row[P + i] = ctl[tl.tokens + r * tl.max_depth + i];
    out_lens[w] = P + ng;
    if (out_best) out_best[w] = best;
  }
  if (max_depth < asked_depth && !all_done)
    WB_REQUIRE(false, WB_ERR_SHAPE, "Token sequence length %d must not exceed %d.", s->Lmax + 1, s->Lmax);
  return WB_OK;
}

}  // namespace wb

extern "C" {

void wb_timestamp_params_default(wb_timestamp_params* p) {
  if (!p) return;
  p->tok_timestamp_begin = 0; p->n_timestamps = 0; p->max_initial_timestamp_index = 50; p->max_timestamp_index = -1;
  p->seconds_per_timestamp = 0.02f; p->temperature = 0.f; p->best_of = 1; p->seed = 0; p->attempt = 0;
}

int wb_session_set_suppress(wb_session* s, const uint8_t* suppress, const uint8_t* suppress_first) {
  WB_REQUIRE(s && suppress, WB_ERR_ARG, "wb_session_set_suppress: null argument");
  wb::GpuTurn turn(s->device);
  const int V = s->m->dims.n_vocab, G = (V + 3) >> 2;
  WB_HIP(hipSetDevice(s->m->device));
  WB_TRY(s->ts_sup.ensure((size_t)2 * G * 4));
  std::vector<uint8_t> key((size_t)2 * V);
  for (int v = 0; v < V; v++) { key[v] = suppress[v] ? 1 : 0; key[(size_t)V + v] = (suppress_first && suppress_first[v]) ? 1 : 0; }
  if (s->ts_sup_dev_ptr == s->ts_sup.p && s->ts_sup_host == key) {     // a pooled session that already holds these masks
    s->has_suppress = true;
    return WB_OK;
  }
  s->ts_sup_host.clear(); s->ts_sup_dev_ptr = nullptr;                  // void the cache key before the contents change
  std::vector<uint32_t> words((size_t)2 * G);
  pack_suppress(suppress, nullptr, V, words.data());
  pack_suppress(suppress, suppress_first, V, words.data() + G);
  WB_HIP(hipMemcpyAsync(s->ts_sup.p, words.data(), words.size() * 4, hipMemcpyHostToDevice, s->st));
  WB_HIP(hipStreamSynchronize(s->st));
  s->ts_sup_host.swap(key); s->ts_sup_dev_ptr = s->ts_sup.p;
  s->has_suppress = true;
  return WB_OK;
}

int wb_session_decode_timestamps(wb_session* s, const wb_decode_params* p, const wb_timestamp_params* tp, const int32_t* prompt,
                                 int32_t prompt_len, const uint8_t* active, const int32_t* stream_ids, int32_t* out_tokens,
                                 int32_t row_stride, int32_t* out_lens, double* out_sum_logprob, int32_t* out_best) {
  WB_REQUIRE(s && p && tp && prompt && out_tokens && out_lens, WB_ERR_ARG, "wb_session_decode_timestamps: null argument");
  wb::GpuTurn turn(s->device);
  return session_ts_chain(s, *tp, prompt, prompt_len, active, stream_ids, p->tok_end_of_text, p->max_depth, out_tokens, row_stride,
                          out_lens, out_sum_logprob, out_best);
}

int wb_timestamp_rows(int device, const float* logits, int32_t R, int32_t ld, int32_t V, const uint8_t* suppress,
                      const uint8_t* suppress_first, int32_t tok_timestamp_begin, int32_t n_timestamps,
                      int32_t max_initial_timestamp_index, int32_t max_timestamp_index, float temperature, uint64_t seed,
                      int32_t attempt, const int32_t* n_gen, const int32_t* prev1, const int32_t* prev2, const int32_t* last_ts,
                      const int32_t* stream, const int32_t* position, int32_t eot, int32_t* out_token, float* out_logprob,
                      int32_t* out_forced, float* out_stats, int32_t* out_err) {
  WB_REQUIRE(logits && n_gen && prev1 && prev2 && last_ts && stream && position && out_token && out_logprob && out_forced &&
                 out_stats && out_err, WB_ERR_ARG, "wb_timestamp_rows: null argument");
  WB_REQUIRE(R >= 1 && V >= 1 && ld >= V && (int64_t)R * ld < ((int64_t)1 << 31), WB_ERR_ARG, "wb_timestamp_rows: R %d, V %d, ld %d", R, V, ld);
  wb_timestamp_params tp;
  wb_timestamp_params_default(&tp);
  tp.tok_timestamp_begin = tok_timestamp_begin; tp.n_timestamps = n_timestamps;
  tp.max_initial_timestamp_index = max_initial_timestamp_index; tp.max_timestamp_index = max_timestamp_index;
  tp.temperature = temperature; tp.attempt = attempt;
  WB_TRY(check_ts_params(tp, V, eot, "wb_timestamp_rows"));
  for (int r = 0; r < R; r++)
    WB_REQUIRE(n_gen[r] >= 0 && last_ts[r] >= -1 && last_ts[r] < V, WB_ERR_ARG, "wb_timestamp_rows: row %d: n_gen %d / last_ts %d", r,
               n_gen[r], last_ts[r]);
  wb::GpuTurn turn(device);
  WB_HIP(hipSetDevice(device));
  const int G = (V + 3) >> 2;
  DevMem dx, dsup, dmax, di32, dout;
  WB_TRY(dx.alloc((size_t)R * ld * 4));
  WB_TRY(dsup.alloc((size_t)2 * G * 4));
  WB_TRY(dmax.alloc((size_t)R * 4));
  WB_TRY(di32.alloc((size_t)R * 6 * 4));
  // the key's shift: the row maximum over all ids (NaN ignored: the kernel finds it)
  std::vector<float> rmax((size_t)R, -INFINITY);
  for (int r = 0; r < R; r++)
    for (int v = 0; v < V; v++) {
      const float x = logits[(size_t)r * ld + v];
      if (x > rmax[r]) rmax[r] = x;
    }
  std::vector<uint32_t> words((size_t)2 * G);
  pack_suppress(suppress, nullptr, V, words.data());
  pack_suppress(suppress, suppress_first, V, words.data() + G);
  std::vector<int32_t> rowi((size_t)R * 6);
  const int32_t* cols[6] = {n_gen, prev1, prev2, last_ts, stream, position};
  for (int c = 0; c < 6; c++) memcpy(rowi.data() + (size_t)c * R, cols[c], (size_t)R * 4);
  // the five outputs sit between guard bands of poisoned words, checked after the run
  constexpr size_t GUARD = 64;
  const size_t out_words = (size_t)5 * R + 1;
  WB_TRY(dout.alloc((out_words + 2 * GUARD) * 4));
  hipStream_t st = nullptr;
  WB_HIP(hipMemsetAsync(dout.p, 0xFF, dout.bytes, st));
  WB_HIP(hipMemcpyAsync(dx.p, logits, (size_t)R * ld * 4, hipMemcpyHostToDevice, st));
  WB_HIP(hipMemcpyAsync(dsup.p, words.data(), words.size() * 4, hipMemcpyHostToDevice, st));
  WB_HIP(hipMemcpyAsync(dmax.p, rmax.data(), (size_t)R * 4, hipMemcpyHostToDevice, st));
  WB_HIP(hipMemcpyAsync(di32.p, rowi.data(), rowi.size() * 4, hipMemcpyHostToDevice, st));
  TsRowsArgs a;
  a.logits = dx.as<float>(); a.R = R; a.ld = ld; a.V = V;
  a.sup = dsup.as<uint32_t>(); a.sup_first = a.sup + G; a.row_max = dmax.as<float>();
  a.rules.tb = tok_timestamp_begin; a.rules.n_ts = n_timestamps; a.rules.max_init = max_initial_timestamp_index;
  a.rules.max_ts = max_timestamp_index; a.rules.eot = eot;
  a.inv_t = temperature > 0.f ? 1.0f / temperature : 0.f;
  a.seed_lo = (uint32_t)(seed & 0xffffffffull); a.seed_hi = (uint32_t)(seed >> 32); a.attempt = (uint32_t)attempt;
  a.n_gen = di32.as<int32_t>(); a.prev1 = a.n_gen + R; a.prev2 = a.n_gen + 2 * R; a.last_ts = a.n_gen + 3 * R;
  a.stream = a.n_gen + 4 * R; a.position = a.n_gen + 5 * R;
  a.out_token = dout.as<int32_t>() + GUARD; a.out_logprob = reinterpret_cast<float*>(a.out_token + R);
  a.out_forced = a.out_token + 2 * R; a.out_stats = reinterpret_cast<float*>(a.out_token + 3 * R);
  a.out_err = a.out_token + 5 * R;
  WB_HIP(hipMemsetAsync(a.out_err, 0, 4, st));
  prof_tag(KC_TS_UPDATE, 5.0 * (double)R * V);
  launch_ts_rows(st, a);
  WB_HIP(hipGetLastError());
  WB_HIP(hipMemcpyAsync(out_token, a.out_token, (size_t)R * 4, hipMemcpyDeviceToHost, st));
  WB_HIP(hipMemcpyAsync(out_logprob, a.out_logprob, (size_t)R * 4, hipMemcpyDeviceToHost, st));
  WB_HIP(hipMemcpyAsync(out_forced, a.out_forced, (size_t)R * 4, hipMemcpyDeviceToHost, st));
  WB_HIP(hipMemcpyAsync(out_stats, a.out_stats, (size_t)R * 2 * 4, hipMemcpyDeviceToHost, st));
  WB_HIP(hipMemcpyAsync(out_err, a.out_err, 4, hipMemcpyDeviceToHost, st));
  uint32_t guards[2][GUARD];
  WB_HIP(hipMemcpyAsync(guards[0], dout.p, GUARD * 4, hipMemcpyDeviceToHost, st));
  WB_HIP(hipMemcpyAsync(guards[1], dout.as<int32_t>() + GUARD + out_words, GUARD * 4, hipMemcpyDeviceToHost, st));
  WB_HIP(hipStreamSynchronize(st));
  for (int b = 0; b < 2; b++)
    for (size_t i = 0; i < GUARD; i++)
      WB_REQUIRE(guards[b][i] == 0xFFFFFFFFu, WB_ERR_STATE, "wb_timestamp_rows: guard band %d overwritten at word %zu", b, i);
  return WB_OK;
}

int wb_segments_from_tokens(const int32_t* tokens, int32_t n, int32_t tok_timestamp_begin, int32_t n_timestamps,
                            int32_t tok_end_of_text, int32_t window_index, float seconds_per_timestamp, int32_t* seg_begin,
                            int32_t* seg_end, float* seg_start, float* seg_end_time, int32_t cap, int32_t* n_segments,
                            int32_t* advance_index) {
  WB_REQUIRE((tokens || n == 0) && n >= 0 && seg_begin && seg_end && seg_start && seg_end_time && n_segments && advance_index &&
                 window_index >= 0 && n_timestamps >= 0, WB_ERR_ARG, "wb_segments_from_tokens: bad argument");
  const int tb = tok_timestamp_begin;
  auto is_ts = [&](int i) { return (unsigned)(tokens[i] - tb) < (unsigned)n_timestamps; };
  int len = 0;
  while (len < n && tokens[len] != tok_end_of_text) len++;
  int ns = 0;
  auto emit = [&](int b, int e, int i0, int i1) -> bool {
    if (ns >= cap) return false;
    seg_begin[ns] = b; seg_end[ns] = e;
    seg_start[ns] = (float)i0 * seconds_per_timestamp; seg_end_time[ns] = (float)i1 * seconds_per_timestamp;
    ns++;
    return true;
  };
  const bool single_ending = len >= 1 && is_ts(len - 1) && (len < 2 || !is_ts(len - 2));
  std::vector<int> slices;                          // the index behind every pair of consecutive timestamps
  for (int i = 1; i < len; i++)
    if (is_ts(i - 1) && is_ts(i)) slices.push_back(i);
  *advance_index = window_index;
  if (!slices.empty()) {
    if (single_ending) slices.push_back(len);
    int last = 0, prev_end = 0;
    for (int cur : slices) {
      const int i0 = is_ts(last) ? tokens[last] - tb : prev_end, i1 = tokens[cur - 1] - tb;     // (cur - 1 is a timestamp)
      WB_REQUIRE(emit(last, cur, i0, i1), WB_ERR_ARG, "wb_segments_from_tokens: more than cap = %d segments", cap);
      last = cur; prev_end = i1;
    }
    if (!single_ending) *advance_index = tokens[last - 1] - tb;
  } else if (len > 0) {
    int dur = window_index;
    for (int i = len - 1; i >= 0; i--)
      if (is_ts(i)) { if (tokens[i] != tb) dur = tokens[i] - tb; break; }
    WB_REQUIRE(emit(0, len, 0, dur), WB_ERR_ARG, "wb_segments_from_tokens: more than cap = %d segments", cap);
  }
  *n_segments = ns;
  return WB_OK;
}

// What wb_waveform_to_segments_conditioned adds to the seek loop (the rule is stated once, in whisper_hip.h)
struct SeekCond {
  int32_t sot_prev, on, max_prompt;
  const int32_t* initial; int32_t n_initial;
  int64_t* win_seek; int32_t* win_prompt_len; int32_t win_cap;
};

// The seek loop of wb_waveform_to_segments; bp non-null: every window by beam search (wb_waveform_to_segments_beam); cond
// non-null: every window's prompt carries the history (wb_waveform_to_segments_conditioned).
static int waveform_segments_loop(wb_model* m, const float* pcm, int64_t n, int sample_rate, const wb_decode_params* p,
                                  const wb_timestamp_params* tp, const wb_beam_params* bp, const uint8_t* suppress,
                                  const uint8_t* suppress_first, const int32_t* prompt, int32_t prompt_len, float* seg_start,
                                  float* seg_end_time, int32_t* seg_tok_begin, int32_t* seg_tok_end, int32_t seg_cap,
                                  int32_t* n_segments, int32_t* text_tokens, int64_t text_cap, int64_t* n_text_tokens,
                                  int32_t* n_windows, const SeekCond* cond = nullptr) {
  WB_REQUIRE(m && pcm && p && tp && suppress && prompt && seg_start && seg_end_time && seg_tok_begin && seg_tok_end && n_segments &&
                 text_tokens && n_text_tokens, WB_ERR_ARG, "wb_waveform_to_segments: null argument");
  WB_REQUIRE(sample_rate > 0 && tp->seconds_per_timestamp > 0.f && prompt_len >= 1 && p->max_depth >= 0, WB_ERR_ARG,
             "wb_waveform_to_segments: sample_rate %d / seconds_per_timestamp %g / prompt_len %d", sample_rate,
             (double)tp->seconds_per_timestamp, prompt_len);
  WB_REQUIRE(p->padding >= 0 && p->padding < m->max_mel_frames(), WB_ERR_ARG, "bad padding");
  // what every window's decode would refuse, refused before the first window is encoded
  WB_TRY(check_ts_params(*tp, m->dims.n_vocab, p->tok_end_of_text, "wb_waveform_to_segments"));
  WB_REQUIRE(tp->best_of >= 1 && tp->best_of <= MAX_BEAMS && (tp->temperature > 0.f || tp->best_of == 1), WB_ERR_ARG,
             "wb_waveform_to_segments: best_of %d (temperature %g)", tp->best_of, (double)tp->temperature);
  int max_cand = 0;
  if (bp) WB_TRY(check_beam_params(*tp, *bp, MAX_BEAMS, &max_cand));
  for (int i = 0; i < prompt_len; i++)
    WB_REQUIRE(prompt[i] >= 0 && prompt[i] < m->dims.n_vocab, WB_ERR_ARG, "prompt token %d out of range", prompt[i]);
  std::vector<int32_t> history, wprompt;
  int hist_cap = 0;
  if (cond) {
    const int V = m->dims.n_vocab;
    WB_REQUIRE(cond->n_initial >= 0 && (cond->n_initial == 0 || cond->initial) && cond->win_cap >= 0, WB_ERR_ARG,
               "wb_waveform_to_segments_conditioned: bad argument");
    WB_REQUIRE(cond->sot_prev >= 0 && cond->sot_prev < V, WB_ERR_ARG, "start-of-prev token %d out of range [0,%d)", cond->sot_prev, V);
    for (int i = 0; i < cond->n_initial; i++)
      WB_REQUIRE(cond->initial[i] >= 0 && cond->initial[i] < V, WB_ERR_ARG, "initial prompt token %d out of range [0,%d)",
                 cond->initial[i], V);
    history.assign(cond->initial, cond->initial + cond->n_initial);
    hist_cap = cond->max_prompt < 0 ? std::max(0, m->dims.n_text_ctx / 2 - 1) : cond->max_prompt;
  }
  const int64_t wlen = wb_max_waveform_samples(m->max_mel_frames() - p->padding);
  const double samples_per_ts = (double)tp->seconds_per_timestamp * (double)sample_rate;
  const int tb = tp->tok_timestamp_begin, nts = tp->n_timestamps;
  const int base_prompt_len = prompt_len;
  const int32_t* base_prompt = prompt;
  const int stride = (hist_cap > 0 ? 1 + hist_cap : 0) + prompt_len + p->max_depth;
  std::vector<int32_t> row((size_t)stride), sb((size_t)p->max_depth + 1), se((size_t)p->max_depth + 1);
  std::vector<float> t0((size_t)p->max_depth + 1), t1((size_t)p->max_depth + 1);
  int ns = 0, nw = 0;
  int64_t nt = 0, seek = 0;
  while (n - seek >= MEL_N_FFT) {                  // (a tail shorter than one analysis frame is not decoded)
    const int64_t len = std::min(wlen, n - seek);
    const int win_index = (int)((double)len / samples_per_ts);       // whole timestamp units inside the window
    wb_timestamp_params wtp = *tp;
    if (wtp.max_timestamp_index < 0 || wtp.max_timestamp_index > win_index) wtp.max_timestamp_index = win_index;
    // the window's prompt: [start-of-prev] + the last hist_cap tokens of the history + prompt; no history section: prompt alone
    const int n_hist = (int)std::min<size_t>(history.size(), (size_t)hist_cap);
    if (n_hist > 0) {
      wprompt.assign(1, cond->sot_prev);
      wprompt.insert(wprompt.end(), history.end() - n_hist, history.end());
      wprompt.insert(wprompt.end(), base_prompt, base_prompt + base_prompt_len);
      prompt = wprompt.data(); prompt_len = (int32_t)wprompt.size();
    } else {
      prompt = base_prompt; prompt_len = base_prompt_len;
    }
    if (cond && nw < cond->win_cap) {
      if (cond->win_seek) cond->win_seek[nw] = seek;
      if (cond->win_prompt_len) cond->win_prompt_len[nw] = prompt_len;
    }
    wb_session* s = nullptr;
    int rc = session_create(m, 1, bp ? bp->beam_size : std::max(1, tp->best_of), p->padding, &s);
    int32_t rlen = 0;
    if (rc == WB_OK) {
      s->sample_rate = (double)sample_rate;
      rc = session_encode_pcm(s, pcm, n, &seek, &len, false);
      if (rc == WB_OK) rc = wb_session_set_suppress(s, suppress, suppress_first);
      if (rc == WB_OK && n_hist > 0) rc = wb_session_set_prefill(s, 1);     // a history section: the prompt is prefilled by one pass
      if (rc == WB_OK)
        rc = bp ? wb_session_decode_timestamps_beam(s, p, &wtp, bp, prompt, prompt_len, nullptr, row.data(), stride, &rlen, nullptr, nullptr)
                : wb_session_decode_timestamps(s, p, &wtp, prompt, prompt_len, nullptr, nullptr, row.data(), stride, &rlen, nullptr,
                                               nullptr);
      wb_session_free(s);
    }
    WB_TRY(rc);
    nw++;
    const int32_t* gen = row.data() + prompt_len;
    int32_t k = 0, adv = 0;
    WB_TRY(wb_segments_from_tokens(gen, rlen - prompt_len, tb, nts, p->tok_end_of_text, win_index, tp->seconds_per_timestamp, sb.data(),
                                   se.data(), t0.data(), t1.data(), (int32_t)sb.size(), &k, &adv));
    const double off = (double)seek / (double)sample_rate;
    for (int i = 0; i < k; i++) {
      WB_REQUIRE(ns < seg_cap, WB_ERR_ARG, "wb_waveform_to_segments: more than seg_cap = %d segments", seg_cap);
      seg_start[ns] = (float)(off + t0[i]); seg_end_time[ns] = (float)(off + t1[i]);
      seg_tok_begin[ns] = (int32_t)nt;
      for (int j = sb[i]; j < se[i]; j++)
        if (!((unsigned)(gen[j] - tb) < (unsigned)nts)) {
          WB_REQUIRE(nt < text_cap, WB_ERR_ARG, "wb_waveform_to_segments: more than text_cap = %lld tokens", (long long)text_cap);
          text_tokens[nt++] = gen[j];
        }
      seg_tok_end[ns] = (int32_t)nt;
      ns++;
    }
    if (cond) {
      // the tokens the window's segments cover (timestamps included, end-of-text and the tail behind the last pair not), then
      // Whisper's two reset rules
      if (k > 0) history.insert(history.end(), gen + sb[0], gen + se[k - 1]);
      if (!cond->on || tp->temperature > 0.5f) history.clear();
    }
    int64_t step = (int64_t)std::llround((double)adv * samples_per_ts);
    if (step <= 0) step = len;                     // progress: an advance of 0 moves a whole window
    seek += std::min(step, len);
  }
  *n_segments = ns; *n_text_tokens = nt;
  if (n_windows) *n_windows = nw;
  return WB_OK;
}

int wb_waveform_to_segments(wb_model* m, const float* pcm, int64_t n, int sample_rate, const wb_decode_params* p,
                            const wb_timestamp_params* tp, const uint8_t* suppress, const uint8_t* suppress_first,
                            const int32_t* prompt, int32_t prompt_len, float* seg_start, float* seg_end_time,
                            int32_t* seg_tok_begin, int32_t* seg_tok_end, int32_t seg_cap, int32_t* n_segments,
                            int32_t* text_tokens, int64_t text_cap, int64_t* n_text_tokens, int32_t* n_windows) {
  return waveform_segments_loop(m, pcm, n, sample_rate, p, tp, nullptr, suppress, suppress_first, prompt, prompt_len, seg_start,
                                seg_end_time, seg_tok_begin, seg_tok_end, seg_cap, n_segments, text_tokens, text_cap, n_text_tokens,
                                n_windows);
}

int wb_waveform_to_segments_beam(wb_model* m, const float* pcm, int64_t n, int sample_rate, const wb_decode_params* p,
                                 const wb_timestamp_params* tp, const wb_beam_params* bp, const uint8_t* suppress,
                                 const uint8_t* suppress_first, const int32_t* prompt, int32_t prompt_len, float* seg_start,
                                 float* seg_end_time, int32_t* seg_tok_begin, int32_t* seg_tok_end, int32_t seg_cap,
                                 int32_t* n_segments, int32_t* text_tokens, int64_t text_cap, int64_t* n_text_tokens,
                                 int32_t* n_windows) {
  WB_REQUIRE(bp, WB_ERR_ARG, "wb_waveform_to_segments_beam: null argument");
  return waveform_segments_loop(m, pcm, n, sample_rate, p, tp, bp, suppress, suppress_first, prompt, prompt_len, seg_start,
                                seg_end_time, seg_tok_begin, seg_tok_end, seg_cap, n_segments, text_tokens, text_cap, n_text_tokens,
                                n_windows);
}

int wb_waveform_to_segments_conditioned(wb_model* m, const float* pcm, int64_t n, int sample_rate, const wb_decode_params* p,
                                        const wb_timestamp_params* tp, const wb_beam_params* bp, const uint8_t* suppress,
                                        const uint8_t* suppress_first, const int32_t* prompt, int32_t prompt_len,
                                        int32_t tok_start_of_prev, int32_t condition_on_previous_text, int32_t max_prompt_tokens,
                                        const int32_t* initial_prompt, int32_t n_initial_prompt, float* seg_start,
                                        float* seg_end_time, int32_t* seg_tok_begin, int32_t* seg_tok_end, int32_t seg_cap,
                                        int32_t* n_segments, int32_t* text_tokens, int64_t text_cap, int64_t* n_text_tokens,
                                        int32_t* n_windows, int64_t* win_seek, int32_t* win_prompt_len, int32_t win_cap) {
  const SeekCond cond{tok_start_of_prev, condition_on_previous_text, max_prompt_tokens, initial_prompt, n_initial_prompt,
                      win_seek, win_prompt_len, win_cap};
  return waveform_segments_loop(m, pcm, n, sample_rate, p, tp, bp, suppress, suppress_first, prompt, prompt_len, seg_start,
                                seg_end_time, seg_tok_begin, seg_tok_end, seg_cap, n_segments, text_tokens, text_cap, n_text_tokens,
                                n_windows, &cond);
}

}  // extern "C"
