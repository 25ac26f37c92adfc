// Device-chained temperature sampling: the host side of sample.hip's dec_sample_update_kernel (control block, prompt
// prefill, chunks of steps as one graph, the best-of-n pick), its C ABI and the test hook that runs the draw alone.
#include <cmath>
#include <cstring>
#include <limits>

#include "decode_step.h"

using namespace wb;

namespace wb {

// Sampling with the draw and the row bookkeeping on the device.  Rows are a * best_of + j over the ACTIVE windows in order
// (a: ordinal of the window among them): an inactive window has no row at all -- nothing of it is prefetched, streamed or
// written.  What the host does: the prompt prefill (P - 1 ordinary steps over one row per active window), the control block
// and the first step's state block, enqueueing the steps (whole chunks as one graph launch), one header read-back per
// chunk, and the pick of each window's best sample at the end.
int session_sample_chain(wb_session* s, const int32_t* prompt, int P, const SampleCall& sp, const uint8_t* active,
                         const int32_t* stream_ids, int eot, int max_depth, int mask_until_len, int32_t* out_tokens,
                         int32_t row_stride, int32_t* out_lens, double* out_sum, int32_t* out_best) {
  wb_model* m = s->m;
  const wb_dims& D = m->dims;
  const int W = s->W, V = D.n_vocab, bo = sp.best_of;
  WB_REQUIRE(sp.temperature > 0.f && std::isfinite(sp.temperature) && std::isfinite(1.0f / sp.temperature), WB_ERR_ARG,
             "sampling: temperature %g must be finite and > 0, and so must 1 / temperature", (double)sp.temperature);
  WB_REQUIRE(bo >= 1 && bo <= s->max_beams, WB_ERR_ARG, "sampling: best_of %d outside [1, %d]", bo, s->max_beams);
  WB_REQUIRE(P >= 1 && max_depth >= 0, WB_ERR_ARG, "sampling: prompt_len %d / max_depth %d", P, max_depth);
  WB_REQUIRE(row_stride >= P + max_depth, WB_ERR_ARG, "row_stride %d < %d", row_stride, P + max_depth);
  for (int i = 0; i < P; i++) WB_REQUIRE(prompt[i] >= 0 && prompt[i] < V, WB_ERR_ARG, "prompt token %d out of range", prompt[i]);
  WB_REQUIRE(eot >= 0 && eot < V, WB_ERR_ARG, "end-of-text token out of range");
  WB_REQUIRE(sp.attempt >= 0, WB_ERR_ARG, "sampling: attempt %d", sp.attempt);
  WB_REQUIRE(s->step == 0, WB_ERR_STATE, "wb_session_decode_sample: the session is at step %d (wb_session_rewind first)", s->step);
  WB_REQUIRE(s->has_mask || mask_until_len < P || max_depth == 0, WB_ERR_STATE, "wb_session_decode_sample: special mask not set");
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
  const SampleChainLayout sl = make_sample_layout(S, W, std::max(max_depth, 0));
  WB_TRY(s->sc_ctl.ensure((size_t)sl.total_ints * 4));
  WB_TRY(s->sc_topk.ensure((size_t)S * TOPK_MAX * 8));
  std::vector<int> ctl((size_t)sl.total_ints, 0);
  const float inv_t = 1.0f / sp.temperature;
  ctl[SC_NROWS] = R; ctl[SC_BEST_OF] = bo; ctl[SC_ATTEMPT] = sp.attempt;
  ctl[SC_SEED_LO] = (int)(uint32_t)(sp.seed & 0xffffffffull); ctl[SC_SEED_HI] = (int)(uint32_t)(sp.seed >> 32);
  memcpy(&ctl[SC_INVT], &inv_t, 4);
  const bool start_finished = prompt[P - 1] == eot;       // transcribe.rs:235-241: nothing is generated behind an end-of-text
  for (int a = 0; a < nA; a++)
    for (int j = 0; j < bo; j++) {
      const int r = a * bo + j;
      ctl[sl.stream + r] = (int)((uint32_t)(stream_ids ? stream_ids[wa[a]] : wa[a] * bo) + (uint32_t)j);
      ctl[sl.fin + r] = start_finished ? 1 : 0;
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
    WB_HIP(hipMemcpyAsync(s->sc_ctl.p, ctl.data(), ctl.size() * 4, hipMemcpyHostToDevice, st));
    WB_HIP(hipStreamSynchronize(st));
    // launch shape: the bucket of the most rows a call on this session can have (W best_of), so that one graph serves every
    // set of active windows
    const StepPlan plan = plan_step(s, W * bo, true);
    SampleStepIO sio;
    sio.topk_id = s->sc_topk.as<int32_t>();
    sio.topk_lp = reinterpret_cast<float*>(s->sc_topk.as<int32_t>() + (size_t)S * TOPK_MAX);
    SampleChainArgs& u = sio.upd;
    u.ctl = s->sc_ctl.as<int>(); u.sl = sl; u.logits = s->logits.as<float>(); u.V = V; u.mask = s->mask.as<float>();
    u.row_stats = s->row_stats.as<float>(); u.state = s->state.as<int>(); u.lay = L; u.eot = eot;
    u.tabs = s->tabs.as<int>(); u.Lmax = s->Lmax; u.E = m->tok_emb; u.pos = m->dec_pos; u.d = D.n_text_state; u.x = s->x.as<float>();
    // the captured sampling steps bake in the control block and its layout (S, W: the buffer signature of launch_step;
    // max_depth: here): drop THEM when those differ from the last call -- temperature, seed, attempt, streams do not
    const uint64_t ssig = ((uint64_t)(uintptr_t)s->sc_ctl.p * 1099511628211ull) ^ ((uint64_t)max_depth << 20) ^ (uint64_t)(unsigned)eot ^ 1u;
    if (ssig != s->sample_sig) {
      for (auto it = s->graphs.begin(); it != s->graphs.end();)
        if (it->first & GRAPH_KEY_SAMPLE) { (void)hipGraphExecDestroy(it->second); it = s->graphs.erase(it); }
        else ++it;
      s->sample_sig = ssig;
    }
    ScopedTimer tm(st, 3);
    prof_tag(KC_PREPARE, 8.0 * R * D.n_text_state);
    launch_dec_prepare(st, reinterpret_cast<const int*>(s->host_block_dev), s->state.as<int>(), L, R, s->tabs.as<int>(), s->Lmax,
                       m->tok_emb, m->dec_pos, D.n_text_state, s->x.as<float>(), nullptr);
    const int chunk = 16;
    int depth = 0;
    int hdr[SC_HDR] = {0};
    while (depth < max_depth) {
      int enq = 0;
      while (depth + enq < max_depth && enq < chunk) {
        const int d0 = depth + enq;
        const int use_mask = (P + d0) <= mask_until_len ? 1 : 0;     // transcribe.rs:271-275
        const int run = (!use_mask && max_depth - d0 >= chunk && enq == 0) ? chunk : 1;
        StepCall call;
        // (call.eot stays at its default: the step kernels take no end-of-text without a greedy control block, and launch_step's
        // buffer signature carries it -- the prefill steps' value, so that prefill and sampling steps keep each other's graphs)
        call.k = 1; call.use_mask = use_mask; call.reps = run; call.sio = &sio;
        WB_TRY(launch_step(s, plan, call));
        if (profile().on) profile().ms[4] += run;
        enq += run;
      }
      depth += enq;
      WB_HIP(hipMemcpyAsync(hdr, s->sc_ctl.p, sizeof(hdr), hipMemcpyDeviceToHost, st));
      WB_HIP(hipStreamSynchronize(st));
      if (hdr[SC_ALLDONE] || hdr[SC_ERR]) break;   // every row has ended: the kernels of further steps would exit at once
    }
    tm.stop();
    WB_HIP(hipMemcpyAsync(ctl.data(), s->sc_ctl.p, ctl.size() * 4, hipMemcpyDeviceToHost, st));
    WB_HIP(hipStreamSynchronize(st));
    tm.collect();
    if (profile().on) prof_collect();
    s->prof_step_off = 0;
    for (int r = 0; r < R; r++) steps_done = std::max(steps_done, ctl[sl.ngen + r]);   // (an unfinished row drew once per step)
  }
  s->step += steps_done;
  s->prev_n = 0; s->prev_len.clear(); s->prev_win.clear();     // (the device-side slots are not mirrored: no host-driven step may follow)
  s->last_had_logits = 0;
  WB_TRY(dec_split_check(s));
  WB_REQUIRE(ctl[SC_ERR] == 0, WB_ERR_STATE, "sampling: a logits row was not finite");
  const double* sum = reinterpret_cast<const double*>(ctl.data() + sl.sum);
  bool all_done = true;
  s->smp_best_of = bo; s->smp_depth = sl.max_depth;
  s->smp_tokens.assign((size_t)W * bo * sl.max_depth, 0);
  s->smp_len.assign((size_t)W * bo, -1);
  for (int a = 0; a < nA; a++) {
    const int w = wa[a];
    int best = 0;
    double best_rank = -INFINITY;
    for (int j = 0; j < bo; j++) {
      const int r = a * bo + j, ng = ctl[sl.ngen + r];
      const int n_text = ng - ((ng > 0 && ctl[sl.tokens + r * sl.max_depth + ng - 1] == eot) ? 1 : 0);
      const double rank = n_text > 0 ? sum[r] / (double)n_text : -INFINITY;
      if (rank > best_rank) { best_rank = rank; best = j; }       // (the first of equal maxima)
      if (out_sum) out_sum[(size_t)w * bo + j] = sum[r];
      s->smp_len[(size_t)w * bo + j] = ng;
      for (int i = 0; i < ng; i++) s->smp_tokens[((size_t)w * bo + j) * sl.max_depth + i] = ctl[sl.tokens + r * sl.max_depth + i];
      all_done = all_done && ctl[sl.fin + r] != 0;
    }
    const int r = a * bo + best, ng = ctl[sl.ngen + r];
    int32_t* row = out_tokens + (size_t)w * row_stride;
    for (int i = 0; i < P; i++) row[i] = prompt[i];
    for (int i = 0; i < ng; i++) row[P + i] = ctl[sl.tokens + r * sl.max_depth + i];
    out_lens[w] = P + ng;
    if (out_best) out_best[w] = best;
  }
  if (max_depth < asked_depth && !all_done)
    WB_REQUIRE(false, WB_ERR_SHAPE, "Token sequence length %d must not exceed %d.", s->Lmax + 1, s->Lmax);
  return WB_OK;
}

}  // namespace wb

extern "C" {

void wb_sample_params_default(wb_sample_params* p) {
  if (!p) return;
  p->temperature = 1.0f; p->best_of = 5; p->seed = 0; p->attempt = 0;
}

int wb_session_rewind(wb_session* s) {
  WB_REQUIRE(s, WB_ERR_ARG, "wb_session_rewind: null argument");
  wb::GpuTurn turn(s->device);
  session_rewind(s);
  return WB_OK;
}

int wb_session_last_samples(wb_session* s, int32_t* tokens, int32_t row_stride, int32_t* lens) {
  WB_REQUIRE(s && tokens && lens, WB_ERR_ARG, "wb_session_last_samples: null argument");
  WB_REQUIRE(s->smp_best_of > 0 && (int)s->smp_len.size() == s->W * s->smp_best_of, WB_ERR_STATE,
             "wb_session_last_samples: no sampling call on this session");
  WB_REQUIRE(row_stride >= s->smp_depth, WB_ERR_ARG, "row_stride %d < %d", row_stride, s->smp_depth);
  for (size_t i = 0; i < s->smp_len.size(); i++) {
    lens[i] = s->smp_len[i];
    for (int l = 0; l < s->smp_len[i]; l++) tokens[i * row_stride + l] = s->smp_tokens[i * s->smp_depth + l];
  }
  return WB_OK;
}

int wb_session_graph_count(const wb_session* s) { return s ? (int)s->graphs.size() : 0; }
int64_t wb_session_graph_captures(const wb_session* s) { return s ? s->n_captures : 0; }
int wb_persist_resident_geometry(int32_t n_state, int32_t n_rows, int32_t max_keys, int32_t* out5) {
  WB_REQUIRE(out5, WB_ERR_ARG, "wb_persist_resident_geometry: null argument");
  int g[5] = {0, 0, 0, 0, 0};
  WB_REQUIRE(dec_persist_resident_geometry(n_state, n_rows, max_keys, g), WB_ERR_SHAPE,
             "wb_persist_resident_geometry: no persistent instance serves n_state %d with %d rows and %d keys", n_state, n_rows, max_keys);
  for (int i = 0; i < 5; i++) out5[i] = g[i];
  return WB_OK;
}

int wb_session_decode_sample(wb_session* s, const wb_decode_params* p, const wb_sample_params* sp, const int32_t* prompt,
                             int32_t prompt_len, const uint8_t* active, const int32_t* stream_ids, int32_t* out_tokens,
                             int32_t row_stride, int32_t* out_lens, double* out_sum_logprob, int32_t* out_best) {
  WB_REQUIRE(s && p && sp && prompt && out_tokens && out_lens, WB_ERR_ARG, "wb_session_decode_sample: null argument");
  wb::GpuTurn turn(s->device);
  const SampleCall c{sp->temperature, sp->best_of, sp->seed, sp->attempt};
  return session_sample_chain(s, prompt, prompt_len, c, active, stream_ids, p->tok_end_of_text, p->max_depth, p->mask_until_len,
                              out_tokens, row_stride, out_lens, out_sum_logprob, out_best);
}

int wb_sample_rows(int device, const float* logits, int32_t R, int32_t ld, int32_t V, const float* mask,
                   const uint8_t* row_masked, const float* row_stats, float temperature, uint64_t seed, int32_t attempt,
                   const int32_t* stream, const int32_t* position, int32_t eot, int32_t* out_token, float* out_logprob,
                   int32_t* out_err) {
  WB_REQUIRE(logits && row_stats && stream && position && out_token && out_logprob && out_err, WB_ERR_ARG, "wb_sample_rows: null argument");
  WB_REQUIRE(R >= 1 && V >= 1 && ld >= V && (int64_t)R * ld < ((int64_t)1 << 31), WB_ERR_ARG, "wb_sample_rows: R %d, V %d, ld %d", R, V, ld);
  WB_REQUIRE((mask != nullptr) == (row_masked != nullptr), WB_ERR_ARG, "wb_sample_rows: mask and row_masked go together");
  WB_REQUIRE(temperature > 0.f && std::isfinite(temperature) && std::isfinite(1.0f / temperature), WB_ERR_ARG, "wb_sample_rows: temperature %g", (double)temperature);
  WB_REQUIRE(eot >= 0 && eot < V && attempt >= 0, WB_ERR_ARG, "wb_sample_rows: eot %d / attempt %d", eot, attempt);
  wb::GpuTurn turn(device);
  WB_HIP(hipSetDevice(device));
  DevMem dx, dmask, du8, dst, di32, dout;
  WB_TRY(dx.alloc((size_t)R * ld * 4));
  WB_TRY(dmask.alloc((size_t)V * 4));
  WB_TRY(du8.alloc((size_t)R));
  WB_TRY(dst.alloc((size_t)R * 2 * 4));
  WB_TRY(di32.alloc((size_t)R * 2 * 4));
  // the three outputs sit between guard bands of poisoned words, checked after the run
  constexpr size_t GUARD = 64;
  const size_t out_words = (size_t)2 * R + 1;
  WB_TRY(dout.alloc((out_words + 2 * GUARD) * 4));
  hipStream_t st = nullptr;
  WB_HIP(hipMemsetAsync(dout.p, 0xFF, dout.bytes, st));
  WB_HIP(hipMemcpyAsync(dx.p, logits, (size_t)R * ld * 4, hipMemcpyHostToDevice, st));
  WB_HIP(hipMemcpyAsync(dst.p, row_stats, (size_t)R * 2 * 4, hipMemcpyHostToDevice, st));
  WB_HIP(hipMemcpyAsync(di32.p, stream, (size_t)R * 4, hipMemcpyHostToDevice, st));
  WB_HIP(hipMemcpyAsync(di32.as<int32_t>() + R, position, (size_t)R * 4, hipMemcpyHostToDevice, st));
  if (mask) {
    WB_HIP(hipMemcpyAsync(dmask.p, mask, (size_t)V * 4, hipMemcpyHostToDevice, st));
    WB_HIP(hipMemcpyAsync(du8.p, row_masked, (size_t)R, hipMemcpyHostToDevice, st));
  }
  SampleRowsArgs a;
  a.logits = dx.as<float>(); a.R = R; a.ld = ld; a.V = V;
  a.mask = mask ? dmask.as<float>() : nullptr; a.row_masked = mask ? du8.as<uint8_t>() : nullptr;
  a.row_stats = dst.as<float>();
  a.inv_t = 1.0f / temperature; a.seed_lo = (uint32_t)(seed & 0xffffffffull); a.seed_hi = (uint32_t)(seed >> 32);
  a.attempt = (uint32_t)attempt;
  a.stream = di32.as<int32_t>(); a.position = a.stream + R; a.eot = eot;
  a.out_token = dout.as<int32_t>() + GUARD; a.out_logprob = reinterpret_cast<float*>(a.out_token + R);
  a.out_err = a.out_token + 2 * R;
  WB_HIP(hipMemsetAsync(a.out_err, 0, 4, st));
  prof_tag(KC_SAMPLE_UPDATE, 4.0 * (double)R * V);
  launch_sample_rows(st, a);
  WB_HIP(hipGetLastError());
  WB_HIP(hipMemcpyAsync(out_token, a.out_token, (size_t)R * 4, hipMemcpyDeviceToHost, st));
  WB_HIP(hipMemcpyAsync(out_logprob, a.out_logprob, (size_t)R * 4, hipMemcpyDeviceToHost, st));
  WB_HIP(hipMemcpyAsync(out_err, a.out_err, 4, hipMemcpyDeviceToHost, st));
  uint32_t guards[2][GUARD];
  WB_HIP(hipMemcpyAsync(guards[0], dout.p, GUARD * 4, hipMemcpyDeviceToHost, st));
  WB_HIP(hipMemcpyAsync(guards[1], dout.as<int32_t>() + GUARD + out_words, GUARD * 4, hipMemcpyDeviceToHost, st));
  WB_HIP(hipStreamSynchronize(st));
  for (int b = 0; b < 2; b++)
    for (size_t i = 0; i < GUARD; i++)
      WB_REQUIRE(guards[b][i] == 0xFFFFFFFFu, WB_ERR_STATE, "wb_sample_rows: guard band %d overwritten at word %zu", b, i);
  return WB_OK;
}

}  // extern "C"
