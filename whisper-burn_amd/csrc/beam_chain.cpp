// Device-chained beam search: beam.rs bookkeeping as a kernel between two steps (decode.hip: dec_beam_update_kernel), its
// control block on the host side, and the test hook that drives the same kernel with a scripted step function.
#include "decode_step.h"
#include "switches.h"

using namespace wb;

namespace wb {

// The result of a device-chained beam search from its control block (copied to the host): per window the sequence of the
// max-log-prob beam -- beam.rs:33-36, the LAST of the equal maxima -- walked back through the node tree.
static int beam_chain_extract(const std::vector<int>& ctl, const BeamChainLayout& bl, const int32_t* prompt, int P,
                              int32_t* out_tokens, int32_t row_stride, int32_t* out_lens, bool* all_done_out) {
  const double* lp = reinterpret_cast<const double*>(ctl.data() + bl.lp);
  const int* nodes = ctl.data() + bl.nodes;
  bool all_done = true;
  for (int w = 0; w < bl.W; w++) {
    const int nb = ctl[bl.nb + w];
    int best = -1;
    for (int i = 0; i < nb; i++) {
      WB_REQUIRE(lp[w * BEAM_KB + i] == lp[w * BEAM_KB + i], WB_ERR_STATE, "beam search: NaN log-probability (reference panics)");
      if (best < 0 || lp[w * BEAM_KB + i] >= lp[w * BEAM_KB + best]) best = i;
    }
    std::vector<int32_t> seq;
    for (int nd = best >= 0 ? ctl[bl.node + w * BEAM_KB + best] : -1; nd >= 0; nd = nodes[2 * nd + 1]) seq.push_back(nodes[2 * nd]);
    std::reverse(seq.begin(), seq.end());
    const int len = (P - 1) + (int)seq.size();
    WB_REQUIRE(len <= row_stride, WB_ERR_ARG, "row_stride too small");
    int32_t* row = out_tokens + (size_t)w * row_stride;
    for (int i = 0; i < P - 1; i++) row[i] = prompt[i];
    for (size_t i = 0; i < seq.size(); i++) row[P - 1 + i] = seq[i];
    out_lens[w] = len;
    all_done = all_done && (ctl[bl.done + w] != 0 || (best >= 0 && ctl[bl.fin + w * BEAM_KB + best]));
  }
  *all_done_out = all_done;
  return WB_OK;
}

// The initial control block: one beam per window holding the prompt's last token (the rest of the prompt is the KV prefill).
static void beam_chain_init(std::vector<int>& ctl, const BeamChainLayout& bl, const int32_t* prompt, int P, int eot) {
  ctl.assign((size_t)bl.total_ints, 0);
  double* lp = reinterpret_cast<double*>(ctl.data() + bl.lp);
  int* nodes = ctl.data() + bl.nodes;
  for (int w = 0; w < bl.W; w++) {
    const int nd = w * BEAM_KB;                   // level 0 of the pool
    ctl[bl.nb + w] = 1;
    ctl[bl.node + w * BEAM_KB] = nd;
    nodes[2 * nd] = prompt[P - 1]; nodes[2 * nd + 1] = -1;
    ctl[bl.fin + w * BEAM_KB] = prompt[P - 1] == eot ? 1 : 0;     // transcribe.rs:235-241
    ctl[bl.prev_slot + w * BEAM_KB] = P > 1 ? w : -1;
    lp[w * BEAM_KB] = 0.0;
  }
}

// Beam search with the bookkeeping on the device.  What the host still does: the prompt prefill (P - 1 ordinary steps), the
// initial control block, enqueueing the steps (whole chunks as one graph launch), one synchronisation per chunk to see whether
// every window has ended, and the walk back through the node tree at the end.  Results are those of beam_search_windows
// (transcribe.cpp) step for step: same top-k rows, same f64 sums, same insertion and tie rules.
int session_beam_chain(wb_session* s, const int32_t* prompt, int P, int k, int eot, int max_depth, int mask_until_len,
                       int32_t* out_tokens, int32_t row_stride, int32_t* out_lens, bool* handled) {
  *handled = false;
  wb_model* m = s->m;
  const wb_dims& D = m->dims;
  const int W = s->W, S = s->S, V = D.n_vocab;
  if (!sw::beam_chain() || W > 64 || k < 1 || k > TOPK_MAX || k > s->max_beams || max_depth <= 0 || s->step != 0 || P < 1 || W * k > S)
    return WB_OK;
  WB_REQUIRE(s->has_mask || mask_until_len < P, WB_ERR_STATE, "wb_session_decode: special mask not set");
  *handled = true;
  const int asked_depth = max_depth;
  max_depth = std::min(max_depth, s->Lmax - (P - 1));
  WB_HIP(hipSetDevice(m->device));
  hipStream_t st = s->st;
  const StepLayout& L = s->lay;
  {  // prefill: all prompt tokens but the last only feed the KV cache (beam_search_windows does the same) -- P - 1 steps, or one
     // pass when the session's prefill mode asks for it (prefill.cpp)
    std::vector<int> win(W);
    for (int w = 0; w < W; w++) win[w] = w;
    WB_TRY(session_prefill_prompt(s, prompt, P, win.data(), W));
  }
  const BeamChainLayout bl = make_beam_layout(W, std::max(max_depth, 0));
  WB_TRY(s->bc_ctl.ensure((size_t)bl.total_ints * 4));
  WB_TRY(s->bc_topk.ensure((size_t)S * TOPK_MAX * 8));
  std::vector<int> ctl;
  beam_chain_init(ctl, bl, prompt, P, eot);
  WB_HIP(hipMemcpyAsync(s->bc_ctl.p, ctl.data(), ctl.size() * 4, hipMemcpyHostToDevice, st));
  WB_HIP(hipStreamSynchronize(st));
  // launch shape: the bucket wb_session_step would pick for the most rows the search can have live (W k)
  const StepPlan plan = plan_step(s, W * k, true);
  BeamStepIO bio;
  bio.state_src = s->state.as<int>();
  bio.topk_id = s->bc_topk.as<int32_t>();
  bio.topk_lp = reinterpret_cast<float*>(s->bc_topk.as<int32_t>() + (size_t)S * TOPK_MAX);
  bio.upd.ctl = s->bc_ctl.as<int>(); bio.upd.bl = bl; bio.upd.topk_id = bio.topk_id; bio.upd.topk_lp = bio.topk_lp;
  // the bookkeeping kernel writes the device state block the step kernels read, and prepares the step's rows itself
  bio.upd.state_out = s->state.as<int>(); bio.upd.lay = L;
  bio.upd.tabs = s->tabs.as<int>(); bio.upd.Lmax = s->Lmax; bio.upd.E = m->tok_emb; bio.upd.pos = m->dec_pos;
  bio.upd.d = D.n_text_state; bio.upd.x = s->x.as<float>(); bio.upd.k = k; bio.upd.eot = eot; bio.upd.V = V;
  bio.upd.first = 0; bio.upd.step_pos = P - 1;
  // the captured graphs bake in the search's constants: drop them when those differ from the last search of this session
  const uint64_t bsig = ((uint64_t)max_depth << 40) ^ ((uint64_t)(P - 1) << 24) ^ ((uint64_t)k << 16) ^ (uint64_t)(unsigned)eot;
  if (bsig != s->beam_sig) { s->clear_graphs(); s->beam_sig = bsig; }
  ScopedTimer tm(st, 3);
  {
    BeamChainArgs a0 = bio.upd;
    a0.first = 1;                                  // termination test + slots of the first step (beam.rs:23-27 runs BEFORE the step)
    launch_dec_beam_update(st, a0);
  }
  const int chunk = 16;
  int depth = 0;
  int hdr[BC_HDR] = {0};
  while (depth < max_depth) {
    int enq = 0;
    while (depth + enq < max_depth && enq < chunk) {
      const int d0 = depth + enq;
      const int use_mask = (P + d0) <= mask_until_len ? 1 : 0;     // transcribe.rs:271-275
      const int run = (!use_mask && max_depth - d0 >= chunk && enq == 0) ? chunk : 1;
      StepCall call;
      call.k = k; call.use_mask = use_mask; call.eot = eot; call.reps = run; call.bio = &bio;
      WB_TRY(launch_step(s, plan, call));
      if (profile().on) profile().ms[4] += run;
      enq += run;
    }
    depth += enq;
    WB_HIP(hipMemcpyAsync(hdr, s->bc_ctl.p, sizeof(hdr), hipMemcpyDeviceToHost, st));
    WB_HIP(hipStreamSynchronize(st));
    if (hdr[BC_ALLDONE] || hdr[BC_ERR]) break;     // every window has ended: the kernels of further steps would exit at once
  }
  tm.stop();
  WB_HIP(hipMemcpyAsync(ctl.data(), s->bc_ctl.p, ctl.size() * 4, hipMemcpyDeviceToHost, st));
  WB_HIP(hipStreamSynchronize(st));
  tm.collect();
  if (profile().on) prof_collect();
  s->prof_step_off = 0;
  const int steps_done = ctl[BC_DEPTH];
  s->step += steps_done;
  s->prev_n = 0; s->prev_len.clear(); s->prev_win.clear();     // (the device-side slots are not mirrored: no host-driven step may follow)
  s->last_had_logits = 0;
  WB_TRY(dec_split_check(s));
  WB_REQUIRE(ctl[BC_ERR] == 0, WB_ERR_STATE, "beam search: NaN log-probability (reference panics)");
  {
    bool all_done = true;
    WB_TRY(beam_chain_extract(ctl, bl, prompt, P, out_tokens, row_stride, out_lens, &all_done));
    if (max_depth < asked_depth && !all_done)
      WB_REQUIRE(false, WB_ERR_SHAPE, "Token sequence length %d must not exceed %d.", s->Lmax + 1, s->Lmax);
  }
  return WB_OK;
}

}  // namespace wb

// Test hook: beam.rs's bookkeeping as the DEVICE runs it (dec_beam_update_kernel), driven by a caller-supplied step function
// with wb_session_step's contract instead of the decoder -- the counterpart of wb_beam_search (the host restatement), so that
// the two can be compared on scripted log-prob rows with exact ties, finished beams and windows ending at different depths.
// No model: `device` only hosts the three small buffers.
extern "C" int wb_beam_search_device(int device, const wb_decode_params* p, int n_windows, int n_vocab, wb_step_fn step,
                                     void* user, int32_t* out_tokens, int32_t row_stride, int32_t* out_lens) {
  using namespace wb;
  WB_REQUIRE(p && step && out_tokens && out_lens && n_windows >= 1 && n_windows <= 64, WB_ERR_ARG, "wb_beam_search_device: bad argument");
  WB_REQUIRE(p->beam_size >= 1 && p->beam_size <= TOPK_MAX && p->max_depth >= 0, WB_ERR_ARG, "wb_beam_search_device: bad beam_size / max_depth");
  const int W = n_windows, k = p->beam_size, S = W * MAX_BEAMS, P = 4, V = n_vocab, eot = p->tok_end_of_text;
  const int32_t prompt[4] = {p->tok_start_of_transcript, p->tok_language, p->tok_transcribe, p->tok_no_timestamps};
  WB_REQUIRE(row_stride >= P + p->max_depth, WB_ERR_ARG, "row_stride %d < %d", row_stride, P + p->max_depth);
  wb::GpuTurn turn(device);
  WB_HIP(hipSetDevice(device));
  const StepLayout L = make_step_layout(S, W);
  const BeamChainLayout bl = make_beam_layout(W, p->max_depth);
  DevMem d_ctl, d_state, d_topk;
  WB_TRY(d_ctl.ensure((size_t)bl.total_ints * 4));
  WB_TRY(d_state.ensure((size_t)L.total * 4));
  WB_TRY(d_topk.ensure((size_t)S * TOPK_MAX * 8));
  std::vector<int32_t> tok(S), par(S), win(S);
  for (int t = 0; t < P - 1; t++) {               // the prompt prefill: steps without logits, as beam_search_windows issues them
    for (int w = 0; w < W; w++) { tok[w] = prompt[t]; par[w] = t == 0 ? -1 : w; win[w] = w; }
    WB_TRY(step(user, tok.data(), par.data(), win.data(), W, 0, 0, nullptr, nullptr));
  }
  std::vector<int> ctl;
  beam_chain_init(ctl, bl, prompt, P, eot);
  WB_HIP(hipMemcpy(d_ctl.p, ctl.data(), ctl.size() * 4, hipMemcpyHostToDevice));
  BeamChainArgs a;
  a.ctl = d_ctl.as<int>(); a.bl = bl; a.topk_id = d_topk.as<int32_t>();
  a.topk_lp = reinterpret_cast<float*>(d_topk.as<int32_t>() + (size_t)S * TOPK_MAX);
  a.state_out = d_state.as<int>(); a.lay = L; a.k = k; a.eot = eot; a.V = V; a.step_pos = P - 1;
  a.first = 1;
  launch_dec_beam_update(nullptr, a);
  a.first = 0;
  std::vector<int> st(L.total);
  std::vector<int32_t> ids((size_t)S * TOPK_MAX), cid((size_t)S * k);
  std::vector<float> lps((size_t)S * TOPK_MAX), clp((size_t)S * k);
  for (int depth = 0; depth < p->max_depth; depth++) {
    WB_HIP(hipMemcpy(st.data(), d_state.p, st.size() * 4, hipMemcpyDeviceToHost));
    const int n = st[ST_N];
    if (n == 0) break;
    WB_REQUIRE(n <= S, WB_ERR_STATE, "wb_beam_search_device: %d live rows", n);
    for (int i = 0; i < n; i++) { tok[i] = st[L.tok + i]; par[i] = st[L.parent + i]; win[i] = st[L.win + i]; }
    const int apply_mask = (P + depth) <= p->mask_until_len;
    WB_TRY(step(user, tok.data(), par.data(), win.data(), n, apply_mask, k, cid.data(), clp.data()));
    for (int i = 0; i < n; i++)
      for (int j = 0; j < k; j++) { ids[(size_t)i * TOPK_MAX + j] = cid[(size_t)i * k + j]; lps[(size_t)i * TOPK_MAX + j] = clp[(size_t)i * k + j]; }
    WB_HIP(hipMemcpy(d_topk.p, ids.data(), ids.size() * 4, hipMemcpyHostToDevice));
    WB_HIP(hipMemcpy(d_topk.as<int32_t>() + (size_t)S * TOPK_MAX, lps.data(), lps.size() * 4, hipMemcpyHostToDevice));
    launch_dec_beam_update(nullptr, a);
  }
  WB_HIP(hipMemcpy(ctl.data(), d_ctl.p, ctl.size() * 4, hipMemcpyDeviceToHost));
  WB_REQUIRE(ctl[BC_ERR] == 0, WB_ERR_STATE, "beam search: NaN log-probability (reference panics)");
  bool all_done = true;
  return beam_chain_extract(ctl, bl, prompt, P, out_tokens, row_stride, out_lens, &all_done);
}
