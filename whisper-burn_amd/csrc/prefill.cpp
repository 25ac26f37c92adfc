// Prompt prefill by one teacher-forced pass (kernels: prefill.hip, the pass: engine.cpp run_prefill): the session side, its
// C ABI and the two test hooks (the store kernel alone on caller arrays; a slot's cached rows through its position table).
#include <cstring>

#include "decode_step.h"
#include "switches.h"

namespace wb {

int session_prefill(wb_session* s, const int32_t* tokens, int n, const int* wa, int nA) {
  wb_model* m = s->m;
  const wb_dims& D = m->dims;
  const int d = D.n_text_state, V = D.n_vocab;
  WB_REQUIRE(n >= 0 && nA >= 1 && nA <= s->W, WB_ERR_ARG, "prefill: %d tokens for %d windows (the session has %d)", n, nA, s->W);
  WB_REQUIRE(s->step == 0, WB_ERR_STATE, "prefill: the session is at step %d (wb_session_rewind first)", s->step);
  WB_REQUIRE((int)s->C.size() == s->W && s->ckv.p, WB_ERR_STATE, "prefill: the session holds no encoded windows");
  for (int t = 0; t < n; t++) WB_REQUIRE(tokens[t] >= 0 && tokens[t] < V, WB_ERR_ARG, "token id %d out of range [0,%d)", tokens[t], V);
  for (int a = 0; a < nA; a++) {
    WB_REQUIRE(wa[a] >= 0 && wa[a] < s->W, WB_ERR_ARG, "prefill: window %d out of range", wa[a]);
    WB_REQUIRE(a == 0 || wa[a] > wa[a - 1], WB_ERR_ARG, "prefill: the active windows are not ascending");
  }
  if (n == 0) return WB_OK;
  WB_HIP(hipSetDevice(m->device));
  if (!s->decode_ready) WB_TRY(session_reserve(s, D.n_text_ctx));
  WB_REQUIRE(n < s->Lmax, WB_ERR_SHAPE, "Token sequence length %d must not exceed %d.", n + 1, s->Lmax);   // mod.rs:134-139
  if (s->enc_guard_pending) {            // a deferred range check of the encode pass: settle it before its output is read
    WB_HIP(hipStreamSynchronize(s->st));
    bool reencoded = false;
    WB_TRY(session_enc_guard_resolve(s, &reencoded));
  }
  PrefillJob& J = s->prefill_job;        // (its host arrays outlive the enqueued copies: nothing waits here)
  J.nA = nA; J.n = n;
  J.tokens.assign(tokens, tokens + n);
  J.C.resize(nA); J.kv_row0.resize(nA);
  for (int a = 0; a < nA; a++) { J.C[a] = s->C[wa[a]]; J.kv_row0[a] = s->row0[wa[a]]; }
  J.ckv = s->ckv.as<float>(); J.ckv_layer_stride = (int64_t)s->enc_rows * 2 * d; J.ldkv = 2 * d;   // as session_score
  J.S = s->S; J.Lmax = s->Lmax;
  J.kc = s->kc.as<float>(); J.vc = s->vc.as<float>(); J.kv_layer_stride = (int64_t)s->Lmax * s->S * d;
  J.tabs = s->tabs.as<int>();
  ScopedTimer tm(s->st, 3);
  WB_TRY(run_prefill(m, s->st, s->ws, J));
  tm.stop();
  if (tm.on) { WB_HIP(hipStreamSynchronize(s->st)); tm.collect(); prof_collect(); }
  s->step = n;
  s->prev_n = nA;
  s->prev_len.assign(nA, n);
  s->prev_win.assign(wa, wa + nA);
  s->last_had_logits = 0;
  return WB_OK;
}

int session_prefill_prompt(wb_session* s, const int32_t* prompt, int P, const int* wa, int nA) {
  if (P <= 1) return WB_OK;
  if (s->prefill_mode == 1 && sw::prefill_pass() && s->step == 0) return session_prefill(s, prompt, P - 1, wa, nA);
  std::vector<int32_t> tok(nA), par(nA);
  for (int t = 0; t < P - 1; t++) {
    for (int a = 0; a < nA; a++) { tok[a] = prompt[t]; par[a] = t == 0 ? -1 : a; }
    WB_TRY(wb_session_step(s, tok.data(), par.data(), wa, nA, 0, 0, nullptr, nullptr));
  }
  return WB_OK;
}

}  // namespace wb

using namespace wb;

extern "C" {

int wb_session_set_prefill(wb_session* s, int mode) {
  WB_REQUIRE(s && (mode == 0 || mode == 1), WB_ERR_ARG, "wb_session_set_prefill: mode %d (0: steps, 1: one pass)", mode);
  s->prefill_mode = mode;
  return WB_OK;
}

int wb_session_prefill(wb_session* s, const int32_t* tokens, int32_t n, const uint8_t* active) {
  WB_REQUIRE(s && (tokens || n == 0) && n >= 0, WB_ERR_ARG, "wb_session_prefill: bad argument");
  wb::GpuTurn turn(s->device);
  std::vector<int> wa;
  for (int w = 0; w < s->W; w++)
    if (!active || active[w]) wa.push_back(w);
  WB_REQUIRE(!wa.empty(), WB_ERR_ARG, "wb_session_prefill: no active window");
  WB_TRY(session_prefill(s, tokens, n, wa.data(), (int)wa.size()));
  if (n > 0) WB_HIP(hipStreamSynchronize(s->st));
  return WB_OK;
}

int wb_prefill_store(int device, const float* qkv, int32_t nA, int32_t n, int32_t d, int32_t ld, int32_t S, int32_t Lmax,
                     float* Kc, float* Vc, int32_t* tabs) {
  WB_REQUIRE(qkv && Kc && Vc && tabs && nA >= 1 && n >= 1 && d >= 1 && S >= 1 && Lmax >= 1, WB_ERR_ARG, "wb_prefill_store: bad argument");
  WB_REQUIRE(nA <= S && n <= Lmax && d % 4 == 0 && ld % 4 == 0 && ld >= 3 * d, WB_ERR_SHAPE,
             "wb_prefill_store: nA %d / S %d, n %d / Lmax %d, d %d, ld %d", nA, S, n, Lmax, d, ld);
  WB_REQUIRE((int64_t)Lmax * S * d < ((int64_t)1 << 31) && (int64_t)nA * n * ld < ((int64_t)1 << 31), WB_ERR_SHAPE,
             "wb_prefill_store: too large");
  wb::GpuTurn turn(device);
  WB_HIP(hipSetDevice(device));
  const size_t rows = (size_t)nA * n, pool = (size_t)Lmax * S * d, tw = (size_t)2 * S * Lmax;
  // the three arrays the kernel writes travel to the device as the caller filled them (canaries included) and come back whole
  DevMem dq, dk, dv, dt;
  WB_TRY(dq.alloc(rows * ld * 4));
  WB_TRY(dk.alloc(pool * 4));
  WB_TRY(dv.alloc(pool * 4));
  WB_TRY(dt.alloc(tw * 4));
  hipStream_t st = nullptr;
  WB_HIP(hipMemcpyAsync(dq.p, qkv, rows * ld * 4, hipMemcpyHostToDevice, st));
  WB_HIP(hipMemcpyAsync(dk.p, Kc, pool * 4, hipMemcpyHostToDevice, st));
  WB_HIP(hipMemcpyAsync(dv.p, Vc, pool * 4, hipMemcpyHostToDevice, st));
  WB_HIP(hipMemcpyAsync(dt.p, tabs, tw * 4, hipMemcpyHostToDevice, st));
  prof_tag(KC_PREFILL_STORE, 16.0 * rows * d);
  WB_REQUIRE(launch_prefill_store(st, dq.as<float>(), nA, n, d, ld, S, Lmax, dk.as<float>(), dv.as<float>(), dt.as<int>()) == 0,
             WB_ERR_SHAPE, "wb_prefill_store: unsupported shape");
  WB_HIP(hipGetLastError());
  WB_HIP(hipMemcpyAsync(Kc, dk.p, pool * 4, hipMemcpyDeviceToHost, st));
  WB_HIP(hipMemcpyAsync(Vc, dv.p, pool * 4, hipMemcpyDeviceToHost, st));
  WB_HIP(hipMemcpyAsync(tabs, dt.p, tw * 4, hipMemcpyDeviceToHost, st));
  WB_HIP(hipStreamSynchronize(st));
  return WB_OK;
}

int wb_session_self_kv(wb_session* s, int32_t layer, int32_t slot, int32_t n_pos, float* K, float* V) {
  WB_REQUIRE(s && K && V, WB_ERR_ARG, "wb_session_self_kv: null argument");
  const wb_dims& D = s->m->dims;
  const int d = D.n_text_state;
  WB_REQUIRE(s->decode_ready && s->step >= 1, WB_ERR_STATE, "wb_session_self_kv: the session has run no step");
  WB_REQUIRE(layer >= 0 && layer < D.n_text_layer && slot >= 0 && slot < s->prev_n && n_pos >= 1 && n_pos <= s->prev_len[slot],
             WB_ERR_ARG, "wb_session_self_kv: layer %d / slot %d / n_pos %d", layer, slot, n_pos);
  wb::GpuTurn turn(s->device);
  WB_HIP(hipSetDevice(s->m->device));
  hipStream_t st = s->st;
  // the tables the LAST step (or prefill) wrote: parity (step - 1) & 1
  std::vector<int> tab((size_t)n_pos);
  const int* tdev = s->tabs.as<int>() + (size_t)((s->step - 1) & 1) * s->S * s->Lmax + (size_t)slot * s->Lmax;
  WB_HIP(hipMemcpyAsync(tab.data(), tdev, (size_t)n_pos * 4, hipMemcpyDeviceToHost, st));
  WB_HIP(hipStreamSynchronize(st));
  const size_t pool = (size_t)s->Lmax * s->S;
  for (int p = 0; p < n_pos; p++) {
    WB_REQUIRE(tab[p] >= 0 && (size_t)tab[p] < pool, WB_ERR_STATE, "wb_session_self_kv: table entry %d of slot %d is %d", p, slot, tab[p]);
    const size_t off = ((size_t)layer * pool + (size_t)tab[p]) * d;
    WB_HIP(hipMemcpyAsync(K + (size_t)p * d, s->kc.as<float>() + off, (size_t)d * 4, hipMemcpyDeviceToHost, st));
    WB_HIP(hipMemcpyAsync(V + (size_t)p * d, s->vc.as<float>() + off, (size_t)d * 4, hipMemcpyDeviceToHost, st));
  }
  WB_HIP(hipStreamSynchronize(st));
  return WB_OK;
}

}  // extern "C"
