// C ABI of the token scoring: per-token log-probabilities, probe log-probabilities (no-speech, language ids) and language
// detection (kernels: score.hip, the teacher-forced pass: engine.cpp run_score).
#include <cmath>
#include <cstring>
#include <limits>
#include <mutex>

#include "engine.h"
#include "session.h"

namespace wb {

// tokens [n][stride] + lens -> compact job rows; validates every argument that does not depend on the K/V source
static int score_rows(const wb_model* m, const int32_t* tokens, int n, int stride, const int32_t* lens,
                      int32_t mask_until_len, const int32_t* probe_ids, int32_t n_probe, int32_t probe_pos, ScoreJob* J) {
  const int V = m->dims.n_vocab;
  WB_REQUIRE(mask_until_len >= 0, WB_ERR_ARG, "score: mask_until_len %d", mask_until_len);
  WB_REQUIRE(n_probe >= 0 && (n_probe == 0 || probe_ids) && probe_pos >= 0, WB_ERR_ARG, "score: n_probe %d / probe_pos %d",
             n_probe, probe_pos);
  for (int p = 0; p < n_probe; p++)
    WB_REQUIRE(probe_ids[p] >= 0 && probe_ids[p] < V, WB_ERR_ARG, "probe id %d out of range [0,%d)", probe_ids[p], V);
  int L = 0;
  for (int i = 0; i < n; i++) {
    const int len = lens ? lens[i] : stride;
    WB_REQUIRE(len >= 1 && len <= stride, WB_ERR_ARG, "score: row %d has length %d (row stride %d)", i, len, stride);
    // mod.rs:134-139
    WB_REQUIRE(len <= m->dims.n_text_ctx, WB_ERR_SHAPE, "Token sequence length %d must not exceed %d.", len,
               (int)m->dims.n_text_ctx);
    // (a probe position may also be a masked one: the kernel keeps both statistics of such a row)
    WB_REQUIRE(n_probe == 0 || probe_pos < len, WB_ERR_ARG, "score: probe_pos %d is outside row %d of length %d", probe_pos, i,
               len);
    L = std::max(L, len);
  }
  J->n = n; J->L = L;
  J->mask_until_len = mask_until_len; J->probe_pos = probe_pos;
  J->probe_ids.assign(probe_ids, probe_ids + n_probe);
  J->len.resize(n);
  J->tokens.assign((size_t)n * L, 0);
  for (int i = 0; i < n; i++) {
    J->len[i] = lens ? lens[i] : stride;
    for (int l = 0; l < J->len[i]; l++) {
      const int32_t t = tokens[(size_t)i * stride + l];
      WB_REQUIRE(t >= 0 && t < V, WB_ERR_ARG, "token id %d out of range [0,%d)", t, V);
      J->tokens[(size_t)i * L + l] = t;
    }
  }
  return WB_OK;
}

// after the stream was synchronised: the job's results in the caller's layout
static void score_scatter(const ScoreJob& J, int stride, float* token_logprobs, float* probe_logprobs) {
  const float nan = std::numeric_limits<float>::quiet_NaN();
  const size_t NP = J.probe_ids.size();
  for (int i = 0; i < J.n; i++) {
    if (token_logprobs) {
      float* out = token_logprobs + (size_t)i * stride;
      for (int l = 0; l < stride; l++) out[l] = nan;                       // entry 0 and entries >= len
      for (int l = 1; l < J.len[i]; l++) out[l] = J.result_host[(size_t)i * J.L + l - 1];
    }
    if (probe_logprobs && NP)
      memcpy(probe_logprobs + (size_t)i * NP, J.result_host.data() + (size_t)J.n * J.L + (size_t)i * NP, NP * 4);
  }
}

int session_score(wb_session* s, const int32_t* tokens, int32_t row_stride, const int32_t* lens, int32_t mask_until_len,
                  const int32_t* probe_ids, int32_t n_probe, int32_t probe_pos, float* token_logprobs,
                  float* probe_logprobs) {
  wb_model* m = s->m;
  WB_REQUIRE((int)s->C.size() == s->W && s->W > 0 && s->ckv.p, WB_ERR_STATE, "wb_session_score: the session holds no encoded windows");
  ScoreJob J;
  WB_TRY(score_rows(m, tokens, s->W, row_stride, lens, mask_until_len, probe_ids, n_probe, probe_pos, &J));
  WB_REQUIRE(mask_until_len == 0 || s->has_mask, WB_ERR_STATE,
             "wb_session_score: mask_until_len %d needs wb_session_set_special_mask first", mask_until_len);
  wb::GpuTurn turn(s->device);
  WB_HIP(hipSetDevice(m->device));
  if (s->enc_guard_pending) {            // a deferred range check of the encode pass: settle it before its output is read
    WB_HIP(hipStreamSynchronize(s->st));
    bool reencoded = false;
    WB_TRY(session_enc_guard_resolve(s, &reencoded));
  }
  const int d = m->dims.n_text_state;
  J.C = s->C; J.kv_row0 = s->row0;
  J.ckv = s->ckv.as<float>(); J.ckv_layer_stride = (int64_t)s->enc_rows * 2 * d; J.ldkv = 2 * d;
  J.mask_dev = s->mask.as<float>();
  WB_TRY(run_score(m, s->st, s->ws, J));
  WB_HIP(hipStreamSynchronize(s->st));
  score_scatter(J, row_stride, token_logprobs, probe_logprobs);
  return WB_OK;
}

}  // namespace wb

using namespace wb;

extern "C" {

int wb_score_tokens(wb_model* m, const int32_t* tokens, int n, int L, const int32_t* lens, const float* enc, int C,
                    const uint8_t* is_special, int32_t mask_until_len, const int32_t* probe_ids, int32_t n_probe,
                    int32_t probe_pos, float* token_logprobs, float* probe_logprobs) {
  WB_REQUIRE(m && tokens && enc && token_logprobs && n > 0 && L > 0 && C > 0, WB_ERR_ARG, "wb_score_tokens: bad argument");
  WB_REQUIRE(mask_until_len <= 0 || is_special, WB_ERR_ARG, "wb_score_tokens: mask_until_len %d needs is_special", mask_until_len);
  WB_REQUIRE(n_probe <= 0 || probe_logprobs, WB_ERR_ARG, "wb_score_tokens: probes without probe_logprobs");
  ScoreJob J;
  WB_TRY(score_rows(m, tokens, n, L, lens, mask_until_len, probe_ids, n_probe, probe_pos, &J));
  wb::GpuTurn turn(m->device);
  std::lock_guard<std::mutex> lk(g_stateless_mu);
  WB_HIP(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  const int d = m->dims.n_text_state, V = m->dims.n_vocab;
  WB_TRY(m->io_b.ensure((size_t)n * C * d * 4));
  WB_HIP(hipMemcpyAsync(m->io_b.p, enc, (size_t)n * C * d * 4, hipMemcpyHostToDevice, st));
  std::vector<float> mk;
  if (mask_until_len > 0) {
    ScoreBufs& B = m->ws.score;
    // (the usual case, one tokenizer per process: the mask is on the device already -- as wb_session_set_special_mask)
    if (!B.mask.p || (int)B.mask_host.size() != V || memcmp(B.mask_host.data(), is_special, (size_t)V) != 0) {
      B.mask_host.clear();                                                  // void the key before the contents change
      mk.resize(V);
      for (int i = 0; i < V; i++) mk[i] = is_special[i] ? -INFINITY : 0.f;   // transcribe.rs:244
      WB_TRY(B.mask.ensure((size_t)V * 4));
      WB_HIP(hipMemcpyAsync(B.mask.p, mk.data(), (size_t)V * 4, hipMemcpyHostToDevice, st));
      WB_HIP(hipStreamSynchronize(st));
      B.mask_host.assign(is_special, is_special + V);
    }
    J.mask_dev = B.mask.as<float>();
  }
  J.C.assign(n, C); J.kv_row0.resize(n);
  for (int i = 0; i < n; i++) J.kv_row0[i] = i * C;
  J.enc_dev = m->io_b.as<float>(); J.enc_rows = n * C;
  // (guarded: the cross-K/V projection runs on the split-precision kernel, as in wb_forward_decoder)
  WB_TRY(split_guarded(m, st, m->split_flag_host, m->split_flag_dev, nullptr, [&]() { return run_score(m, st, m->ws, J); }));
  WB_HIP(hipStreamSynchronize(st));      // (a model on the exact-f32 kernels runs the pass unguarded: nothing waited yet)
  score_scatter(J, L, token_logprobs, probe_logprobs);
  return WB_OK;
}

int wb_session_score(wb_session* s, const int32_t* tokens, int32_t row_stride, const int32_t* lens,
                     int32_t mask_until_len, const int32_t* probe_ids, int32_t n_probe, int32_t probe_pos,
                     float* token_logprobs, float* probe_logprobs) {
  WB_REQUIRE(s && tokens && token_logprobs && row_stride > 0, WB_ERR_ARG, "wb_session_score: bad argument");
  WB_REQUIRE(n_probe <= 0 || probe_logprobs, WB_ERR_ARG, "wb_session_score: probes without probe_logprobs");
  return session_score(s, tokens, row_stride, lens, mask_until_len, probe_ids, n_probe, probe_pos, token_logprobs,
                       probe_logprobs);
}

int wb_waveform_detect_language(wb_model* m, const float* pcm, int64_t n, int sample_rate, int32_t padding,
                                int32_t tok_start_of_transcript, const int32_t* lang_ids, int32_t n_lang,
                                int32_t max_windows, float* win_probs, float* mean_probs, int32_t* best) {
  WB_REQUIRE(m && pcm && lang_ids && n_lang > 0 && max_windows >= 0, WB_ERR_ARG, "wb_waveform_detect_language: bad argument");
  const int V = m->dims.n_vocab;
  WB_REQUIRE(tok_start_of_transcript >= 0 && tok_start_of_transcript < V, WB_ERR_ARG, "start-of-transcript token out of range");
  for (int j = 0; j < n_lang; j++)
    WB_REQUIRE(lang_ids[j] >= 0 && lang_ids[j] < V, WB_ERR_ARG, "language id %d out of range [0,%d)", lang_ids[j], V);
  WB_REQUIRE(padding >= 0 && padding < m->max_mel_frames(), WB_ERR_ARG, "bad padding");
  wb::GpuTurn turn(m->device);
  wb_decode_params dp;
  wb_decode_params_default(&dp);
  const int64_t wlen = wb_max_waveform_samples(m->max_mel_frames() - padding);          // transcribe.rs:32-34
  const int64_t n_win = wb_window_extents(n, sample_rate, wlen, dp.overlap_seconds, nullptr, nullptr, 0);
  std::vector<int64_t> starts((size_t)n_win), lens((size_t)n_win);
  wb_window_extents(n, sample_rate, wlen, dp.overlap_seconds, starts.data(), lens.data(), n_win);
  const int W = (int)(max_windows > 0 ? std::min<int64_t>(max_windows, n_win) : n_win);
  WB_REQUIRE(W > 0, WB_ERR_ARG, "wb_waveform_detect_language: the waveform holds no window");
  std::vector<float> lp((size_t)W * n_lang);
  for (int b0 = 0; b0 < W; b0 += 64) {
    const int nb = std::min(64, W - b0);
    wb_session* s = nullptr;
    int rc = session_create(m, nb, 1, padding, &s);
    if (rc == WB_OK) {
      s->sample_rate = (double)sample_rate;
      rc = session_encode_pcm(s, pcm, n, starts.data() + b0, lens.data() + b0, false);
      const std::vector<int32_t> sot((size_t)nb, tok_start_of_transcript);
      // Whisper's detect_language: the distribution after [SOT] alone, no mask
      if (rc == WB_OK) rc = session_score(s, sot.data(), 1, nullptr, 0, lang_ids, n_lang, 0, nullptr, lp.data() + (size_t)b0 * n_lang);
      wb_session_free(s);
    }
    WB_TRY(rc);
  }
  std::vector<double> mean((size_t)n_lang, 0.0);
  for (int w = 0; w < W; w++) {          // softmax restricted to lang_ids, in f64 from the f32 log-probs
    const float* r = lp.data() + (size_t)w * n_lang;
    double mx = -INFINITY, sum = 0.0;
    for (int j = 0; j < n_lang; j++) mx = std::max(mx, (double)r[j]);
    for (int j = 0; j < n_lang; j++) sum += std::exp((double)r[j] - mx);
    for (int j = 0; j < n_lang; j++) {
      const double pj = std::exp((double)r[j] - mx) / sum;
      if (win_probs) win_probs[(size_t)w * n_lang + j] = (float)pj;
      mean[j] += pj / W;
    }
  }
  int arg = 0;
  for (int j = 1; j < n_lang; j++)
    if (mean[j] > mean[arg]) arg = j;    // (lowest index on a tie)
  if (mean_probs)
    for (int j = 0; j < n_lang; j++) mean_probs[j] = (float)mean[j];
  if (best) *best = arg;
  return WB_OK;
}

int wb_logprob_gather(int device, const float* h, int32_t R, int32_t d, const float* E, int32_t V, const float* mask,
                      const uint8_t* row_masked, const int32_t* target, const int32_t* probe_row, const int32_t* probe_id,
                      int32_t n_probe, int32_t v_splits, float* logprob, float* lse, float* probe_lp) {
  WB_REQUIRE(h && E && logprob && lse && R >= 1 && d >= 1 && V >= 1 && n_probe >= 0 && v_splits >= 0, WB_ERR_ARG,
             "wb_logprob_gather: bad argument");
  WB_REQUIRE(n_probe == 0 || (probe_row && probe_id && probe_lp), WB_ERR_ARG, "wb_logprob_gather: null probe argument");
  WB_REQUIRE((mask != nullptr) == (row_masked != nullptr), WB_ERR_ARG, "wb_logprob_gather: mask and row_masked go together");
  WB_REQUIRE(d % 32 == 0, WB_ERR_SHAPE, "wb_logprob_gather: d %d is not a multiple of 32", d);
  WB_REQUIRE((int64_t)R * d < ((int64_t)1 << 31) && (int64_t)V * d < ((int64_t)1 << 31), WB_ERR_SHAPE, "wb_logprob_gather: too large");
  for (int r = 0; target && r < R; r++)
    WB_REQUIRE(target[r] >= -1 && target[r] < V, WB_ERR_ARG, "wb_logprob_gather: target %d of row %d outside [-1,%d)", target[r], r, V);
  for (int p = 0; p < n_probe; p++)
    WB_REQUIRE(probe_row[p] >= 0 && probe_row[p] < R && probe_id[p] >= 0 && probe_id[p] < V, WB_ERR_ARG,
               "wb_logprob_gather: probe %d = (%d, %d) outside %d rows x %d ids", p, probe_row[p], probe_id[p], R, V);
  const int ldv = (V + 63) / 64 * 64, vs = score_splits(R, V, v_splits);
  // E^T with the pad columns poisoned: a kernel that lets them into a sum fails visibly
  std::vector<float> et((size_t)d * ldv, std::numeric_limits<float>::quiet_NaN());
  for (int v = 0; v < V; v++)
    for (int k = 0; k < d; k++) et[(size_t)k * ldv + v] = E[(size_t)v * d + k];
  wb::GpuTurn turn(device);
  WB_HIP(hipSetDevice(device));
  const size_t NP = (size_t)n_probe;
  DevMem dh, det, dmask, du8, di32, dpart, df32;
  WB_TRY(dh.alloc((size_t)R * d * 4));
  WB_TRY(det.alloc(et.size() * 4));
  WB_TRY(dmask.alloc((size_t)V * 4));
  WB_TRY(du8.alloc((size_t)R));
  WB_TRY(di32.alloc(((size_t)R + 2 * NP) * 4));
  // every buffer a kernel writes sits between two guard bands of GUARD poisoned words, checked after the run
  constexpr size_t GUARD = 64;
  const size_t part_words = (size_t)vs * R * 4, f32_words = (size_t)3 * R + 2 * NP;
  WB_TRY(dpart.alloc((part_words + 2 * GUARD) * 4));
  WB_TRY(df32.alloc((f32_words + 2 * GUARD) * 4));
  hipStream_t st = nullptr;
  WB_HIP(hipMemsetAsync(dpart.p, 0xFF, dpart.bytes, st));
  WB_HIP(hipMemsetAsync(df32.p, 0xFF, df32.bytes, st));
  WB_HIP(hipMemcpyAsync(dh.p, h, (size_t)R * d * 4, hipMemcpyHostToDevice, st));
  WB_HIP(hipMemcpyAsync(det.p, et.data(), et.size() * 4, hipMemcpyHostToDevice, st));
  if (mask) {
    WB_HIP(hipMemcpyAsync(dmask.p, mask, (size_t)V * 4, hipMemcpyHostToDevice, st));
    WB_HIP(hipMemcpyAsync(du8.p, row_masked, (size_t)R, hipMemcpyHostToDevice, st));
  }
  ScoreArgs a;
  a.h = dh.as<float>(); a.R = R; a.d = d; a.Et = det.as<float>(); a.ldv = ldv; a.V = V;
  a.mask = mask ? dmask.as<float>() : nullptr; a.row_masked = mask ? du8.as<uint8_t>() : nullptr;
  if (target) {
    WB_HIP(hipMemcpyAsync(di32.p, target, (size_t)R * 4, hipMemcpyHostToDevice, st));
    a.target = di32.as<int32_t>();
  }
  if (n_probe) {
    WB_HIP(hipMemcpyAsync(di32.as<int32_t>() + R, probe_row, NP * 4, hipMemcpyHostToDevice, st));
    WB_HIP(hipMemcpyAsync(di32.as<int32_t>() + R + NP, probe_id, NP * 4, hipMemcpyHostToDevice, st));
  }
  a.probe_row = di32.as<int32_t>() + R; a.probe_id = a.probe_row + NP; a.n_probe = n_probe;
  a.vs = vs;
  a.part = reinterpret_cast<float4*>(dpart.as<float>() + GUARD);
  a.target_logit = df32.as<float>() + GUARD; a.lse = a.target_logit + R; a.logprob = a.lse + R;
  a.probe_logit = a.logprob + R; a.probe_lp = a.probe_logit + NP;
  prof_tag(KC_SCORE_LOGITS, 0);
  WB_REQUIRE(launch_score_logits(st, a) == 0, WB_ERR_SHAPE, "wb_logprob_gather: unsupported shape");
  prof_tag(KC_SCORE_MERGE, 0);
  launch_score_merge(st, a);
  WB_HIP(hipGetLastError());
  WB_HIP(hipMemcpyAsync(logprob, a.logprob, (size_t)R * 4, hipMemcpyDeviceToHost, st));
  WB_HIP(hipMemcpyAsync(lse, a.lse, (size_t)R * 4, hipMemcpyDeviceToHost, st));
  if (n_probe) WB_HIP(hipMemcpyAsync(probe_lp, a.probe_lp, NP * 4, hipMemcpyDeviceToHost, st));
  uint32_t guards[4][GUARD];
  WB_HIP(hipMemcpyAsync(guards[0], dpart.p, GUARD * 4, hipMemcpyDeviceToHost, st));
  WB_HIP(hipMemcpyAsync(guards[1], dpart.as<float>() + GUARD + part_words, GUARD * 4, hipMemcpyDeviceToHost, st));
  WB_HIP(hipMemcpyAsync(guards[2], df32.p, GUARD * 4, hipMemcpyDeviceToHost, st));
  WB_HIP(hipMemcpyAsync(guards[3], df32.as<float>() + GUARD + f32_words, GUARD * 4, hipMemcpyDeviceToHost, st));
  WB_HIP(hipStreamSynchronize(st));
  for (int b = 0; b < 4; b++)
    for (size_t i = 0; i < GUARD; i++)
      WB_REQUIRE(guards[b][i] == 0xFFFFFFFFu, WB_ERR_STATE, "wb_logprob_gather: guard band %d overwritten at word %zu", b, i);
  return WB_OK;
}

}  // extern "C"
