// Whisper's decode fallback over the windows of a waveform: the accept / retry / no-speech decision (host only) and the
// driver that decodes a window batch, scores it on the same session and decodes the failing windows again by sampling at the
// next temperature -- after a rewind, over the cached cross K/V, without a re-encode.
#include <cmath>
#include <cstring>
#include <limits>

#include "engine.h"
#include "session.h"

using namespace wb;

extern "C" {

void wb_fallback_params_default(wb_fallback_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  const float t[6] = {0.f, 0.2f, 0.4f, 0.6f, 0.8f, 1.0f};
  for (int i = 0; i < 6; i++) p->temperatures[i] = t[i];
  p->n_temperatures = 6;
  p->best_of = 5;
  p->logprob_threshold = -1.0f;
  p->no_speech_threshold = 0.6f;
  p->compression_ratio_threshold = 2.4f;
  p->seed = 0;
  p->tok_no_speech = -1;
}

// decode_with_fallback: a window fails when its text is too repetitive or too unlikely -- unless it is silence -- and an
// accepted window is skipped (transcribe) when it is silence and not likely enough to be kept.  A NaN input to an enabled
// rule fails the window: it is decoded again rather than accepted or dropped on a number that does not exist.
int wb_fallback_decide(const wb_fallback_params* fp, float avg_logprob, float no_speech_prob, float ratio) {
  if (!fp) return WB_FALLBACK_ACCEPT;
  const bool lp_on = fp->logprob_threshold == fp->logprob_threshold;
  const bool cr_on = fp->compression_ratio_threshold == fp->compression_ratio_threshold;
  const bool ns_on = fp->tok_no_speech >= 0 && fp->no_speech_threshold == fp->no_speech_threshold;
  const bool silent = ns_on && no_speech_prob > fp->no_speech_threshold;
  bool retry = false;
  if (cr_on && !(ratio <= fp->compression_ratio_threshold)) retry = true;
  if (lp_on && !(avg_logprob >= fp->logprob_threshold)) retry = true;
  if (ns_on && no_speech_prob != no_speech_prob) retry = true;
  if (silent) retry = false;
  if (retry) return WB_FALLBACK_RETRY;
  if (silent && (!lp_on || !(avg_logprob > fp->logprob_threshold))) return WB_FALLBACK_NO_SPEECH;
  return WB_FALLBACK_ACCEPT;
}

int wb_waveform_to_tokens_fallback(wb_model* m, const float* pcm, int64_t n, int sample_rate, const wb_decode_params* p,
                                   const uint8_t* is_special, int win_begin, int win_end, int32_t* win_tokens,
                                   int32_t row_stride, int32_t* win_lens, int32_t* stitched, int64_t stitched_cap,
                                   int64_t* n_stitched, const wb_fallback_params* fp_in, wb_ratio_fn ratio, void* user,
                                   float* win_temperature, int32_t* win_status, float* win_avg_logprob,
                                   float* win_no_speech_prob, float* win_ratio, int32_t* win_attempts) {
  WB_REQUIRE(m && pcm && p && is_special && win_tokens && win_lens && fp_in, WB_ERR_ARG, "wb_waveform_to_tokens_fallback: null argument");
  WB_REQUIRE(win_temperature && win_status && win_avg_logprob && win_no_speech_prob && win_ratio && win_attempts, WB_ERR_ARG,
             "wb_waveform_to_tokens_fallback: null per-window output");
  WB_REQUIRE(!stitched || n_stitched, WB_ERR_ARG, "n_stitched is null");
  wb_fallback_params fp = *fp_in;
  const float nan = std::numeric_limits<float>::quiet_NaN();
  if (!ratio) fp.compression_ratio_threshold = nan;       // nobody to compute it: the rule is off
  const int nT = fp.n_temperatures;
  WB_REQUIRE(nT >= 1 && nT <= WB_FALLBACK_MAX_TEMPERATURES, WB_ERR_ARG, "fallback: %d temperatures (1 .. %d)", nT,
             (int)WB_FALLBACK_MAX_TEMPERATURES);
  WB_REQUIRE(fp.temperatures[0] == 0.f, WB_ERR_ARG, "fallback: the first temperature must be 0 (the ordinary decode)");
  for (int i = 1; i < nT; i++)
    WB_REQUIRE(fp.temperatures[i] > 0.f && std::isfinite(fp.temperatures[i]) && std::isfinite(1.0f / fp.temperatures[i]), WB_ERR_ARG, "fallback: temperature %d = %g", i,
               (double)fp.temperatures[i]);
  WB_REQUIRE(fp.best_of >= 1 && fp.best_of <= MAX_BEAMS, WB_ERR_ARG, "fallback: best_of %d outside [1, %d]", fp.best_of, MAX_BEAMS);
  WB_REQUIRE(fp.tok_no_speech < m->dims.n_vocab, WB_ERR_ARG, "fallback: no-speech token %d out of range", fp.tok_no_speech);
  WB_REQUIRE(p->beam_size >= 1 && p->beam_size <= MAX_BEAMS, WB_ERR_ARG, "beam_size %d outside [1, %d]", p->beam_size, MAX_BEAMS);
  WB_REQUIRE(p->padding >= 0 && p->padding < m->max_mel_frames(), WB_ERR_ARG, "bad padding");
  WB_REQUIRE(row_stride >= 4 + p->max_depth, WB_ERR_ARG, "row_stride %d < %d", row_stride, 4 + p->max_depth);
  wb::GpuTurn turn(m->device);
  const bool lp_on = fp.logprob_threshold == fp.logprob_threshold;
  const bool cr_on = fp.compression_ratio_threshold == fp.compression_ratio_threshold;
  const bool ns_on = fp.tok_no_speech >= 0 && fp.no_speech_threshold == fp.no_speech_threshold;
  // no rule can ask for a retry: the session is the one wb_waveform_to_tokens creates (same kernels, same rows)
  const bool can_retry = nT > 1 && (lp_on || cr_on || ns_on);
  const int max_beams = can_retry ? std::max(p->beam_size, fp.best_of) : p->beam_size;
  const int64_t wlen = wb_max_waveform_samples(m->max_mel_frames() - p->padding);          // transcribe.rs:32-34
  const int64_t n_win = wb_window_extents(n, sample_rate, wlen, p->overlap_seconds, nullptr, nullptr, 0);
  std::vector<int64_t> starts((size_t)n_win), lens((size_t)n_win);
  wb_window_extents(n, sample_rate, wlen, p->overlap_seconds, starts.data(), lens.data(), n_win);
  if (win_end < 0 || win_end > n_win) win_end = (int)n_win;
  win_begin = std::max(0, std::min(win_begin, win_end));
  const int n_local = win_end - win_begin;
  const int batch = p->max_batch_windows > 0 ? p->max_batch_windows : 64;
  const int32_t prompt[4] = {p->tok_start_of_transcript, p->tok_language, p->tok_transcribe, p->tok_no_timestamps};
  std::vector<float> lp((size_t)std::min(batch, std::max(n_local, 1)) * row_stride);

  auto run_batch = [&](int b0, int nb, wb_session* s) -> int {
    s->sample_rate = (double)sample_rate;
    int32_t* rows = win_tokens + (size_t)b0 * row_stride;
    WB_TRY(session_encode_pcm(s, pcm, n, starts.data() + win_begin + b0, lens.data() + win_begin + b0, false, true));
    WB_TRY(wb_session_set_special_mask(s, is_special));
    WB_TRY(session_reserve(s, 4 + p->max_depth + 1));
    for (int pass = 0; pass < 2; pass++) {         // attempt 0: the ordinary decode, as wb_waveform_to_tokens runs it
      const int rc = wb_session_decode(s, p, rows, row_stride, win_lens + b0);
      bool reencoded = false;
      WB_TRY(session_enc_guard_resolve(s, &reencoded));
      if (!reencoded) { WB_TRY(rc); break; }
      session_rewind(s);                           // (whatever the decode made of the non-finite encoder output is void)
      WB_REQUIRE(pass == 0, WB_ERR_STATE, "fallback: the encoder's range guard tripped twice");
    }
    std::vector<uint8_t> act((size_t)nb, 1);
    std::vector<int32_t> streams((size_t)nb);
    std::vector<float> probe((size_t)nb);
    for (int w = 0; w < nb; w++) streams[w] = (int32_t)((uint32_t)(win_begin + b0 + w) * (uint32_t)fp.best_of);
    for (int i = 0; i < nT; i++) {
      if (i > 0) {
        session_rewind(s);
        wb_sample_params sp;
        sp.temperature = fp.temperatures[i]; sp.best_of = fp.best_of; sp.seed = fp.seed; sp.attempt = i;
        WB_TRY(wb_session_decode_sample(s, p, &sp, prompt, 4, act.data(), streams.data(), rows, row_stride, win_lens + b0, nullptr,
                                        nullptr));
      }
      // the scoring pass over the rows as they stand; the no-speech probability is a property of the window: computed once
      const int32_t np = (i == 0 && fp.tok_no_speech >= 0) ? 1 : 0;
      WB_TRY(session_score(s, rows, row_stride, win_lens + b0, p->mask_until_len, &fp.tok_no_speech, np, 0, lp.data(), probe.data()));
      bool any = false;
      for (int w = 0; w < nb; w++) {
        const int g = b0 + w;
        if (i == 0) win_no_speech_prob[g] = np ? std::exp(probe[w]) : nan;
        if (!act[w]) continue;
        const int len = win_lens[g];
        const int32_t* row = rows + (size_t)w * row_stride;
        double sum = 0.0;                          // Whisper's avg_logprob: the generated tokens, a final end-of-text included
        for (int l = 4; l < len; l++) sum += lp[(size_t)w * row_stride + l];
        win_avg_logprob[g] = len > 4 ? (float)(sum / (len - 4)) : nan;
        const int n_text = std::max(0, len - 4 - ((len > 4 && row[len - 1] == p->tok_end_of_text) ? 1 : 0));
        win_ratio[g] = ratio ? (float)ratio(user, row + 4, n_text) : nan;
        win_temperature[g] = fp.temperatures[i];
        win_attempts[g] = i + 1;
        win_status[g] = wb_fallback_decide(&fp, win_avg_logprob[g], win_no_speech_prob[g], win_ratio[g]);
        act[w] = win_status[g] == WB_FALLBACK_RETRY ? 1 : 0;
        any = any || act[w];
      }
      if (!any) break;
    }
    return WB_OK;
  };
  for (int b0 = 0; b0 < n_local; b0 += batch) {
    const int nb = std::min(batch, n_local - b0);
    wb_session* s = nullptr;
    WB_TRY(session_create(m, nb, max_beams, p->padding, &s));
    const int rc = run_batch(b0, nb, s);
    wb_session_free(s);
    WB_TRY(rc);
  }
  if (stitched) {
    // windows without speech are left out of the fold; the others are stitched in order
    int kept = 0;
    for (int w = 0; w < n_local; w++) kept += win_status[w] != WB_FALLBACK_NO_SPEECH;
    if (kept == n_local) {
      WB_TRY(wb_stitch_windows(win_tokens, row_stride, win_lens, n_local, p->max_n_offsets, p->min_n_overlaps, stitched, stitched_cap,
                               n_stitched));
    } else {
      std::vector<int32_t> kt((size_t)std::max(kept, 1) * row_stride), kl((size_t)std::max(kept, 1));
      int q = 0;
      for (int w = 0; w < n_local; w++) {
        if (win_status[w] == WB_FALLBACK_NO_SPEECH) continue;
        memcpy(kt.data() + (size_t)q * row_stride, win_tokens + (size_t)w * row_stride, (size_t)row_stride * 4);
        kl[q++] = win_lens[w];
      }
      WB_TRY(wb_stitch_windows(kt.data(), row_stride, kl.data(), kept, p->max_n_offsets, p->min_n_overlaps, stitched, stitched_cap,
                               n_stitched));
    }
  }
  return WB_OK;
}

}  // extern "C"
