//! Raw bindings of include/whisper_hip.h (plain pointers and sizes; nothing unwinds across the ABI).
//! Every function returns 0 or a negative `wb_status`; `wb_last_error()` holds the thread-local message.
//! tests/test_rust_shim.py checks names and argument counts of this block against the header.
#![allow(non_camel_case_types)]
use std::os::raw::{c_char, c_double, c_float, c_int, c_void};

#[repr(C)]
pub struct wb_model {
    _private: [u8; 0],
}
#[repr(C)]
pub struct wb_session {
    _private: [u8; 0],
}
#[repr(C)]
pub struct wb_comm {
    _private: [u8; 0],
}

#[repr(C)]
#[derive(Default, Clone, Copy, Debug, PartialEq, Eq)]
pub struct wb_dims {
    pub n_mels: i32,
    pub n_audio_ctx: i32,
    pub n_audio_state: i32,
    pub n_audio_head: i32,
    pub n_audio_layer: i32,
    pub n_vocab: i32,
    pub n_text_ctx: i32,
    pub n_text_state: i32,
    pub n_text_head: i32,
    pub n_text_layer: i32,
}

#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct wb_decode_params {
    pub beam_size: i32,
    pub max_depth: i32,
    pub padding: i32,
    pub overlap_seconds: i32,
    pub max_n_offsets: i32,
    pub min_n_overlaps: i32,
    pub mask_until_len: i32,
    pub max_batch_windows: i32,
    pub tok_start_of_transcript: i32,
    pub tok_language: i32,
    pub tok_transcribe: i32,
    pub tok_no_timestamps: i32,
    pub tok_end_of_text: i32,
}

#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct wb_sample_params {
    pub temperature: c_float,
    pub best_of: i32,
    pub seed: u64,
    pub attempt: i32,
}

#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct wb_fallback_params {
    pub temperatures: [c_float; 8],
    pub n_temperatures: i32,
    pub best_of: i32,
    pub logprob_threshold: c_float,
    pub no_speech_threshold: c_float,
    pub compression_ratio_threshold: c_float,
    pub seed: u64,
    pub tok_no_speech: i32,
}

#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct wb_timestamp_params {
    pub tok_timestamp_begin: i32,
    pub n_timestamps: i32,
    pub max_initial_timestamp_index: i32,
    pub max_timestamp_index: i32,
    pub seconds_per_timestamp: c_float,
    pub temperature: c_float,
    pub best_of: i32,
    pub seed: u64,
    pub attempt: i32,
}

#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct wb_beam_params {
    pub beam_size: i32,
    pub patience: c_float,
    pub length_penalty: c_float,
}

/// Fills the logits `[n][V]` of the live rows of one step of `wb_timestamp_beam_search_device` (a test hook).
pub type wb_tsbeam_logits_fn = Option<unsafe extern "C" fn(user: *mut c_void, step: i32, n: i32, window: *const i32,
                                                           beam: *const i32, token: *const i32, parent: *const i32,
                                                           logits: *mut c_float) -> c_int>;

/// Compression ratio of one window's generated tokens, computed on the caller's side (it owns the tokenizer).
pub type wb_ratio_fn = Option<unsafe extern "C" fn(user: *mut c_void, tokens: *const i32, n: i32) -> c_double>;

pub const WB_OK: c_int = 0;
pub const WB_ERR_ARG: c_int = -1;
pub const WB_ERR_SHAPE: c_int = -2;
pub const WB_ERR_IO: c_int = -3;
pub const WB_ERR_HIP: c_int = -4;
pub const WB_ERR_OOM: c_int = -5;
pub const WB_ERR_STATE: c_int = -6;
pub const WB_F32: c_int = 0;
pub const WB_BF16: c_int = 1; // retired: wb_model_load_* return an error
pub const WB_FRONTEND_FFT: c_int = 0;
pub const WB_FRONTEND_REFERENCE: c_int = 1;

extern "C" {
    pub fn wb_model_load_dump_dir(dir: *const c_char, device: c_int, compute_dtype: c_int, out: *mut *mut wb_model) -> c_int;
    pub fn wb_model_load_burn_record(mpk_gz_path: *const c_char, cfg_path: *const c_char, device: c_int,
                                     compute_dtype: c_int, out: *mut *mut wb_model) -> c_int;
    pub fn wb_model_dims(m: *const wb_model, out: *mut wb_dims) -> c_int;
    pub fn wb_model_free(m: *mut wb_model);
    pub fn wb_model_set_frame_limit(m: *mut wb_model, whisper_geometry: c_int) -> c_int;
    pub fn wb_model_set_frontend(m: *mut wb_model, frontend: c_int) -> c_int;
    pub fn wb_model_frontend(m: *const wb_model) -> c_int;
    pub fn wb_model_encoder_gemm(m: *const wb_model) -> c_int;
    pub fn wb_model_decoder_gemm(m: *const wb_model) -> c_int;
    pub fn wb_max_waveform_samples(n_frame_max: i64) -> i64;
    pub fn wb_prep_audio(device: c_int, pcm: *const c_float, n: i64, sample_rate: c_double, mel: *mut c_float,
                         n_frames: *mut i64) -> c_int;
    pub fn wb_prep_audio_frontend(device: c_int, pcm: *const c_float, n: i64, sample_rate: c_double, mel: *mut c_float,
                                  n_frames: *mut i64, frontend: c_int) -> c_int;
    // the number of mel rows chosen per call: 80, or 128 (large-v3 and later; K1 only)
    pub fn wb_prep_audio_mels(device: c_int, pcm: *const c_float, n: i64, sample_rate: c_double, n_mels: c_int,
                              mel: *mut c_float, n_frames: *mut i64) -> c_int;
    pub fn wb_waveform_to_mels_dev_mels(device: c_int, pcm_dev: *const c_float, n_samples: i64, sample_rate: c_double,
                                        starts: *const i64, lens: *const i64, n_windows: i32, clip_frames: i32,
                                        padding: i32, mel_dev: *mut c_float, win_stride: i64, row_stride: i32,
                                        frames_out: *mut i32, iters: i32, elapsed_ms: *mut c_double, n_mels: i32,
                                        frontend: i32) -> c_int;
    pub fn wb_mel_filterbank(sample_rate: c_double, n_mels: c_int, filters: *mut c_float) -> c_int;
    pub fn wb_mel_dft_table(table_402x400: *mut c_float) -> c_int;
    pub fn wb_forward_encoder(m: *mut wb_model, mel: *const c_float, b: c_int, t: c_int, out: *mut c_float) -> c_int;
    pub fn wb_forward_decoder(m: *mut wb_model, tokens: *const i32, n: c_int, l: c_int, enc: *const c_float, c: c_int,
                              logits: *mut c_float) -> c_int;
    pub fn wb_forward(m: *mut wb_model, mel: *const c_float, b: c_int, t: c_int, tokens: *const i32, l: c_int,
                      logits: *mut c_float) -> c_int;
    pub fn wb_decode_params_default(p: *mut wb_decode_params);
    pub fn wb_window_extents(n_samples: i64, sample_rate: c_int, window_len: i64, overlap_seconds: c_int,
                             starts: *mut i64, lens: *mut i64, cap: i64) -> i64;
    pub fn wb_waveform_to_tokens(m: *mut wb_model, pcm: *const c_float, n: i64, sample_rate: c_int,
                                 p: *const wb_decode_params, is_special: *const u8, win_begin: c_int, win_end: c_int,
                                 win_tokens: *mut i32, row_stride: i32, win_lens: *mut i32, stitched: *mut i32,
                                 stitched_cap: i64, n_stitched: *mut i64) -> c_int;
    // token timestamps: cross-attention alignment + DTW on the device (no counterpart in the reference)
    pub fn wb_align_tokens(m: *mut wb_model, tokens: *const i32, n: c_int, L: c_int, lens: *const i32, enc: *const c_float,
                           C: c_int, heads: *const i32, n_heads: i32, n_prefix: i32, drop_last: i32, filter_width: i32,
                           start_pos: *mut i32, matrix: *mut c_float) -> c_int;
    pub fn wb_session_align(s: *mut wb_session, tokens: *const i32, row_stride: i32, lens: *const i32, heads: *const i32,
                            n_heads: i32, n_prefix: i32, drop_last: i32, filter_width: i32, start_pos: *mut i32,
                            matrix: *mut c_float) -> c_int;
    pub fn wb_dtw_start_positions(device: c_int, x: *const c_float, N: i32, C: i32, start_pos: *mut i32) -> c_int;
    pub fn wb_waveform_to_token_times(m: *mut wb_model, pcm: *const c_float, n: i64, sample_rate: c_int,
                                      p: *const wb_decode_params, is_special: *const u8, win_begin: c_int, win_end: c_int,
                                      win_tokens: *mut i32, row_stride: i32, win_lens: *mut i32, stitched: *mut i32,
                                      stitched_cap: i64, n_stitched: *mut i64, heads: *const i32, n_heads: i32,
                                      filter_width: i32, win_times: *mut c_float, stitched_times: *mut c_float) -> c_int;
    pub fn wb_stitch_windows_times(win_tokens: *const i32, row_stride: i32, win_lens: *const i32, n_windows: c_int,
                                   max_n_offsets: c_int, min_n_overlaps: c_int, out: *mut i32, cap: i64, n_out: *mut i64,
                                   win_times: *const c_float, out_times: *mut c_float) -> c_int;
    // token log-probabilities, no-speech probability, language detection: a teacher-forced pass ended by a fused
    // log-softmax product that never forms the logits (no counterpart in the reference)
    pub fn wb_score_tokens(m: *mut wb_model, tokens: *const i32, n: c_int, L: c_int, lens: *const i32, enc: *const c_float,
                           C: c_int, is_special: *const u8, mask_until_len: i32, probe_ids: *const i32, n_probe: i32,
                           probe_pos: i32, token_logprobs: *mut c_float, probe_logprobs: *mut c_float) -> c_int;
    pub fn wb_session_score(s: *mut wb_session, tokens: *const i32, row_stride: i32, lens: *const i32, mask_until_len: i32,
                            probe_ids: *const i32, n_probe: i32, probe_pos: i32, token_logprobs: *mut c_float,
                            probe_logprobs: *mut c_float) -> c_int;
    pub fn wb_waveform_detect_language(m: *mut wb_model, pcm: *const c_float, n: i64, sample_rate: c_int, padding: i32,
                                       tok_start_of_transcript: i32, lang_ids: *const i32, n_lang: i32, max_windows: i32,
                                       win_probs: *mut c_float, mean_probs: *mut c_float, best: *mut i32) -> c_int;
    pub fn wb_waveform_to_token_scores(m: *mut wb_model, pcm: *const c_float, n: i64, sample_rate: c_int,
                                       p: *const wb_decode_params, is_special: *const u8, win_begin: c_int, win_end: c_int,
                                       win_tokens: *mut i32, row_stride: i32, win_lens: *mut i32, stitched: *mut i32,
                                       stitched_cap: i64, n_stitched: *mut i64, tok_no_speech: i32,
                                       win_logprobs: *mut c_float, stitched_logprobs: *mut c_float,
                                       win_avg_logprob: *mut c_float, win_no_speech_prob: *mut c_float) -> c_int;
    pub fn wb_logprob_gather(device: c_int, h: *const c_float, R: i32, d: i32, E: *const c_float, V: i32,
                             mask: *const c_float, row_masked: *const u8, target: *const i32, probe_row: *const i32,
                             probe_id: *const i32, n_probe: i32, v_splits: i32, logprob: *mut c_float, lse: *mut c_float,
                             probe_lp: *mut c_float) -> c_int;
    pub fn wb_session_rewind(s: *mut wb_session) -> c_int;
    pub fn wb_session_graph_count(s: *const wb_session) -> c_int;
    pub fn wb_session_graph_captures(s: *const wb_session) -> i64;
    pub fn wb_persist_resident_geometry(n_state: i32, n_rows: i32, max_keys: i32, out5: *mut i32) -> c_int;
    pub fn wb_persist_role_plan(n_layer: i32, n_head: i32, n_state: i32, n_rows: i32, n_vocab: i32, grid: i32, legacy: i32,
                                out_kinds: *mut i32, out_block: *mut i32, cap: i32) -> c_int;
    pub fn wb_session_last_samples(s: *mut wb_session, tokens: *mut i32, row_stride: i32, lens: *mut i32) -> c_int;
    pub fn wb_sample_rows(device: c_int, logits: *const c_float, R: i32, ld: i32, V: i32, mask: *const c_float,
                          row_masked: *const u8, row_stats: *const c_float, temperature: c_float, seed: u64, attempt: i32,
                          stream: *const i32, position: *const i32, eot: i32, out_token: *mut i32,
                          out_logprob: *mut c_float, out_err: *mut i32) -> c_int;
    // timestamp-token decoding: Whisper's timestamp rules on the device, segments (no counterpart in the reference)
    pub fn wb_session_set_suppress(s: *mut wb_session, suppress: *const u8, suppress_first: *const u8) -> c_int;
    pub fn wb_timestamp_rows(device: c_int, logits: *const c_float, R: i32, ld: i32, V: i32, suppress: *const u8,
                             suppress_first: *const u8, tok_timestamp_begin: i32, n_timestamps: i32,
                             max_initial_timestamp_index: i32, max_timestamp_index: i32, temperature: c_float, seed: u64,
                             attempt: i32, n_gen: *const i32, prev1: *const i32, prev2: *const i32, last_ts: *const i32,
                             stream: *const i32, position: *const i32, eot: i32, out_token: *mut i32,
                             out_logprob: *mut c_float, out_forced: *mut i32, out_stats: *mut c_float,
                             out_err: *mut i32) -> c_int;
    pub fn wb_segments_from_tokens(tokens: *const i32, n: i32, tok_timestamp_begin: i32, n_timestamps: i32,
                                   tok_end_of_text: i32, window_index: i32, seconds_per_timestamp: c_float,
                                   seg_begin: *mut i32, seg_end: *mut i32, seg_start: *mut c_float,
                                   seg_end_time: *mut c_float, cap: i32, n_segments: *mut i32,
                                   advance_index: *mut i32) -> c_int;
    // beam search under the timestamp rules: results of the last call, the rows kernel's test hook
    pub fn wb_session_last_beams(s: *mut wb_session, cap: i32, tokens: *mut i32, row_stride: i32, lens: *mut i32,
                                 scores: *mut c_double, ranks: *mut c_double, n: *mut i32) -> c_int;
    pub fn wb_session_last_beam_trace(s: *mut wb_session, max_steps: i32, n_steps: *mut i32, n_live: *mut i32,
                                      n_finished: *mut i32, tokens: *mut i32, parents: *mut i32,
                                      scores: *mut c_double) -> c_int;
    pub fn wb_timestamp_beam_rows(device: c_int, logits: *const c_float, R: i32, ld: i32, V: i32, suppress: *const u8,
                                  suppress_first: *const u8, tok_timestamp_begin: i32, n_timestamps: i32,
                                  max_initial_timestamp_index: i32, max_timestamp_index: i32, n_gen: *const i32,
                                  prev1: *const i32, prev2: *const i32, last_ts: *const i32, eot: i32, k: i32,
                                  out_ids: *mut i32, out_logprobs: *mut c_float, out_count: *mut i32,
                                  out_forced: *mut i32, out_stats: *mut c_float, out_err: *mut i32) -> c_int;
    pub fn wb_session_begin(m: *mut wb_model, pcm: *const c_float, n_pcm: i64, starts: *const i64, lens: *const i64,
                            n_windows: c_int, max_beams: c_int, padding: c_int, out: *mut *mut wb_session) -> c_int;
    pub fn wb_session_set_special_mask(s: *mut wb_session, is_special: *const u8) -> c_int;
    pub fn wb_session_step(s: *mut wb_session, new_tokens: *const i32, parent: *const i32, window: *const i32, n: c_int,
                           apply_special_mask: c_int, k: c_int, top_ids: *mut i32, top_logprobs: *mut c_float) -> c_int;
    pub fn wb_session_decode(s: *mut wb_session, p: *const wb_decode_params, out_tokens: *mut i32, row_stride: i32,
                             out_lens: *mut i32) -> c_int;
    pub fn wb_session_free(s: *mut wb_session);
    pub fn wb_wav_read_f32(path: *const c_char, out: *mut c_float, capacity: i64, n_samples: *mut i64) -> c_int;
    pub fn wb_wav_read_f32_any_rate(path: *const c_char, out: *mut c_float, capacity: i64, n_samples: *mut i64) -> c_int;
    pub fn wb_resample_len(n_in: i64, rate_in: i32, rate_out: i32) -> i64;
    pub fn wb_resample_dev(device: c_int, src_dev: *const c_float, n_in: i64, rate_in: i32, rate_out: i32,
                           dst_dev: *mut c_float, capacity: i64, n_out: *mut i64) -> c_int;
    pub fn wb_comm_unique_id(id128: *mut u8) -> c_int;
    pub fn wb_comm_init(id128: *const u8, rank: c_int, world: c_int, device: c_int, out: *mut *mut wb_comm) -> c_int;
    pub fn wb_comm_free(c: *mut wb_comm);
    pub fn wb_comm_allgather(comm: *mut c_void, send: *const c_void, recv: *mut c_void, bytes_per_rank: i64) -> c_int;
    pub fn wb_shard_partition(n_windows: i64, rank: c_int, world: c_int, lo: *mut i64, hi: *mut i64) -> c_int;
    pub fn wb_waveform_to_tokens_sharded(m: *mut wb_model, pcm: *const c_float, pcm_on_device: c_int, n: i64,
                                         sample_rate: c_int, p: *const wb_decode_params, is_special: *const u8,
                                         rank: c_int, world: c_int, allgather: wb_allgather_fn, user: *mut c_void,
                                         win_tokens: *mut i32, row_stride: i32, win_lens: *mut i32, win_cap: i64,
                                         stitched: *mut i32, stitched_cap: i64, n_stitched: *mut i64) -> c_int;
    pub fn wb_last_error() -> *const c_char;
    pub fn wb_version() -> *const c_char;
}

// Temperature sampling, the decode fallback and timestamp decoding: the entry points whose arguments are the parameter structs / the callback
// type defined above (their own block: tests/test_rust_shim.py type-checks the first block against the header's scalars).
extern "C" {
    pub fn wb_sample_params_default(p: *mut wb_sample_params);
    pub fn wb_session_decode_sample(s: *mut wb_session, p: *const wb_decode_params, sp: *const wb_sample_params,
                                    prompt: *const i32, prompt_len: i32, active: *const u8, stream_ids: *const i32,
                                    out_tokens: *mut i32, row_stride: i32, out_lens: *mut i32,
                                    out_sum_logprob: *mut c_double, out_best: *mut i32) -> c_int;
    pub fn wb_timestamp_params_default(p: *mut wb_timestamp_params);
    pub fn wb_session_decode_timestamps(s: *mut wb_session, p: *const wb_decode_params, tp: *const wb_timestamp_params,
                                        prompt: *const i32, prompt_len: i32, active: *const u8, stream_ids: *const i32,
                                        out_tokens: *mut i32, row_stride: i32, out_lens: *mut i32,
                                        out_sum_logprob: *mut c_double, out_best: *mut i32) -> c_int;
    pub fn wb_waveform_to_segments(m: *mut wb_model, pcm: *const c_float, n: i64, sample_rate: c_int,
                                   p: *const wb_decode_params, tp: *const wb_timestamp_params, suppress: *const u8,
                                   suppress_first: *const u8, prompt: *const i32, prompt_len: i32,
                                   seg_start: *mut c_float, seg_end_time: *mut c_float, seg_tok_begin: *mut i32,
                                   seg_tok_end: *mut i32, seg_cap: i32, n_segments: *mut i32, text_tokens: *mut i32,
                                   text_cap: i64, n_text_tokens: *mut i64, n_windows: *mut i32) -> c_int;
    pub fn wb_beam_params_default(p: *mut wb_beam_params);
    pub fn wb_session_decode_timestamps_beam(s: *mut wb_session, p: *const wb_decode_params, tp: *const wb_timestamp_params,
                                             bp: *const wb_beam_params, prompt: *const i32, prompt_len: i32,
                                             active: *const u8, out_tokens: *mut i32, row_stride: i32, out_lens: *mut i32,
                                             out_score: *mut c_double, out_n_candidates: *mut i32) -> c_int;
    pub fn wb_timestamp_beam_search_device(device: c_int, tp: *const wb_timestamp_params, bp: *const wb_beam_params,
                                           n_windows: i32, V: i32, suppress: *const u8, suppress_first: *const u8, eot: i32,
                                           max_depth: i32, fill: wb_tsbeam_logits_fn, user: *mut c_void,
                                           cand_tokens: *mut i32, row_stride: i32, cand_lens: *mut i32,
                                           cand_scores: *mut c_double, cand_ranks: *mut c_double, n_cand: *mut i32,
                                           best: *mut i32, n_steps: *mut i32, n_live: *mut i32, n_finished: *mut i32,
                                           tr_tokens: *mut i32, tr_parents: *mut i32, tr_scores: *mut c_double) -> c_int;
    pub fn wb_waveform_to_segments_beam(m: *mut wb_model, pcm: *const c_float, n: i64, sample_rate: c_int,
                                        p: *const wb_decode_params, tp: *const wb_timestamp_params,
                                        bp: *const wb_beam_params, suppress: *const u8, suppress_first: *const u8,
                                        prompt: *const i32, prompt_len: i32, seg_start: *mut c_float,
                                        seg_end_time: *mut c_float, seg_tok_begin: *mut i32, seg_tok_end: *mut i32,
                                        seg_cap: i32, n_segments: *mut i32, text_tokens: *mut i32, text_cap: i64,
                                        n_text_tokens: *mut i64, n_windows: *mut i32) -> c_int;
    pub fn wb_session_set_prefill(s: *mut wb_session, mode: c_int) -> c_int;
    pub fn wb_session_prefill(s: *mut wb_session, tokens: *const i32, n: i32, active: *const u8) -> c_int;
    pub fn wb_prefill_store(device: c_int, qkv: *const c_float, nA: i32, n: i32, d: i32, ld: i32, S: i32, Lmax: i32,
                            Kc: *mut c_float, Vc: *mut c_float, tabs: *mut i32) -> c_int;
    pub fn wb_session_self_kv(s: *mut wb_session, layer: i32, slot: i32, n_pos: i32, K: *mut c_float,
                              V: *mut c_float) -> c_int;
    pub fn wb_waveform_to_segments_conditioned(m: *mut wb_model, pcm: *const c_float, n: i64, sample_rate: c_int,
                                               p: *const wb_decode_params, tp: *const wb_timestamp_params,
                                               bp: *const wb_beam_params, suppress: *const u8, suppress_first: *const u8,
                                               prompt: *const i32, prompt_len: i32, tok_start_of_prev: i32,
                                               condition_on_previous_text: i32, max_prompt_tokens: i32,
                                               initial_prompt: *const i32, n_initial_prompt: i32, seg_start: *mut c_float,
                                               seg_end_time: *mut c_float, seg_tok_begin: *mut i32, seg_tok_end: *mut i32,
                                               seg_cap: i32, n_segments: *mut i32, text_tokens: *mut i32, text_cap: i64,
                                               n_text_tokens: *mut i64, n_windows: *mut i32, win_seek: *mut i64,
                                               win_prompt_len: *mut i32, win_cap: i32) -> c_int;
    pub fn wb_fallback_params_default(p: *mut wb_fallback_params);
    pub fn wb_fallback_decide(fp: *const wb_fallback_params, avg_logprob: c_float, no_speech_prob: c_float,
                              ratio: c_float) -> c_int;
    pub fn wb_waveform_to_tokens_fallback(m: *mut wb_model, pcm: *const c_float, n: i64, sample_rate: c_int,
                                          p: *const wb_decode_params, is_special: *const u8, win_begin: c_int,
                                          win_end: c_int, win_tokens: *mut i32, row_stride: i32, win_lens: *mut i32,
                                          stitched: *mut i32, stitched_cap: i64, n_stitched: *mut i64,
                                          fp: *const wb_fallback_params, ratio: wb_ratio_fn, user: *mut c_void,
                                          win_temperature: *mut c_float, win_status: *mut i32,
                                          win_avg_logprob: *mut c_float, win_no_speech_prob: *mut c_float,
                                          win_ratio: *mut c_float, win_attempts: *mut i32) -> c_int;
}

/// The exchange of the sharded path: `send` = this rank's bytes, `recv` = world x bytes_per_rank bytes in rank order.
pub type wb_allgather_fn = Option<unsafe extern "C" fn(user: *mut c_void, send: *const c_void, recv: *mut c_void,
                                                       bytes_per_rank: i64) -> c_int>;

/// `wb_comm_allgather` under the callback's exact type (same symbol, `comm` as the user pointer).
pub unsafe extern "C" fn wb_comm_allgather_thunk(user: *mut c_void, send: *const c_void, recv: *mut c_void,
                                                  bytes_per_rank: i64) -> c_int {
    wb_comm_allgather(user, send, recv, bytes_per_rank)
}

/// Opaque user pointer type of callbacks (kept for completeness of the C vocabulary).
pub type wb_user = *mut c_void;
