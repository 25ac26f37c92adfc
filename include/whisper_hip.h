/* whisper_hip.h -- C ABI of libwhisper_hip.so, the MI355X (gfx950) drop-in for the
 * tensor seams of Gadersd/whisper-burn.
 *
 * The reference has no FFI: its only seam is the `B: Backend` type parameter.  The
 * boundary is therefore cut at the three tensor call sites of src/transcribe.rs
 * (prep_audio :134, Whisper::forward_encoder :222, Whisper::forward_decoder :270) plus
 * the public Whisper::forward / waveform_to_text, and a Rust `extern "C"` shim keeps
 * the reference's signatures on top of these entry points.
 *
 * Conventions
 *  - every function returns WB_OK (0) or a negative wb_status; nothing aborts or
 *    throws across the boundary (the reference's assert!/panic sites are mapped to
 *    WB_ERR_SHAPE); wb_last_error() gives a thread-local message.
 *  - the caller owns every host buffer it passes; the library owns device memory
 *    behind opaque handles.  All pointers below are HOST pointers unless the
 *    parameter name ends in `_dev`.
 *  - all floating point data is IEEE f32 (the reference runs TchBackend<f32>,
 *    src/bin/transcribe/main.rs:80); token ids are int32.
 *  - a wb_model may be shared by threads: its weights never change after load.  The one
 *    piece of state it carries is the arithmetic switches (wb_model_encoder_gemm /
 *    wb_model_decoder_gemm), which can go from 1 to 0 once, atomically, when a range guard of
 *    the split-precision kernels trips (the guard words themselves are per session).  A
 *    wb_session is not thread-safe.
 *  - calls from different threads are safe and give the single-threaded results, but they TAKE
 *    TURNS on the GPU: every entry point that enqueues kernels holds its device's turn (one per
 *    GPU and process) from its first launch to its last synchronisation.  (On gfx950 a wave's packed-FP32
 *    instructions return wrong results while another kernel's f16 MFMAs run on the same
 *    SIMD: kernels of two calls must not share the device.  DESIGN.md section 9,
 *    tools/pk_mfma_probe.cpp.)  One process per GPU is the scaling model.
 */
#ifndef WHISPER_HIP_H
#define WHISPER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum wb_status {
  WB_OK = 0,
  WB_ERR_ARG = -1,     /* null pointer / bad enum / bad handle                     */
  WB_ERR_SHAPE = -2,   /* a shape contract the reference assert!s on was violated  */
  WB_ERR_IO = -3,      /* dump-dir / npy read error (load.rs:29-45 Box<dyn Error>) */
  WB_ERR_HIP = -4,     /* HIP runtime error (message carries hipGetErrorString)    */
  WB_ERR_OOM = -5,
  WB_ERR_STATE = -6    /* call sequence error on a session                         */
} wb_status;

/* compute_dtype for wb_model_load_*: the arithmetic the GEMMs run in. */
enum { WB_F32 = 0,     /* f32 results: exact-f32 MFMA, and the split-precision fp16 MFMA kernel (three products per pair,
                          f32 accumulate: f32-grade) for the encoder side -- see wb_model_encoder_gemm */
       WB_BF16 = 1 };  /* RETIRED in round 4 (wb_model_load_* return WB_ERR_ARG): plain bf16 inputs cannot hold the
                          path's 1e-3 logit tolerance; the 16-bit matrix path is the split-precision kernel above */

typedef struct wb_model wb_model;     /* Whisper<B>            src/model/mod.rs:41-45   */
typedef struct wb_session wb_session; /* per window-batch decode state (new: the
                                         reference has no KV cache, transcribe.rs:270) */

/* WhisperConfig = AudioEncoderConfig + TextDecoderConfig, src/model/mod.rs:16-20,
 * :73-80, :164-171 */
typedef struct wb_dims {
  int32_t n_mels, n_audio_ctx, n_audio_state, n_audio_head, n_audio_layer;
  int32_t n_vocab, n_text_ctx, n_text_state, n_text_head, n_text_layer;
} wb_dims;

/* ---- model ---------------------------------------------------------------------- */

/* load_whisper(path), src/model/load.rs:295-310: reads the dump directory written by
 * python/dump.py (1-D f32 .npy files, shape stored as leading floats). */
int wb_model_load_dump_dir(const char* dir, int device, int compute_dtype, wb_model** out);

/* Same model from tensors already in host memory, named by their dump-dir relative
 * path without ".npy" (e.g. "encoder/block_0/attn/query/weight"); lets a Rust caller
 * hand over the tensors of a Burn record (src/bin/transcribe/main.rs:63-70).
 * shapes[i] points at ranks[i] dims.  Scalars (n_head, n_layer, eps ...) have rank 1. */
int wb_model_load_tensors(const char* const* names, const float* const* data,
                          const int64_t* const* shapes, const int32_t* ranks, int n,
                          int device, int compute_dtype, wb_model** out);

/* load_whisper_model_file, src/bin/transcribe/main.rs:63-70 (+ WhisperConfig::load of `<name>.cfg`, :116-123):
 * the converter's output (src/bin/convert/main.rs:17-19, :51), NamedMpkGzFileRecorder<FullPrecisionSettings> =
 * gzip(MessagePack with field names) of the Whisper module record.  cfg_path may be NULL (head counts then
 * follow from n_state / 64).  Burn 0.9.0 is not vendored with the reference: the reader walks the record
 * structurally (any map with "value" + "shape" is a tensor named by its key path) -- format parity unpinned. */
int wb_model_load_burn_record(const char* mpk_gz_path, const char* cfg_path, int device, int compute_dtype,
                              wb_model** out);
/* The same reader without a device: calls fn(user, dump-style name, data, shape, rank) per tensor (host logic,
 * testable without a GPU); a non-zero return of fn stops the walk and is returned. */
typedef int (*wb_tensor_fn)(void* user, const char* name, const float* data, const int64_t* shape, int32_t rank);
int wb_burn_record_read(const char* mpk_gz_path, const char* cfg_path, wb_tensor_fn fn, void* user);

/* Whisper::encoder_ctx_size / decoder_ctx_size (mod.rs:64-70) and the rest of the config. */
int wb_model_dims(const wb_model* m, wb_dims* out);
void wb_model_free(wb_model* m);

/* LayerNorm epsilon placement: 0 = (x-mu)/(sqrt(var)+eps)  [Burn 0.9.0 @ fb2a71bb, default]
 *                              1 = (x-mu)/sqrt(var+eps)    [later Burn releases, HF]      */
int wb_model_set_ln_variant(wb_model* m, int eps_inside_sqrt);

/* Mel frames per window: 0 = at most n_audio_ctx FRAMES, exactly as the reference asserts (mod.rs:236-241; its
 *                            windows are therefore 14.9 s, transcribe.rs:32-34)                     [default]
 *                        1 = at most n_audio_ctx encoder POSITIONS = 2 n_audio_ctx frames: Whisper's own 30 s
 *                            window ("perf geometry": T = 3000, C = 1500).  NOT reference behaviour -- the
 *                            reference panics there; window length, clipping and padding follow the same
 *                            formulas (transcribe.rs:32-34, :171-177) with the larger bound. */
int wb_model_set_frame_limit(wb_model* m, int whisper_geometry);

/* Log-mel frontend of every PCM entry point of this model (wb_session_begin, wb_waveform_to_tokens and its _prompted /
 * _dev / _sharded forms):
 *   0 = WB_FRONTEND_FFT        K1: 20x20 FFT with exact twiddles -- closer to the true log-mel than the
 *                              reference                                                              [default]
 *   1 = WB_FRONTEND_REFERENCE  the reference's own recipe (stfft, audio.rs:284-367): a dense f32 DFT against its f32
 *                              angle table b[k][n] = f32(f32(k) * f32(2 pi / 400)) * f32(n) on exact-f32 MFMA, the
 *                              log10 as ln(x) / f32(ln 10) and the clamp as relu(x - m8) + m8 on every element
 *                              (audio.rs:34-56, helper.rs:8-27): what the reference computes, to ~1e-5 on every bin.
 * Any other value -> WB_ERR_ARG (the mode is unchanged).  A session takes the mode at wb_session_begin.
 * The reference recipe exists for 80 mel rows only (audio.rs:7): mode 1 on a 128-bin model (large-v3 and later) ->
 * WB_ERR_ARG, the mode is unchanged. */
enum { WB_FRONTEND_FFT = 0, WB_FRONTEND_REFERENCE = 1 };
int wb_model_set_frontend(wb_model* m, int frontend);
/* The current mode (0 / 1), WB_ERR_ARG for a null model. */
int wb_model_frontend(const wb_model* m);

/* Arithmetic of the encoder-side Linear layers of this model (chosen at load time; 1 can turn into 0 ONCE, see below):
 *   0 = exact-f32 MFMA (v_mfma_f32_32x32x2_f32)
 *   1 = split precision: three fp16 MFMAs per product on fp16 hi / lo pieces, f32 accumulation -- f32-grade results
 *       (default for f32 models; WHISPER_HIP_ENCODER_SPLIT=0 at load time selects 0, and a model whose activations leave
 *       fp16's range, |x| >= 65504, falls back to 0 by itself: the pass is repeated, the answer changes from then on)
 * Replaces nothing in the reference (its Linear is Burn's, mod.rs:377-379); a caller reports it next to its timings. */
int wb_model_encoder_gemm(const wb_model* m);

/* Arithmetic of the decoder's Linear layers in BATCH MODE (more than 8 -- at d <= 512: 16 -- live rows per step):
 *   0 = exact-f32 MFMA (v_mfma_f32_16x16x4_f32)
 *   1 = split precision on fp16 hi / lo weight tiles (v_mfma_f32_16x16x32_f16 x 3, f32 accumulation; default for f32 models;
 *       WHISPER_HIP_DECODER_SPLIT=0 at load time selects 0).  1 can turn into 0 ONCE: when a decoder activation leaves fp16's
 *       range the decode call that observes it fails with WB_ERR_STATE (its rows are invalid), the model switches to 0 and
 *       the caller's retry succeeds.  The guard word is per SESSION: only the session whose rows were invalid fails.
 * Replaces nothing in the reference (mod.rs:345-350 runs Burn's Linear). */
int wb_model_decoder_gemm(const wb_model* m);

/* ---- stateless, reference-shaped entry points (the parity surface) -------------- */

/* max_waveform_samples(n_frame_max), src/audio.rs:12-17 */
int64_t wb_max_waveform_samples(int64_t n_frame_max);

/* prep_audio(waveform [1,n], sample_rate) -> [1,80,n/160], src/audio.rs:34-56.
 * mel must hold 80*(n/160) floats; *n_frames receives n/160.  n < 400 -> WB_ERR_SHAPE
 * (audio.rs:292 assert). */
int wb_prep_audio(int device, const float* pcm, int64_t n, double sample_rate, float* mel,
                  int64_t* n_frames);
/* The same with the frontend chosen per call (WB_FRONTEND_FFT = wb_prep_audio, WB_FRONTEND_REFERENCE; see
 * wb_model_set_frontend); any other value -> WB_ERR_ARG. */
int wb_prep_audio_frontend(int device, const float* pcm, int64_t n, double sample_rate, float* mel,
                           int64_t* n_frames, int frontend);
/* wb_prep_audio with the number of mel rows chosen per call: n_mels = 80 (= wb_prep_audio, bit for bit) or 128 (the
 * frontend of large-v3 and later: a filterbank designed in f64, see wb_mel_filterbank) -> [1,n_mels,n/160]; mel must hold
 * n_mels*(n/160) floats.  K1 (WB_FRONTEND_FFT) always.  Any other n_mels -> WB_ERR_ARG. */
int wb_prep_audio_mels(int device, const float* pcm, int64_t n, double sample_rate, int n_mels, float* mel,
                       int64_t* n_frames);

/* ---- WAV ingest with the reference's sample scaling (next to the hot path) ---------- */

/* load_audio_waveform, src/bin/transcribe/main.rs:31-55 (hound): header of a RIFF/WAVE file.
 * n_samples is per channel.  Any out pointer may be NULL. */
int wb_wav_info(const char* path, int64_t* n_samples, int32_t* sample_rate, int32_t* channels,
                int32_t* bits, int32_t* is_float);
/* The samples as f32: integer PCM (8 / 16 / 24 / 32 bit) as s / (2^(bits-1) - 1) (main.rs:45-52), IEEE
 * float as stored (main.rs:48).  A sample rate other than 16 000 Hz or more than one channel ->
 * WB_ERR_SHAPE (the asserts of main.rs:42-43); capacity < samples -> WB_ERR_ARG. */
int wb_wav_read_f32(const char* path, float* out, int64_t capacity, int64_t* n_samples);
/* wb_wav_read_f32 without the 16 kHz assert (still mono): the input of wb_resample_dev. */
int wb_wav_read_f32_any_rate(const char* path, float* out, int64_t capacity, int64_t* n_samples);

/* Sample-rate conversion in HBM for inputs the reference's CLI rejects (main.rs:42; its README sends them through
 * `sox`, README.md:69-74 -- the bundled audio.wav is 22 050 Hz).  Rational polyphase resampler with the design of
 * SciPy's resample_poly(x, up, down): up/down = rate_out/rate_in reduced, Kaiser(beta 5) windowed sinc of half
 * length 10*max(up,down), cut-off 1/max(up,down) of Nyquist, zero extension; taps designed in f64, f32 arithmetic.
 *   wb_resample_len     ceil(n_in*up/down), or -1 on a bad argument / a reduced ratio above 1600
 *   wb_resample_filter  the taps (host only; taps may be NULL to query n_taps = 20*max(up,down)+1, up, down)
 *   wb_resample_dev     src_dev[n_in] -> dst_dev[*n_out] (DEVICE pointers), one pass, synchronises before returning */
int64_t wb_resample_len(int64_t n_in, int32_t rate_in, int32_t rate_out);
int wb_resample_filter(int32_t rate_in, int32_t rate_out, float* taps, int32_t capacity, int32_t* n_taps, int32_t* up,
                       int32_t* down);
int wb_resample_dev(int device, const float* src_dev, int64_t n_in, int32_t rate_in, int32_t rate_out, float* dst_dev,
                    int64_t capacity, int64_t* n_out);

/* The same scaling for 16-bit PCM already resident in HBM: dst_dev[i] = src_dev[i] / 32767 (correctly
 * rounded, bit-identical to the host path); halves the host->device bytes of wb_waveform_to_tokens_dev. */
int wb_pcm_s16_to_f32_dev(int device, const int16_t* src_dev, int64_t n, float* dst_dev);

/* The frontend alone, batched and device-resident: the window iterator of waveform_to_mel_tensor
 * (src/transcribe.rs:114-138: window w = pcm[starts[w], +lens[w]) -> prep_audio) followed by the clip /
 * zero-pad of mels_to_text (src/transcribe.rs:171-177: keep clip_frames frames, append `padding` zero
 * frames), for all windows in one launch pair.  pcm_dev / mel_dev are DEVICE pointers; window w is written
 * to mel_dev + w * win_stride as [80][row_stride] (row_stride % 4 == 0, >= frames_out[w]); frames_out[w]
 * = min(lens[w] / 160, clip_frames) + padding.  iters >= 1 repeats the pass; elapsed_ms (optional)
 * receives the HIP-event time of all passes on the launch stream (the mel-frames/s measurement). */
int wb_waveform_to_mels_dev(int device, const float* pcm_dev, int64_t n_samples, double sample_rate,
                            const int64_t* starts, const int64_t* lens, int32_t n_windows, int32_t clip_frames,
                            int32_t padding, float* mel_dev, int64_t win_stride, int32_t row_stride,
                            int32_t* frames_out, int32_t iters, double* elapsed_ms);
/* The same with the frontend chosen per call (WB_FRONTEND_FFT = wb_waveform_to_mels_dev, WB_FRONTEND_REFERENCE); any
 * other value -> WB_ERR_ARG.  Serves the batched reference-recipe frontend and its mel-frames/s measurement. */
int wb_waveform_to_mels_dev_frontend(int device, const float* pcm_dev, int64_t n_samples, double sample_rate,
                                     const int64_t* starts, const int64_t* lens, int32_t n_windows, int32_t clip_frames,
                                     int32_t padding, float* mel_dev, int64_t win_stride, int32_t row_stride,
                                     int32_t* frames_out, int32_t iters, double* elapsed_ms, int32_t frontend);
/* The same with the number of mel rows chosen per call as well: window w is written as [n_mels][row_stride]
 * (win_stride >= n_mels * row_stride).  n_mels = 80 is wb_waveform_to_mels_dev_frontend bit for bit; n_mels = 128 (large-v3
 * and later) has K1 only: WB_FRONTEND_REFERENCE there, or any other n_mels -> WB_ERR_ARG. */
int wb_waveform_to_mels_dev_mels(int device, const float* pcm_dev, int64_t n_samples, double sample_rate,
                                 const int64_t* starts, const int64_t* lens, int32_t n_windows, int32_t clip_frames,
                                 int32_t padding, float* mel_dev, int64_t win_stride, int32_t row_stride,
                                 int32_t* frames_out, int32_t iters, double* elapsed_ms, int32_t n_mels, int32_t frontend);

/* Whisper::forward_encoder(mel [B,n_mels,T]; n_mels = the model's, 80 or 128) -> [B,C,d], C=(T-1)/2+1, src/model/mod.rs:52-54,
 * :228-260.  T > n_audio_ctx -> WB_ERR_SHAPE (mod.rs:236-241). */
int wb_forward_encoder(wb_model* m, const float* mel, int B, int T, float* out);

/* Whisper::forward_decoder(tokens [n,L], encoder_output [n,C,d]) -> logits [n,L,V],
 * src/model/mod.rs:56-62, :131-157.  Stateless: cross-attention K/V are re-projected
 * (mod.rs:482-490).  L > n_text_ctx -> WB_ERR_SHAPE (mod.rs:134-139). */
int wb_forward_decoder(wb_model* m, const int32_t* tokens, int n, int L, const float* enc, int C,
                       float* logits);

/* Whisper::forward(mel [B,n_mels,T], tokens [B,L]) -> logits [B,L,V], src/model/mod.rs:48-50 */
int wb_forward(wb_model* m, const float* mel, int B, int T, const int32_t* tokens, int L,
               float* logits);

/* ---- stateful fast path (result-equivalent to transcribe.rs:148-312) ------------ */

/* Decode constants the reference hard-codes; wb_decode_params_default() fills them in. */
typedef struct wb_decode_params {
  int32_t beam_size;            /* transcribe.rs:232 (5).  1 == greedy */
  int32_t max_depth;            /* transcribe.rs:233 (100)                            */
  int32_t padding;              /* transcribe.rs:33  (10 zero mel frames)             */
  int32_t overlap_seconds;      /* transcribe.rs:120 (3)                              */
  int32_t max_n_offsets;        /* transcribe.rs:57  (40)                             */
  int32_t min_n_overlaps;       /* transcribe.rs:57  (3)                              */
  int32_t mask_until_len;       /* transcribe.rs:271 (5): special mask while len <= 5 */
  int32_t max_batch_windows;    /* engine knob: windows encoded/decoded together (0 = all) */
  /* special tokens by id (transcribe.rs:179-185; looked up by name in tokenizer.json
   * by the reference -- the tokenizer stays on the caller's side of the boundary) */
  int32_t tok_start_of_transcript, tok_language, tok_transcribe, tok_no_timestamps,
      tok_end_of_text;
} wb_decode_params;
void wb_decode_params_default(wb_decode_params* p);

/* mel (+clip, +`padding` zero frames) -> encoder -> cross-attention K/V once, for
 * n_windows windows cut from `pcm` at [starts[i], starts[i]+lens[i]).
 * transcribe.rs:134, :171-177, :222.  max_beams = live beams per window. */
int wb_session_begin(wb_model* m, const float* pcm, int64_t n_pcm, const int64_t* starts,
                     const int64_t* lens, int n_windows, int max_beams, int padding,
                     wb_session** out);
/* Same, from already-prepared mel windows mel[i] = [n_mels, T[i]] (n_mels = the model's) packed back to back. */
int wb_session_begin_mel(wb_model* m, const float* mel, const int32_t* T, int n_windows,
                         int max_beams, int padding, wb_session** out);

/* is_special[V] != 0 where bpe.is_special(id); transcribe.rs:243-251 */
int wb_session_set_special_mask(wb_session* s, const uint8_t* is_special);

/* One decode step for n live beams (KV-cached equivalent of the closure
 * `beamsearch_next`, transcribe.rs:253-307).  Beam i of this step continues the beam
 * that occupied slot parent[i] in the previous step (-1: a fresh, empty beam) of window
 * window[i], and appends new_tokens[i].  If k > 0 the k best continuations of each beam
 * by (log-prob descending, token id ascending) are returned: log_softmax over the
 * (optionally special-masked, transcribe.rs:271-275) logits of the last position.
 * WB_ERR_STATE with "... left fp16's range ..." in wb_last_error(): with more than 8 live rows (16 at d <= 512) the decoder's
 * Linear layers run on fp16 hi / lo weight pieces (f32-grade results); an activation of |x| >= 65504 there makes this
 * step's rows invalid.  The call says so, the model switches to the exact-f32 kernels for good, and decoding again
 * (a new session, or wb_waveform_to_tokens again) succeeds.  Whisper's decoder activations are O(10): a backstop. */
int wb_session_step(wb_session* s, const int32_t* new_tokens, const int32_t* parent,
                    const int32_t* window, int n, int apply_special_mask, int k, int32_t* top_ids,
                    float* top_logprobs);

/* Debug/parity: full log-prob row [V] of beam slot i after the last step. */
int wb_session_last_logprobs(wb_session* s, int slot, float* out);
/* Debug/parity: encoder output of window w, [C_w, d]; *C receives C_w. */
int wb_session_encoder_output(wb_session* s, int w, float* out, int32_t* C);
void wb_session_free(wb_session* s);

/* mels_to_text (transcribe.rs:148-383) without the tokenizer, for a batch of windows:
 * beam search (src/beam.rs:9-110) driven by wb_session_step.  out_tokens holds
 * n_windows rows of `row_stride` ints; out_lens[i] = sequence length of window i
 * (prompt included, transcribe.rs:309-312). */
int wb_session_decode(wb_session* s, const wb_decode_params* p, int32_t* out_tokens,
                      int32_t row_stride, int32_t* out_lens);

/* Optional mode (not the reference's live behaviour): the same beam search from a caller-supplied initial
 * sequence instead of the four-token prompt of transcribe.rs:203 -- the building block of the prompt
 * conditioning the reference wrote and then disabled (transcribe.rs:188-199, shadowed at :201).  The special-token
 * mask still applies while the sequence length is <= mask_until_len (transcribe.rs:271-275), i.e. never for a
 * prompt longer than that.  row_stride >= prompt_len + max_depth. */
int wb_session_decode_prompt(wb_session* s, const wb_decode_params* p, const int32_t* prompt, int32_t prompt_len,
                             int32_t* out_tokens, int32_t row_stride, int32_t* out_lens);

/* Optional mode: waveform_to_text with that prompt conditioning switched back on -- every window after the first
 * starts from [tok_start_of_prev, the last n_prev_tokens (reference: 5) non-special tokens of the transcript so far,
 * start_of_transcript, language, transcribe, no_timestamps] (transcribe.rs:43-50, :188-199, :203), and its row
 * (prompt included, as mels_to_text returns it) is stitched with find_chunk_overlap (:56-63).  Windows depend on
 * their predecessors, so they are decoded one at a time; win_tokens holds one row of `row_stride` ints per window,
 * row_stride >= 1 + n_prev_tokens + 4 + max_depth.  PCM on the host. */
int wb_waveform_to_tokens_prompted(wb_model* m, const float* pcm, int64_t n, int sample_rate,
                                   const wb_decode_params* p, const uint8_t* is_special, int32_t tok_start_of_prev,
                                   int32_t n_prev_tokens, int32_t* win_tokens, int32_t row_stride, int32_t* win_lens,
                                   int32_t* stitched, int64_t stitched_cap, int64_t* n_stitched);

/* The same beam search (src/beam.rs:9-110 driving the closure of transcribe.rs:253-307) over a
 * caller-supplied step function with wb_session_step's contract -- the host logic without the
 * GPU, e.g. for a Rust caller that owns its own model, and for CPU tests of the bookkeeping. */
typedef int (*wb_step_fn)(void* user, const int32_t* new_tokens, const int32_t* parent,
                          const int32_t* window, int n, int apply_special_mask, int k,
                          int32_t* top_ids, float* top_logprobs);
int wb_beam_search(const wb_decode_params* p, int n_windows, int n_vocab, wb_step_fn step, void* user,
                   int32_t* out_tokens, int32_t row_stride, int32_t* out_lens);
/* The same search with the bookkeeping of src/beam.rs:39-79 done by the DEVICE kernel that wb_session_decode chains between
 * decode steps (beam_size > 1; WHISPER_HIP_BEAM_CHAIN=0 keeps the host loop above), driven by a caller's step function: a test
 * hook that lets the device restatement be compared with the host one on scripted log-prob rows (exact ties, finished beams).
 * n_windows <= 64; `device` only hosts three small buffers (no model). */
int wb_beam_search_device(int device, const wb_decode_params* p, int n_windows, int n_vocab, wb_step_fn step,
                          void* user, int32_t* out_tokens, int32_t row_stride, int32_t* out_lens);

/* waveform_to_text (transcribe.rs:23-74) without the tokenizer: windows
 * (transcribe.rs:114-128), per-window decode, token-overlap stitch
 * (find_chunk_overlap, transcribe.rs:76-110).  Only windows [win_begin, win_end) are
 * decoded (multi-GPU sharding: SURVEY 8e); pass 0, -1 for all.  Per-window token rows go
 * to win_tokens [n_local, row_stride] / win_lens; when stitched != NULL the stitched
 * stream of the local windows is written there (capacity stitched_cap, length *n_stitched). */
int wb_waveform_to_tokens(wb_model* m, const float* pcm, int64_t n, int sample_rate,
                          const wb_decode_params* p, const uint8_t* is_special, int win_begin,
                          int win_end, int32_t* win_tokens, int32_t row_stride, int32_t* win_lens,
                          int32_t* stitched, int64_t stitched_cap, int64_t* n_stitched);

/* Same with the waveform already resident in device memory (`pcm_dev` is a DEVICE pointer
 * on the model's GPU; no copy is made -- the mel kernel reads the windows in place). */
int wb_waveform_to_tokens_dev(wb_model* m, const float* pcm_dev, int64_t n, int sample_rate,
                              const wb_decode_params* p, const uint8_t* is_special, int win_begin,
                              int win_end, int32_t* win_tokens, int32_t row_stride, int32_t* win_lens,
                              int32_t* stitched, int64_t stitched_cap, int64_t* n_stitched);

/* ---- multi-GPU: windows sharded over ranks -------------------------------------------------------
 * The reference is single-device and decodes its windows one after another (transcribe.rs:35-66); they are independent
 * (the previous-window prompt is discarded, transcribe.rs:195-201), so rank r of R decodes the contiguous block
 * [ceil(r K / R), ceil((r + 1) K / R)) of the K windows and the ranks exchange ONE fixed-shape buffer of token rows;
 * every rank then folds the stitch (transcribe.rs:56-63) over all K rows -- identical to world size 1 by construction.
 *
 * The exchange is an all-gather the caller supplies: `send` holds bytes_per_rank bytes of this rank, `recv` receives
 * world x bytes_per_rank bytes in rank order (host memory both).  wb_comm_allgather is the built-in RCCL transport
 * (RCCL over xGMI; librccl is opened at run time, on first use): rank 0 makes an id with wb_comm_unique_id and ships its
 * 128 bytes to the other ranks by its own means (a file, a socket, MPI, torch.distributed ...), every rank calls
 * wb_comm_init with its own device, and passes (wb_comm_allgather, comm) below. */
typedef int (*wb_allgather_fn)(void* user, const void* send, void* recv, int64_t bytes_per_rank);
typedef struct wb_comm wb_comm;
int wb_comm_unique_id(uint8_t* id128);
int wb_comm_init(const uint8_t* id128, int rank, int world, int device, wb_comm** out);
void wb_comm_free(wb_comm* c);
int wb_comm_allgather(void* comm, const void* send, void* recv, int64_t bytes_per_rank);

/* The block of rank `rank`: [*lo, *hi) = [ceil(rank K / world), ceil((rank + 1) K / world)). */
int wb_shard_partition(int64_t n_windows, int rank, int world, int64_t* lo, int64_t* hi);

/* waveform_to_text (transcribe.rs:23-74) without the tokenizer, sharded: this rank decodes its block of windows of the
 * WHOLE waveform `pcm` (host memory, or device memory of the model's GPU when pcm_on_device != 0), all-gathers the
 * rows and stitches.  On return EVERY rank holds all K per-window rows (win_tokens [K][row_stride], win_lens [K],
 * K <= win_cap) and the stitched stream.  world == 1 needs no all-gather (allgather may be NULL).
 * Failure: a rank whose local decode fails (out of memory, a HIP error) STILL enters the all-gather -- its rows carry a
 * sentinel -- so no rank is left blocked in the collective; every rank then returns an error (the failing rank its own
 * status, the others WB_ERR_STATE naming the rank).  Argument errors are reported before the collective on the rank that
 * has them: validate identically on every rank. */
int wb_waveform_to_tokens_sharded(wb_model* m, const float* pcm, int pcm_on_device, int64_t n, int sample_rate,
                                  const wb_decode_params* p, const uint8_t* is_special, int rank, int world,
                                  wb_allgather_fn allgather, void* user, int32_t* win_tokens, int32_t row_stride,
                                  int32_t* win_lens, int64_t win_cap, int32_t* stitched, int64_t stitched_cap,
                                  int64_t* n_stitched);

/* Window extents of waveform_to_mel_tensor (transcribe.rs:114-128).  Returns the window
 * count; fills starts/lens when non-NULL (capacity cap). */
int64_t wb_window_extents(int64_t n_samples, int sample_rate, int64_t window_len, int overlap_seconds,
                          int64_t* starts, int64_t* lens, int64_t cap);

/* find_chunk_overlap(prev, curr, max_n_offsets, min_n_overlaps), transcribe.rs:76-110.
 * Returns 1 and sets the indices if an overlap >= min_n_overlaps was found, else 0. */
int wb_find_chunk_overlap(const int32_t* prev, int64_t n_prev, const int32_t* curr, int64_t n_curr,
                          int max_n_offsets, int min_n_overlaps, int64_t* prev_index,
                          int64_t* curr_index);

/* Fold the stitch (transcribe.rs:56-63) over per-window token rows in window order. */
int wb_stitch_windows(const int32_t* win_tokens, int32_t row_stride, const int32_t* win_lens,
                      int n_windows, int max_n_offsets, int min_n_overlaps, int32_t* out,
                      int64_t cap, int64_t* n_out);

/* ---- token timestamps: cross-attention alignment + DTW (the technique behind `word_timestamps`) ------------------
 * The reference decodes with <|notimestamps|> (transcribe.rs:203); token times come from the decoder's cross-attention
 * instead.  Per row: one teacher-forced pass of the decoder over the finished tokens; for every alignment head the
 * softmax weights W[l][c] over the window's C encoder positions (exact f32); z-score over the token axis per position
 * (biased variance; a constant column gives zeros); median filter of width filter_width along c (reflect padding; skipped
 * when C <= filter_width / 2); M = mean over the heads; DTW over X = -M[n_prefix .. len - drop_last) in f32 (strict
 * comparisons, diagonal before up before left).  A token's start position is the column of the first path cell of its
 * row; its time is window start + 0.02 s * position.  All of it runs on the device (align.hip).
 *
 * heads: n_heads pairs (layer, head); NULL / 0 = every head of layers [n_text_layer / 2, n_text_layer).  The pass meets
 *        the layers in ascending order; heads of one layer are summed in the order given.
 * lens:  per-row length, NULL = L.  start_pos [n][L]: entry l of a DTW row = its start position, every other entry -1.
 * matrix (optional, parity / debug): M, [n][L][C], zero outside a row's len.
 * Errors (nothing is launched): unknown layer / head, filter_width even or outside 1 .. 15, n_prefix + drop_last >= len
 * -> WB_ERR_ARG; len > n_text_ctx -> WB_ERR_SHAPE. */
int wb_align_tokens(wb_model* m, const int32_t* tokens, int n, int L, const int32_t* lens, const float* enc, int C,
                    const int32_t* heads, int32_t n_heads, int32_t n_prefix, int32_t drop_last, int32_t filter_width,
                    int32_t* start_pos, float* matrix);
/* The same over a session's windows, after (or without) a decode: row w belongs to window w and uses the session's
 * encoder output and cached cross-attention K -- no re-encode.  start_pos [W][row_stride]; matrix [W][row_stride][maxC]
 * (maxC: the largest C of the session's windows). */
int wb_session_align(wb_session* s, const int32_t* tokens, int32_t row_stride, const int32_t* lens, const int32_t* heads,
                     int32_t n_heads, int32_t n_prefix, int32_t drop_last, int32_t filter_width, int32_t* start_pos,
                     float* matrix);
/* The DTW alone on a caller's f32 cost matrix x [N][C] (host memory): start position of every row.  N <= 512.
 * `device` only hosts the buffers (no model). */
int wb_dtw_start_positions(int device, const float* x, int32_t N, int32_t C, int32_t* start_pos);
/* wb_waveform_to_tokens + alignment of every window's row as decoded (n_prefix = 4, the prompt; drop_last = 1 exactly when
 * the row ends in tok_end_of_text), on the session that decoded it.  win_times [n_local][row_stride]: seconds from the
 * start of the waveform, NaN where the token is not aligned; stitched_times parallel to `stitched` (required with it). */
int wb_waveform_to_token_times(wb_model* m, const float* pcm, int64_t n, int sample_rate, const wb_decode_params* p,
                               const uint8_t* is_special, int win_begin, int win_end, int32_t* win_tokens,
                               int32_t row_stride, int32_t* win_lens, int32_t* stitched, int64_t stitched_cap,
                               int64_t* n_stitched, const int32_t* heads, int32_t n_heads, int32_t filter_width,
                               float* win_times, float* stitched_times);
/* wb_stitch_windows carrying a parallel float per token (win_times [n_windows][row_stride]) through the same fold: a
 * stitched token keeps the value it had in the window the stitch took it from (transcribe.rs:56-63).  Host only. */
int wb_stitch_windows_times(const int32_t* win_tokens, int32_t row_stride, const int32_t* win_lens, int n_windows,
                            int max_n_offsets, int min_n_overlaps, int32_t* out, int64_t cap, int64_t* n_out,
                            const float* win_times, float* out_times);

/* ---- token log-probabilities, no-speech probability, language detection ------------------------------------------
 * One teacher-forced pass of the decoder over finished token rows, ended by a fused logits product (score.hip) that keeps
 * only log-softmax statistics: exact f32 MFMA, no [rows][V] logits in memory, run-to-run bit-identical.
 *
 * token_logprobs [n][L]: for 1 <= l < len, entry l = log_softmax(logits at position l - 1)[tokens[l]]; the special mask
 *        (is_special, as wb_session_set_special_mask) is added first when l <= mask_until_len (transcribe.rs:271-275: a
 *        sequence of length l predicts index l; 0 = never).  Entry 0 and entries >= len are NaN.
 * probe_logprobs [n][n_probe] (optional, NULL / 0): the UNMASKED log_softmax at position probe_pos of the ids probe_ids
 *        (the no-speech token after [SOT], the language ids).  probe_pos may be a masked position: both statistics of such
 *        a row are kept.
 * A NaN in the decoder's output row gives NaN for that position (never a finite-looking number); a position whose whole
 * vocabulary is masked (no real special mask does that) has lse = -inf and a NaN log-prob.
 * lens:  per-row length, NULL = L.
 * Errors (nothing is launched): a token / probe id outside the vocabulary, len outside 1 .. L, probe_pos >= len of any
 * row, mask_until_len > 0 without is_special -> WB_ERR_ARG; len > n_text_ctx -> WB_ERR_SHAPE. */
int wb_score_tokens(wb_model* m, const int32_t* tokens, int n, int L, const int32_t* lens, const float* enc, int C,
                    const uint8_t* is_special, int32_t mask_until_len, const int32_t* probe_ids, int32_t n_probe,
                    int32_t probe_pos, float* token_logprobs, float* probe_logprobs);
/* The same over a session's windows, after (or without) a decode: row w belongs to window w and uses the session's cached
 * cross-attention K/V -- no re-encode.  The mask is the one set by wb_session_set_special_mask: WB_ERR_STATE when
 * mask_until_len > 0 and none was set.  token_logprobs [W][row_stride]. */
int wb_session_score(wb_session* s, const int32_t* tokens, int32_t row_stride, const int32_t* lens,
                     int32_t mask_until_len, const int32_t* probe_ids, int32_t n_probe, int32_t probe_pos,
                     float* token_logprobs, float* probe_logprobs);
/* Whisper's detect_language: encode the first max_windows windows of the waveform (0 = all; the windows of
 * wb_waveform_to_tokens with its default overlap), score the one-token rows [tok_start_of_transcript] with lang_ids as
 * probes, and restrict the softmax to lang_ids (on the host, in f64): win_probs [W][n_lang] (optional), mean_probs [n_lang]
 * (optional) = the mean over the W windows, *best = its argmax as an index into lang_ids (lowest on a tie). */
int wb_waveform_detect_language(wb_model* m, const float* pcm, int64_t n, int sample_rate, int32_t padding,
                                int32_t tok_start_of_transcript, const int32_t* lang_ids, int32_t n_lang,
                                int32_t max_windows, float* win_probs, float* mean_probs, int32_t* best);
/* wb_waveform_to_tokens + the scores of every window's row as decoded, on the session that decoded it (mask_until_len from
 * p).  win_logprobs [n_local][row_stride] as token_logprobs above; stitched_logprobs parallel to `stitched` (required with
 * it); win_avg_logprob [n_local] = mean of entries [4, len) -- Whisper's avg_logprob: the generated tokens, a final
 * end-of-text included; NaN when empty; win_no_speech_prob [n_local] = exp of the unmasked log-prob of tok_no_speech after
 * [SOT] (NaN when tok_no_speech < 0). */
int wb_waveform_to_token_scores(wb_model* m, const float* pcm, int64_t n, int sample_rate, const wb_decode_params* p,
                                const uint8_t* is_special, int win_begin, int win_end, int32_t* win_tokens,
                                int32_t row_stride, int32_t* win_lens, int32_t* stitched, int64_t stitched_cap,
                                int64_t* n_stitched, int32_t tok_no_speech, float* win_logprobs,
                                float* stitched_logprobs, float* win_avg_logprob, float* win_no_speech_prob);
/* Test hook: the two launches of score.hip alone on caller data (host memory).  h [R][d] (d % 32 == 0), E [V][d]; E^T is
 * built inside with leading dimension V rounded up to 64 and NaN in the pad columns.  mask [V] (0 / -inf) applies to the
 * rows with row_masked[r] != 0 (both NULL: no mask); target[r] in [0, V) or -1; probes (probe_row[p], probe_id[p]) are
 * scored unmasked; v_splits 0 = auto.  logprob [R] (NaN without a target), lse [R] (under the row's mask), probe_lp
 * [n_probe].  `device` only hosts the buffers (no model). */
int wb_logprob_gather(int device, const float* h, int32_t R, int32_t d, const float* E, int32_t V, const float* mask,
                      const uint8_t* row_masked, const int32_t* target, const int32_t* probe_row,
                      const int32_t* probe_id, int32_t n_probe, int32_t v_splits, float* logprob, float* lse,
                      float* probe_lp);

/* ---- temperature sampling and Whisper's decode fallback (an extension: the reference has beam search only) -----------
 * The draw (sample.hip): token = argmax_v [(x_v + mask_v - M) / T + g_v] by (key descending, id ascending), with
 * g_v = -logf(-logf(u_v)), u_v = ((word >> 9) + 0.5) 2^-23 and word = output (v & 3) of Philox4x32-10 under
 * key = (seed low 32, seed high 32), counter = (v >> 2, position, stream, attempt).  position: the index in the token row of
 * the token being drawn.  A sampled token is therefore a pure function of its logits row and five integers: it does not
 * depend on the launch shape, on the rows that share the batch or on the rank that decodes the window.  Recorded with each
 * token: log_softmax of the (masked) logits -- not of logits / T -- as Whisper's sum_logprobs. */
typedef struct wb_sample_params {
  float temperature;            /* > 0 */
  int32_t best_of;              /* samples per window, 1 .. max_beams of the session */
  uint64_t seed;
  int32_t attempt;              /* index of the temperature in the fallback list: the fourth counter word */
} wb_sample_params;
void wb_sample_params_default(wb_sample_params* p);      /* 1.0, 5, 0, 0 */
/* Back to step 0 over the same encoded window batch: the encoder output and the cached cross K/V stay, so another decode
 * costs decode steps only. */
int wb_session_rewind(wb_session* s);
/* Debug / tests: the number of captured step graphs the session holds. */
int wb_session_graph_count(const wb_session* s);
/* Debug / tests: step graphs captured over the session's life (a replayed graph does not count). */
int64_t wb_session_graph_captures(const wb_session* s);
/* Debug / tests: the LDS-resident operand geometry of the persistent greedy kernel's instance that serves (n_state, live rows,
 * longest encoder context in keys) -- out5 = {resident float4 slots per thread, resident QKV weight rounds, resident Wo rows
 * of the self-attention role, resident V tiles and resident Wo rows of the cross-attention role}.  Needs no device.
 * WB_ERR_SHAPE if no instance serves the shape. */
int wb_persist_resident_geometry(int32_t n_state, int32_t n_rows, int32_t max_keys, int32_t* out5);
/* Debug / tests: one step's roles of the persistent greedy kernel as they are dealt to a grid of `grid` blocks (clamped to
 * the roles of a step) -- per role, grouped by block, out_kinds = kind | layer << 8 | row << 16 (kind: 0 self-attention,
 * 1 cross-attention, 2 MLP, 3 logits, 4 merge, 5 final LayerNorm; the encoding of the WHISPER_HIP_PS_STAMPS file) and
 * out_block = its block.  legacy != 0: the dealing of WHISPER_HIP_PERSIST_DEAL=legacy.  The plan is the one of the `planes`
 * MLP form (WHISPER_HIP_PERSIST_MLP=planes, and every grid below 4 n_state / 64 blocks); the default two-phase form deals the
 * same roles to the same blocks without the final-LayerNorm roles, and a block with a last-layer MLP role takes one logits tile
 * where the others can absorb the rest (WHISPER_HIP_PERSIST_DEAL=log reports that deal).  Needs no device.  Returns the
 * number of roles (at most cap), or a negative status: WB_ERR_SHAPE if no instance serves the shape. */
int wb_persist_role_plan(int32_t n_layer, int32_t n_head, int32_t n_state, int32_t n_rows, int32_t n_vocab, int32_t grid,
                         int32_t legacy, int32_t* out_kinds, int32_t* out_block, int32_t cap);
/* best_of independent sampled sequences per window from `prompt`, on a fresh or rewound session; the draw and the row
 * bookkeeping run on the device, chunks of steps replay as one graph (the same graph for every temperature and seed).
 * active [W] (NULL = all): windows with active[w] == 0 are not decoded and nothing of theirs is written.
 * stream_ids [W] (NULL = w * best_of): sample j of window w draws from stream stream_ids[w] + j.
 * out_tokens / out_lens: per window the sample with the largest sum_logprob / n_text (n_text = generated tokens without a
 * final end-of-text; f64; the first of equal maxima; n_text == 0 ranks -inf), prompt included.  out_sum_logprob
 * [W][best_of] f64 and out_best [W] are optional.  p supplies max_depth, mask_until_len and tok_end_of_text.
 * Errors with nothing launched: temperature <= 0 or not finite, best_of outside 1 .. max_beams, row_stride <
 * prompt_len + max_depth, a token outside the vocabulary -> WB_ERR_ARG; the special mask needed and not set, or a session
 * that is not at step 0 -> WB_ERR_STATE. */
int wb_session_decode_sample(wb_session* s, const wb_decode_params* p, const wb_sample_params* sp, const int32_t* prompt,
                             int32_t prompt_len, const uint8_t* active, const int32_t* stream_ids, int32_t* out_tokens,
                             int32_t row_stride, int32_t* out_lens, double* out_sum_logprob, int32_t* out_best);

/* Debug / parity: every sample of the last wb_session_decode_sample on this session -- the generated tokens (without the
 * prompt) of sample j of window w at tokens[(w * best_of + j) * row_stride], lens[w * best_of + j] of them (-1: the window
 * was not active).  row_stride >= the call's max_depth. */
int wb_session_last_samples(wb_session* s, int32_t* tokens, int32_t row_stride, int32_t* lens);

enum { WB_FALLBACK_MAX_TEMPERATURES = 8 };
enum { WB_FALLBACK_ACCEPT = 0, WB_FALLBACK_RETRY = 1, WB_FALLBACK_NO_SPEECH = 2 };
typedef struct wb_fallback_params {
  float temperatures[WB_FALLBACK_MAX_TEMPERATURES];   /* 0, 0.2, 0.4, 0.6, 0.8, 1.0; the first must be 0 (the ordinary decode) */
  int32_t n_temperatures;
  int32_t best_of;                       /* 5 */
  float logprob_threshold;               /* -1.0   (NaN: rule off) */
  float no_speech_threshold;             /* 0.6    (NaN: rule off) */
  float compression_ratio_threshold;     /* 2.4    (NaN: rule off) */
  uint64_t seed;
  int32_t tok_no_speech;                 /* -1: the no-speech rule is off */
} wb_fallback_params;
void wb_fallback_params_default(wb_fallback_params* p);
/* Whisper's decode_with_fallback and the skip test of transcribe, host only: retry when ratio >
 * compression_ratio_threshold or avg_logprob < logprob_threshold, unless no_speech_prob > no_speech_threshold; no speech
 * when no_speech_prob > no_speech_threshold and (avg_logprob < logprob_threshold, or that rule is off).  A NaN input to an
 * enabled rule fails it.  Returns WB_FALLBACK_ACCEPT / _RETRY / _NO_SPEECH. */
int wb_fallback_decide(const wb_fallback_params* fp, float avg_logprob, float no_speech_prob, float ratio);
/* Compression ratio of one window's generated tokens, computed by the caller (text lives on its side of the boundary). */
typedef double (*wb_ratio_fn)(void* user, const int32_t* tokens, int32_t n);
/* wb_waveform_to_tokens with the fallback: per window batch the ordinary decode (p->beam_size) is attempt 0; the scoring
 * pass on the same session gives avg_logprob (entries [4, len)) and the no-speech probability; windows that must retry are
 * decoded again by wb_session_decode_sample at temperatures[1], [2], ... (attempt i, stream = global window index *
 * best_of) after a rewind -- no re-encode -- and scored again, until they pass or the list ends (such a window keeps its
 * last row, status 1).  Windows of status 2 are left out of the stitch; their rows are still returned.  ratio NULL: the
 * compression-ratio rule is off and win_ratio is NaN.  Per-window outputs [n_local]: win_temperature, win_status,
 * win_avg_logprob, win_no_speech_prob, win_ratio, win_attempts.  With every rule off the rows and the stitched stream are
 * wb_waveform_to_tokens' bit for bit, after one attempt per window. */
int wb_waveform_to_tokens_fallback(wb_model* m, const float* pcm, int64_t n, int sample_rate, const wb_decode_params* p,
                                   const uint8_t* is_special, int win_begin, int win_end, int32_t* win_tokens,
                                   int32_t row_stride, int32_t* win_lens, int32_t* stitched, int64_t stitched_cap,
                                   int64_t* n_stitched, const wb_fallback_params* fp, wb_ratio_fn ratio, void* user,
                                   float* win_temperature, int32_t* win_status, float* win_avg_logprob,
                                   float* win_no_speech_prob, float* win_ratio, int32_t* win_attempts);
/* Test hook: the draw alone (the device function of the chain kernel) on caller data in host memory.  logits [R][ld]
 * (ld >= V); mask [V] (0 / -inf) applies to the rows with row_masked[r] != 0 (both NULL: no mask); row_stats [R][2] = the
 * row maximum and log-sum-exp under the row's mask; stream / position [R].  out_token / out_logprob [R]; a row with a NaN
 * logit or without a finite key gives eot, log-prob 0 and *out_err = 1.  `device` only hosts the buffers. */
int wb_sample_rows(int device, const float* logits, int32_t R, int32_t ld, int32_t V, const float* mask,
                   const uint8_t* row_masked, const float* row_stats, float temperature, uint64_t seed, int32_t attempt,
                   const int32_t* stream, const int32_t* position, int32_t eot, int32_t* out_token, float* out_logprob,
                   int32_t* out_err);

/* ---- timestamp-token decoding: Whisper's timestamp rules on the device, segments (an extension) ----------------------
 * Ids T = [tok_timestamp_begin, tok_timestamp_begin + n_timestamps) are timestamps (id tb + i stands for i *
 * seconds_per_timestamp), N is every other id, end-of-text included.  gen = the tokens generated so far; the allowed set
 * of the position being decided is everything not suppressed (wb_session_set_suppress) minus
 *   (a) gen[-1] in T and (len(gen) < 2 or gen[-2] in T): all of T;
 *   (b) gen[-1] in T and gen[-2] not in T: every id < tok_end_of_text outside T;
 *   (c) with t the last generated timestamp: ids of T below t in case (b), below t + 1 otherwise;
 *   (d) len(gen) == 0: all of N, and ids of T above tb + max_initial_timestamp_index (-1: no upper limit) -- when
 *       n_timestamps > 0: a vocabulary without timestamps switches the rules off;
 *   (e) ids of T above tb + max_timestamp_index (-1: none) -- for windows shorter than the timestamp range;
 *   (f) with ts_lse = logsumexp over the allowed T and mN = max over the allowed N: if ts_lse > mN, all of N.
 * The token is the argmax over what is left: by (logit descending, id ascending) at temperature 0, by the keys and
 * counters of the sampling draw above at temperature > 0 (key (x - M) / T + g with M the row maximum over all ids).
 * Recorded with it: x[token] - logsumexp(allowed).  The special mask (mask_until_len) is NOT applied in this mode:
 * `suppress` takes its place.  (a) - (d) and (f) are Whisper's ApplyTimestampRules; (e) is this engine's. */
typedef struct wb_timestamp_params {
  int32_t tok_timestamp_begin;          /* <|0.00|> */
  int32_t n_timestamps;                 /* 1501 in Whisper's vocabularies; 0: no id is a timestamp (the rules are off) */
  int32_t max_initial_timestamp_index;  /* 50 (1.0 s); -1: no limit */
  int32_t max_timestamp_index;          /* -1: none */
  float seconds_per_timestamp;          /* 0.02 */
  float temperature;                    /* 0: greedy; > 0: the Gumbel-max draw */
  int32_t best_of;                      /* 1; > 1 needs temperature > 0 */
  uint64_t seed;
  int32_t attempt;
} wb_timestamp_params;
void wb_timestamp_params_default(wb_timestamp_params* p);   /* 0, 0, 50, -1, 0.02, 0, 1, 0, 0 */
/* The static masks of timestamp decoding, u8 [n_vocab] each: suppress[v] != 0 removes id v at every step, suppress_first
 * (may be NULL) additionally at the first generated position.  Kept on the device for the session's life. */
int wb_session_set_suppress(wb_session* s, const uint8_t* suppress, const uint8_t* suppress_first);
/* wb_session_decode_sample under the timestamp rules: best_of sequences per window from `prompt` (which must not pin
 * <|notimestamps|>), on a fresh or rewound session; the rules, the pick and the row bookkeeping run on the device, chunks
 * of steps replay as one graph -- the same graph for every temperature, seed and rule parameter.  active, stream_ids,
 * out_tokens, out_lens, out_sum_logprob [W][best_of] (the f64 sum of the recorded log-probs) and out_best as there; the
 * best-of pick (temperature > 0) is by sum_logprob / n_text.  p supplies max_depth and tok_end_of_text.  A row with a NaN
 * logit or without an allowed id ends on end-of-text and the call fails with WB_ERR_STATE.
 * Errors with nothing launched: those of wb_session_decode_sample, and temperature < 0 or not finite, temperature == 0 with
 * best_of != 1, a timestamp range outside [0, n_vocab), end-of-text inside T -> WB_ERR_ARG; wb_session_set_suppress not
 * called on this session -> WB_ERR_STATE (pass all-zero masks for none). */
int wb_session_decode_timestamps(wb_session* s, const wb_decode_params* p, const wb_timestamp_params* tp,
                                 const int32_t* prompt, int32_t prompt_len, const uint8_t* active, const int32_t* stream_ids,
                                 int32_t* out_tokens, int32_t row_stride, int32_t* out_lens, double* out_sum_logprob,
                                 int32_t* out_best);
/* Test hook: the rules + pick alone (the device function of the chain kernel) on caller data in host memory.  logits
 * [R][ld] (ld >= V); suppress / suppress_first u8 [V] (NULL: none); per row the state of the rules: n_gen = len(gen),
 * prev1 / prev2 = gen[-1] / gen[-2] (read when n_gen >= 1 / 2), last_ts = the last generated timestamp id or -1; stream /
 * position [R] as wb_sample_rows.  out_token / out_logprob / out_forced [R] (forced: rule (f) removed N), out_stats [R][2]
 * = (ts_lse, mN).  A row with a NaN logit or without an allowed id gives eot, log-prob 0 and *out_err = 1.  `device` only
 * hosts the buffers. */
int wb_timestamp_rows(int device, const float* logits, int32_t R, int32_t ld, int32_t V, const uint8_t* suppress,
                      const uint8_t* suppress_first, int32_t tok_timestamp_begin, int32_t n_timestamps,
                      int32_t max_initial_timestamp_index, int32_t max_timestamp_index, float temperature, uint64_t seed,
                      int32_t attempt, const int32_t* n_gen, const int32_t* prev1, const int32_t* prev2,
                      const int32_t* last_ts, const int32_t* stream, const int32_t* position, int32_t eot,
                      int32_t* out_token, float* out_logprob, int32_t* out_forced, float* out_stats, int32_t* out_err);
/* Whisper transcribe()'s slicing of one window's generated tokens (host only).  tokens [n]: the generated tokens (no
 * prompt); everything from the first end-of-text on is ignored.  Every pair of consecutive timestamps closes a segment; a
 * row that ends on a single timestamp closes a last segment there; a row without a pair is one segment from 0 to its last
 * timestamp (if that is not <|0.00|>) or to the window end.  window_index: the window's length in timestamp units.
 * Per segment: seg_begin / seg_end = its token index range [begin, end) (timestamps included), seg_start / seg_end_time in
 * seconds relative to the window.  *advance_index: the timestamp index by which the window moves on -- the last closing
 * timestamp, or window_index when the row ends on a single timestamp or has no pair.  cap: capacity of the four arrays
 * (n + 1 always suffices); WB_ERR_ARG when it is too small. */
int wb_segments_from_tokens(const int32_t* tokens, int32_t n, int32_t tok_timestamp_begin, int32_t n_timestamps,
                            int32_t tok_end_of_text, int32_t window_index, float seconds_per_timestamp, int32_t* seg_begin,
                            int32_t* seg_end, float* seg_start, float* seg_end_time, int32_t cap, int32_t* n_segments,
                            int32_t* advance_index);
/* Long-form transcription by timestamps: the window at `seek` (at most the model's window length) is decoded by
 * wb_session_decode_timestamps from `prompt` (max_timestamp_index clamped to the window's length), sliced by
 * wb_segments_from_tokens, and seek advances by advance_index * seconds_per_timestamp * sample_rate samples -- a whole
 * window when that is 0, so the loop always ends.  Windows are sequential, one at a time.  Outputs: flat segment arrays
 * (seg_start / seg_end_time in seconds of the waveform; seg_tok_begin / seg_tok_end index `text_tokens`), the concatenated
 * non-timestamp tokens of all segments (end-of-text dropped) in text_tokens, and the number of windows decoded.  WB_ERR_ARG
 * when seg_cap or text_cap is too small. */
int wb_waveform_to_segments(wb_model* m, const float* pcm, int64_t n, int sample_rate, const wb_decode_params* p,
                            const wb_timestamp_params* tp, const uint8_t* suppress, const uint8_t* suppress_first,
                            const int32_t* prompt, int32_t prompt_len, float* seg_start, float* seg_end_time,
                            int32_t* seg_tok_begin, int32_t* seg_tok_end, int32_t seg_cap, int32_t* n_segments,
                            int32_t* text_tokens, int64_t text_cap, int64_t* n_text_tokens, int32_t* n_windows);

/* ---- beam search under the timestamp rules (an extension: Whisper's BeamSearchDecoder on the device) ------------------
 * Per window, with B = beam_size and C = max_candidates = round-half-even(B * patience), computed once on the host:
 *   1. One live beam holds the prompt with cumulative score 0.0 (Whisper's B identical copies collapse to it: its
 *      candidate dictionary is keyed by sequence).
 *   2. Each live beam j has its own rule state (gen_j: last / penultimate token a timestamp, last timestamp); n_gen, the
 *      depth, is the same for all.  Its allowed set is rules (a) - (f) above with suppress / suppress_first;
 *      lp_v = x_v - logsumexp(allowed) in f32; its candidates are its min(B + 1, |allowed|) best ids by (logit descending,
 *      id ascending); a candidate's score is score_j + (double)lp_v.
 *   3. All candidates of the window are sorted by (score descending, beam index ascending, rank within the beam
 *      ascending) and walked: an end-of-text candidate goes to this step's newly finished list, any other becomes a live
 *      beam of the next step; the walk stops behind the B-th live beam (end-of-text candidates ranked behind that point
 *      are dropped).  Fewer than B other candidates: fewer live beams (Whisper would fail; this engine goes on).
 *   4. The newly finished are appended to the window's store in walk order while it holds fewer than C; the rest is
 *      dropped.  The window ends when the store holds C entries, no live beam is left or max_depth steps have run --
 *      each window by itself.
 *   5. Finalize (host): a store with fewer than B entries is filled up with the live beams in descending score order
 *      (ties: lower beam index); they keep their score and carry no end-of-text.  rank = score / n_text when
 *      length_penalty < 0 (n_text: tokens without the end-of-text; n_text == 0 ranks -inf), else
 *      score / ((5 + n_text) / 6)^length_penalty.  The result is the first of equal maxima in store order.
 *   6. A child's rule state is its parent's, updated by the child's token.
 * Deviations from Whisper: ties (equal scores) are ordered as in 3; windows end individually; fewer than B live beams
 * are accepted; scores are f64 sums of f32 log-probs. */
typedef struct wb_beam_params {
  int32_t beam_size;      /* 5; 1 .. 7 and <= the session's max_beams */
  float patience;         /* 1.0; >= 1, max_candidates <= 16 */
  float length_penalty;   /* -1 (any negative value): rank by score / n_text; >= 0: Google NMT's ((5 + n) / 6)^alpha */
} wb_beam_params;
void wb_beam_params_default(wb_beam_params* p);   /* 5, 1.0, -1 */
/* wb_session_decode_timestamps by beam search, on a fresh or rewound session: candidates and bookkeeping run on the
 * device, chunks of steps replay as one graph -- the same graph for every rule parameter, patience and length penalty.
 * prompt, active, out_tokens [W][row_stride] (prompt + the best candidate) and out_lens as there; out_score [W] the best
 * candidate's cumulative log-prob and out_n_candidates [W] the number of finalized candidates (both may be NULL).  p
 * supplies max_depth and tok_end_of_text; tp the rules.  A NaN logit, an allowed +inf logit, a live beam without an
 * allowed id or a NaN score ends that beam on end-of-text and fails the call with WB_ERR_STATE.
 * Errors with nothing launched (WB_ERR_ARG): tp->temperature != 0, tp->best_of != 1, beam_size outside [1, 7] or above the
 * session's max_beams, patience < 1 or not finite, max_candidates > 16, length_penalty not finite, and those of
 * wb_session_decode_timestamps; wb_session_set_suppress not called -> WB_ERR_STATE. */
int wb_session_decode_timestamps_beam(wb_session* s, const wb_decode_params* p, const wb_timestamp_params* tp,
                                      const wb_beam_params* bp, const int32_t* prompt, int32_t prompt_len,
                                      const uint8_t* active, int32_t* out_tokens, int32_t row_stride, int32_t* out_lens,
                                      double* out_score, int32_t* out_n_candidates);
/* Every finalized candidate of the last wb_session_decode_timestamps_beam, in store order: n [W] candidates per window
 * (-1: the window was not active; at most cap are written, cap = 16 always suffices), tokens [W][cap][row_stride] the
 * generated tokens (no prompt), lens / scores / ranks [W][cap]. */
int wb_session_last_beams(wb_session* s, int32_t cap, int32_t* tokens, int32_t row_stride, int32_t* lens, double* scores,
                          double* ranks, int32_t* n);
/* The trace of the last wb_session_decode_timestamps_beam: n_steps [W] steps the window took part in; for step t <
 * max_steps and window w: n_live [t][W] live beams behind the step, n_finished [t][W] candidates newly finished in it
 * (before the store's cap), and per live beam q < n_live the token, the index of its parent among the live beams in front
 * of the step and its f64 score: tokens / parents / scores [t][W][8]. */
int wb_session_last_beam_trace(wb_session* s, int32_t max_steps, int32_t* n_steps, int32_t* n_live, int32_t* n_finished,
                               int32_t* tokens, int32_t* parents, double* scores);
/* Test hook: the candidates of dec_tsbeam_rows_kernel alone on caller data (wb_timestamp_rows' inputs at temperature 0,
 * plus k in [1, 8]).  out_ids / out_logprobs [R][k]: the row's min(k, |allowed|) best allowed ids in (logit descending, id
 * ascending) order with x - logsumexp(allowed) (entries past the count are not written); out_count / out_forced [R];
 * out_stats [R][2] = (ts_lse, mN).  A row with a NaN logit or without an allowed id gives the single candidate eot with
 * log-prob 0 and *out_err = 1.  Outputs sit between guard bands on the device. */
int wb_timestamp_beam_rows(int device, const float* logits, int32_t R, int32_t ld, int32_t V, const uint8_t* suppress,
                           const uint8_t* suppress_first, int32_t tok_timestamp_begin, int32_t n_timestamps,
                           int32_t max_initial_timestamp_index, int32_t max_timestamp_index, const int32_t* n_gen,
                           const int32_t* prev1, const int32_t* prev2, const int32_t* last_ts, int32_t eot, int32_t k,
                           int32_t* out_ids, float* out_logprobs, int32_t* out_count, int32_t* out_forced, float* out_stats,
                           int32_t* out_err);
/* Fills the logits [n][V] of the n live rows of step `step` (0-based).  Row i is live beam beam[i] of window window[i];
 * behind step 0 it holds the prompt (token[i] = -1, parent[i] = -1), later the token it was extended by and the index of
 * its parent among the previous step's live beams of that window.  Returns 0, or an error code that ends the search. */
typedef int (*wb_tsbeam_logits_fn)(void* user, int32_t step, int32_t n, const int32_t* window, const int32_t* beam,
                                   const int32_t* token, const int32_t* parent, float* logits);
/* Test hook without a model: both kernels of the beam search driven by a caller callback, the counterpart of
 * wb_beam_search_device.  n_windows <= 64 windows of a vocabulary of V ids; results as wb_session_last_beams (cap = 16,
 * row_stride >= max_depth) and wb_session_last_beam_trace (max_steps = max_depth) write them, plus best [W] = the index of
 * the returned candidate. */
int wb_timestamp_beam_search_device(int device, const wb_timestamp_params* tp, const wb_beam_params* bp, int32_t n_windows,
                                    int32_t V, const uint8_t* suppress, const uint8_t* suppress_first, int32_t eot,
                                    int32_t max_depth, wb_tsbeam_logits_fn fill, void* user, int32_t* cand_tokens,
                                    int32_t row_stride, int32_t* cand_lens, double* cand_scores, double* cand_ranks,
                                    int32_t* n_cand, int32_t* best, int32_t* n_steps, int32_t* n_live, int32_t* n_finished,
                                    int32_t* tr_tokens, int32_t* tr_parents, double* tr_scores);
/* wb_waveform_to_segments with every window decoded by wb_session_decode_timestamps_beam (sessions of max_beams =
 * beam_size). */
int wb_waveform_to_segments_beam(wb_model* m, const float* pcm, int64_t n, int sample_rate, const wb_decode_params* p,
                                 const wb_timestamp_params* tp, const wb_beam_params* bp, const uint8_t* suppress,
                                 const uint8_t* suppress_first, const int32_t* prompt, int32_t prompt_len, float* seg_start,
                                 float* seg_end_time, int32_t* seg_tok_begin, int32_t* seg_tok_end, int32_t seg_cap,
                                 int32_t* n_segments, int32_t* text_tokens, int64_t text_cap, int64_t* n_text_tokens,
                                 int32_t* n_windows);

/* ---- prompt prefill by one pass, and the seek loop conditioned on previous text (an extension) -----------------------
 * Every decode entry point feeds its prompt's first P - 1 tokens to the self-KV cache by P - 1 decode steps (one host round
 * trip each).  Prefill mode 1 replaces them by ONE teacher-forced pass over all prompt positions on the matrix cores that
 * writes the paged cache and the position tables directly; the chained steps continue from there.  The pass leaves the
 * session where the steps leave it, up to rounding (exact-f32 MFMA GEMMs instead of f32 GEMVs).
 * mode: 0 (default; a pooled session starts there) steps, 1 the pass.  It applies to wb_session_decode,
 * wb_session_decode_prompt, wb_session_decode_sample, wb_session_decode_timestamps and wb_session_decode_timestamps_beam on a
 * fresh or rewound session.  WHISPER_HIP_PREFILL_PASS=0 forces steps everywhere.  Any other mode -> WB_ERR_ARG. */
int wb_session_set_prefill(wb_session* s, int mode);
/* The pass alone, on a fresh or rewound session: equivalent to the n calls wb_session_step(tokens[t], parent = t == 0 ? -1 :
 * a, window = the a-th active window, k = 0), t = 0 .. n - 1, with one synchronisation at its end; wb_session_step continues
 * behind it with parent = a.  active: u8 [W] or NULL (all).  n == 0 is a no-op.  A session that is not at step 0 ->
 * WB_ERR_STATE; a token outside the vocabulary -> WB_ERR_ARG; n >= the cache's capacity (min(n_text_ctx, 448) unless a decode
 * call reserved less) -> WB_ERR_SHAPE; nothing is launched in any of these. */
int wb_session_prefill(wb_session* s, const int32_t* tokens, int32_t n, const uint8_t* active);
/* Test hook: the store kernel of the pass alone on caller arrays in host memory.  qkv [nA * n][ld] (row a * n + p; ld >= 3 d,
 * d and ld multiples of 4); Kc / Vc [Lmax * S][d] and tabs [2][S][Lmax] are read AND written: the kernel's writes land in
 * the caller's contents.  It copies columns [d, 2d) / [2d, 3d) of row a * n + p to row p * S + a of Kc / Vc and sets
 * tabs[(n - 1) & 1][a][p] = p * S + a; nothing else.  `device` only hosts the buffers. */
int wb_prefill_store(int device, const float* qkv, int32_t nA, int32_t n, int32_t d, int32_t ld, int32_t S, int32_t Lmax,
                     float* Kc, float* Vc, int32_t* tabs);
/* Test hook: the cached self-attention rows of live slot `slot` (a row of the last step or prefill) in decoder layer `layer`,
 * positions [0, n_pos), read through the slot's current position table: K (pre-scaled by (d / heads)^-0.25) and V, [n_pos][d]. */
int wb_session_self_kv(wb_session* s, int32_t layer, int32_t slot, int32_t n_pos, float* K, float* V);
/* wb_waveform_to_segments_beam (bp NULL: wb_waveform_to_segments, greedy or best-of-n as tp says) with every window's prompt
 * conditioned on the text before it -- Whisper transcribe()'s condition_on_previous_text / initial_prompt.  The rule:
 *   - `history` starts as initial_prompt [n_initial_prompt].
 *   - The prompt of a window is [tok_start_of_prev] + the last min(cap, len(history)) tokens of history + prompt, with
 *     cap = max_prompt_tokens < 0 ? n_text_ctx / 2 - 1 : max_prompt_tokens; when that history section is empty the prompt is
 *     `prompt` alone, without tok_start_of_prev.
 *   - After a window, the generated tokens its segments cover -- gen[seg_begin[0], seg_end[k - 1]): timestamps included,
 *     end-of-text excluded, nothing when it has no segment -- are appended to history.  Tokens behind the last closed pair
 *     are not appended (the next window decodes them again).
 *   - Then history is emptied if condition_on_previous_text == 0 or tp->temperature > 0.5 (so with conditioning off the
 *     initial prompt reaches the first window only).
 * A window whose prompt carries a history section is decoded in prefill mode 1, any other in mode 0: with conditioning off
 * and no initial prompt the result is wb_waveform_to_segments' bit for bit.  max_depth is clamped by the decode calls as
 * always (capacity - (prompt length - 1)).  win_seek / win_prompt_len [win_cap] (may be NULL): per window its first sample
 * and the length of its prompt.  tok_start_of_prev or an initial_prompt token outside [0, n_vocab) -> WB_ERR_ARG before
 * anything is encoded. */
int wb_waveform_to_segments_conditioned(wb_model* m, const float* pcm, int64_t n, int sample_rate, const wb_decode_params* p,
                                        const wb_timestamp_params* tp, const wb_beam_params* bp, const uint8_t* suppress,
                                        const uint8_t* suppress_first, const int32_t* prompt, int32_t prompt_len,
                                        int32_t tok_start_of_prev, int32_t condition_on_previous_text, int32_t max_prompt_tokens,
                                        const int32_t* initial_prompt, int32_t n_initial_prompt, float* seg_start,
                                        float* seg_end_time, int32_t* seg_tok_begin, int32_t* seg_tok_end, int32_t seg_cap,
                                        int32_t* n_segments, int32_t* text_tokens, int64_t text_cap, int64_t* n_text_tokens,
                                        int32_t* n_windows, int64_t* win_seek, int32_t* win_prompt_len, int32_t win_cap);

/* The reference's retired greedy decoder kept its repetition detectors (transcribe.rs:385-447, dead code there):
 *   wb_first_repetition_end        :385-393   (period > n, a usize underflow panic there -> WB_ERR_ARG)
 *   wb_repetition_period           :395-417   returns the period, 0 for None
 *   wb_find_repeated_tokens_index  :419-447   returns 1 and the (first, second) window indices, else 0
 * They serve the optional legacy greedy mode (whisper_burn_amd.legacy.legacy_greedy over the session API). */
int64_t wb_first_repetition_end(const int32_t* tokens, int64_t n, int64_t period);
int64_t wb_repetition_period(const int32_t* tokens, int64_t n, int64_t min_repetitions);
int wb_find_repeated_tokens_index(const int32_t* tokens, int64_t n, int64_t window_size, int64_t min_repeat_count,
                                  int64_t* first_repeat_index, int64_t* end);

/* The constant tables of the frontend, built on the host in the reference's f32 op order: periodic Hann window
 * (hann_window_device, audio.rs:272-278) and the dense [80][201] Slaney filterbank (get_mel_filters_device,
 * audio.rs:67-143; the kernel keeps it sparse).  No GPU needed; for table-vs-oracle tests. */
int wb_mel_constants(double sample_rate, float* hann400, float* filters_80x201);

/* The dense [n_mels][201] filterbank of the frontend instance for n_mels rows, as its kernel uses it (host only).
 * n_mels = 80: the table of wb_mel_constants, bit for bit.  n_mels = 128 (large-v3 and later): the Slaney bank designed in
 * f64 as librosa evaluates it and rounded once to f32 -- the reference has no 128-row recipe, and its f32 op order loses
 * too much on the narrow low rows.  Any other n_mels -> WB_ERR_ARG; a sample rate whose rows outgrow the kernel's tap
 * capacity (16 per row at 80 rows, 12 at 128) -> WB_ERR_SHAPE. */
int wb_mel_filterbank(double sample_rate, int n_mels, float* filters);

/* The dense DFT table of the reference-recipe frontend (WB_FRONTEND_REFERENCE), built on the host as the kernel uses it
 * (before its padding to 416 rows): [402][400], row 2k = cos(b[k][n]) * w[n], row 2k+1 = sin(b[k][n]) * (-w[n]) for
 * bin k < 201 (audio.rs:348-364), b[k][n] = f32(f32(k) * f32(2 pi / 400)) * f32(n), cos / sin of that f32 angle
 * correctly rounded to f32, w the Hann window of wb_mel_constants.  No GPU needed. */
int wb_mel_dft_table(float* table_402x400);

/* ---- measurement hooks ----------------------------------------------------------- */

/* Per-stage device time (ms, HIP events on the engine's stream) accumulated since the
 * last reset: [0]=mel [1]=encoder [2]=cross-KV [3]=decode steps [4]=number of decode
 * steps [5]=mel kernel launches [6]=logits kernel ms [7]=logits kernel launches. */
int wb_profile_enable(int on);
int wb_profile_read(double* out8, int reset);

/* Per-kernel statistics of the decode-step launches made while profiling was on: every launch carries its own
 * start / stop HIP events (the dispatch's begin -> end, what `rocprofv3 --kernel-trace` reports) and the
 * algorithmic bytes it streams (weights + cached K/V).  Fills at most `cap` entries, returns the number of
 * kernel classes that ran (may exceed cap).  New: the reference has no profiling hooks. */
typedef struct wb_kernel_stat {
  char name[96];
  int64_t calls;
  double total_ms;      /* sum of the launches' own durations */
  double algo_bytes;    /* sum of their algorithmic bytes     */
} wb_kernel_stat;
int wb_profile_kernels(wb_kernel_stat* out, int cap, int reset);

const char* wb_last_error(void);
const char* wb_version(void);

#ifdef __cplusplus
}
#endif
#endif /* WHISPER_HIP_H */
