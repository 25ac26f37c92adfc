"""`python -m whisper_burn_amd.transcribe <model name> <audio file> <lang> <transcription file>`

The reference's CLI (/root/reference/src/bin/transcribe/main.rs:85-157) over the HIP engine, argument for argument:
`<model name>` is the converter's output prefix (`<name>.mpk.gz` + `<name>.cfg`, main.rs:113-126) or a dump
directory (load.rs:295), the audio must be a 16 kHz mono WAV (main.rs:41-42; 16-bit PCM is scaled by 1 / 32767 as
hound does, :44-51), `tokenizer.json` is read from the working directory (token.rs:13-19), the transcript is
written to `<transcription file>` (main.rs:151-154).  Exit code 1 with the reference's messages on bad input.

`--frontend reference` after the four positional arguments computes the log-mel with the reference's own recipe
(dense f32 DFT, wb_model_set_frontend) instead of the default exact-twiddle FFT.

`--token-times PATH` additionally writes one JSON object per line for every stitched non-special token:
`{"id", "text", "start"}` with the token's start time in seconds (2 decimals), from the decoder's cross-attention
alignment (wb_waveform_to_token_times).  Without the flag the output is what it always was.

`--scores PATH` additionally writes one JSON object per line for every stitched non-special token, `{"id", "text",
"logprob"}`, and then one per window, `{"window", "avg_logprob", "no_speech_prob"}` (wb_waveform_to_token_scores;
`no_speech_prob` is null when the tokenizer has no no-speech token, and so is any value that is not finite).  Together
with `--token-times` the audio is decoded once per option: each is one library call that decodes and then aligns / scores.

`<lang>` = `auto` detects the language from the first windows of the audio (wb_waveform_detect_language over the
language tokens the tokenizer knows) and prints it before decoding; a tokenizer without language tokens is an error.

`--fallback` switches Whisper's decode fallback on (wb_waveform_to_tokens_fallback): a window whose decode fails the
thresholds is decoded again by sampling at the next temperature, and windows without speech are left out of the transcript.
Optional with it: `--temperatures 0,0.2,...` (the first must be 0), `--best-of N`, `--seed N`, `--logprob-threshold X`,
`--no-speech-threshold X`, `--compression-ratio-threshold X` (`none` switches a rule off).  With `--scores PATH` the file then
holds the per-window lines only, and each gains `temperature` and `status` (0 accepted, 1 failed every temperature, 2 no
speech).

`--segments PATH` decodes WITH timestamp tokens (wb_waveform_to_segments: Whisper's timestamp rules on the device, the
window moves by the last decoded timestamp) and writes one JSON line per segment, {"start", "end", "text", "tokens"} with
times in seconds; the transcript is then the segments' text.  Not together with --fallback, --token-times or --scores.
With it, `--beam-size N` (1 .. 7) decodes every window by beam search under the timestamp rules
(wb_waveform_to_segments_beam: Whisper's BeamSearchDecoder on the device), optionally with `--patience X` (>= 1, default 1)
and `--length-penalty A` (default: rank by average log-prob); the three flags are rejected without `--segments`.
`--condition-on-previous-text` prompts every window with the text decoded before it (behind <|startofprev|>, Whisper's
condition_on_previous_text) and `--initial-prompt TEXT` starts that history with TEXT, encoded by the tokenizer
(wb_waveform_to_segments_conditioned; such prompts are prefilled by one pass); both are rejected without `--segments`.

One addition: with `WHISPER_HIP_RESAMPLE=1` in the environment a mono WAV of another sample rate (the bundled
22 050 Hz audio.wav, which the reference sends through `sox`, README.md:69-74) is resampled to 16 kHz on the GPU
(wb_resample_dev) instead of being rejected.
"""
from __future__ import annotations

import os
import sys

from .tokens import LANGUAGES  # noqa: E402  (token.rs:50-60)


def main(argv=None) -> int:
    argv = list(sys.argv if argv is None else argv)
    if len(argv) < 5:
        print(f"Usage: {argv[0]} <model name> <audio file> <lang> <transcription file>", file=sys.stderr)
        return 1
    model_name, wav_file, lang, text_file = argv[1:5]
    frontend = None
    times_file = None
    scores_file = None
    segments_file = None
    extra = argv[5:]
    usage = (f"Usage: {argv[0]} <model name> <audio file> <lang> <transcription file> [--frontend fft|reference] "
             f"[--token-times PATH] [--scores PATH] [--segments PATH [--beam-size N [--patience X] [--length-penalty A]] [--condition-on-previous-text] [--initial-prompt TEXT]] [--fallback [--temperatures T0,T1,..] [--best-of N] [--seed N] "
             f"[--logprob-threshold X] [--no-speech-threshold X] [--compression-ratio-threshold X]]")
    fallback = False
    fb = {}                                     # keyword arguments of FallbackParams given on the command line
    fb_opts = {"--temperatures": ("temperatures", lambda v: [float(t) for t in v.split(",")]), "--best-of": ("best_of", int),
               "--seed": ("seed", int), "--logprob-threshold": ("logprob_threshold", float),
               "--no-speech-threshold": ("no_speech_threshold", float),
               "--compression-ratio-threshold": ("compression_ratio_threshold", float)}
    beam = {}                                   # keyword arguments of BeamParams given on the command line
    beam_opts = {"--beam-size": ("beam_size", int), "--patience": ("patience", float), "--length-penalty": ("length_penalty", float)}
    condition = False
    initial_prompt = None
    while extra:                                # (other trailing arguments are ignored, as before)
        if extra[0] == "--condition-on-previous-text":
            condition = True
            extra = extra[1:]
        elif extra[0] == "--initial-prompt":
            if len(extra) < 2:
                print(usage, file=sys.stderr)
                return 1
            initial_prompt = extra[1]
            extra = extra[2:]
        elif extra[0] in beam_opts:
            key, conv = beam_opts[extra[0]]
            try:
                beam[key] = conv(extra[1])
            except (IndexError, ValueError):
                print(usage, file=sys.stderr)
                return 1
            extra = extra[2:]
        elif extra[0] == "--fallback":
            fallback = True
            extra = extra[1:]
        elif extra[0] in fb_opts:
            key, conv = fb_opts[extra[0]]
            try:
                fb[key] = None if key.endswith("threshold") and extra[1] == "none" else conv(extra[1])
            except (IndexError, ValueError):
                print(usage, file=sys.stderr)
                return 1
            extra = extra[2:]
        elif extra[0] in ("--frontend", "--token-times", "--scores", "--segments"):
            if len(extra) < 2 or (extra[0] == "--frontend" and extra[1] not in ("fft", "reference")):
                print(usage, file=sys.stderr)
                return 1
            if extra[0] == "--frontend":
                frontend = extra[1]
            elif extra[0] == "--scores":
                scores_file = extra[1]
            elif extra[0] == "--segments":
                segments_file = extra[1]
            else:
                times_file = extra[1]
            extra = extra[2:]
        else:
            extra = extra[1:]
    if fb and not fallback:
        print("The fallback options (--temperatures, --best-of, --seed, --*-threshold) need --fallback\n" + usage, file=sys.stderr)
        return 1
    if beam and (segments_file is None or "beam_size" not in beam):
        print("--beam-size / --patience / --length-penalty (beam search under the timestamp rules) need --segments and --beam-size\n"
              + usage, file=sys.stderr)
        return 1
    if (condition or initial_prompt is not None) and segments_file is None:
        print("--condition-on-previous-text / --initial-prompt (prompts conditioned on previous text) need --segments\n" + usage,
              file=sys.stderr)
        return 1
    if fallback and times_file is not None:
        print("--token-times is not available together with --fallback\n" + usage, file=sys.stderr)
        return 1
    if segments_file is not None and (fallback or times_file is not None or scores_file is not None):
        print("--segments (decoding with timestamp tokens) is not available together with --fallback, --token-times or --scores\n"
              + usage, file=sys.stderr)
        return 1
    if lang != "auto" and lang not in LANGUAGES:
        print(f"Invalid language abbreviation: {lang}", file=sys.stderr)
        return 1
    import whisper_burn_amd as wb
    from .tokens import TokenizerAdapter

    print("Loading waveform...")
    try:
        if os.environ.get("WHISPER_HIP_RESAMPLE", "0") == "1":
            waveform, sample_rate = wb.load_audio_waveform(wav_file, any_rate=True)
            if sample_rate != 16000:
                print(f"Resampling {sample_rate} Hz -> 16000 Hz...")
                waveform, sample_rate = wb.resample(waveform, sample_rate, 16000), 16000
        else:
            waveform, sample_rate = wb.load_audio_waveform(wav_file)      # asserts 16 kHz mono like main.rs:41-42
    except Exception as e:                                                 # noqa: BLE001
        print(f"Failed to load audio file: {e}", file=sys.stderr)
        return 1
    try:
        bpe = TokenizerAdapter.from_file("tokenizer.json")
    except Exception as e:                                                 # noqa: BLE001
        print(f"Failed to load tokenizer: {e}", file=sys.stderr)
        return 1
    known, sot = [], None
    if lang == "auto":
        known = bpe.language_tokens()
        sot = bpe.special_token("<|startoftranscript|>")
        if not known or sot is None:
            print("Cannot detect the language: the tokenizer has no language tokens (an English-only vocabulary); "
                  "name the language instead of 'auto'", file=sys.stderr)
            return 1
    print("Loading model...")
    try:
        if os.path.isdir(model_name):
            whisper = wb.Whisper.load_dump_dir(model_name)
        else:
            whisper = wb.Whisper.load_burn_record(model_name + ".mpk.gz", model_name + ".cfg")
    except Exception as e:                                                 # noqa: BLE001
        print(f"Failed to load whisper model file: {e}", file=sys.stderr)
        return 1
    if frontend is not None:
        whisper.set_frontend(frontend)

    class Bpe:                                                             # what waveform_to_text needs (transcribe.rs:23-29)
        def special_tokens(self, language):
            return bpe.special_tokens(language)

        def decode(self, tokens, skip_special):
            return bpe.decode(tokens, skip_special)

    if lang == "auto":
        try:
            best, probs, _ = wb.detect_language(whisper, [t for _, t in known], waveform, sample_rate, sot=int(sot),
                                                max_windows=3)
        except Exception as e:                                             # noqa: BLE001
            print(f"Error during language detection: {e}", file=sys.stderr)
            return 1
        lang = known[best][0]
        print(f"Detected language: {lang} (p = {float(probs[best]):.3f})")

    token_times = None
    scores = None
    fb_result = None
    segments = None
    try:
        if segments_file is not None:
            # decoding WITH timestamp tokens: the window moves by the last decoded timestamp, the text is the segments' text
            from .tokens import default_suppress
            st = bpe.special_tokens(lang)
            if st.n_timestamps == 0:
                raise ValueError("the tokenizer has no timestamp tokens (<|0.00|> ...)")
            sup, sup_first = default_suppress(st, bpe)
            init = None
            if initial_prompt is not None and initial_prompt.strip():       # Whisper: tokenizer.encode(" " + initial_prompt.strip())
                init = bpe.encode(" " + initial_prompt.strip())
            if (condition or init) and st.start_of_prev < 0:
                raise ValueError("the tokenizer has no <|startofprev|> token")
            segments, _tokens, _ = wb.waveform_to_segments(whisper, st, waveform, sample_rate, suppress=sup, suppress_first=sup_first,
                                                           beam=wb.BeamParams(**beam) if beam else None,
                                                           condition_on_previous_text=condition, initial_prompt=init)
            text = bpe.decode(_tokens, True)
        elif fallback:
            st = bpe.special_tokens(lang)
            fb_result = wb.waveform_to_tokens_fallback(whisper, st, waveform, sample_rate,
                                                       fallback=wb.FallbackParams(tok_no_speech=st.no_speech, **fb),
                                                       ratio=wb.ratio_from_tokenizer(bpe))
            _tokens = fb_result["tokens"]
            text = bpe.decode(_tokens, True)
        elif times_file is None and scores_file is None:
            text, _tokens = wb.waveform_to_text(whisper, Bpe(), lang, waveform, sample_rate)
        else:
            st = bpe.special_tokens(lang)
            if times_file is not None:
                _tokens, token_times, _, _ = wb.waveform_to_token_times(whisper, st, waveform, sample_rate)
            if scores_file is not None:
                scores = wb.waveform_to_token_scores(whisper, st, waveform, sample_rate, no_speech=st.no_speech)
                _tokens = scores["tokens"]
            text = bpe.decode(_tokens, True)
    except Exception as e:                                                 # noqa: BLE001
        print(f"Error during transcription: {e}", file=sys.stderr)
        return 1
    try:
        with open(text_file, "w") as fh:
            fh.write(text)
    except OSError as e:
        print(f"Error writing transcription file: {e}", file=sys.stderr)
        return 1
    if segments_file is not None:
        import json
        try:
            with open(segments_file, "w") as fh:
                for seg in segments:
                    fh.write(json.dumps({"start": round(seg["start"], 2), "end": round(seg["end"], 2),
                                         "text": bpe.decode(seg["tokens"], True), "tokens": [int(t) for t in seg["tokens"]]}) + "\n")
        except OSError as e:
            print(f"Error writing segments file: {e}", file=sys.stderr)
            return 1
    if times_file is not None:
        import json
        import math
        try:
            with open(times_file, "w") as fh:
                for tok, t in zip(_tokens, token_times):
                    if st.is_special[tok] or math.isnan(t):
                        continue
                    fh.write(json.dumps({"id": int(tok), "text": bpe.decode([tok], True), "start": round(float(t), 2)}) + "\n")
        except OSError as e:
            print(f"Error writing token times file: {e}", file=sys.stderr)
            return 1
    if scores_file is not None:
        import json
        import math

        def num(x):
            return float(x) if math.isfinite(float(x)) else None         # (NaN: no value; -inf cannot be JSON either)
        try:
            with open(scores_file, "w") as fh:
                if fb_result is not None:
                    # (the fallback call returns no per-token log-probs: the file holds the per-window lines only)
                    r = fb_result
                    for w in range(len(r["status"])):
                        fh.write(json.dumps({"window": w, "avg_logprob": num(r["avg_logprob"][w]),
                                             "no_speech_prob": num(r["no_speech_prob"][w]),
                                             "temperature": num(r["temperature"][w]), "status": int(r["status"][w])}) + "\n")
                else:
                    for tok, lp in zip(scores["tokens"], scores["logprobs"]):
                        if st.is_special[tok]:
                            continue
                        fh.write(json.dumps({"id": int(tok), "text": bpe.decode([tok], True), "logprob": num(lp)}) + "\n")
                    for w, (a, n) in enumerate(zip(scores["avg_logprob"], scores["no_speech_prob"])):
                        fh.write(json.dumps({"window": w, "avg_logprob": num(a), "no_speech_prob": num(n)}) + "\n")
        except OSError as e:
            print(f"Error writing scores file: {e}", file=sys.stderr)
            return 1
    print("Transcription finished.")
    return 0


if __name__ == "__main__":
    sys.exit(main())
