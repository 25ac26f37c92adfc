"""GPU, end to end: sampled decode (wb_session_decode_sample) and the decode fallback (wb_waveform_to_tokens_fallback).

  S1  sampled decode against the oracle, teacher-forced: every sample of every window (wb_session_last_samples) is put through
      ONE oracle forward (so a divergence cannot cascade); every token must equal the oracle's Gumbel-max argmax for the same
      counters unless the oracle's top-two key gap is at most delta_model = 2e-3 / T + delta_op (the 1e-3 log-prob gate of
      DESIGN.md section 5, once per candidate); at most 5 % of a run's positions may be excluded.  Micro model (64, 1, 1,
      1031) in the three launch shapes W x best_of = 3 x 1 (fused), 3 x 5 (the 16-row bucket), 4 x 5 (batch mode, both GEMM
      arithmetic modes), and the tiny.en shape of tests/workloads.py (3 windows, depth 32, best_of 1 and 5), at T = 1.0 and 0.2.
  S2  out_sum_logprob agrees with the oracle's log-probs of the same rows (S1) and with Session.score within 1e-3 per token;
      out_best is the first argmax of sum / n_text (S1).
  S3  two runs are bit-identical, two seeds differ, a second temperature / seed / attempt replays the same captured graphs
      (neither the session's graph count nor its capture counter moves) and still matches its own restatement.
  S4  `active` leaves the other windows' output untouched (S1's last call).
  S5  the fallback scenarios of tests/sample_emu_checks.py on the GPU build; `--fallback` through the CLI."""
import json

import numpy as np
import pytest

import sample_ref as sr
import whisper_burn_amd as wb
import workloads
from oracle.model import OracleWhisper
from whisper_burn_amd import synth

pytestmark = pytest.mark.gpu


def _session_checks(eng, o32, st, audio, W, best_of, depth, tag):
    starts, lens = sr.windows(eng, audio, W)
    sess = wb.Session.begin(eng, audio, starts, lens, max_beams=max(best_of, 1))
    sess.set_special_mask(st.is_special)
    p = wb.decode_params(st, 1, depth)
    rec = []
    (T1, seed1, att1), (T2, seed2, att2) = sr.SESSION_DRAWS
    r1 = sr.check_sampled_session(sess, o32, st, p, T1, seed1, att1, best_of, record=rec)
    n_graphs, n_cap = sess.graph_count(), sess.graph_captures()
    assert n_graphs >= 1 and n_cap >= n_graphs
    # S2: the sums against the scoring pass of the same session
    sr.check_sums_against_score(sess, st, p, best_of, r1[1])
    sess.rewind()
    r2 = sr.check_sampled_session(sess, o32, st, p, T1, seed1, att1, best_of)
    assert r1[0] == r2[0] and np.array_equal(r1[1], r2[1]) and np.array_equal(r1[2], r2[2])       # S3: bit-identical
    sess.rewind()
    sr.check_sampled_session(sess, o32, st, p, T2, seed2, att2, best_of, record=rec)
    assert sess.graph_count() == n_graphs and sess.graph_captures() == n_cap                     # S3: replayed, nothing captured
    sess.rewind()
    r4 = sr.check_sampled_session(sess, o32, st, p, T1, seed1 + 1, att1, best_of)
    assert r4[0] != r1[0]                                                                        # S3: another seed
    sess.rewind()
    act = np.ones(W, dtype=np.uint8)
    act[1] = 0
    sr.check_sampled_session(sess, o32, st, p, T1, seed1, att1, best_of, stream_ids=[7 * w + 100 for w in range(W)], active=act)
    print(f"sample S1 {tag} W {W} best_of {best_of}: (T, best_of, positions, excluded, mismatches) {rec}")
    sess.close()


def run_micro(W, best_of, tag="micro"):
    dims = synth.micro_dims(n_state=64, n_head=1, n_layer=1, n_vocab=1031)
    weights = synth.synth_weights(dims, seed=5)
    eng, o32 = wb.Whisper.from_tensors(weights), OracleWhisper(weights)
    st = wb.SpecialTokens.for_vocab(1031)
    _session_checks(eng, o32, st, synth.synth_audio(16000 * 3, 3), W, best_of, 20, tag)
    gemm = eng.decoder_gemm()
    eng.close()
    return gemm


@pytest.mark.parametrize("W,best_of", [(3, 1), (3, 5), (4, 5)])
def test_sampled_decode_micro_model(W, best_of):
    assert run_micro(W, best_of) == "f16x3"


def test_sampled_decode_batch_mode_exact_f32():
    """The > 16-row shape on the exact-f32 decoder GEMMs, the other arithmetic mode of batch mode (the switch is read once per
    process: a child process)."""
    import os
    import subprocess
    import sys
    env = dict(os.environ, WHISPER_HIP_DECODER_SPLIT="0")
    here = os.path.dirname(os.path.abspath(__file__))
    env["PYTHONPATH"] = os.pathsep.join([here, env.get("PYTHONPATH", "")] + sys.path)
    r = subprocess.run([sys.executable, "-c", "import test_gpu_sample as t; assert t.run_micro(4, 5, 'micro-f32') == 'f32'; print('OK f32')"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK f32" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("best_of", [1, 5])
def test_sampled_decode_tiny_en_shape(best_of):
    wl = workloads.WORKLOADS["tiny_bench"]
    weights = wl.weights()
    eng, o32 = wb.Whisper.from_tensors(weights), OracleWhisper(weights)
    st = wb.SpecialTokens.for_vocab(eng.dims["n_vocab"])
    audio = wl.audio()
    p = wb.decode_params(st, 1, 32)
    wlen = wb.max_waveform_samples(eng.max_mel_frames() - p.padding)
    starts, lens = wb.window_extents(len(audio), 16000, wlen, p.overlap_seconds)
    assert len(starts) == 3
    sess = wb.Session.begin(eng, audio, starts, lens, max_beams=best_of)
    sess.set_special_mask(st.is_special)
    rec = []
    for T, seed, att in sr.SESSION_DRAWS:
        r = sr.check_sampled_session(sess, o32, st, p, T, seed, att, best_of, record=rec)
        sr.check_sums_against_score(sess, st, p, best_of, r[1])
        sess.rewind()
    print(f"sample S1 tiny.en best_of {best_of}: (T, best_of, positions, excluded, mismatches) {rec}")
    sess.close()
    eng.close()


def test_fallback_scenarios():
    dims = synth.micro_dims(n_state=64, n_head=1, n_layer=1, n_vocab=1031, n_audio_ctx=400)
    eng = wb.Whisper.from_tensors(synth.synth_weights(dims, seed=5))
    st = wb.SpecialTokens.for_vocab(1031)
    audio = synth.synth_audio(16000 * 11, 3)
    sr.check_fallback_scenarios(eng, st, audio, wb.decode_params(st, 1, 6, overlap_seconds=1))
    sr.check_fallback_scenarios(eng, st, audio, wb.decode_params(st, 5, 6, overlap_seconds=1), best_of=5)
    eng.close()


def test_cli_fallback(tmp_path, monkeypatch, capsys):
    import wave
    from test_tokenizer_integration import N_VOCAB, write_synthetic_tokenizer_json
    from whisper_burn_amd import dumpdir
    from whisper_burn_amd import transcribe as cli
    monkeypatch.chdir(tmp_path)
    write_synthetic_tokenizer_json(str(tmp_path / "tokenizer.json"))
    dims = synth.micro_dims(n_state=128, n_head=2, n_layer=2, n_vocab=N_VOCAB)
    dumpdir.write_dump_dir(synth.synth_weights(dims, seed=4242), str(tmp_path / "micro"))
    audio = synth.synth_audio(16000 * 6, 52)
    pcm = np.clip(np.round(audio * 32767.0), -32768, 32767).astype("<i2")
    with wave.open(str(tmp_path / "a.wav"), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(pcm.tobytes())
    assert cli.main(["transcribe", "micro", "a.wav", "en", "plain.txt"]) == 0
    # every rule off: the transcript of the plain run
    off = ["--logprob-threshold", "none", "--no-speech-threshold", "none", "--compression-ratio-threshold", "none"]
    assert cli.main(["transcribe", "micro", "a.wav", "en", "off.txt", "--fallback", "--scores", "off.jsonl"] + off) == 0
    assert open(tmp_path / "plain.txt", "rb").read() == open(tmp_path / "off.txt", "rb").read()
    recs = [json.loads(ln) for ln in open(tmp_path / "off.jsonl")]
    assert recs and all(set(r) == {"window", "avg_logprob", "no_speech_prob", "temperature", "status"} for r in recs)
    assert all(r["temperature"] == 0 and r["status"] == 0 for r in recs)
    # a threshold nothing passes: every temperature of the list is used
    capsys.readouterr()
    assert cli.main(["transcribe", "micro", "a.wav", "en", "hot.txt", "--fallback", "--scores", "hot.jsonl", "--temperatures",
                     "0,0.5", "--best-of", "2", "--seed", "5", "--logprob-threshold", "1e9", "--no-speech-threshold", "none",
                     "--compression-ratio-threshold", "none"]) == 0
    recs = [json.loads(ln) for ln in open(tmp_path / "hot.jsonl")]
    assert recs and all(r["temperature"] == 0.5 and r["status"] == 1 for r in recs)
    assert cli.main(["transcribe", "micro", "a.wav", "en", "x.txt", "--fallback", "--best-of", "many"]) == 1
    # rejected while the arguments are parsed: options without --fallback, --token-times with it
    assert cli.main(["transcribe", "micro", "a.wav", "en", "x.txt", "--best-of", "2"]) == 1
    assert cli.main(["transcribe", "micro", "a.wav", "en", "x.txt", "--fallback", "--token-times", "t.jsonl"]) == 1
    assert not (tmp_path / "x.txt").exists()
