"""GPU, end to end: token log-probabilities, no-speech probability and language detection (wb_score_tokens / wb_session_score /
wb_waveform_to_token_scores / wb_waveform_detect_language) against the oracle.

  C1  log-probs and probes vs OracleWhisper.forward_decoder + oracle.model.log_softmax (special mask for l <= 5), both sides
      fed the oracle's f32 encoder output: |hip - o32| <= 1e-3 (the project's asserted log-prob gate) on
      the micro model (128, 2, 2, 1031; seed 77) and the workloads tiny_bench and large_window with the committed golden rows.
      For scale: on the micro fixtures the f32 oracle is 1.1e-5 from its f64 twin on log-probs of magnitude 25 - 33.
  C2  two ragged rows (len 448 and 1) in one call: NaN exactly at entry 0 and past len.
  C3  the session entry and the stateless entry agree within 2e-3 (each is within 1e-3 of the oracle); a second session
      call is bit-identical.
  C4  consistency with the decode itself: top-1 log-probs of Session.step vs Session.score of the resulting rows, <= 2e-3;
      the first two generated tokens are the masked ones.
  C5  wb_waveform_to_token_scores: tokens and stitched stream of wb_waveform_to_tokens, avg_logprob = the mean of its own
      entries, no_speech_prob within 1e-3 of the oracle's exp.
  C6  language detection: win_probs within 1e-3 of the oracle's restricted softmax, best = the f64 oracle's argmax (whose
      top-2 gap of mean_probs is first asserted to be >= 0.05).
  C7  launch structure: one score_logits and one score_merge launch per call; the partials are vs x R float4; the device
      memory a call takes is below half of R x V floats.  (Only tagged launches are counted: the decoder GEMMs of a
      stateless pass carry no tag, so it is the memory delta, not the launch names, that rules out an [R][V] logits buffer.)
  C8  the CLI: --scores and `auto` produce their files, a run without them writes what it always wrote.
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

import parity_log
import parity_util as pu
import score_ref as sr
import whisper_burn_amd as wb
import workloads
from oracle.model import OracleWhisper
from whisper_burn_amd import _lib, synth

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_outputs.npz")
TOL = 1e-3


def rows_of(name):
    g = np.load(GOLD)
    t, n = g[f"{name}_tokens"], g[f"{name}_lens"]
    return [t[i, :n[i]].tolist() for i in range(len(n))]


@functools.lru_cache(maxsize=None)
def micro(n_vocab=1031, seed=77):
    """(weights, f32 oracle, special tokens, audio, the oracle's window mels, its f32 encoder outputs): computed once."""
    dims = synth.micro_dims(n_state=128, n_head=2, n_layer=2, n_vocab=n_vocab) if n_vocab == 1031 else \
        synth.micro_dims(n_state=64, n_head=1, n_layer=1, n_vocab=n_vocab)
    w = synth.synth_weights(dims, seed=seed)
    o32 = OracleWhisper(w)
    st = wb.SpecialTokens.for_vocab(n_vocab)
    audio = synth.synth_audio(16000 * 20, 4)
    mels = pu.window_mels(o32, audio)
    encs = [o32.forward_encoder(m)[0].numpy() for m in mels]
    return w, o32, st, audio, mels, encs


def lang_ids(st):
    """Ten ids of the synthetic special range (the last 16 ids), standing in for language tokens."""
    V = len(st.is_special)
    return list(range(V - 14, V - 4))


def _check_rows(name, eng, o32, st, rows, encs):
    """C1 for rows with their own encoder outputs (one call per row: the rows' C differ)."""
    nsp = len(st.is_special) - 9
    probe_ids = [nsp] + lang_ids(st)
    worst = mag = 0.0
    for i, (row, enc) in enumerate(zip(rows, encs)):
        lp, plp = eng.score_tokens([row], enc[None], is_special=st.is_special, mask_until_len=5, probe_ids=probe_ids)
        ref, pref = sr.oracle_scores(o32, st.is_special, enc, row, 5, probe_ids, 0)
        assert np.isnan(lp[0, 0]) and not np.isnan(lp[0, 1:]).any()
        assert np.isneginf(lp[0, 1:4]).all() and np.isneginf(ref[1:4]).all()        # the prompt's specials under the mask
        e = max(float(sr.absdiff(lp[0, 1:], ref[1:]).max()), float(np.abs(plp[0] - pref).max()))
        fin = np.isfinite(ref)
        mag = max(mag, float(np.abs(ref[fin]).max()), float(np.abs(pref).max()))
        print(f"score C1 {name} row {i}: len {len(row)} worst |hip - o32| {e:.3e}")
        worst = max(worst, e)
    parity_log.record(f"score_logprobs[{name}]", worst, TOL, max_abs_logprob=mag, n_rows=len(rows))
    assert worst <= TOL, (name, worst)


def test_logprobs_micro_model():
    w, o32, st, audio, _, encs = micro()
    eng = wb.Whisper.from_tensors(w)
    _, wins = wb.waveform_to_tokens(eng, st, audio, 16000, 1, 40)
    _check_rows("micro", eng, o32, st, wins, encs)
    eng.close()


@pytest.mark.parametrize("name", ["tiny_bench", "large_window"])
def test_logprobs_of_workload(name):
    wl = workloads.WORKLOADS[name]
    w = wl.weights()
    eng, o32 = wb.Whisper.from_tensors(w), OracleWhisper(w)
    st = wb.SpecialTokens.for_vocab(eng.dims["n_vocab"])
    encs = [o32.forward_encoder(m)[0].numpy() for m in pu.window_mels(o32, wl.audio())]
    _check_rows(name, eng, o32, st, rows_of(name), encs)
    eng.close()


def test_ragged_rows_in_one_call():
    w, o32, st, _, _, encs = micro()
    eng = wb.Whisper.from_tensors(w)
    g = np.random.default_rng(448)
    lens = [448, 1]
    toks = np.zeros((2, 448), dtype=np.int32)
    for i, n in enumerate(lens):
        toks[i, :n] = g.integers(0, 1015, n)
    enc = np.stack([encs[0], encs[0]])
    lp, plp = eng.score_tokens(toks, enc, lens=lens, is_special=st.is_special, mask_until_len=5, probe_ids=[1022])
    assert np.isnan(lp[0, 0]) and not np.isnan(lp[0, 1:]).any()
    assert np.isnan(lp[1]).all()                                    # len 1: entry 0 and everything past it
    for i, n in enumerate(lens):
        ref, pref = sr.oracle_scores(o32, st.is_special, enc[i], toks[i, :n], 5, [1022], 0)
        e = max(float(sr.absdiff(lp[i, 1:n], ref[1:]).max()) if n > 1 else 0.0, float(np.abs(plp[i] - pref).max()))
        print(f"score C2 row {i}: len {n} worst {e:.3e}")
        parity_log.record(f"score_logprobs[ragged/{i}]", e, TOL, n_rows=n)
        assert e <= TOL
    eng.close()


def _micro_session(eng, st, audio, depth=24):
    wlen = wb.max_waveform_samples(eng.max_mel_frames() - 10)
    starts, lens = wb.window_extents(len(audio), 16000, wlen)
    sess = wb.Session.begin(eng, audio, starts, lens, max_beams=1)
    sess.set_special_mask(st.is_special)
    return sess, starts, lens


def test_session_entry_against_stateless_entry():
    w, o32, st, audio, _, _ = micro()
    eng = wb.Whisper.from_tensors(w)
    sess, _, _ = _micro_session(eng, st, audio)
    rows = sess.decode(wb.decode_params(st, 1, 24))
    ids = lang_ids(st)
    a, pa = sess.score(rows, mask_until_len=5, probe_ids=ids)
    b, pb = sess.score(rows, mask_until_len=5, probe_ids=ids)
    assert np.array_equal(a.view(np.int32), b.view(np.int32)) and np.array_equal(pa.view(np.int32), pb.view(np.int32))
    worst = 0.0
    for i, row in enumerate(rows):
        enc = sess.encoder_output(i)
        c, pc = eng.score_tokens([row], enc[None], is_special=st.is_special, mask_until_len=5, probe_ids=ids)
        n = len(row)
        assert np.isnan(a[i, 0]) and np.isnan(a[i, n:]).all()
        worst = max(worst, float(sr.absdiff(a[i, 1:n], c[0, 1:]).max()), float(np.abs(pa[i] - pc[0]).max()))
        ref, pref = sr.oracle_scores(o32, st.is_special, enc, row, 5, ids, 0)
        assert sr.absdiff(a[i, 1:n], ref[1:]).max() <= TOL and np.abs(pa[i] - pref).max() <= TOL
    parity_log.record("score_session_vs_stateless[micro]", worst, 2 * TOL, n_rows=len(rows))
    assert worst <= 2 * TOL
    # the scoring pass ran on the session's workspace and left the decode alone
    sess.close()
    fresh, _, _ = _micro_session(eng, st, audio)
    a0 = fresh.score(rows, mask_until_len=5)                         # before any decode: settles the encode pass's range check
    assert np.array_equal(a0.view(np.int32), a.view(np.int32))
    assert fresh.decode(wb.decode_params(st, 1, 24)) == rows
    fresh.close()
    eng.close()


def test_scores_agree_with_the_decode_steps():
    w, _, st, audio, _, _ = micro()
    eng = wb.Whisper.from_tensors(w)
    sess, starts, _ = _micro_session(eng, st, audio)
    W = len(starts)
    prompt = [st.start_of_transcript, st.language, st.transcribe, st.no_timestamps]
    rows = [list(prompt) for _ in range(W)]
    step_lp = [[] for _ in range(W)]
    n_gen = 12
    for p in range(3 + n_gen):
        toks = [r[p] for r in rows]
        length = p + 1                                                # tokens in the sequence once this one is fed
        k = 1 if p >= 3 else 0
        ids, lps = sess.step(toks, [-1] * W if p == 0 else list(range(W)), list(range(W)),
                             apply_special_mask=(k == 1 and length <= 5), k=k)
        if k:
            for i in range(W):
                rows[i].append(int(ids[i, 0]))
                step_lp[i].append(float(lps[i, 0]))
    sess.close()
    sess, _, _ = _micro_session(eng, st, audio)
    lp = sess.score(rows, mask_until_len=5)
    lp0 = sess.score(rows, mask_until_len=0)
    worst = float(np.abs(lp[:, 4:] - np.asarray(step_lp, dtype=np.float32)).max())
    print(f"score C4: worst |score - step top-1| {worst:.3e}")
    parity_log.record("score_vs_decode_steps[micro]", worst, 2 * TOL, n_rows=W * n_gen)
    assert worst <= 2 * TOL
    # entries 4 and 5 (sequence length <= 5 when they were chosen) are the masked ones: without the mask the specials take
    # probability mass and the log-prob drops; from entry 6 on the mask plays no part
    assert (lp[:, 4:6] >= lp0[:, 4:6]).all() and (lp[:, 4:6] > lp0[:, 4:6]).any() and np.array_equal(lp[:, 6:].view(np.int32), lp0[:, 6:].view(np.int32))
    sess.close()
    eng.close()


def test_waveform_to_token_scores():
    w, o32, st, audio, _, _ = micro()
    eng = wb.Whisper.from_tensors(w)
    nsp = len(st.is_special) - 9
    full, wins = wb.waveform_to_tokens(eng, st, audio, 16000, 1, 24)
    r = wb.waveform_to_token_scores(eng, st, audio, 16000, 1, 24, no_speech=nsp)
    assert r["tokens"] == full and r["win_tokens"] == wins and len(r["logprobs"]) == len(full)
    sess, _, _ = _micro_session(eng, st, audio)
    ref_lp, ref_probe = sess.score(wins, mask_until_len=5, probe_ids=[nsp])
    worst = 0.0
    for i, row in enumerate(wins):
        lp = r["win_logprobs"][i]
        assert np.array_equal(lp.view(np.int32), ref_lp[i, :len(row)].view(np.int32))
        assert abs(float(r["avg_logprob"][i]) - float(np.mean(lp[4:].astype(np.float64)))) <= 1e-6 * max(1.0, abs(float(r["avg_logprob"][i])))
        _, pref = sr.oracle_scores(o32, st.is_special, sess.encoder_output(i), row, 5, [nsp], 0)
        worst = max(worst, abs(float(r["no_speech_prob"][i]) - float(np.exp(pref[0]))))
        assert 0.0 <= r["no_speech_prob"][i] <= 1.0
    parity_log.record("score_no_speech_prob[micro]", worst, TOL, n_rows=len(wins))
    assert worst <= TOL
    # the stitched log-probs went through the stitch of the tokens themselves
    wt = np.zeros(ref_lp.shape, dtype=np.int32)
    for i, row in enumerate(wins):
        wt[i, :len(row)] = row
    st_t, st_lp = wb.stitch_windows(wt, [len(row) for row in wins], times=ref_lp)
    assert st_t == full and np.array_equal(st_lp, r["logprobs"], equal_nan=True)
    r0 = wb.waveform_to_token_scores(eng, st, audio, 16000, 1, 24)
    assert r0["tokens"] == full and np.isnan(r0["no_speech_prob"]).all()
    sess.close()
    eng.close()


# f64 oracle, real encoder output of the 20 s audio (CPU): top-2 gap of mean_probs 0.97 for (1031, seed 77) and 0.46 for
# (263, seed 8); seed 5 of the 263-id fixture falls to 0.049 there, so it is not used
@pytest.mark.parametrize("n_vocab,seed", [(1031, 77), (263, 8)])
def test_language_detection(n_vocab, seed):
    w, o32, st, audio, mels, encs32 = micro(n_vocab, seed)
    o64 = OracleWhisper(w, dtype=torch.float64)
    ids = lang_ids(st)
    sot = st.start_of_transcript

    def restricted(oracle, enc):
        _, p = sr.oracle_scores(oracle, st.is_special, enc, [sot], 0, ids, 0)
        e = np.exp(p - p.max())
        return e / e.sum()

    win64 = np.stack([restricted(o64, o64.forward_encoder(m.to(torch.float64))[0].numpy()) for m in mels])
    mean64 = win64.mean(axis=0)
    top2 = np.sort(mean64)[-2:]
    print(f"score C6 V {n_vocab}: f64 oracle top-2 gap of mean_probs {top2[1] - top2[0]:.3f}")
    assert top2[1] - top2[0] >= 0.05, "the fixture is a near-tie: choose another seed"
    win32 = np.stack([restricted(o32, e) for e in encs32])
    eng = wb.Whisper.from_tensors(w)
    best, mean, win = wb.detect_language(eng, ids, audio, 16000, sot=sot, max_windows=0)
    worst = float(np.abs(win - win32).max())
    parity_log.record(f"score_language_probs[V{n_vocab}]", worst, TOL, n_rows=len(mels), gap=float(top2[1] - top2[0]))
    assert win.shape == win32.shape and worst <= TOL
    assert best == int(np.argmax(mean64)) and np.abs(mean - win.mean(axis=0)).max() <= 1e-6
    # the first window alone, and the session form of the same thing
    b1, m1, w1 = wb.detect_language(eng, ids, audio, 16000, sot=sot, max_windows=1)
    assert w1.shape[0] == 1 and np.array_equal(w1[0], win[0]) and b1 == int(np.argmax(win[0]))
    sess, _, _ = _micro_session(eng, st, audio)
    b2, m2, w2 = sess.detect_language(sot, ids)
    assert b2 == best and np.abs(w2 - win).max() <= 1e-6
    # the SpecialTokens form: its own language ids (two in the synthetic layout) and start-of-transcript
    assert len(st.language_ids) == 2 and set(st.language_ids) <= set(ids)
    b3, m3, w3 = wb.detect_language(eng, st, audio, 16000, max_windows=0)
    b4, m4, w4 = wb.detect_language(eng, list(st.language_ids), audio, 16000, sot=sot, max_windows=0)
    assert b3 == b4 and np.array_equal(w3, w4) and w3.shape == (len(mels), 2)
    sub = win[:, [ids.index(t) for t in st.language_ids]].astype(np.float64)
    assert np.abs(w3 - sub / sub.sum(axis=1, keepdims=True)).max() <= 1e-5
    sess.close()
    eng.close()


def test_launch_structure_and_memory():
    """One score_logits and one score_merge launch per call whatever the rows, and the merge reads vs x R float4 partials.
    The launch names cannot show that no [R][V] logits GEMM ran (the stateless pass's GEMMs carry no profiling tag); the
    device memory the first call takes -- every workspace of the pass included -- does: it is far below R x V floats."""
    wl = workloads.WORKLOADS["tiny_bench"]
    eng = wb.Whisper.from_tensors(wl.weights())
    V = eng.dims["n_vocab"]
    st = wb.SpecialTokens.for_vocab(V)
    g = np.random.default_rng(3)
    enc = (g.standard_normal((3, 64, eng.dims["n_text_state"])) * 0.3).astype(np.float32)
    toks = g.integers(0, 50000, (3, 448)).astype(np.int32)
    lib = _lib.load()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    lib.wb_profile_enable(1)
    try:
        def stats(fn):
            _lib.profile_kernels(reset=True)
            fn()
            return {k["name"].split(" ")[0]: k for k in _lib.profile_kernels(reset=True)}
        s = stats(lambda: eng.score_tokens(toks, enc, is_special=st.is_special, mask_until_len=5, probe_ids=[V - 9]))
        assert {k: v["calls"] for k, v in s.items()} == {"score_logits": 1, "score_merge": 1}, s
        R = 3 * 448
        assert s["score_merge"]["algo_bytes"] <= 16 * R * 16            # the partials: vs x R float4, vs <= 16 at 42 row tiles
        free1 = torch.cuda.mem_get_info()[0]
        print(f"score C7: device memory taken by the call {(free0 - free1) / 2**20:.1f} MiB, R x V floats {R * V * 4 / 2**20:.1f} MiB")
        assert free0 - free1 < R * V * 4 // 2
        s = stats(lambda: eng.score_tokens(toks[:1, :7], enc[:1]))                                  # 1 row, 7 tokens
        assert {k: v["calls"] for k, v in s.items()} == {"score_logits": 1, "score_merge": 1}, s
        s = stats(lambda: eng.score_tokens(toks[:, :1], enc, probe_ids=lang_ids(st)))               # language detection's shape
        assert {k: v["calls"] for k, v in s.items()} == {"score_logits": 1, "score_merge": 1}, s
    finally:
        lib.wb_profile_enable(0)
    eng.close()


def test_cli_scores_and_auto(tmp_path, monkeypatch, capsys):
    import wave
    from test_tokenizer_integration import N_VOCAB, write_synthetic_tokenizer_json
    from whisper_burn_amd import dumpdir
    from whisper_burn_amd import transcribe as cli
    monkeypatch.chdir(tmp_path)
    write_synthetic_tokenizer_json(str(tmp_path / "tokenizer.json"))
    dims = synth.micro_dims(n_state=128, n_head=2, n_layer=2, n_vocab=N_VOCAB)
    weights = synth.synth_weights(dims, seed=4242)
    dumpdir.write_dump_dir(weights, str(tmp_path / "micro"))
    audio = synth.synth_audio(16000 * 6, 52)
    pcm = np.clip(np.round(audio * 32767.0), -32768, 32767).astype("<i2")
    with wave.open(str(tmp_path / "a.wav"), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(pcm.tobytes())
    assert cli.main(["transcribe", "micro", "a.wav", "en", "plain.txt"]) == 0
    plain_out = capsys.readouterr().out
    # what the library itself transcribes to: the plain run is untouched by the new options
    eng = wb.Whisper.from_tensors(weights)
    st = wb.SpecialTokens.for_vocab(N_VOCAB)
    from whisper_burn_amd.tokens import TokenizerAdapter
    bpe = TokenizerAdapter.from_file(str(tmp_path / "tokenizer.json"))
    toks, _ = wb.waveform_to_tokens(eng, st, pcm.astype(np.float32) / np.float32(32767.0), 16000)
    assert open(tmp_path / "plain.txt").read() == bpe.decode(toks, True)
    assert plain_out == "Loading waveform...\nLoading model...\nTranscription finished.\n"
    assert cli.main(["transcribe", "micro", "a.wav", "en", "scored.txt", "--scores", "scores.jsonl"]) == 0
    assert open(tmp_path / "plain.txt", "rb").read() == open(tmp_path / "scored.txt", "rb").read()
    recs = [json.loads(ln) for ln in open(tmp_path / "scores.jsonl")]
    tok_recs = [r for r in recs if "id" in r]
    win_recs = [r for r in recs if "window" in r]
    assert len(tok_recs) >= 2 and all(set(r) == {"id", "text", "logprob"} for r in tok_recs)
    assert recs == tok_recs + win_recs and [r["window"] for r in win_recs] == list(range(len(win_recs))) and win_recs
    assert all(set(r) == {"window", "avg_logprob", "no_speech_prob"} for r in win_recs)
    assert all(r["logprob"] <= 0.0 and r["id"] < N_VOCAB - 16 for r in tok_recs)
    assert " ".join(r["text"] for r in tok_recs) == open(tmp_path / "plain.txt").read()
    capsys.readouterr()
    assert cli.main(["transcribe", "micro", "a.wav", "auto", "auto.txt"]) == 0
    out = capsys.readouterr().out
    assert "Detected language: " in out and out.index("Detected language: ") < out.index("Transcription finished.")
    lang = out.split("Detected language: ")[1].split()[0]
    assert lang in ("en", "zh")                                          # the synthetic tokenizer's two language tokens
    best, _, _ = wb.detect_language(eng, [bpe.special_token("<|en|>"), bpe.special_token("<|zh|>")],
                                    pcm.astype(np.float32) / np.float32(32767.0), 16000, sot=st.start_of_transcript, max_windows=3)
    assert lang == ("en", "zh")[best]
    assert cli.main(["transcribe", "micro", "a.wav", lang, "named.txt"]) == 0
    assert open(tmp_path / "auto.txt", "rb").read() == open(tmp_path / "named.txt", "rb").read()
    eng.close()
