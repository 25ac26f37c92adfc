"""Driven by tests/test_score_emu.py in a subprocess with WHISPER_HIP_LIB = lib/libwhisper_hip_emu.so: score.hip and its host
side executed through the hipemu functional model at micro shapes, compared with tests/score_ref.py and the oracle.  A check
of the kernel sources' logic on a machine without a GPU; tests/test_gpu_score_kernel.py / test_gpu_score.py are the parity
tests proper."""
import sys

import numpy as np
import torch

import score_ref as sr
import whisper_burn_amd as wb
from oracle.model import OracleWhisper
from whisper_burn_amd import _lib, synth

V = 263
TOL = 1e-3               # the project's asserted log-prob gate


def _micro():
    dims = synth.micro_dims(n_state=64, n_head=1, n_layer=1, n_vocab=V)
    weights = synth.synth_weights(dims, seed=5)
    return weights, wb.Whisper.from_tensors(weights)


def _enc(o32, C, seed):
    g = np.random.default_rng(seed)
    mel = torch.from_numpy(g.standard_normal((1, 80, 2 * C)).astype(np.float32) * 0.5)
    return o32.forward_encoder(mel)[0].numpy()


def check_hook():
    for shape in sr.SHAPES[:2]:
        for case in sr.make_cases(shape):
            sr.check_hook_case(case)
    sr.check_hook_nan_row((5, 64, 263, 0))
    # run-to-run bit-identical
    case = sr.make_cases(sr.SHAPES[0])[1]
    a, b = sr.run_hook(case), sr.run_hook(case)
    assert all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b))


def check_entries():
    weights, eng = _micro()
    o32 = OracleWhisper(weights)
    st = wb.SpecialTokens.for_vocab(V)
    g = np.random.default_rng(9)
    C, lens = 24, [9, 1, 6]
    enc = np.stack([_enc(o32, C, 40 + i) for i in range(len(lens))])
    L = max(lens) + 2                                   # a row stride larger than every len
    toks = np.zeros((len(lens), L), dtype=np.int32)
    for i, n in enumerate(lens):
        toks[i, :n] = g.integers(0, V - 16, n)
        toks[i, 0] = st.start_of_transcript
    probe_ids = [V - 3, 7, V - 1, 7]
    lp, plp = eng.score_tokens(toks, enc, lens=lens, is_special=st.is_special, mask_until_len=5, probe_ids=probe_ids)
    worst = 0.0
    for i, n in enumerate(lens):
        ref, pref = sr.oracle_scores(o32, st.is_special, enc[i], toks[i, :n], 5, probe_ids, 0)
        assert np.isnan(lp[i, 0]) and np.isnan(lp[i, n:]).all() and not np.isnan(lp[i, 1:n]).any(), (i, lp[i])
        worst = max(worst, float(sr.absdiff(lp[i, 1:n], ref[1:]).max()) if n > 1 else 0.0, float(np.abs(plp[i] - pref).max()))
    print(f"score_tokens vs oracle: worst {worst:.3e}")
    assert worst <= TOL
    # no mask, no probes: another path through the kernel (one statistic per row)
    lp0 = eng.score_tokens(toks, enc, lens=lens)
    for i, n in enumerate(lens):
        ref, _ = sr.oracle_scores(o32, st.is_special, enc[i], toks[i, :n], 0)
        assert n == 1 or sr.absdiff(lp0[i, 1:n], ref[1:]).max() <= TOL
    # a probe at a later position
    _, p2 = eng.score_tokens(toks[:1], enc[:1], lens=lens[:1], probe_ids=[3], probe_pos=lens[0] - 1)
    _, r2 = sr.oracle_scores(o32, st.is_special, enc[0], toks[0, :lens[0]], 0, [3], lens[0] - 1)
    assert abs(p2[0, 0] - r2[0]) <= TOL
    # the session entry: its own encoder output, against the stateless entry on that output; twice, bit-identical
    audio = synth.synth_audio(16000 * 2, 3)
    starts, wl = wb.window_extents(len(audio), 16000, wb.max_waveform_samples(eng.max_mel_frames() - 10))
    sess = wb.Session.begin(eng, audio, starts, wl, max_beams=1)
    W = len(starts)
    rows = toks[:W, :lens[0]].copy()
    rows[:, :] = toks[0, :lens[0]]
    try:
        sess.score(rows, mask_until_len=5)
        raise AssertionError("a mask was needed and none was set")
    except wb.WbError as e:
        assert e.status == -6, e.status           # WB_ERR_STATE
    sess.set_special_mask(st.is_special)
    a, pa = sess.score(rows, mask_until_len=5, probe_ids=probe_ids)
    b, pb = sess.score(rows, mask_until_len=5, probe_ids=probe_ids)
    assert np.array_equal(a.view(np.int32), b.view(np.int32)) and np.array_equal(pa.view(np.int32), pb.view(np.int32))
    encs = np.stack([sess.encoder_output(w) for w in range(W)])
    c, pc = eng.score_tokens(rows, encs, is_special=st.is_special, mask_until_len=5, probe_ids=probe_ids)
    assert sr.absdiff(a[:, 1:], c[:, 1:]).max() <= 2 * TOL and np.abs(pa - pc).max() <= 2 * TOL
    best, mean, win = sess.detect_language(st.start_of_transcript, list(range(V - 14, V - 4)))
    assert win.shape == (W, 10) and abs(float(win.sum()) - W) < 1e-4 and best == int(np.argmax(mean))
    sess.close()
    eng.close()


def check_waveform():
    """wb_waveform_to_token_scores and wb_waveform_detect_language end to end under the functional model."""
    weights, eng = _micro()
    o32 = OracleWhisper(weights)
    st = wb.SpecialTokens.for_vocab(V)
    audio = synth.synth_audio(16000 * 2, 3)
    nsp = V - 9
    full, wins = wb.waveform_to_tokens(eng, st, audio, 16000, 1, 6)
    r = wb.waveform_to_token_scores(eng, st, audio, 16000, 1, 6, no_speech=nsp)
    assert r["tokens"] == full and r["win_tokens"] == wins
    starts, wl = wb.window_extents(len(audio), 16000, wb.max_waveform_samples(eng.max_mel_frames() - 10))
    sess = wb.Session.begin(eng, audio, starts, wl, max_beams=1)
    for w, row in enumerate(wins):
        lp = r["win_logprobs"][w]
        ref, pref = sr.oracle_scores(o32, st.is_special, sess.encoder_output(w), row, 5, [nsp], 0)
        assert sr.absdiff(lp[1:], ref[1:]).max() <= TOL and np.isnan(lp[0])
        assert abs(r["avg_logprob"][w] - np.float32(np.mean(lp[4:].astype(np.float64)))) <= 1e-6
        assert abs(r["no_speech_prob"][w] - np.exp(pref[0])) <= TOL
    assert len(r["logprobs"]) == len(full)
    r0 = wb.waveform_to_token_scores(eng, st, audio, 16000, 1, 6)
    assert np.isnan(r0["no_speech_prob"]).all() and r0["tokens"] == full
    ids = list(range(V - 14, V - 4))
    best, mean, win = wb.detect_language(eng, ids, audio, 16000, sot=st.start_of_transcript, max_windows=0)
    b2, m2, w2 = sess.detect_language(st.start_of_transcript, ids)
    assert best == b2 and np.allclose(mean, m2, atol=1e-6) and np.allclose(win, w2, atol=1e-6)
    for w in range(len(wins)):
        _, pref = sr.oracle_scores(o32, st.is_special, sess.encoder_output(w), [st.start_of_transcript], 0, ids, 0)
        e = np.exp(pref - pref.max())
        assert np.abs(win[w] - e / e.sum()).max() <= TOL
    sess.close()
    eng.close()


def check_errors():
    weights, eng = _micro()
    o32 = OracleWhisper(weights)
    st = wb.SpecialTokens.for_vocab(V)
    enc = _enc(o32, 16, 1)[None]
    toks = np.arange(8, dtype=np.int32)[None]
    lib = _lib.load()
    lib.wb_profile_enable(1)
    _lib.profile_kernels(reset=True)

    def status(fn):
        try:
            fn()
        except wb.WbError as e:
            return e.status
        return 0

    bad = toks.copy(); bad[0, 3] = V
    assert status(lambda: eng.score_tokens(bad, enc)) == -1                                   # token id out of range
    neg = toks.copy(); neg[0, 0] = -1
    assert status(lambda: eng.score_tokens(neg, enc)) == -1
    assert status(lambda: eng.score_tokens(toks, enc, probe_ids=[V])) == -1                   # probe id out of range
    assert status(lambda: eng.score_tokens(toks, enc, probe_ids=[-1])) == -1
    assert status(lambda: eng.score_tokens(toks, enc, probe_ids=[1], probe_pos=8)) == -1      # probe_pos >= len
    assert status(lambda: eng.score_tokens(toks, enc, lens=[3], probe_ids=[1], probe_pos=3)) == -1
    assert status(lambda: eng.score_tokens(toks, enc, probe_ids=[1], probe_pos=-1)) == -1
    assert status(lambda: eng.score_tokens(toks, enc, mask_until_len=5)) == -1                # a mask is needed, none given
    assert status(lambda: eng.score_tokens(toks, enc, mask_until_len=-1)) == -1
    assert status(lambda: eng.score_tokens(toks, enc, lens=[0])) == -1 and status(lambda: eng.score_tokens(toks, enc, lens=[9])) == -1
    long = np.zeros((1, 449), dtype=np.int32)
    assert status(lambda: eng.score_tokens(long, enc)) == -2                                  # len > n_text_ctx
    # the hook's own argument checks
    case = sr.make_cases(sr.SHAPES[0])[0]
    for key, val in (("target", np.array([V], dtype=np.int32)), ("probes", [(1, 0)]), ("probes", [(0, V)])):
        c = dict(case); c[key] = val
        assert status(lambda: sr.run_hook(c)) == -1, key
    c = dict(case); c["h"] = case["h"][:, :48]; c["E"] = case["E"][:, :48]
    assert status(lambda: sr.run_hook(c)) == -2                                               # d not a multiple of 32
    # language detection / token scores: argument errors
    audio = synth.synth_audio(16000 * 2, 3)
    assert status(lambda: wb.detect_language(eng, [V], audio, 16000, sot=st.start_of_transcript)) == -1
    assert status(lambda: wb.detect_language(eng, [1], audio, 16000, sot=V)) == -1
    assert status(lambda: wb.waveform_to_token_scores(eng, st, audio, 16000, 1, 2, no_speech=V)) == -1
    assert _lib.profile_kernels(reset=True) == [], "an error case launched a kernel"
    assert status(lambda: eng.score_tokens(toks, enc, is_special=st.is_special, mask_until_len=5, probe_ids=[1])) == 0
    names = {k["name"].split(" ")[0]: k["calls"] for k in _lib.profile_kernels(reset=True)}
    assert names == {"score_logits": 1, "score_merge": 1}, names
    lib.wb_profile_enable(0)
    eng.close()


if __name__ == "__main__":
    assert b"hipemu" in _lib.load().wb_version()
    {"hook": check_hook, "entries": check_entries, "waveform": check_waveform, "errors": check_errors}[sys.argv[1]]()
    print("OK", sys.argv[1])
