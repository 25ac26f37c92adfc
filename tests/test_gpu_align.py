"""GPU: token alignment (wb_align_tokens / wb_session_align / wb_dtw_start_positions / wb_waveform_to_token_times) against
its restatement on the oracle (tests/align_ref.py).

  A  the token x position matrix M vs the f64 restatement, bound 4 x d32 where d32 = max |M_f32 - M_f64| of the
     restatement itself (a second, differently ordered f32 evaluation + the exp argument rounding); both sides are fed the
     oracle's f32 encoder output, so only the new path differs.  Measured ratios: LABLOG.md.
  B  start positions == the NumPy f32 DTW of the RETURNED matrix, exactly; wb_dtw_start_positions == NumPy.
  C  wb_session_align after wb_session_decode vs the f64 restatement's positions (>= 98 % equal, never more than 1 apart),
     decoded tokens untouched, a second call bit-identical, session and stateless entry agree exactly.
  D  the synthetic checkpoints' ground truth (positional heads look at encoder position ~3 p), the opt-in 30 s geometry,
     token times end to end, the CLI, and the launch structure (at most two launches per layer + one DTW).
"""
import json
import math
import os

import numpy as np
import pytest
import torch

import align_ref as ar
import parity_log
import parity_util as pu
import whisper_burn_amd as wb
import workloads
from whisper_burn_amd import _lib, synth

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_outputs.npz")


def rows_of(name):
    g = np.load(GOLD)
    t, n = g[f"{name}_tokens"], g[f"{name}_lens"]
    return [t[i, :n[i]].tolist() for i in range(len(n))]


def _drop_last(row, st):
    return 1 if row[-1] == st.end_of_text else 0


def _check_matrix(name, eng, o32, o64, rows, encs, st, heads=None, fw=7):
    """A + B for rows with their own encoder outputs (one call per row: the rows' C differ)."""
    for i, (row, enc) in enumerate(zip(rows, encs)):
        dl = _drop_last(row, st)
        pos, mat = eng.align_tokens([row], enc[None], heads=heads, drop_last=dl, filter_width=fw, return_matrix=True)
        m32 = ar.alignment_matrix(o32, row, enc, heads, fw).numpy()
        m64 = ar.alignment_matrix(o64, row, enc, heads, fw).numpy()
        d32 = float(np.abs(m32 - m64).max())
        err = float(np.abs(mat[0] - m64).max())
        print(f"align A {name} row {i}: len {len(row)} C {enc.shape[0]} d32 {d32:.3e} err {err:.3e} ratio {err / d32:.2f}")
        parity_log.record(f"align_matrix[{name}/{i}]", err, 4 * d32, ratio=err / d32)
        assert err <= 4 * d32, (name, i, err, d32)
        assert np.array_equal(pos[0], ar.start_positions(mat[0], 4, dl)), (name, i)            # B


def _oracle_encs(o32, audio):
    return [o32.forward_encoder(m)[0].numpy() for m in pu.window_mels(o32, audio)]


def test_matrix_micro_model():
    dims = synth.micro_dims(n_state=128, n_head=2, n_layer=2, n_vocab=1031)
    w = synth.synth_weights(dims, seed=77)
    eng, o32, o64 = wb.Whisper.from_tensors(w), ar.AlignOracle(w), ar.AlignOracle(w, dtype=torch.float64)
    st = wb.SpecialTokens.for_vocab(1031)
    audio = synth.synth_audio(16000 * 20, 4)
    _, wins = wb.waveform_to_tokens(eng, st, audio, 16000, 1, 40)
    encs = _oracle_encs(o32, audio)
    _check_matrix("micro", eng, o32, o64, wins, encs, st)
    _check_matrix("micro/heads", eng, o32, o64, wins, encs, st, heads=[(1, 1), (0, 0)], fw=3)
    eng.close()


def test_matrix_of_rows_up_to_the_text_context():
    """Two teacher-forced rows of 448 (= n_text_ctx) and 300 arbitrary tokens in ONE call: the accumulate kernel's LDS tile is
    sized by the longest row (114 KB here, above the 64 KB a launch gets without asking), the DTW block has 444 live threads."""
    dims = synth.micro_dims(n_state=128, n_head=2, n_layer=2, n_vocab=1031)
    w = synth.synth_weights(dims, seed=77)
    eng, o32, o64 = wb.Whisper.from_tensors(w), ar.AlignOracle(w), ar.AlignOracle(w, dtype=torch.float64)
    enc = _oracle_encs(o32, synth.synth_audio(16000 * 20, 4))[0]
    g = np.random.default_rng(448)
    lens = [448, 300]
    toks = np.zeros((2, 448), dtype=np.int32)
    for i, n in enumerate(lens):
        toks[i, :n] = g.integers(0, 1015, n)
    pos, mat = eng.align_tokens(toks, np.stack([enc, enc]), lens=lens, drop_last=0, return_matrix=True)
    for i, n in enumerate(lens):
        m32 = ar.alignment_matrix(o32, toks[i, :n], enc).numpy()
        m64 = ar.alignment_matrix(o64, toks[i, :n], enc).numpy()
        d32, err = float(np.abs(m32 - m64).max()), float(np.abs(mat[i, :n] - m64).max())
        print(f"align A long row {i}: len {n} d32 {d32:.3e} err {err:.3e} ratio {err / d32:.2f}")
        parity_log.record(f"align_matrix[long/{i}]", err, 4 * d32, ratio=err / d32)
        assert err <= 4 * d32, (i, err, d32)
        assert np.array_equal(pos[i, :n], ar.start_positions(mat[i, :n], 4, 0)), i
        assert not mat[i, n:].any() and (pos[i, n:] == -1).all()
    eng.close()


@pytest.mark.parametrize("name", ["tiny_bench", "base_beam5_eot", "large_window"])
def test_matrix_of_workload(name):
    wl = workloads.WORKLOADS[name]
    w = wl.weights()
    eng, o32, o64 = wb.Whisper.from_tensors(w), ar.AlignOracle(w), ar.AlignOracle(w, dtype=torch.float64)
    st = wb.SpecialTokens.for_vocab(eng.dims["n_vocab"])
    _check_matrix(name, eng, o32, o64, rows_of(name), _oracle_encs(o32, wl.audio()), st)
    eng.close()


@pytest.mark.parametrize("shape", [(1, 1), (1, 1500), (444, 1500), (448, 300)])
def test_dtw_matches_numpy_exactly(shape):
    g = np.random.default_rng(shape[0] * 7 + shape[1])
    x = g.standard_normal(shape).astype(np.float32)
    assert np.array_equal(wb.dtw_start_positions(x), ar.dtw_start_positions(x))


def test_dtw_on_ties():
    g = np.random.default_rng(1)
    for shape in [(40, 90), (90, 40), (17, 17)]:
        x = g.integers(-2, 3, shape).astype(np.float32)
        assert np.array_equal(wb.dtw_start_positions(x), ar.dtw_start_positions(x))
    x = np.zeros((9, 14), dtype=np.float32)
    assert np.array_equal(wb.dtw_start_positions(x), ar.dtw_start_positions(x))


def _session_case(name):
    wl = workloads.WORKLOADS[name]
    w = wl.weights()
    eng = wb.Whisper.from_tensors(w)
    if wl.frame_limit_x2:
        eng.set_frame_limit(True)
    st = wb.SpecialTokens.for_vocab(eng.dims["n_vocab"])
    audio = wl.audio()
    wlen = wb.max_waveform_samples(eng.max_mel_frames() - 10)
    starts, lens = wb.window_extents(len(audio), 16000, wlen)
    sess = wb.Session.begin(eng, audio, starts, lens, max_beams=wl.beam)
    sess.set_special_mask(st.is_special)
    rows = sess.decode(wb.decode_params(st, wl.beam, wl.depth))
    return wl, w, eng, st, audio, sess, rows, starts


@pytest.mark.parametrize("name", ["tiny_bench", "base_beam5_eot", "large_window"])
def test_session_align_end_to_end(name):
    wl, w, eng, st, audio, sess, rows, _ = _session_case(name)
    assert rows == rows_of(name)
    # rows of one call share drop_last: 1 when every row ends in <|endoftext|>, else 0 (the restatement uses the same)
    dl = int(all(_drop_last(r, st) for r in rows))
    pos, mat = sess.align(rows, drop_last=dl, return_matrix=True)
    pos2, mat2 = sess.align(rows, drop_last=dl, return_matrix=True)
    assert np.array_equal(pos, pos2) and np.array_equal(mat.view(np.int32), mat2.view(np.int32))
    o64 = ar.AlignOracle(w, dtype=torch.float64)
    o32 = ar.AlignOracle(w)
    mels = pu.window_mels(o32, audio)
    n_tok = n_diff = 0
    for i, row in enumerate(rows):
        n = len(row)
        C = sess.encoder_output(i).shape[0]
        assert np.array_equal(pos[i, :n], ar.start_positions(mat[i, :n, :C], 4, dl)), (name, i)          # B
        assert (pos[i, n:] == -1).all() and (pos[i, :4] == -1).all()
        # the stateless entry on the session's own encoder output: the same arithmetic, exactly
        p1, m1 = eng.align_tokens([row], sess.encoder_output(i)[None], drop_last=dl, return_matrix=True)
        assert np.array_equal(p1[0], pos[i, :n]) and np.array_equal(m1[0].view(np.int32), mat[i, :n, :C].view(np.int32))
        enc64 = o64.forward_encoder(mels[i].to(torch.float64))[0]
        ref = ar.start_positions(ar.alignment_matrix(o64, row, enc64.numpy()).numpy(), 4, dl, dtw_dtype=np.float64)
        a, b = pos[i, 4:n - dl], ref[4:n - dl]
        n_tok += len(a)
        n_diff += int((a != b).sum())
        assert np.abs(a - b).max() <= 1, (name, i, np.abs(a - b).max())
    print(f"align C {name}: {n_diff} of {n_tok} aligned tokens differ from the f64 restatement")
    parity_log.record(f"align_positions[{name}]", n_diff, 0.02 * n_tok, n_rows=n_tok)
    assert n_diff <= 0.02 * n_tok
    sess.close()
    # without a decode: a fresh session over the same windows aligns the rows to the same bits (it settles the encode
    # pass's deferred range check itself) ...
    starts, lens = wb.window_extents(len(audio), 16000, wb.max_waveform_samples(eng.max_mel_frames() - 10))
    fresh = wb.Session.begin(eng, audio, starts, lens, max_beams=wl.beam)
    pos0, mat0 = fresh.align(rows, drop_last=dl, return_matrix=True)
    assert np.array_equal(pos0, pos) and np.array_equal(mat0.view(np.int32), mat.view(np.int32))
    # ... and the alignment pass, which ran on the session's workspace, left the decode alone: the golden rows again
    fresh.set_special_mask(st.is_special)
    assert fresh.decode(wb.decode_params(st, wl.beam, wl.depth)) == rows_of(name)
    fresh.close()
    # the stateless entry ran on the model's scratch (workspace, staging buffers): the engine still transcribes to the rows
    _, wins = wb.waveform_to_tokens(eng, st, audio, 16000, wl.beam, wl.depth)
    assert wins == rows_of(name)
    eng.close()


def _slope(pos, n_fit=80):
    """Least-squares slope of (token index, start position) over the first `n_fit` aligned tokens: the DTW path must end
    in the last encoder position, which pulls the final tokens of a row that stops before the audio does far to the
    right (the 750-position window holds ~100 tokens x 3 positions), so the tail is not part of the ground truth."""
    idx = np.nonzero(pos >= 0)[0][:n_fit]
    assert len(idx) == n_fit
    return float(np.polyfit(idx.astype(np.float64), pos[idx].astype(np.float64), 1)[0])


def test_positional_heads_follow_three_positions_per_token():
    """The synthetic checkpoints' own ground truth: in the positional half of the heads, step p looks at position ~3 p."""
    wl, w, eng, st, audio, sess, rows, _ = _session_case("tiny_bench")
    H, NL = eng.dims["n_text_head"], eng.dims["n_text_layer"]
    heads = [(l, h) for l in range(NL) for h in range(H // 2)]
    pos = sess.align(rows, heads=heads, drop_last=0)
    s = _slope(pos[0, :len(rows[0])])
    print(f"align D slope {s:.3f}")
    assert abs(s - 3.0) <= 0.1, s
    sess.close()
    eng.close()


def test_thirty_second_geometry():
    wl, w, eng, st, audio, sess, rows, _ = _session_case("tiny_whisper30")
    assert sess.encoder_output(0).shape[0] == 1500
    dl = int(all(_drop_last(r, st) for r in rows))
    pos, mat = sess.align(rows, drop_last=dl, return_matrix=True)
    for i, row in enumerate(rows):
        C = sess.encoder_output(i).shape[0]
        assert np.array_equal(pos[i, :len(row)], ar.start_positions(mat[i, :len(row), :C], 4, dl))
    sess.close()
    eng.close()


def test_waveform_to_token_times():
    wl = workloads.WORKLOADS["tiny_bench"]
    eng = wb.Whisper.from_tensors(wl.weights())
    st = wb.SpecialTokens.for_vocab(eng.dims["n_vocab"])
    audio = wl.audio()
    full, wins = wb.waveform_to_tokens(eng, st, audio, 16000, wl.beam, wl.depth)
    toks, times, wtoks, wtimes = wb.waveform_to_token_times(eng, st, audio, 16000, wl.beam, wl.depth)
    assert toks == full and wtoks == wins
    starts, lens = wb.window_extents(len(audio), 16000, wb.max_waveform_samples(eng.max_mel_frames() - 10))
    sess = wb.Session.begin(eng, audio, starts, lens, max_beams=1)
    for i, row in enumerate(wins):
        dl = _drop_last(row, st)
        p = eng.align_tokens([row], sess.encoder_output(i)[None], drop_last=dl)[0]
        ref = np.where(p >= 0, starts[i] / 16000.0 + 0.02 * p, np.nan).astype(np.float32)
        assert np.array_equal(wtimes[i], ref, equal_nan=True), i
        assert np.isnan(wtimes[i][:4]).all() and (not dl or math.isnan(wtimes[i][-1]))
        t = wtimes[i][~np.isnan(wtimes[i])]
        assert (np.diff(t) >= 0).all()
    rt, rtt = ar.stitch_with_times(wins, [t.tolist() for t in wtimes])
    assert rt == toks and np.array_equal(np.asarray(rtt, dtype=np.float32), times, equal_nan=True)
    sess.close()
    eng.close()


def test_cli_token_times(tmp_path, monkeypatch):
    import wave
    from test_tokenizer_integration import N_VOCAB, write_synthetic_tokenizer_json
    from whisper_burn_amd import dumpdir
    from whisper_burn_amd import transcribe as cli
    monkeypatch.chdir(tmp_path)
    write_synthetic_tokenizer_json(str(tmp_path / "tokenizer.json"))
    dims = synth.micro_dims(n_state=128, n_head=2, n_layer=2, n_vocab=N_VOCAB)
    dumpdir.write_dump_dir(synth.synth_weights(dims, seed=4242), str(tmp_path / "micro"))
    pcm = np.clip(np.round(synth.synth_audio(16000 * 6, 52) * 32767.0), -32768, 32767).astype("<i2")
    with wave.open(str(tmp_path / "a.wav"), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(pcm.tobytes())
    assert cli.main(["transcribe", "micro", "a.wav", "en", "plain.txt"]) == 0
    assert cli.main(["transcribe", "micro", "a.wav", "en", "timed.txt", "--token-times", "times.jsonl"]) == 0
    assert open(tmp_path / "plain.txt", "rb").read() == open(tmp_path / "timed.txt", "rb").read()
    recs = [json.loads(ln) for ln in open(tmp_path / "times.jsonl")]
    assert len(recs) >= 2 and all(set(r) == {"id", "text", "start"} for r in recs)
    # 6 s of audio = 600 mel frames + 10 frames of zero padding = 305 encoder positions of 0.02 s
    assert all(0.0 <= r["start"] <= 0.02 * 304 + 0.005 and r["id"] < N_VOCAB - 16 for r in recs), recs
    assert " ".join(r["text"] for r in recs) == open(tmp_path / "plain.txt").read()


def test_launch_structure():
    """At most two launches per decoder layer that owns an alignment head plus one DTW launch, whatever the number of
    rows and their lengths."""
    wl, w, eng, st, audio, sess, rows, _ = _session_case("tiny_bench")
    lib = _lib.load()
    NL = eng.dims["n_text_layer"]
    assert sorted(len(r) for r in rows)[0] <= 7 and max(len(r) for r in rows) == 104
    enc = [sess.encoder_output(i) for i in range(len(rows))]
    lib.wb_profile_enable(1)
    try:
        def counts(fn):
            _lib.profile_kernels(reset=True)
            fn()
            return {k["name"].split(" ")[0]: k["calls"] for k in _lib.profile_kernels(reset=True) if k["name"].startswith("align_")}
        short = min(range(len(rows)), key=lambda i: len(rows[i]))
        long = max(range(len(rows)), key=lambda i: len(rows[i]))
        want = {"align_row_stats": NL - NL // 2, "align_accumulate": NL - NL // 2, "align_dtw": 1}
        assert counts(lambda: sess.align(rows, drop_last=0)) == want                                     # 3 rows
        assert counts(lambda: eng.align_tokens([rows[short]], enc[short][None], drop_last=0)) == want    # 1 row, 7 tokens
        assert counts(lambda: eng.align_tokens([rows[long]], enc[long][None], drop_last=0)) == want      # 1 row, 104 tokens
        one = {"align_row_stats": 1, "align_accumulate": 1, "align_dtw": 1}
        assert counts(lambda: sess.align(rows, heads=[(1, 0), (1, 3), (1, 2)], drop_last=0)) == one
    finally:
        lib.wb_profile_enable(0)
    sess.close()
    eng.close()
