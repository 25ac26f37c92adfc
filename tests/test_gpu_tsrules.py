"""GPU: Session.decode_timestamps / waveform_to_segments on the micro fixture of tests/tsrules_ref.py (micro_dims(64, 1, 1,
1031), synth_weights(seed=5), T = [800, 951), max_initial_timestamp_index = 50, depth 40, suppress = the specials but
end-of-text) in the three launch shapes.

Every generated position is checked against ONE teacher-forced oracle pass over the device's own row (exclusion outside
delta_model capped at 5 %, f64 sums within 1e-3 per token); every device row satisfies the invariants outright (starts on a
timestamp <= tb + 50, timestamps never decrease, no lone timestamp between text, no suppressed id); rewind + decode again gives
identical bits; another temperature, seed or rule parameter captures no graph; `active` leaves the other windows untouched;
with the rules off the rows are decode_sample's (T = 1) and Session.decode's (T = 0); the seek loop tiles the stream, ends, and
equals per-window decode_timestamps at the same seeks."""
import pytest

import tsrules_ref as tr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def micro():
    import whisper_burn_amd as wb
    from oracle.model import OracleWhisper
    weights = tr.fixture()[0]
    eng = wb.Whisper.from_tensors(weights)
    yield eng, OracleWhisper(weights)
    eng.close()


@pytest.mark.parametrize("W,best_of", [(3, 1), (3, 5), (4, 5)], ids=["3x1_fused", "3x5_16row_bucket", "4x5_batch_mode"])
def test_decode_timestamps_against_the_teacher_forced_oracle(micro, W, best_of):
    eng, o32 = micro
    rec = []
    rows, sums, best = tr.check_session_shape(eng, o32, W, best_of, record=rec)
    print("(T, best_of, positions, excluded, mismatches):", rec)
    assert all(len(r) > 3 for r in rows)


def test_greedy_rows_are_the_oracle_s_own_rows(micro):
    """At temperature 0 nothing of the fixture lies inside delta_model (tests/test_tsrules_ref.py asserts it on the oracle
    alone), so the device rows are the oracle's, token for token: 5, 6 and 2 timestamps with pairs and text between them."""
    import whisper_burn_amd as wb
    eng, o32 = micro
    weights, st, audio, R, sup, prompt = tr.fixture()
    sess = tr.fixture_session(eng, audio, 3, 1)
    sess.set_suppress(sup)
    p = wb.decode_params(st, 1, tr.FIX_DEPTH)
    rows, _, _ = sess.decode_timestamps(p, wb.TimestampParams(R["tb"], R["n_ts"], R["max_init"], R["max_ts"]))
    encs = tr.fixture_encs(o32, audio, 3)
    want = [tr.oracle_decode(o32, enc, prompt, R, st.end_of_text, sup, None, tr.FIX_DEPTH)[0] for enc in encs]
    assert rows == want
    assert [sum(tr.is_ts(R, t) for t in r[3:]) for r in rows] == [5, 6, 2]
    sess.close()


def test_rules_off_is_plain_sampling_and_plain_greedy(micro):
    tr.check_rules_off(micro[0])


def test_waveform_to_segments_on_the_short_context_model():
    eng = tr.short_context_engine()
    segs, seeks = tr.check_seek_loop(eng)
    print("seeks", seeks, "segments", len(segs))
    eng.close()


def test_cli_segments(tmp_path, monkeypatch):
    """`--segments PATH`: one {"start", "end", "text", "tokens"} line per segment, in order; the transcript is the segments'
    text.  (The synthetic tokenizer has nine timestamp tokens, 0.00 .. 0.16 s: the window moves in small steps.)"""
    import json
    import wave
    import numpy as np
    pytest.importorskip("tokenizers")
    from test_tokenizer_integration import N_VOCAB, write_synthetic_tokenizer_json
    from whisper_burn_amd import dumpdir, synth
    from whisper_burn_amd import transcribe as cli
    monkeypatch.chdir(tmp_path)
    write_synthetic_tokenizer_json(str(tmp_path / "tokenizer.json"))
    dims = synth.micro_dims(n_state=64, n_head=1, n_layer=1, n_vocab=N_VOCAB)
    dumpdir.write_dump_dir(synth.synth_weights(dims, seed=5), str(tmp_path / "micro"))
    audio = synth.synth_audio(16000, 52)
    pcm = np.clip(np.round(audio * 32767.0), -32768, 32767).astype("<i2")
    with wave.open(str(tmp_path / "a.wav"), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(pcm.tobytes())
    assert cli.main(["transcribe", "micro", "a.wav", "en", "seg.txt", "--segments", "seg.jsonl"]) == 0
    recs = [json.loads(ln) for ln in open(tmp_path / "seg.jsonl")]
    assert recs and all(set(r) == {"start", "end", "text", "tokens"} for r in recs)
    assert all(0.0 <= r["start"] <= r["end"] <= 1.0 + 0.17 for r in recs)
    assert [r["start"] for r in recs] == sorted(r["start"] for r in recs)
    assert not any(t >= N_VOCAB - 16 for r in recs for t in r["tokens"])
    assert " ".join(r["text"] for r in recs if r["text"]) == open(tmp_path / "seg.txt").read()
    # rejected while the arguments are parsed
    assert cli.main(["transcribe", "micro", "a.wav", "en", "x.txt", "--segments", "s.jsonl", "--fallback"]) == 1
    assert cli.main(["transcribe", "micro", "a.wav", "en", "x.txt", "--segments"]) == 1
    assert not (tmp_path / "x.txt").exists()
