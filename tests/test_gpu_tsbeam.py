"""GPU: Session.decode_timestamps_beam / waveform_to_segments(beam=...) on the micro fixture of tests/tsrules_ref.py, depth 40,
at W x B = 3 x 2 (fused, <= 8 rows), 3 x 5 (the 16-row bucket), 4 x 5 (batch mode), 3 x 3 and 3 x 5 with patience 2.

Every window-step of last_beam_trace is replayed by the restatement on oracle logits teacher-forced on the device's own beams
and scores: outside the replay rule's exclusions (capped at 10 % of the window-steps) beams, parents and newly-finished counts
match; recorded f64 scores are within 1e-3 per generated token of the oracle's; every candidate of last_beams satisfies the
invariants of timestamp decoding; the returned row is the finalize rule over the device's candidates; rewind + decode again
gives identical results; other rule parameters, patience or length penalty drop no graph and capture none of their own;
`active` leaves the other windows untouched.  Beam 1 returns decode_timestamps' greedy rows; on (5, 1) the rows are the
oracle's own beam search wherever that search has no excluded step; the seek loop tiles the stream, ends and equals per-window
beam decodes; the CLI takes --beam-size only together with --segments."""
import pytest

import tsbeam_ref as tb
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


@pytest.mark.parametrize("W,B,patience", [(3, 2, 1.0), (3, 5, 1.0), (4, 5, 1.0), (3, 3, 2.0), (3, 5, 2.0)],
                         ids=["3x2_fused", "3x5_16row_bucket", "4x5_batch_mode", "3x3_patience2", "3x5_patience2"])
def test_beam_search_replays_on_the_teacher_forced_oracle(micro, W, B, patience):
    eng, o32 = micro
    rec = []
    rows, score, ncand, beams = tb.check_session_shape(eng, o32, W, B, patience, record=rec)
    print("(B, patience, window-steps, excluded):", rec)
    assert all(len(r) > 3 for r in rows)


def test_beam_5_rows_are_the_oracle_s_own_beam_search(micro):
    import whisper_burn_amd as wb
    eng, o32 = micro
    weights, st, audio, R, sup, prompt = tr.fixture()
    sess = tr.fixture_session(eng, audio, 3, 5)
    sess.set_suppress(sup)
    p = wb.decode_params(st, 1, tr.FIX_DEPTH)
    rows, _, _ = sess.decode_timestamps_beam(p, wb.TimestampParams(R["tb"], R["n_ts"], R["max_init"], R["max_ts"]), wb.BeamParams(5))
    clean = 0
    for w, enc in enumerate(tr.fixture_encs(o32, audio, 3)):
        res, steps, excluded = tb.oracle_search(o32, enc, prompt, R, st.end_of_text, sup, 5, 1.0, tr.FIX_DEPTH)
        if excluded == 0:
            clean += 1
            assert rows[w] == prompt + res["cands"][res["best"]][0], w
    print("windows without an excluded step:", clean)
    sess.close()


def test_beam_1_is_the_greedy_timestamp_decode(micro):
    tb.check_beam1_is_greedy(micro[0])


def test_waveform_to_segments_by_beam_search_on_the_short_context_model():
    eng = tr.short_context_engine()
    segs, seeks = tb.check_seek_loop_beam(eng)
    print("seeks", seeks, "segments", len(segs))
    eng.close()


def test_cli_segments_with_beam_size(tmp_path, monkeypatch):
    """`--segments PATH --beam-size 3` writes ordered segments; the beam flags without --segments are rejected while the
    arguments are parsed."""
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
    assert cli.main(["transcribe", "micro", "a.wav", "en", "seg.txt", "--segments", "seg.jsonl", "--beam-size", "3", "--patience",
                     "2"]) == 0
    recs = [json.loads(ln) for ln in open(tmp_path / "seg.jsonl")]
    assert recs and all(set(r) == {"start", "end", "text", "tokens"} for r in recs)
    assert all(0.0 <= r["start"] <= r["end"] <= 1.0 + 0.17 for r in recs)
    assert [r["start"] for r in recs] == sorted(r["start"] for r in recs)
    assert " ".join(r["text"] for r in recs if r["text"]) == open(tmp_path / "seg.txt").read()
    for bad in (["--beam-size", "3"], ["--patience", "2"], ["--segments", "s.jsonl", "--patience", "2"],
                ["--segments", "s.jsonl", "--beam-size"], ["--segments", "s.jsonl", "--beam-size", "x"]):
        assert cli.main(["transcribe", "micro", "a.wav", "en", "x.txt"] + bad) == 1, bad
    assert not (tmp_path / "x.txt").exists()
