"""GPU: the one-pass prompt prefill (Session.prefill / set_prefill) and the conditioned seek loop.

 * the cache: for every case of prefill_ref.CACHE_CASES and every layer, self_kv behind Session.prefill against K and V
   restated from the f64 oracle, within 4 x d32 + 1e-7 x max |value| (d32: the f32 oracle's own distance from the f64 one on
   the same entries); the step-prefilled session passes the same bound; then one step and two forking steps behind the pass:
   log-probs within 1e-3 of the f32 oracle, top-1 equal wherever the oracle's top-two gap exceeds 2e-3;
 * the error paths launch nothing;
 * the chains behind [<|startofprev|>] + 20 ids + [sot, lang, transcribe] in mode 1 against the teacher-forced oracle by their
   own schemes (exclusion capped at 5 %); mode 0 gives the rows of a session that never set a mode, bit for bit; rewind + mode
   1 again gives identical bits; the profiled repeat shows prefill_store in mode 1 only;
 * wb_waveform_to_segments_conditioned equals the Python seek loop over per-window decodes (greedy, beam 3), reaches a
   truncated history, and with conditioning off equals waveform_to_segments."""
import pytest

import parity_log
import prefill_ref as pf
import tsrules_ref as tr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cache_model():
    import torch
    import whisper_burn_amd as wb
    from oracle.model import OracleWhisper
    weights = pf.cache_weights()
    eng = wb.Whisper.from_tensors(weights)
    yield eng, OracleWhisper(weights), OracleWhisper(weights, dtype=torch.float64)
    eng.close()


@pytest.fixture(scope="module")
def micro():
    import whisper_burn_amd as wb
    from oracle.model import OracleWhisper
    weights = tr.fixture()[0]
    eng = wb.Whisper.from_tensors(weights)
    yield eng, OracleWhisper(weights)
    eng.close()


@pytest.mark.parametrize("W,active,n", pf.CACHE_CASES, ids=[f"W{w}{'_active' if a else ''}_n{n}" for w, a, n in pf.CACHE_CASES])
def test_cache_and_next_steps_behind_the_pass(cache_model, W, active, n):
    eng, o32, o64 = cache_model
    pf.check_cache_case(eng, o32, o64, W, active, n,
                        record_ratio=lambda case, ratio: parity_log.record_ratio("prefill_cache", case, ratio),
                        record_lp=lambda case, worst: parity_log.record(f"test_gpu_prefill/{case}", worst, 1e-3))
    parity_log.flush_ratios()


def test_error_paths_launch_nothing(cache_model):
    pf.check_prefill_errors(cache_model[0])


@pytest.mark.parametrize("which", pf.CHAINS)
def test_chains_behind_the_long_prompt(micro, which):
    pf.check_chain(micro[0], micro[1], which)


@pytest.mark.parametrize("beam", [None, 3], ids=["greedy", "beam3"])
def test_conditioned_seek_loop_equals_the_python_loop(beam):
    eng = pf.cond_engine()
    pf.check_conditioned_loop(eng, beam=beam)
    eng.close()


def test_conditioning_off_is_waveform_to_segments():
    eng = pf.cond_engine()
    pf.check_conditioning_off(eng)
    eng.close()


def test_cli_segments_conditioned(tmp_path, monkeypatch):
    """`--segments PATH --condition-on-previous-text --initial-prompt TEXT`: the same record layout as --segments alone, the
    initial prompt in window 0's prompt and the decoded text in every later one (2 s of audio, windows of 0.9 s)."""
    import json
    import wave
    import numpy as np
    pytest.importorskip("tokenizers")
    from tokenizers import Tokenizer, models, pre_tokenizers
    from test_tokenizer_integration import N_VOCAB
    from whisper_burn_amd import dumpdir, synth
    from whisper_burn_amd import transcribe as cli
    monkeypatch.chdir(tmp_path)
    # test_tokenizer_integration's synthetic tokenizer with <|startofprev|> in the place of its last timestamp
    eot = N_VOCAB - 16
    vocab = {f"w{i}": i for i in range(eot)}
    vocab["<unk>"] = vocab.pop(f"w{eot - 1}")
    tok = Tokenizer(models.WordLevel(vocab=vocab, unk_token="<unk>"))
    tok.pre_tokenizer = pre_tokenizers.Whitespace()
    names = ["<|endoftext|>", "<|startoftranscript|>", "<|en|>", "<|zh|>", "<|transcribe|>", "<|translate|>", "<|startofprev|>",
             "<|notimestamps|>"] + [f"<|{0.02 * i:.2f}|>" for i in range(8)]
    assert tok.add_special_tokens(names) == 16
    tok.save(str(tmp_path / "tokenizer.json"))
    dims = synth.micro_dims(n_state=64, n_head=1, n_layer=1, n_vocab=N_VOCAB, n_audio_ctx=100)      # windows of 0.9 s
    dumpdir.write_dump_dir(synth.synth_weights(dims, seed=5), str(tmp_path / "micro"))
    audio = synth.synth_audio(32000, 52)
    pcm = np.clip(np.round(audio * 32767.0), -32768, 32767).astype("<i2")
    with wave.open(str(tmp_path / "a.wav"), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(pcm.tobytes())
    # what the flags reach: the call the CLI makes is repeated with return_windows, so the windows' prompt lengths are seen
    import whisper_burn_amd as wb
    real, seen = wb.waveform_to_segments, []

    def recording(*a, **kw):
        out = real(*a, return_windows=True, **kw)
        seen.append((kw, out[3]))
        return out[:3]

    monkeypatch.setattr(wb, "waveform_to_segments", recording)
    assert cli.main(["transcribe", "micro", "a.wav", "en", "plain.txt", "--segments", "plain.jsonl"]) == 0
    assert cli.main(["transcribe", "micro", "a.wav", "en", "seg.txt", "--segments", "seg.jsonl", "--condition-on-previous-text",
                     "--initial-prompt", "w3 w4"]) == 0
    (kw0, win0), (kw1, win1) = seen
    assert not kw0["condition_on_previous_text"] and kw0["initial_prompt"] is None and set(win0["prompt_len"]) == {3}
    assert kw1["condition_on_previous_text"] is True and kw1["initial_prompt"] == [3, 4]          # " w3 w4" through the adapter
    assert len(win1["prompt_len"]) >= 2 and win1["prompt_len"][0] == 1 + 2 + 3                     # the initial prompt, window 0
    assert all(pl > 1 + 2 + 3 for pl in win1["prompt_len"][1:]), win1                              # ... and the text crossed windows
    recs = [json.loads(ln) for ln in open(tmp_path / "seg.jsonl")]
    assert recs and all(set(r) == {"start", "end", "text", "tokens"} for r in recs)
    assert [r["start"] for r in recs] == sorted(r["start"] for r in recs)
    assert " ".join(r["text"] for r in recs if r["text"]) == open(tmp_path / "seg.txt").read()
