"""GPU: the reference-recipe log-mel frontend (wb_model_set_frontend(m, 1), csrc/mel_dft.hip) on the MI355X.

The default frontend (K1, an exact-twiddle FFT) is closer to the true log-mel than the reference, whose dense f32 DFT
uses f32 angles up to ~1250 rad; on the reference's own audio.wav that gap is 1.07e-2 in log-prob units, which is why
test_gpu_budget.py / test_gpu_e2e.py widen their gate by the frontend term.  In reference mode the product path computes
the reference's recipe, so the comparison with the f32 oracle from PCM holds at the project's 1e-3 outright:

  mel        reference mode vs oracle.mel.prep_audio <= 5e-5 on every bin (floor bins included), on audio.wav, the 3
             windows of the tiny_bench workload and the base.en e2e clip; the default mode's distance is recorded next to it
  log-probs  |hip_ref - o32| <= 1e-3 from PCM, no frontend allowance: tiny.en on audio.wav and bench window 0, base.en
             at depth 32
  tokens     waveform_to_tokens in reference mode = the committed oracle rows (tiny_bench greedy, tiny_beam5); the _dev
             and sharded (world 1) entries return the host entry's rows
  default    switching the mode on and off again leaves the default path bit-identical
"""
import numpy as np
import pytest
import torch

import parity_log
import workloads
import whisper_burn_amd as wb
from oracle import mel as omel
from oracle.model import OracleWhisper
from test_oracle_golden import golden
from test_gpu_workloads import rows_of
from whisper_burn_amd import shard, synth

pytestmark = pytest.mark.gpu

MEL_TOL = 5e-5
LOGPROB_TOL = 1e-3
WLEN = 238559            # max_waveform_samples(1490), transcribe.rs:32-34
N_CLIP = 190559          # the base.en e2e clip of test_gpu_e2e.py (one window)


def _clip(name):
    if name == "audio_wav":
        return [np.ascontiguousarray(golden()[1], np.float32)]
    if name == "tiny_bench":
        a = np.ascontiguousarray(workloads.WORKLOADS["tiny_bench"].audio(), np.float32)
        starts, lens = wb.window_extents(len(a), 16000, WLEN)
        assert len(starts) == 3
        return [a[s:s + n] for s, n in zip(starts, lens)]
    return [np.ascontiguousarray(synth.synth_audio(N_CLIP, 1237), np.float32)]


@pytest.mark.parametrize("clip", ["audio_wav", "tiny_bench", "base_e2e"])
def test_reference_mel_matches_oracle(clip):
    worst_ref, worst_fft, floor_bins = 0.0, 0.0, 0
    for a in _clip(clip):
        ref = omel.prep_audio(torch.from_numpy(a)[None])[0].numpy()
        got = wb.prep_audio(a[None], frontend="reference")[0]
        fft = wb.prep_audio(a[None])[0]
        assert got.shape == ref.shape
        worst_ref = max(worst_ref, float(np.abs(got - ref).max()))
        worst_fft = max(worst_fft, float(np.abs(fft - ref).max()))
        floor = ref <= ref.min() + 1e-6
        floor_bins += int(floor.sum())
        # bins at the clamp floor max - 8 are held to the same bound (audio.wav's upper bands sit there)
        assert float(np.abs(got - ref)[floor].max()) <= MEL_TOL
    parity_log.record(f"mel_reference::prep_audio[{clip}] reference mode vs oracle f32 mel", worst_ref, MEL_TOL,
                      default_mode_vs_oracle=worst_fft, floor_bins=floor_bins)
    print(f"{clip}: reference mode {worst_ref:.3e}, default mode {worst_fft:.3e} from the oracle mel; {floor_bins} floor bins")
    assert worst_ref <= MEL_TOL, (worst_ref, worst_fft)


def test_reference_mel_batched_device_entry():
    """wb_waveform_to_mels_dev_frontend over the 3 bench windows: each window equals the single-window reference-mode
    mel (clip 1490, 10 zero frames), frames_out equals the default mode's."""
    wins = _clip("tiny_bench")
    a = np.ascontiguousarray(workloads.WORKLOADS["tiny_bench"].audio(), np.float32)
    starts, lens = wb.window_extents(len(a), 16000, WLEN)
    x = torch.from_numpy(a).cuda()
    rs = 1500
    out = {}
    for fe in ("fft", "reference"):
        mel = torch.full((3, 80, rs), float("nan"), device="cuda")
        torch.cuda.synchronize()
        frames, _ = wb.waveform_to_mels_dev(x.data_ptr(), len(a), starts, lens, mel.data_ptr(), 80 * rs, rs,
                                            frontend=fe)
        out[fe] = (mel.cpu().numpy(), list(frames))
    mel, frames = out["reference"]
    assert frames == out["fft"][1]
    for w, seg in enumerate(wins):
        single = wb.prep_audio(seg[None], frontend="reference")[0]
        n_emit = min(single.shape[1], 1490)
        assert frames[w] == n_emit + 10
        assert np.array_equal(mel[w, :, :n_emit], single[:, :n_emit]), w
        assert np.all(mel[w, :, n_emit:n_emit + 10] == 0.0)


def _rows(o, st, mel, row, dtype=torch.float32):
    """Teacher-forced masked log-softmax rows (transcribe.rs:271-284) of `row` from a [1, 80, T] log-mel (the row
    construction of test_gpu_budget.py)."""
    mel = torch.as_tensor(mel).to(dtype)
    keep = min(mel.shape[2], o.encoder_ctx_size() - 10)
    melp = torch.cat([mel[:, :, :keep], torch.zeros(1, 80, 10, dtype=dtype)], 2)        # transcribe.rs:171-177
    enc = o.forward_encoder(melp)
    lg = o.forward_decoder(torch.tensor([row], dtype=torch.long), enc)[0]
    maskv = torch.tensor(np.where(np.asarray(st.is_special).astype(bool), -np.inf, 0.0), dtype=dtype)
    out = []
    for p in range(3, len(row) - 1):
        v = lg[p] + (maskv if p + 1 <= 5 else 0.0)
        out.append((v - v.max() - torch.log(torch.exp(v - v.max()).sum())).numpy())
    return np.stack(out)


def _hip_rows(eng, st, audio, row):
    """Every step's log-prob row of `row` from a KV-cached session begun from PCM (the model's frontend)."""
    starts, lens = wb.window_extents(len(audio), 16000, WLEN)
    sess = wb.Session.begin(eng, audio, starts[:1], lens[:1], max_beams=1)
    sess.set_special_mask(st.is_special)
    hip = []
    for p in range(len(row) - 1):
        sess.step([row[p]], [-1 if p == 0 else 0], [0], apply_special_mask=(p >= 3 and p + 1 <= 5), k=1 if p >= 3 else 0)
        if p >= 3:
            hip.append(sess.last_logprobs(0).copy())
    sess.close()
    return np.stack(hip)


@pytest.mark.parametrize("case", ["tiny_en-audio_wav", "tiny_en-bench_window0", "base_en-depth32"])
def test_reference_mode_logprobs_from_pcm_within_1e3_of_oracle_f32(case):
    if case.startswith("tiny_en"):
        w = workloads.WORKLOADS["tiny_bench"].weights()
        audio = golden()[1] if case.endswith("audio_wav") else workloads.WORKLOADS["tiny_bench"].audio()[:WLEN]
        depth = 48
    else:
        w = synth.synth_preset("base.en", eot_beta=0.0)
        audio = synth.synth_audio(N_CLIP, 1237)
        depth = 32
    audio = np.ascontiguousarray(audio, np.float32)
    eng = wb.Whisper.from_tensors(w)
    eng.set_frontend("reference")
    assert eng.frontend == "reference"
    st = wb.SpecialTokens.for_vocab(eng.dims["n_vocab"])
    _, wins = wb.waveform_to_tokens(eng, st, audio, 16000, 1, depth)
    row = wins[0]
    assert len(row) >= 6
    if case == "base_en-depth32":
        assert len(row) == 4 + depth
    hip = _hip_rows(eng, st, audio, row)
    eng.close()
    o32 = OracleWhisper(w)
    r32 = _rows(o32, st, omel.prep_audio(torch.from_numpy(audio)[None]), row)
    fin = np.isfinite(r32)
    assert (np.isfinite(hip) == fin).all()
    with np.errstate(invalid="ignore"):          # (-inf - -inf at the masked special tokens: excluded by `fin`)
        d = float(np.abs(hip - r32)[fin].max())
    parity_log.record(f"mel_reference::pcm_to_logprob[{case}] hip(reference frontend) vs oracle f32, from PCM", d,
                      LOGPROB_TOL, float(np.abs(r32[fin]).max()), n_rows=hip.shape[0])
    print(f"{case}: {hip.shape[0]} rows; hip(reference frontend) vs oracle f32 from PCM {d:.3e}")
    assert d <= LOGPROB_TOL, d


@pytest.mark.parametrize("name", ["tiny_bench", "tiny_beam5"])
def test_reference_mode_tokens_match_committed_oracle_rows(name):
    wl = workloads.WORKLOADS[name]
    eng = wb.Whisper.from_tensors(wl.weights())
    eng.set_frontend("reference")
    st = wb.SpecialTokens.for_vocab(eng.dims["n_vocab"])
    audio = np.ascontiguousarray(wl.audio(), np.float32)
    full, wins = wb.waveform_to_tokens(eng, st, audio, 16000, wl.beam, wl.depth)
    ref = rows_of(name)
    assert len(wins) == len(ref)
    for i, (g, r) in enumerate(zip(wins, ref)):
        assert g == r, (name, "window", i)
    if name == "tiny_bench":
        # the device-resident and the sharded (world 1) entries read the same mode
        x = torch.from_numpy(audio).cuda()
        torch.cuda.synchronize()
        full_dev, wins_dev = wb.waveform_to_tokens(eng, st, None, 16000, wl.beam, wl.depth, device_ptr=x.data_ptr(),
                                                   n_samples=len(audio))
        assert wins_dev == wins and full_dev == full
        params = wb.decode_params(st, wl.beam, wl.depth)
        full_sh, wins_sh = shard.waveform_to_tokens_sharded(eng, st, audio, 0, 1, params=params)
        assert wins_sh == wins and full_sh == full
    eng.close()


def test_default_mode_bit_identical_after_switching_back():
    wl = workloads.WORKLOADS["tiny_bench"]
    audio = np.ascontiguousarray(wl.audio()[:WLEN], np.float32)
    eng = wb.Whisper.from_tensors(wl.weights())
    st = wb.SpecialTokens.for_vocab(eng.dims["n_vocab"])
    assert eng.frontend == "fft"
    mel0 = wb.prep_audio(audio[None])[0]
    _, wins0 = wb.waveform_to_tokens(eng, st, audio, 16000, 1, 24)
    lp0 = _hip_rows(eng, st, audio, wins0[0])
    eng.set_frontend("reference")
    mel_r = wb.prep_audio(audio[None], frontend="reference")[0]
    lp_r = _hip_rows(eng, st, audio, wins0[0])
    assert not np.array_equal(mel_r, mel0) and not np.array_equal(lp_r, lp0)     # the mode reached the session
    eng.set_frontend("fft")
    assert eng.frontend == "fft"
    mel1 = wb.prep_audio(audio[None])[0]
    _, wins1 = wb.waveform_to_tokens(eng, st, audio, 16000, 1, 24)
    lp1 = _hip_rows(eng, st, audio, wins0[0])
    assert np.array_equal(mel0, mel1) and wins1 == wins0
    assert np.array_equal(lp0, lp1, equal_nan=True)
    with pytest.raises(ValueError):
        eng.set_frontend("dft")
    assert eng.frontend == "fft"
    eng.close()
