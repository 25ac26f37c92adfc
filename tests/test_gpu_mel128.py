"""GPU: 128-bin log-mel models (large-v3, large-v3-turbo) on the MI355X.

  frontend   every branch of csrc/mel.hip's 128-row instance (tests/mel128_ref.py: frontend_cases) through the product
             library, canary rows and columns around every batched output, and prep_audio(n_mels=128) on 3 s of audio:
             every bin within 5e-5 of the f64 evaluation with the library's own table
  model      the micro fixture (128 bins, 3 encoder layers over 1 decoder layer, seed 4243) through Whisper.from_tensors:
             forward_encoder within 2e-4 and every log-prob row within 1e-3 of the f32 oracle, greedy tokens identical, from
             the exact log-mel and from PCM (the oracle is fed the f64 128-bin log-mel through mels_to_tokens, as
             parity_util.window_mels does at 80 rows); Session.decode_timestamps at depth 24 returns the oracle's rows
  depths     the same fixture shape at 80 bins: the depth change without the bin change
  guard      at 80 rows the new entries return the old entries' bits, and the micro model of __graft_entry__.smoke still
             decodes the oracle's tokens"""
import numpy as np
import pytest

import mel128_ref as mr
import whisper_burn_amd as wb
from whisper_burn_amd import synth

pytestmark = pytest.mark.gpu


def test_frontend_128_every_branch_within_the_mel_bound():
    out = mr.frontend_cases(gpu=True, n_mels=128)
    assert set(out) == {"n400", "n5440", "n10400", "aligned64", "misaligned64", "clip_pad_w0", "clip_pad_w1", "tone_then_zeros"}


def test_prep_audio_128_on_three_seconds():
    a = synth.synth_audio(16000 * 3, 7)
    got = wb.prep_audio(a[None], n_mels=128)[0]
    ref = mr.logmel_f64(a, mr.lib_table(128))
    err = float(np.abs(got - ref).max())
    print(f"prep_audio(n_mels=128), 300 frames: max |kernel - f64| = {err:.3e}")
    assert got.shape == (128, 300) and err <= mr.MEL_TOL, err
    again = wb.prep_audio(a[None], n_mels=128)[0]
    assert np.array_equal(got.view(np.int32), again.view(np.int32))


@pytest.fixture(scope="module")
def fix128():
    dims, weights, st, audio = mr.fixture(128)
    eng = wb.Whisper.from_tensors(weights, device=0)
    yield eng, weights, st, audio
    eng.close()


def test_micro_128_from_the_exact_mel(fix128):
    eng, weights, st, audio = fix128
    assert eng.dims["n_mels"] == 128 and eng.dims["n_audio_layer"] == 3 and eng.dims["n_text_layer"] == 1
    want = mr.model_checks(eng, weights, st, audio, 128, from_pcm=False)["tokens"]
    assert len(want) == 4 + mr.DEPTH and len(set(want[4:])) == mr.DEPTH and st.end_of_text not in want


def test_micro_128_from_pcm(fix128):
    eng, weights, st, audio = fix128
    mr.model_checks(eng, weights, st, audio, 128, from_pcm=True)


def test_micro_128_timestamp_chain(fix128):
    eng, weights, st, audio = fix128
    mr.timestamp_chain_check(eng, weights, st, audio, 128)


def test_micro_128_refuses_the_reference_frontend(fix128):
    eng, _, _, audio = fix128
    with pytest.raises(wb.WbError) as e:
        eng.set_frontend("reference")
    assert e.value.status == -1 and eng.frontend == "fft"
    with pytest.raises(wb.WbError) as e:
        wb.prep_audio(audio[None], frontend="reference", n_mels=128)
    assert e.value.status == -1


def test_micro_80_bins_unequal_depths():
    dims, weights, st, audio = mr.fixture(80, seed=4244)
    eng = wb.Whisper.from_tensors(weights, device=0)
    mr.model_checks(eng, weights, st, audio, 80, from_pcm=False)
    mr.model_checks(eng, weights, st, audio, 80, from_pcm=True)
    eng.close()


def test_80_rows_through_the_new_entries_are_the_old_entries_bits():
    buf = mr.Buffers(True)
    for n, seed in ((400, 5), (5440, 6), (10400, 8), (48000, 7)):
        a = synth.synth_audio(n, seed).astype(np.float32)
        assert np.array_equal(wb.prep_audio(a[None], n_mels=80).view(np.int32), wb.prep_audio(a[None]).view(np.int32)), n
        from whisper_burn_amd import _lib
        import ctypes as C
        new, nf = np.empty((80, n // 160), np.float32), C.c_int64(0)
        _lib.check(_lib.load().wb_prep_audio_mels(0, a.ctypes.data_as(_lib.c_float_p), n, 16000.0, 80,
                                                  new.ctypes.data_as(_lib.c_float_p), C.byref(nf)))
        assert nf.value == n // 160 and np.array_equal(new.view(np.int32), wb.prep_audio(a[None])[0].view(np.int32)), n
    a = synth.synth_audio(16000 * 2 + 333, 9).astype(np.float32)
    cases = [(a, [0, 401], [16000 * 2 + 333, 9000], 150, 10, 164), (a[:10240], [0], [10240], 64, 0, 64),
             (mr.tone_then_zeros(), [0], [24000], 1490, 10, 160)]
    for x, starts, lens, clip, pad, rs in cases:
        new, f1 = mr.batched(buf, x, starts, lens, clip, pad, rs, 80, entry="mels")
        old, f0 = mr.batched(buf, x, starts, lens, clip, pad, rs, 80, entry="old")
        assert list(f0) == list(f1) and np.array_equal(new.view(np.int32), old.view(np.int32)), (starts, rs)
    mr.frontend_cases(gpu=True, n_mels=80)


def test_the_smoke_model_still_decodes_the_oracles_tokens():
    from oracle import transcribe as otr
    from oracle.model import OracleWhisper
    dims = synth.micro_dims(n_state=128, n_head=2, n_layer=2, n_vocab=1031)
    weights = synth.synth_weights(dims, seed=4242)
    eng = wb.Whisper.from_tensors(weights, device=0)
    st = wb.SpecialTokens.for_vocab(dims["n_vocab"])
    audio = synth.synth_audio(16000 * 3, 7)
    got, _ = wb.waveform_to_tokens(eng, st, audio, 16000, beam_size=1, max_depth=6)
    ref = otr.waveform_to_tokens(OracleWhisper(weights), mr.oracle_st(st), audio, 16000, 1, 6)
    assert got == ref
    mel = wb.prep_audio(audio[None])[0]
    enc_a = eng.forward_encoder(mel[None])
    sess = wb.Session.begin_mel(eng, [mel], max_beams=1)
    # the stateless and the session encoder read the same [80][Ts] layout as before: equal to each other on the clipped mel
    assert np.abs(sess.encoder_output(0) - eng.forward_encoder(np.concatenate([mel, np.zeros((80, 10), np.float32)], 1)[None])[0]).max() <= 1e-5
    sess.close()
    assert enc_a.shape == (1, 150, 128)
    eng.close()
