"""Driven by tests/test_mel128.py in a subprocess with WHISPER_HIP_LIB = lib/libwhisper_hip_emu.so: the 128-row instance of
the log-mel frontend (csrc/mel.hip) and a 128-bin model of unequal depths executed through the hipemu functional model,
against the f64 yardstick of tests/mel128_ref.py and the f32 oracle.  A check of the sources' logic on a machine without a
GPU; tests/test_gpu_mel128.py is the parity test proper."""
import sys

import numpy as np

import mel128_ref as mr
import whisper_burn_amd as wb
from whisper_burn_amd import _lib


def check_frontend():
    """Every branch of the 128-row instance, canary rows and columns around every batched output."""
    mr.frontend_cases(gpu=False, n_mels=128)


def check_frontend80():
    """The same cases through the 80-row instantiation of the now shared kernel body, and the new entries at 80 rows
    against the old ones bit for bit."""
    from whisper_burn_amd import synth
    mr.frontend_cases(gpu=False, n_mels=80)
    buf = mr.Buffers(False)
    a = synth.synth_audio(16000 * 2 + 333, 9).astype(np.float32)
    new, f1 = mr.batched(buf, a, [0, 401], [16000 * 2 + 333, 9000], 150, 10, 164, 80, entry="mels")
    old, f0 = mr.batched(buf, a, [0, 401], [16000 * 2 + 333, 9000], 150, 10, 164, 80, entry="old")
    assert list(f0) == list(f1) and np.array_equal(new.view(np.int32), old.view(np.int32))
    assert np.array_equal(wb.prep_audio(a[None], n_mels=80).view(np.int32), wb.prep_audio(a[None]).view(np.int32))


def check_micro():
    """The 128-bin fixture with 3 encoder layers over 1 decoder layer: encoder output, greedy tokens and log-prob rows
    against the f32 oracle from the same log-mel; the timestamp chain runs on it."""
    dims, weights, st, audio = mr.fixture(128)
    eng = wb.Whisper.from_tensors(weights)
    assert eng.dims["n_mels"] == 128 and eng.dims["n_audio_layer"] == 3 and eng.dims["n_text_layer"] == 1
    want = mr.model_checks(eng, weights, st, audio, 128, from_pcm=False)["tokens"]
    assert len(want) == 4 + mr.DEPTH and len(set(want[4:])) == mr.DEPTH and st.end_of_text not in want, want
    mr.timestamp_chain_check(eng, weights, st, audio, 128)
    eng.close()


def check_pcm():
    """From PCM: the session's own 128-row frontend feeds the encoder (the oracle gets the exact log-mel)."""
    dims, weights, st, audio = mr.fixture(128)
    eng = wb.Whisper.from_tensors(weights)
    mr.model_checks(eng, weights, st, audio, 128, from_pcm=True)
    eng.close()


def check_refuse():
    """The reference recipe has no 128-row form: refused at the model, per call, and the mode stays; other row counts are
    refused by the loader with WB_ERR_SHAPE."""
    from whisper_burn_amd import synth
    lib = _lib.load()
    dims, weights, st, audio = mr.fixture(128)
    eng = wb.Whisper.from_tensors(weights)
    assert lib.wb_model_set_frontend(eng._h, 1) == -1 and eng.frontend == "fft"
    assert b"80 mel rows" in lib.wb_last_error()
    try:
        eng.set_frontend("reference")
        raise AssertionError("set_frontend('reference') on a 128-bin model")
    except wb.WbError as e:
        assert e.status == -1
    assert eng.frontend == "fft"
    assert lib.wb_model_set_frontend(eng._h, 0) == 0
    try:
        eng.forward_encoder(np.zeros((1, 80, 32), np.float32))
        raise AssertionError("an 80-row mel into a 128-bin model")
    except wb.WbError as e:
        assert e.status == -2
    eng.close()
    try:
        wb.prep_audio(audio[None], frontend="reference", n_mels=128)
        raise AssertionError("reference recipe at 128 rows")
    except wb.WbError as e:
        assert e.status == -1
    for bad in (0, 64, 96, 129):
        try:
            wb.prep_audio(audio[None], n_mels=bad)
            raise AssertionError(bad)
        except wb.WbError as e:
            assert e.status == -1, (bad, e.status)
    d96 = synth.micro_dims(n_state=64, n_head=1, n_layer=1, n_vocab=263, n_audio_ctx=64, n_mels=96)
    try:
        wb.Whisper.from_tensors(synth.synth_weights(d96, seed=1))
        raise AssertionError("a 96-bin model loaded")
    except wb.WbError as e:
        assert e.status == -2 and "n_mels 96" in str(e), (e.status, str(e))
    eng80 = wb.Whisper.from_tensors(synth.synth_weights(synth.micro_dims(n_state=64, n_head=1, n_layer=1, n_vocab=263,
                                                                         n_audio_ctx=64), seed=1))
    eng80.set_frontend("reference")
    assert eng80.frontend == "reference"
    eng80.close()


def check_depths80():
    """80 bins with 3 encoder layers over 1 decoder layer: the depth change alone."""
    dims, weights, st, audio = mr.fixture(80, seed=4244)
    eng = wb.Whisper.from_tensors(weights)
    mr.model_checks(eng, weights, st, audio, 80, from_pcm=False)
    eng.close()


CHECKS = {"frontend": check_frontend, "frontend80": check_frontend80, "micro": check_micro, "pcm": check_pcm,
          "refuse": check_refuse, "depths80": check_depths80}

if __name__ == "__main__":
    assert b"hipemu" in _lib.load().wb_version()
    CHECKS[sys.argv[1]]()
    print("OK", sys.argv[1])
