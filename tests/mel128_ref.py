"""Shared by the 128-bin tests (tests/mel128_emu_checks.py under the hipemu functional model, tests/test_gpu_mel128.py on the
GPU, tests/test_mel128.py on the host): the f64 yardstick of the log-mel frontend for any number of mel rows, the frontend
cases and the micro fixtures.

Yardstick: oracle.mel.prep_audio_f64's steps (reflect pad, periodic Hann, real FFT, |X|^2, filterbank, log10 with the 1e-10
floor, clamp at max - 8 over ALL frames of the window, (x + 4) / 4) with the filterbank handed in -- prep_audio_f64 itself
binds 80 rows at definition.  The KERNEL is held to 5e-5 (the project's asserted mel bound) of the
evaluation with the library's own table (wb_mel_filterbank cast to f64): table design stays out of the kernel's bound; the
table is checked on its own against oracle.mel.mel_filters_f64(16000, 400, 128)."""
import ctypes as C
import math

import numpy as np

from oracle import mel as omel

MEL_TOL = 5e-5           # every bin of the log-mel
ENC_TOL = 2e-4           # encoder output vs the f32 oracle
LOGPROB_TOL = 1e-3       # log-probs vs the f32 oracle
DEPTH = 24


def logmel_f64(x, filt):
    """[N] -> [n_mels, N // 160] in f64 with the filterbank `filt` [n_mels, 201]."""
    x = np.asarray(x, dtype=np.float64)
    assert x.shape[0] >= omel.N_FFT
    xp = np.pad(x, (omel.N_FFT // 2, omel.N_FFT // 2), mode="reflect")
    n_frame = (xp.shape[0] - omel.N_FFT) // omel.HOP_LENGTH + 1
    frames = np.lib.stride_tricks.as_strided(xp, (n_frame, omel.N_FFT), (xp.strides[0] * omel.HOP_LENGTH, xp.strides[0]))
    win = np.sin(np.arange(omel.N_FFT) * (math.pi / omel.N_FFT)) ** 2
    spec = np.fft.rfft(frames * win[None, :], axis=1)
    power = (spec.real ** 2 + spec.imag ** 2)[:n_frame - 1].T
    log_spec = np.log10(np.maximum(np.asarray(filt, dtype=np.float64) @ power, 1e-10))
    log_spec = np.maximum(log_spec, log_spec.max() - 8.0)
    return (log_spec + 4.0) / 4.0


def lib_table(n_mels):
    import whisper_burn_amd as wb
    return wb.mel_filterbank(16000.0, n_mels).astype(np.float64)


def tone_then_zeros():
    """One window: 0.75 s of a -6 dBFS 1 kHz tone, then exact zeros -- whole tiles of the silence sit 80 dB under the
    window maximum, so the fix-up pass rewrites them."""
    n = 16000 * 3 // 2
    a = np.zeros(n, dtype=np.float32)
    t = np.arange(12000, dtype=np.float64)
    a[:12000] = (10.0 ** (-6.0 / 20.0) * np.sin(2.0 * math.pi * 1000.0 * t / 16000.0)).astype(np.float32)
    return a


class Buffers:
    """Device buffers of the batched entry: plain NumPy under the functional model (its device pointers are host
    pointers), torch tensors on the GPU."""

    def __init__(self, gpu):
        self.gpu = gpu

    def pcm(self, a):
        if self.gpu:
            import torch
            t = torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
            torch.cuda.synchronize()
            return t, t.data_ptr()
        a = np.ascontiguousarray(a, np.float32)
        return a, a.ctypes.data

    def out(self, shape):
        if self.gpu:
            import torch
            t = torch.full(shape, float("nan"), device="cuda")
            torch.cuda.synchronize()
            return t, t.data_ptr()
        a = np.full(shape, np.nan, dtype=np.float32)
        return a, a.ctypes.data

    def host(self, t):
        return t.cpu().numpy() if self.gpu else t


def batched(buf, a, starts, lens, clip, pad, rs, n_mels, entry="mels", offset_floats=0):
    """The batched entry into a canary-framed buffer [W][n_mels + 2][rs] of NaN: returns (mel [W][n_mels + 2][rs], frames).
    entry: "mels" (wb_waveform_to_mels_dev_mels) or "old" (wb_waveform_to_mels_dev_frontend, 80 rows)."""
    from whisper_burn_amd import _lib
    lib = _lib.load()
    W = len(starts)
    starts = np.ascontiguousarray(starts, dtype=np.int64)
    lens = np.ascontiguousarray(lens, dtype=np.int64)
    keep, pcm_ptr = buf.pcm(a)
    mel, mel_ptr = buf.out((W, n_mels + 2, rs))
    frames = np.zeros(W, dtype=np.int32)
    ms = C.c_double(0.0)
    args = [0, C.c_void_p(pcm_ptr), len(a), 16000.0, starts.ctypes.data_as(_lib.c_int64_p), lens.ctypes.data_as(_lib.c_int64_p),
            W, clip, pad, C.c_void_p(mel_ptr + 4 * (rs + offset_floats)), (n_mels + 2) * rs, rs,
            frames.ctypes.data_as(_lib.c_int32_p), 1, C.byref(ms)]
    if entry == "mels":
        _lib.check(lib.wb_waveform_to_mels_dev_mels(*args, n_mels, 0))
    else:
        _lib.check(lib.wb_waveform_to_mels_dev_frontend(*args, 0))
    del keep
    return buf.host(mel), frames


def check_window(name, got, a, n_emit, pad, filt, out):
    """got [n_mels + 2][rs] with canary rows 0 and n_mels + 1: the emitted frames against the yardstick, zero padding
    frames, every other element still NaN."""
    n_mels = got.shape[0] - 2
    ref = logmel_f64(a, filt)[:, :n_emit]
    err = float(np.abs(got[1:-1, :n_emit] - ref).max())
    out[name] = err
    print(f"{name}: {n_emit} frames, max |kernel - f64| = {err:.3e}")
    assert np.all(got[1:-1, n_emit:n_emit + pad] == 0.0), name
    assert np.isnan(got[0]).all() and np.isnan(got[-1]).all() and np.isnan(got[1:-1, n_emit + pad:]).all(), name
    assert err <= MEL_TOL, (name, err)
    assert ref.shape[0] == n_mels
    return ref


def frontend_cases(gpu, n_mels=128):
    """Every branch of the n_mels-row instance (see the module docstring for the bound).  Returns {case: max error}."""
    import whisper_burn_amd as wb
    from whisper_burn_amd import synth
    buf = Buffers(gpu)
    filt = lib_table(n_mels)
    out = {}
    # single-window entry: row stride = frames.  2 frames (one partial tile); 34 frames (a full tile on the element-wise
    # path, the stride is no multiple of 4, plus a partial one); 65 frames (two full tiles, misaligned stride)
    for n, seed in ((400, 5), (5440, 6), (10400, 8)):
        a = synth.synth_audio(n, seed).astype(np.float32)
        got = wb.prep_audio(a[None], n_mels=n_mels)[0]
        ref = logmel_f64(a, filt)
        assert got.shape == ref.shape == (n_mels, n // 160)
        out[f"n{n}"] = float(np.abs(got - ref).max())
        print(f"n{n}: {n // 160} frames, max |kernel - f64| = {out[f'n{n}']:.3e}")
        assert out[f"n{n}"] <= MEL_TOL, (n, out)
    # 64 frames, aligned stride: the 16-byte store path for both tiles
    a = synth.synth_audio(10240, 9).astype(np.float32)
    mel, frames = batched(buf, a, [0], [10240], 64, 0, 64, n_mels)
    assert list(frames) == [64]
    check_window("aligned64", mel[0], a, 64, 0, filt, out)
    # the same window with the output base 4 bytes off a 16-byte boundary: the element-wise path for full tiles
    mel, frames = batched(buf, a, [0], [10240], 64, 0, 68, n_mels, offset_floats=1)
    shifted = np.full((n_mels + 2, 68), np.nan, dtype=np.float32)
    flat = mel[0].reshape(-1)
    shifted.reshape(-1)[:-1] = flat[1:]
    check_window("misaligned64", shifted, a, 64, 0, filt, out)
    # two windows, clip and 10 zero frames: window 0 is clipped inside its third tile, window 1 is shorter (its zero frames
    # fall into tiles that hold no real frame of it)
    a = synth.synth_audio(16000 * 2 + 333, 9).astype(np.float32)
    starts, lens, clip, pad, rs = [0, 401], [16000 * 2 + 333, 9000], 150, 10, 164
    mel, frames = batched(buf, a, starts, lens, clip, pad, rs, n_mels)
    for w in range(2):
        n_emit = min(lens[w] // 160, clip)
        assert frames[w] == n_emit + pad
        check_window(f"clip_pad_w{w}", mel[w], a[starts[w]:starts[w] + lens[w]], n_emit, pad, filt, out)
    # a tile below max - 8: the fix-up pass rewrites it
    a = tone_then_zeros()
    mel, frames = batched(buf, a, [0], [len(a)], 1490, 10, 160, n_mels)
    ref = check_window("tone_then_zeros", mel[0], a, len(a) // 160, 10, filt, out)
    floor = ref.min()
    assert abs((ref.max() - floor) * 4.0 - 8.0) < 1e-9 and int((ref[:, 96:] == floor).sum()) == n_mels * (ref.shape[1] - 96)
    return out


def fixture(n_mels=128, seed=4243):
    """The micro fixture of unequal depths: 3 encoder layers over 1 decoder layer, n_audio_ctx 256."""
    from whisper_burn_amd import synth
    from whisper_burn_amd.tokens import SpecialTokens
    dims = synth.micro_dims(n_state=128, n_head=2, n_layer=3, n_vocab=1031, n_audio_ctx=256, n_mels=n_mels, n_text_layer=1)
    return dims, synth.synth_weights(dims, seed=seed), SpecialTokens.for_vocab(1031), synth.synth_audio(32000, 7)


def oracle_st(st):
    from oracle import transcribe as otr
    return otr.SpecialTokens(st.start_of_transcript, st.language, st.transcribe, st.no_timestamps, st.end_of_text,
                             np.asarray(st.is_special).astype(bool))


def exact_mel(audio, n_mels):
    """[1, n_mels, T] f32: the f64-designed table's exact log-mel, as parity_util.window_mels hands both sides at 80 rows."""
    import torch
    filt = omel.mel_filters_f64(16000.0, 400, n_mels)
    return torch.from_numpy(logmel_f64(audio, filt).astype(np.float32))[None]


def model_checks(eng, weights, st, audio, n_mels, from_pcm):
    """Encoder output, greedy tokens and every step's log-prob row of the fixture against the f32 oracle, which is fed the
    exact log-mel.  from_pcm: the engine side starts from PCM (its own frontend); else from the same log-mel."""
    import torch
    import parity_util
    import whisper_burn_amd as wb
    from oracle import transcribe as otr
    from oracle.model import OracleWhisper
    o32 = OracleWhisper(weights)
    ost = oracle_st(st)
    mel = exact_mel(audio, n_mels)
    T = mel.shape[2]
    melp = torch.cat([mel, torch.zeros(1, n_mels, 10)], 2)
    ref_enc = o32.forward_encoder(melp)[0].numpy()
    got_enc = eng.forward_encoder(melp.numpy())[0]
    e_enc = float(np.abs(got_enc - ref_enc).max())
    want = otr.mels_to_tokens(o32, ost, mel, 10, 1, DEPTH)
    assert len(want) >= 4 + 8, want                      # a decode worth comparing (the 128-bin fixture: 24 distinct tokens)
    if from_pcm:
        # (one window cut by hand: n_audio_ctx 256 is shorter than the 3 s overlap of the reference's window iterator)
        sess = wb.Session.begin(eng, audio, [0], [len(audio)], max_beams=1)
        sess.set_special_mask(st.is_special)
        got = sess.decode(wb.decode_params(st, 1, DEPTH))[0]
        sess.close()
        sess = wb.Session.begin(eng, audio, [0], [len(audio)], max_beams=1)
    else:
        sess = wb.Session.begin_mel(eng, [mel[0].numpy()], max_beams=1)
        sess.set_special_mask(st.is_special)
        got = sess.decode(wb.decode_params(st, 1, DEPTH))[0]
        sess.close()
        sess = wb.Session.begin_mel(eng, [mel[0].numpy()], max_beams=1)
    e_sess = float(np.abs(sess.encoder_output(0) - ref_enc).max())
    sess.set_special_mask(st.is_special)
    rows = []
    for p in range(len(want) - 1):
        sess.step([want[p]], [-1 if p == 0 else 0], [0], apply_special_mask=(p >= 3 and p + 1 <= 5), k=1 if p >= 3 else 0)
        if p >= 3:
            rows.append(sess.last_logprobs(0).copy())
    sess.close()
    ref_rows = parity_util.teacher_forced_logprobs(o32, st, torch.from_numpy(ref_enc), want[:-1])
    hip = np.stack(rows)
    fin = np.isfinite(ref_rows)
    assert np.array_equal(fin, np.isfinite(hip))
    e_lp = float(np.abs(hip[fin] - ref_rows[fin]).max())
    print(f"n_mels {n_mels}, {T} frames, from_pcm={from_pcm}: encoder {e_enc:.3e} (session {e_sess:.3e}), log-probs {e_lp:.3e}, "
          f"tokens {got[4:10]}...")
    assert e_enc <= ENC_TOL and e_lp <= LOGPROB_TOL, (e_enc, e_lp)
    assert got == want, (got, want)
    if not from_pcm:
        assert e_sess <= ENC_TOL, e_sess
    return dict(encoder=e_enc, session_encoder=e_sess, logprob=e_lp, tokens=want)


def timestamp_chain_check(eng, weights, st, audio, n_mels):
    """Session.decode_timestamps at depth 24 on the fixture: the rows of the oracle under the timestamp rules."""
    import torch
    import tsrules_ref as tr
    import whisper_burn_amd as wb
    from oracle.model import OracleWhisper
    o32 = OracleWhisper(weights)
    mel = exact_mel(audio, n_mels)
    enc = o32.forward_encoder(torch.cat([mel, torch.zeros(1, n_mels, 10)], 2))[0].numpy()
    R = tr.rules(tr.FIX_TB, tr.FIX_NTS, 50, -1)
    sup = (np.asarray(st.is_special) != 0).astype(np.uint8)
    sup[st.end_of_text] = 0
    prompt = [st.start_of_transcript, st.language, st.transcribe]
    want = tr.oracle_decode(o32, enc, prompt, R, st.end_of_text, sup, None, DEPTH)[0]
    sess = wb.Session.begin_mel(eng, [mel[0].numpy()], max_beams=1)
    sess.set_suppress(sup)
    rows, _, _ = sess.decode_timestamps(wb.decode_params(st, 1, DEPTH), wb.TimestampParams(R["tb"], R["n_ts"], R["max_init"], R["max_ts"]))
    sess.close()
    assert rows[0] == want, (rows[0], want)
    assert any(tr.is_ts(R, t) for t in want[3:])
    return want
