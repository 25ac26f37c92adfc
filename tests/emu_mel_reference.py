"""Driven by tests/test_mel_reference_frontend.py in a subprocess with WHISPER_HIP_LIB = lib/libwhisper_hip_emu.so: the
reference-recipe log-mel frontend (csrc/mel_dft.hip) executed through the hipemu functional model and compared with the
oracle's f32 restatement of the reference (oracle/mel.py).  Prints one JSON line of measured distances."""
import ctypes as C
import json
import sys

import numpy as np
import torch

import whisper_burn_amd as wb
from oracle import mel as omel
from whisper_burn_amd import _lib, synth

TOL = 5e-5


def silence_tail_clip():
    """~1.2 s: speech-like signal, then digital silence, so that bins sit at the clamp floor max - 8."""
    a = synth.synth_audio(19360, 21).astype(np.float32)
    a[12000:] = 0.0
    return a


def mel_case(name, a, out):
    got = wb.prep_audio(a[None], frontend="reference")[0]
    ref = omel.prep_audio(torch.from_numpy(a)[None])[0].numpy()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    out[name] = dict(ref=float(np.abs(got - ref).max()),
                     fft=float(np.abs(wb.prep_audio(a[None])[0] - ref).max()),
                     floor_bins=int(np.sum(np.isclose(ref, ref.min(), rtol=0, atol=1e-6))),
                     frames=int(ref.shape[1]))
    assert out[name]["ref"] <= TOL, (name, out[name])
    return ref


def main(which):
    assert b"hipemu" in _lib.load().wb_version()
    out = {}
    if which == "mel":
        ref = mel_case("silence_tail", silence_tail_clip(), out)
        # the clamp floor is really reached: the minimum is max - 8 and many bins sit on it
        vmax, vmin = float(ref.max()) * 4 - 4, float(ref.min()) * 4 - 4
        assert abs((vmax - vmin) - 8.0) < 1e-4 and out["silence_tail"]["floor_bins"] > 100, out
        mel_case("n400", synth.synth_audio(400, 5).astype(np.float32), out)          # 2 frames, reflect on both sides
        mel_case("n_odd", synth.synth_audio(16000 + 97, 6).astype(np.float32), out)  # n % 160 != 0
    elif which == "batched":
        lib = _lib.load()
        a = synth.synth_audio(16000 * 2 + 333, 9).astype(np.float32)
        starts = np.array([0, 8000, 401], dtype=np.int64)
        lens = np.array([16000 * 2 + 333, 9000, 12000], dtype=np.int64)
        clip, pad, rs = 150, 10, 212
        res = {}
        for fid, name in ((0, "fft"), (1, "reference")):
            mel = np.full((3, 80, rs), np.nan, dtype=np.float32)
            frames = np.zeros(3, dtype=np.int32)
            ms = C.c_double(0.0)
            _lib.check(lib.wb_waveform_to_mels_dev_frontend(
                0, C.c_void_p(a.ctypes.data), a.shape[0], 16000.0, starts.ctypes.data_as(_lib.c_int64_p),
                lens.ctypes.data_as(_lib.c_int64_p), 3, clip, pad, C.c_void_p(mel.ctypes.data), 80 * rs, rs,
                frames.ctypes.data_as(_lib.c_int32_p), 1, C.byref(ms), fid))
            res[name] = (mel, frames.copy())
        mel, frames = res["reference"]
        assert list(frames) == list(res["fft"][1]), (frames, res["fft"][1])
        dist = []
        for w in range(3):
            n_emit = int(min(lens[w] // 160, clip))
            assert frames[w] == n_emit + pad
            assert np.all(mel[w, :, n_emit:n_emit + pad] == 0.0), w         # padding frames are zero
            seg = a[starts[w]:starts[w] + lens[w]]
            ref = omel.prep_audio(torch.from_numpy(seg)[None])[0].numpy()[:, :n_emit]
            dist.append(float(np.abs(mel[w, :, :n_emit] - ref).max()))
        out["batched"] = dist
        assert max(dist) <= TOL, dist
        eng = wb.Whisper.from_tensors(synth.synth_weights(synth.micro_dims(n_state=128, n_head=2, n_layer=2,
                                                                           n_vocab=1031), seed=4242))
        assert lib.wb_model_set_frontend(eng._h, 2) == -1          # WB_ERR_ARG
        assert eng.frontend == "fft"
    else:
        raise SystemExit(f"unknown check {which}")
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1])
