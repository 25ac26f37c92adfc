"""Frontend throughput of the two log-mel modes (WB_FRONTEND_FFT / WB_FRONTEND_REFERENCE) on one GPU.

  batched   wb_waveform_to_mels_dev_frontend over N reference-length windows (14.9 s, 1490 frames each) of one
            device-resident clip, `iters` passes timed by HIP events on the launch stream -> G frames/s; the reference
            recipe's fraction of its f32-MFMA ceiling (157.3 TF / 332.8 kFLOP per frame = 0.47 G frames/s)
  step      the mel stage of bench.py's tiny.en step (3 windows, greedy, depth 100) from PCM in each mode
            (wb_profile_read: [0] = mel ms, [5] = mel launches)

Prints one JSON object.  `python whisper-burn_amd/tools/mel_reference_rate.py [n_windows] [iters]`
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "whisper-burn_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import whisper_burn_amd as wb  # noqa: E402
from whisper_burn_amd import _lib, synth  # noqa: E402

WLEN = 238559
FLOP_PER_FRAME = 416 * 400 * 2
PEAK_F32_MFMA = 157.3e12


def batched(n_windows, iters):
    hop = 80000
    n = hop * (n_windows - 1) + WLEN
    a = np.ascontiguousarray(synth.synth_audio(n, 31), np.float32)
    x = torch.from_numpy(a).cuda()
    starts = np.arange(n_windows, dtype=np.int64) * hop
    lens = np.full(n_windows, WLEN, dtype=np.int64)
    rs = 1500
    mel = torch.empty((n_windows, 80, rs), device="cuda")
    torch.cuda.synchronize()
    out = {}
    for fe in ("fft", "reference"):
        wb.waveform_to_mels_dev(x.data_ptr(), n, starts, lens, mel.data_ptr(), 80 * rs, rs, frontend=fe)   # warm-up
        frames, ms = wb.waveform_to_mels_dev(x.data_ptr(), n, starts, lens, mel.data_ptr(), 80 * rs, rs, frontend=fe,
                                             iters=iters)
        n_frames = int(n_windows * (WLEN // 160))        # frames computed per pass (emitted + the one past the clip)
        rate = n_frames * iters / (ms * 1e-3)
        out[fe] = dict(ms_per_pass=ms / iters, frames_per_pass=n_frames, G_frames_per_s=rate / 1e9)
    out["reference"]["ceiling_G_frames_per_s"] = PEAK_F32_MFMA / FLOP_PER_FRAME / 1e9
    out["reference"]["frac_of_ceiling"] = out["reference"]["G_frames_per_s"] / out["reference"]["ceiling_G_frames_per_s"]
    out["reference"]["TFLOPs"] = out["reference"]["G_frames_per_s"] * FLOP_PER_FRAME / 1e3
    return dict(n_windows=n_windows, iters=iters, **out)


def step_mel_ms(reps=5):
    import workloads
    lib = _lib.load()
    wl = workloads.WORKLOADS["tiny_bench"]
    eng = wb.Whisper.from_tensors(wl.weights())
    st = wb.SpecialTokens.for_vocab(eng.dims["n_vocab"])
    audio = np.ascontiguousarray(wl.audio(), np.float32)
    out = {}
    buf = np.zeros(8, dtype=np.float64)
    for fe in ("fft", "reference"):
        eng.set_frontend(fe)
        wb.waveform_to_tokens(eng, st, audio, 16000, 1, 100)          # warm-up (tables, sessions, graphs)
        lib.wb_profile_enable(1)
        lib.wb_profile_read(buf.ctypes.data_as(_lib.c_double_p), 1)
        for _ in range(reps):
            wb.waveform_to_tokens(eng, st, audio, 16000, 1, 100)
        lib.wb_profile_read(buf.ctypes.data_as(_lib.c_double_p), 1)
        lib.wb_profile_enable(0)
        out[fe] = dict(mel_ms_per_step=float(buf[0]) / reps, encoder_ms_per_step=float(buf[1]) / reps,
                       decode_ms_per_step=float(buf[3]) / reps, mel_launches=float(buf[5]) / reps)
    eng.close()
    return out


if __name__ == "__main__":
    nw = int(sys.argv[1]) if len(sys.argv) > 1 else 120
    it = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    print(json.dumps(dict(batched=batched(nw, it), tiny_step=step_mel_ms()), indent=1))
