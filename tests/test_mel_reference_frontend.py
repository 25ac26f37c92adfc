"""CPU: the reference-recipe log-mel frontend (WB_FRONTEND_REFERENCE, csrc/mel_dft.hip).

- its DFT operand (wb_mel_dft_table, host only) against the oracle's own operands (oracle/mel.py: stfft);
- the kernel itself through the hipemu functional model (tests/emu_mel_reference.py in a child process, as
  test_emu_functional.py runs its checks) against oracle.mel.prep_audio, <= 5e-5 on every bin;
- the mode switch's argument check on the product library (no GPU needed: it fails before any device work)."""
import ctypes as C
import json
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "whisper-burn_amd")
for _p in (ROOT, PKG):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import whisper_burn_amd as wb  # noqa: E402
from oracle import mel as omel  # noqa: E402
from whisper_burn_amd import _lib  # noqa: E402

EMU_DIR = os.path.join(PKG, "tools", "hipemu")
EMU_LIB = os.path.join(PKG, "lib", "libwhisper_hip_emu.so")
CLANG = os.environ.get("EMUCXX", "/opt/rocm/lib/llvm/bin/clang++")


def _oracle_operands():
    """audio.rs:348-364 as the oracle builds them: (cos(b) * w, sin(b) * (-w)), each [201, 400] f32."""
    win = omel.hann_window(400)
    coe = math.pi * 2.0 / 400
    b = (torch.arange(201).float() * omel._f32(coe))[:, None].repeat(1, 400) * torch.arange(400).float()[None, :]
    return b, (torch.cos(b) * win[None, :]).numpy(), (torch.sin(b) * (-win)[None, :]).numpy()


def test_dft_table_matches_oracle_operands():
    t = wb.mel_dft_table()
    assert t.shape == (402, 400) and t.dtype == np.float32
    b, re, im = _oracle_operands()
    # The table holds the oracle's f32 angles exactly: with the library's own Hann window, its rows are cos / sin of
    # those angles correctly rounded to f32, times w, in f32.
    hann = np.zeros(400, np.float32)
    filt = np.zeros((80, 201), np.float32)
    assert _lib.load().wb_mel_constants(16000.0, hann.ctypes.data_as(_lib.c_float_p),
                                        filt.ctypes.data_as(_lib.c_float_p)) == 0
    b64 = b.numpy().astype(np.float64)
    assert np.array_equal(t[0::2], np.cos(b64).astype(np.float32) * hann[None, :])
    assert np.array_equal(t[1::2], np.sin(b64).astype(np.float32) * (-hann)[None, :])
    # Against the oracle's operands: torch's f32 cos / sin and Hann window are each within 1 ulp of the correctly
    # rounded values (test_host_logic: Hann <= 2e-7), so the products agree to <= 2 ulp of 1.
    d = max(np.abs(t[0::2] - re).max(), np.abs(t[1::2] - im).max())
    assert d <= 2.4e-7, d
    assert np.abs(t[0::2] - re).mean() < 1e-8 and np.abs(t[1::2] - im).mean() < 1e-8


def test_frontend_argument_checks():
    lib = _lib.load()
    with pytest.raises(ValueError):
        wb.prep_audio(np.zeros((1, 400), np.float32), frontend="dft")
    mel = np.zeros((80, 2), np.float32)
    nf = C.c_int64(0)
    pcm = np.zeros(400, np.float32)
    assert lib.wb_prep_audio_frontend(0, pcm.ctypes.data_as(_lib.c_float_p), 400, 16000.0,
                                      mel.ctypes.data_as(_lib.c_float_p), C.byref(nf), 2) == -1    # WB_ERR_ARG
    assert lib.wb_model_set_frontend(None, 1) == -1 and lib.wb_model_frontend(None) == -1


@pytest.fixture(scope="module")
def emu_lib():
    if not (os.path.exists(CLANG) or shutil.which(CLANG)):
        pytest.skip("no host clang++ for the hipemu build")
    subprocess.run(["make", "-C", EMU_DIR, "-j", str(min(8, os.cpu_count() or 1))], check=True,
                   stdout=subprocess.DEVNULL)
    return EMU_LIB


def _emu(emu_lib, which):
    env = dict(os.environ)
    env["WHISPER_HIP_LIB"] = emu_lib
    env["WHISPER_HIP_ALLOW_EMU"] = "1"
    env["PYTHONPATH"] = os.pathsep.join([ROOT, PKG, os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
    env.setdefault("OMP_NUM_THREADS", "2")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "emu_mel_reference.py"), which], env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_emu_reference_mel_matches_oracle(emu_lib):
    """A 1.2 s clip with a digital-silence tail (bins at the clamp floor), a 400-sample window (2 frames, reflect on
    both sides) and n % 160 != 0: reference mode <= 5e-5 from oracle.mel.prep_audio on every bin."""
    out = _emu(emu_lib, "mel")
    assert set(out) == {"silence_tail", "n400", "n_odd"}
    for name, r in out.items():
        assert r["ref"] <= 5e-5, (name, r)
    assert out["silence_tail"]["floor_bins"] > 100
    assert out["n400"]["frames"] == 2


def test_emu_reference_batched_and_bad_mode(emu_lib):
    """wb_waveform_to_mels_dev_frontend with clip and padding: zero padding frames, the default mode's frames_out, every
    emitted bin <= 5e-5 from the oracle; wb_model_set_frontend(m, 2) -> WB_ERR_ARG."""
    out = _emu(emu_lib, "batched")
    assert len(out["batched"]) == 3 and max(out["batched"]) <= 5e-5, out
