"""CPU: 128-bin log-mel models (large-v3, large-v3-turbo).

 * host only: the 128-row filterbank the kernel uses (wb_mel_filterbank) against oracle.mel.mel_filters_f64(16000, 400, 128)
   within one f32 rounding plus the 4e-7 x max|w| allowance test_host_logic gives the 80-row table; at most 9 taps per row,
   no empty row; the 80-row table of the new entry equals wb_mel_constants' bit for bit; bad n_mels -> WB_ERR_ARG;
 * csrc/mel.hip's 128-row instance and a 128-bin model of unequal depths executed through the hipemu functional model
   (tests/mel128_emu_checks.py, one subprocess per check);
 * the presets and the ABI surface: header, library, ctypes binding and Rust shim name the new functions."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import whisper_burn_amd as wb
from oracle import mel as omel
from whisper_burn_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "whisper-burn_amd")
EMU_DIR = os.path.join(PKG, "tools", "hipemu")
EMU_LIB = os.path.join(PKG, "lib", "libwhisper_hip_emu.so")
CLANG = os.environ.get("EMUCXX", "/opt/rocm/lib/llvm/bin/clang++")
NEW = ["wb_prep_audio_mels", "wb_waveform_to_mels_dev_mels", "wb_mel_filterbank"]


def test_filterbank_128_is_the_f64_design_rounded_once():
    filt = wb.mel_filterbank(16000.0, 128)
    ref = omel.mel_filters_f64(16000.0, 400, 128)
    assert filt.shape == ref.shape == (128, 201) and filt.dtype == np.float32
    scale = np.abs(ref).max()
    # one cast: half an ulp of the weight; + the allowance of the 80-row table test for libm's exp / log
    bound = np.abs(ref) * 2.0 ** -24 + 4e-7 * scale
    assert (np.abs(filt.astype(np.float64) - ref) <= bound).all(), float(np.abs(filt - ref).max())
    nz = (filt != 0).sum(1)
    assert nz.min() >= 1 and nz.max() <= 9 and int((filt != 0).sum()) == 394
    for m in range(128):                                       # each row's taps are one contiguous run
        k = np.flatnonzero(filt[m])
        assert k[-1] - k[0] + 1 == len(k)
    # the reference's f32 op order at 128 rows is what the f64 design replaces: further from it than the table is
    f32 = omel.get_mel_filters(16000.0, 400, 128).numpy().astype(np.float64)
    assert np.abs(f32 - ref).max() > 4 * np.abs(filt.astype(np.float64) - ref).max()


def test_filterbank_80_is_the_table_of_wb_mel_constants_bit_for_bit():
    lib = _lib.load()
    hann = np.zeros(400, np.float32)
    old = np.zeros((80, 201), np.float32)
    assert lib.wb_mel_constants(16000.0, hann.ctypes.data_as(_lib.c_float_p), old.ctypes.data_as(_lib.c_float_p)) == 0
    new = wb.mel_filterbank(16000.0, 80)
    assert new.shape == (80, 201) and np.array_equal(new.view(np.int32), old.view(np.int32))


def test_filterbank_refuses_other_row_counts_and_rates_its_taps_cannot_hold():
    lib = _lib.load()
    buf = np.zeros((256, 201), np.float32)
    for bad in (0, -1, 64, 96, 127, 129, 256):
        assert lib.wb_mel_filterbank(16000.0, bad, buf.ctypes.data_as(_lib.c_float_p)) == -1, bad
    assert lib.wb_mel_filterbank(16000.0, 128, None) == -1
    # at 48 kHz the widest of the 128 rows has 13 taps, one more than the kernel's 12 -> refused like an 80-row overflow
    assert (omel.mel_filters_f64(48000.0, 400, 128) != 0).sum(1).max() == 13
    assert lib.wb_mel_filterbank(48000.0, 128, buf.ctypes.data_as(_lib.c_float_p)) == -2
    with pytest.raises(wb.WbError) as e:
        wb.mel_filterbank(16000.0, 100)
    assert e.value.status == -1


def test_batched_entry_validates_n_mels_before_touching_a_device():
    starts = np.array([0], dtype=np.int64)
    lens = np.array([16000], dtype=np.int64)
    for n_mels, stride, want in ((96, 128 * 112, -1), (128, 80 * 112, -1)):       # bad row count; window stride of 80 rows
        with pytest.raises(wb.WbError) as e:
            wb.waveform_to_mels_dev(0x1000, 16000, starts, lens, 0x2000, stride, 112, n_mels=n_mels)
        assert e.value.status == want
    with pytest.raises(wb.WbError) as e:                                            # no reference recipe at 128 rows
        wb.waveform_to_mels_dev(0x1000, 16000, starts, lens, 0x2000, 128 * 112, 112, n_mels=128, frontend="reference")
    assert e.value.status == -1


def test_presets_gain_the_128_bin_models_and_keep_the_old_ones():
    v3, turbo = synth.preset_dims("large-v3"), synth.preset_dims("large-v3-turbo")
    assert (v3["n_mels"], v3["n_audio_state"], v3["n_audio_head"], v3["n_audio_layer"], v3["n_text_layer"], v3["n_vocab"]) == \
        (128, 1280, 20, 32, 32, 51866)
    assert turbo == dict(v3, n_text_layer=4)
    assert synth.preset_dims("large-v2") == dict(n_mels=80, n_audio_ctx=1500, n_audio_state=1280, n_audio_head=20, n_audio_layer=32,
                                                 n_vocab=51865, n_text_ctx=448, n_text_state=1280, n_text_head=20, n_text_layer=32)
    assert [synth.preset_seed(n) - 0x5EED0000 for n in ("tiny.en", "base.en", "small", "medium", "large-v2")] == [0, 1, 2, 3, 4]
    assert synth.micro_dims() == synth.micro_dims(n_mels=80, n_text_layer=None) and synth.micro_dims()["n_mels"] == 80
    d = synth.micro_dims(n_layer=3, n_mels=128, n_text_layer=1)
    assert (d["n_mels"], d["n_audio_layer"], d["n_text_layer"]) == (128, 3, 1)
    w = synth.synth_weights(synth.micro_dims(n_state=64, n_head=1, n_layer=2, n_vocab=263, n_audio_ctx=64, n_mels=128,
                                             n_text_layer=1), seed=3)
    assert w["encoder/conv1/weight"].shape == (64, 128, 3)
    assert "decoder/block_0/attn/query/weight" in w and "decoder/block_1/attn/query/weight" not in w


@pytest.fixture(scope="module")
def emu_lib():
    if not (os.path.exists(CLANG) or shutil.which(CLANG)):
        pytest.skip("no host clang++ for the hipemu build")
    subprocess.run(["make", "-C", EMU_DIR, "-j", str(min(8, os.cpu_count() or 1)), "all", "ktest"], check=True,
                   stdout=subprocess.DEVNULL)
    return EMU_LIB


@pytest.mark.parametrize("which", ["frontend", "frontend80", "micro", "pcm", "refuse", "depths80"])
def test_128_bins_under_the_functional_model(emu_lib, which):
    env = dict(os.environ, WHISPER_HIP_LIB=emu_lib, WHISPER_HIP_ALLOW_EMU="1")
    env["PYTHONPATH"] = os.pathsep.join([ROOT, PKG, os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
    env.setdefault("OMP_NUM_THREADS", "2")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mel128_emu_checks.py"), which], env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and f"OK {which}" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_header_library_binding_and_rust_shim_name_the_new_functions():
    h = open(os.path.join(ROOT, "include", "whisper_hip.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "whisper-hip", "src", "ffi.rs")).read()
    lib = ctypes.CDLL(os.path.join(PKG, "lib", "libwhisper_hip.so"))
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, h), name
        assert re.search(r"pub\s+fn\s+%s\s*\(" % name, ffi), name
        assert hasattr(lib, name), name
        assert getattr(_lib.load(), name).argtypes is not None, name
    # n_mels sits before frontend in the batched entry, before mel in the single-window one
    assert re.search(r"wb_waveform_to_mels_dev_mels\([^;]*int32_t n_mels, int32_t frontend\);", h, re.S)
    assert re.search(r"wb_prep_audio_mels\([^;]*double sample_rate, int n_mels, float\* mel,", h, re.S)
