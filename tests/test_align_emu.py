"""CPU: align.hip and its host side executed through the hipemu functional model at micro shapes
(tests/align_emu_checks.py, one subprocess per check), plus the ABI surface of the feature: the header declares the new
functions, the built library exports them and the Rust shim's extern block names them."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "whisper-burn_amd")
EMU_DIR = os.path.join(PKG, "tools", "hipemu")
EMU_LIB = os.path.join(PKG, "lib", "libwhisper_hip_emu.so")
CLANG = os.environ.get("EMUCXX", "/opt/rocm/lib/llvm/bin/clang++")
NEW = ["wb_align_tokens", "wb_session_align", "wb_dtw_start_positions", "wb_waveform_to_token_times",
       "wb_stitch_windows_times"]


@pytest.fixture(scope="module")
def emu_lib():
    if not (os.path.exists(CLANG) or shutil.which(CLANG)):
        pytest.skip("no host clang++ for the hipemu build")
    subprocess.run(["make", "-C", EMU_DIR, "-j", str(min(8, os.cpu_count() or 1)), "all", "ktest"], check=True,
                   stdout=subprocess.DEVNULL)
    return EMU_LIB


@pytest.mark.parametrize("which", ["dtw", "stitch", "errors", "matrix", "harness", "short_rows"])
def test_alignment_under_the_functional_model(emu_lib, which):
    env = dict(os.environ, WHISPER_HIP_LIB=emu_lib, WHISPER_HIP_ALLOW_EMU="1",
               WHISPER_HIP_KTEST_LIB=os.path.join(os.path.dirname(emu_lib), "libwhisper_hip_ktest_emu.so"))
    env["PYTHONPATH"] = os.pathsep.join([ROOT, PKG, os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
    env.setdefault("OMP_NUM_THREADS", "2")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "align_emu_checks.py"), which], env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and f"OK {which}" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_header_library_and_rust_shim_name_the_new_functions():
    h = open(os.path.join(ROOT, "include", "whisper_hip.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "whisper-hip", "src", "ffi.rs")).read()
    lib = ctypes.CDLL(os.path.join(PKG, "lib", "libwhisper_hip.so"))
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, h), name
        assert re.search(r"pub\s+fn\s+%s\s*\(" % name, ffi), name
        assert hasattr(lib, name), name
