"""CPU: the one-pass prompt prefill and the conditioned seek loop through the functional model, and their ABI surface.

 * prefill.hip, the pass and the seek loop executed through hipemu at micro shapes (tests/prefill_emu_checks.py, one subprocess
   per check): the store kernel at its three shapes against canaries; the cache behind Session.prefill and the next (forking)
   steps for every case of prefill_ref.CACHE_CASES; the error paths; one chain shape behind the long prompt; the conditioned
   seek loop (greedy and beam 3) against the Python loop, with conditioning off, and its argument errors;
 * the header declares the new functions, the built library exports them, the Rust shim names them."""
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
NEW = ["wb_session_prefill", "wb_session_set_prefill", "wb_waveform_to_segments_conditioned", "wb_prefill_store", "wb_session_self_kv"]


@pytest.fixture(scope="module")
def emu_lib():
    if not (os.path.exists(CLANG) or shutil.which(CLANG)):
        pytest.skip("no host clang++ for the hipemu build")
    subprocess.run(["make", "-C", EMU_DIR, "-j", str(min(8, os.cpu_count() or 1)), "all"], check=True, stdout=subprocess.DEVNULL)
    return EMU_LIB


@pytest.mark.parametrize("which", ["store", "cache_0", "cache_1", "cache_2", "cache_3", "cache_4", "errors", "chain_ts_3_1",
                                   "chain_greedy", "seek_0", "seek_3"])
def test_prefill_under_the_functional_model(emu_lib, which):
    env = dict(os.environ, WHISPER_HIP_LIB=emu_lib, WHISPER_HIP_ALLOW_EMU="1")
    env["PYTHONPATH"] = os.pathsep.join([ROOT, PKG, os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
    env.setdefault("OMP_NUM_THREADS", "2")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "prefill_emu_checks.py"), which], env=env,
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


def test_the_switch_has_its_rows():
    sw = open(os.path.join(PKG, "csrc", "switches.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert '"WHISPER_HIP_PREFILL_PASS", DEFAULT_ON' in sw and "WHISPER_HIP_PREFILL_PASS" in doc
