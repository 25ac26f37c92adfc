"""CPU: beam search under the timestamp rules through the functional model, and its ABI surface.

 * tsbeam.hip and its host side executed through hipemu at micro shapes (tests/tsbeam_emu_checks.py, one subprocess per check):
   the rows hook at V = 263 and 1031 against the f64 restatement, the model-free hook on the scripted cases,
   Session.decode_timestamps_beam on the micro fixture in the three launch shapes (W x B = 3 x 2 fused, 3 x 5 the 16-row bucket,
   4 x 5 batch mode) replayed step by step on the teacher-forced oracle, beam 1 = the greedy rows, waveform_to_segments(beam=..)
   against the pure-Python seek loop, every error path;
 * the header declares the new functions, the built library exports them, the Rust shim names them; wb_beam_params lists the
   same fields in the header, the ctypes mirror and the Rust struct."""
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
NEW = ["wb_session_decode_timestamps_beam", "wb_session_last_beams", "wb_session_last_beam_trace", "wb_timestamp_beam_rows",
       "wb_timestamp_beam_search_device", "wb_waveform_to_segments_beam"]


@pytest.fixture(scope="module")
def emu_lib():
    if not (os.path.exists(CLANG) or shutil.which(CLANG)):
        pytest.skip("no host clang++ for the hipemu build")
    subprocess.run(["make", "-C", EMU_DIR, "-j", str(min(8, os.cpu_count() or 1)), "all"], check=True, stdout=subprocess.DEVNULL)
    return EMU_LIB


@pytest.mark.parametrize("which", ["rows", "script", "session_3_2_1.0", "session_3_5_1.0", "session_4_5_1.0", "greedy_segments",
                                   "errors"])
def test_beam_search_under_the_functional_model(emu_lib, which):
    env = dict(os.environ, WHISPER_HIP_LIB=emu_lib, WHISPER_HIP_ALLOW_EMU="1")
    env["PYTHONPATH"] = os.pathsep.join([ROOT, PKG, os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
    env.setdefault("OMP_NUM_THREADS", "2")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tsbeam_emu_checks.py"), which], env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and f"OK {which}" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_header_library_and_rust_shim_name_the_new_functions():
    h = open(os.path.join(ROOT, "include", "whisper_hip.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "whisper-hip", "src", "ffi.rs")).read()
    lib = ctypes.CDLL(os.path.join(PKG, "lib", "libwhisper_hip.so"))
    from whisper_burn_amd._lib import SIGNATURES
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, h), name
        assert re.search(r"pub\s+fn\s+%s\s*\(" % name, ffi), name
        assert hasattr(lib, name) and name in SIGNATURES, name
    name = "wb_beam_params_default"
    assert re.search(r"\bvoid\s+%s\s*\(" % name, h) and re.search(r"pub\s+fn\s+%s\s*\(" % name, ffi) and hasattr(lib, name)
    assert re.search(r"pub\s+type\s+wb_tsbeam_logits_fn\b", ffi) and re.search(r"\(\*wb_tsbeam_logits_fn\)", h)


def test_beam_params_struct_matches_the_header_field_by_field():
    import test_rust_shim as trs
    from whisper_burn_amd._lib import WbBeamParams
    h = trs._strip_comments(open(os.path.join(ROOT, "include", "whisper_hip.h")).read())
    r = trs._strip_comments(open(os.path.join(ROOT, "rust", "whisper-hip", "src", "ffi.rs")).read())
    fields = trs.struct_fields_c(h, "wb_beam_params")
    assert fields == [f for f, _ in WbBeamParams._fields_] == trs.struct_fields_rust(r, "wb_beam_params") == \
        ["beam_size", "patience", "length_penalty"]
    p = WbBeamParams()
    ctypes.CDLL(os.path.join(PKG, "lib", "libwhisper_hip.so")).wb_beam_params_default(ctypes.byref(p))
    assert (p.beam_size, p.patience, p.length_penalty) == (5, 1.0, -1.0)
