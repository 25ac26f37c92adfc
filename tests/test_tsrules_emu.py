"""CPU: timestamp-token decoding through the functional model, and its ABI surface.

 * tsrules.hip and its host side executed through hipemu at micro shapes (tests/tsrules_emu_checks.py, one subprocess per
   check): the test hook at the two smallest operator shapes (and two cases of the larger ones), Session.decode_timestamps
   on the micro fixture in the three launch shapes (W x best_of = 3 x 1 fused, 3 x 5 the 16-row bucket, 4 x 5 batch mode)
   against the teacher-forced oracle, the rules-off equivalences, every error path, segments_from_tokens and
   waveform_to_segments against their pure-Python restatements (the seek loop on a short-context model with >= 4 windows);
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
NEW = ["wb_session_set_suppress", "wb_session_decode_timestamps", "wb_timestamp_rows", "wb_segments_from_tokens",
       "wb_waveform_to_segments"]


@pytest.fixture(scope="module")
def emu_lib():
    if not (os.path.exists(CLANG) or shutil.which(CLANG)):
        pytest.skip("no host clang++ for the hipemu build")
    subprocess.run(["make", "-C", EMU_DIR, "-j", str(min(8, os.cpu_count() or 1)), "all"], check=True, stdout=subprocess.DEVNULL)
    return EMU_LIB


@pytest.mark.parametrize("which,extra", [("hook", {}), ("session_3_1", {}), ("session_3_5", {}), ("session_4_5", {}),
                                         ("session_4_5", {"WHISPER_HIP_DECODER_SPLIT": "0"}), ("rules_off", {}), ("segments", {}),
                                         ("errors", {})])
def test_timestamp_decoding_under_the_functional_model(emu_lib, which, extra):
    env = dict(os.environ, WHISPER_HIP_LIB=emu_lib, WHISPER_HIP_ALLOW_EMU="1", **extra)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, PKG, os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
    env.setdefault("OMP_NUM_THREADS", "2")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tsrules_emu_checks.py"), which], env=env,
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
    name = "wb_timestamp_params_default"
    assert re.search(r"\bvoid\s+%s\s*\(" % name, h) and re.search(r"pub\s+fn\s+%s\s*\(" % name, ffi) and hasattr(lib, name)


def test_timestamp_params_struct_matches_the_header_field_by_field():
    """wb_timestamp_params in the header, the ctypes mirror and the Rust repr(C) struct list the same fields in the same order."""
    import test_rust_shim as trs
    from whisper_burn_amd._lib import WbTimestampParams
    h = trs._strip_comments(open(os.path.join(ROOT, "include", "whisper_hip.h")).read())
    r = trs._strip_comments(open(os.path.join(ROOT, "rust", "whisper-hip", "src", "ffi.rs")).read())
    fields = trs.struct_fields_c(h, "wb_timestamp_params")
    assert fields == [f for f, _ in WbTimestampParams._fields_] == trs.struct_fields_rust(r, "wb_timestamp_params")
    p = WbTimestampParams()
    ctypes.CDLL(os.path.join(PKG, "lib", "libwhisper_hip.so")).wb_timestamp_params_default(ctypes.byref(p))
    assert (p.tok_timestamp_begin, p.n_timestamps, p.max_initial_timestamp_index, p.max_timestamp_index, p.best_of, p.seed,
            p.attempt) == (0, 0, 50, -1, 1, 0, 0) and abs(p.seconds_per_timestamp - 0.02) < 1e-9 and p.temperature == 0.0


def test_special_tokens_carry_the_timestamp_range_and_the_default_masks():
    import numpy as np
    from whisper_burn_amd.tokens import SpecialTokens, default_suppress
    for V, tb in ((51864, 50363), (51865, 50364)):
        st = SpecialTokens.for_vocab(V)
        assert (st.timestamp_begin, st.n_timestamps) == (tb, 1501) and tb + 1501 == V and st.no_timestamps == tb - 1
        sup, first = default_suppress(st)
        assert sup[st.no_timestamps] and sup[st.start_of_transcript] and not sup[st.end_of_text] and not sup[tb:].any()
        assert not sup[:st.end_of_text].any() and first[st.end_of_text] and first.sum() == 1
    st = SpecialTokens.for_vocab(1031)
    assert st.n_timestamps == 0 and default_suppress(st)[0].sum() == 15
    old = SpecialTokens(1, 2, 3, 4, 5, np.zeros(8, dtype=np.uint8))        # existing constructors keep working
    assert old.n_timestamps == 0 and old.timestamp_begin == 0
