"""CPU: temperature sampling and the decode fallback.

 * sample.hip and its host side executed through the hipemu functional model at micro shapes (tests/sample_emu_checks.py, one
   subprocess per check): the test hook at the two smallest operator shapes, Session.decode_sample on the micro model in the
   three launch shapes (W x best_of = 3 x 1 fused, 3 x 5 the 16-row bucket, 4 x 5 batch mode) against the teacher-forced
   oracle, waveform_to_tokens_fallback's scenarios, every error path, wb_fallback_decide against its restatement;
 * the NumPy restatement (tests/sample_ref.py): the generator's known answers, the uniform's range, and the exclusion caps of
   the GPU tests on the f64 restatement / the oracle alone;
 * the ABI surface: the header declares the new functions, the built library exports them, the Rust shim names them."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import sample_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "whisper-burn_amd")
EMU_DIR = os.path.join(PKG, "tools", "hipemu")
EMU_LIB = os.path.join(PKG, "lib", "libwhisper_hip_emu.so")
CLANG = os.environ.get("EMUCXX", "/opt/rocm/lib/llvm/bin/clang++")
NEW = ["wb_session_rewind", "wb_session_decode_sample", "wb_session_last_samples", "wb_session_graph_count", "wb_fallback_decide",
       "wb_waveform_to_tokens_fallback", "wb_sample_rows"]


@pytest.fixture(scope="module")
def emu_lib():
    if not (os.path.exists(CLANG) or shutil.which(CLANG)):
        pytest.skip("no host clang++ for the hipemu build")
    subprocess.run(["make", "-C", EMU_DIR, "-j", str(min(8, os.cpu_count() or 1)), "all"], check=True, stdout=subprocess.DEVNULL)
    return EMU_LIB


@pytest.mark.parametrize("which,extra", [("hook", {}), ("session_3_1", {}), ("session_3_5", {}), ("session_4_5", {}),
                                         ("session_4_5", {"WHISPER_HIP_DECODER_SPLIT": "0"}), ("fallback", {}), ("errors", {}),
                                         ("decide", {})])
def test_sampling_under_the_functional_model(emu_lib, which, extra):
    env = dict(os.environ, WHISPER_HIP_LIB=emu_lib, WHISPER_HIP_ALLOW_EMU="1", **extra)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, PKG, os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
    env.setdefault("OMP_NUM_THREADS", "2")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sample_emu_checks.py"), which], env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and f"OK {which}" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_philox_known_answers():
    for ctr, key, out in sr.KAT:
        assert tuple(int(v) for v in sr.philox4x32_10(*ctr, *key)) == out


def test_uniform_is_exact_in_f32_and_inside_the_open_interval():
    w = np.array([0, 0x1FF, 0x200, 0xFFFFFFFF, 0x80000000], dtype=np.uint64)
    u = sr.uniform(w)
    assert u.min() == 2.0 ** -24 and u.max() == 1.0 - 2.0 ** -24
    assert np.array_equal(u, u.astype(np.float32).astype(np.float64))
    g = sr.gumbel(w)
    assert -2.82 < g.min() and g.max() < 16.64


CASES = [c for shape in sr.SHAPES for c in sr.make_cases(shape)]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_operator_cases_stay_inside_the_exclusion_cap_on_the_restatement_alone(case):
    ref = sr.reference(case)
    assert sr.excluded(ref, case["T"]).sum() <= 0.01 * case["R"]
    # an f32 evaluation of the same keys picks the same tokens outside the excluded draws: the bound is not vacuous
    for r, d in enumerate(ref):
        V = case["V"]
        mk = case["mask"] if case["row_masked"][r] else None
        x = case["logits"][r, :V] + (np.float32(0) if mk is None else mk)
        g = sr.gumbel(sr.words(V, case["seed"], int(case["stream"][r]), case["attempt"], int(case["position"][r]))).astype(np.float32)
        k32 = (x - case["stats"][r, 0]) * (np.float32(1) / np.float32(case["T"])) + g
        assert int(np.argmax(k32)) == d["token"] or not d["gap"] > sr.delta_op(d["A"], case["T"])


def test_the_cases_cover_what_the_operator_test_promises():
    assert sr.SHAPES == [(1, 263), (5, 1031), (33, 7001), (3, 51865)] and sr.TEMPS == [0.2, 1.0]
    for shape in sr.SHAPES:
        R, V = shape
        cases = sr.make_cases(shape)
        assert {c["kind"] for c in cases} == {"mixed", "single", "heavy"} and {c["T"] for c in cases} == {0.2, 1.0}
        assert {c["attempt"] for c in cases} >= {0, sr.I31}
        for c in cases:
            assert c["logits"].shape == (R, V + sr.PAD) and np.isnan(c["logits"][:, V:]).all()
            assert {0, sr.I31} & set(c["stream"].tolist()) and {0, sr.I31} & set(c["position"].tolist())
            if R > 1:
                assert 0 < c["row_masked"].sum() < R                      # masked and unmasked rows in one call
            if c["kind"] == "single":
                assert (c["mask"] == 0).sum() == 1
            if c["kind"] == "heavy":
                assert np.isneginf(c["mask"]).mean() > 0.8


def test_chi_square_case_expectation():
    case, exp = sr.chi_square_case()
    assert case["R"] == 4096 and abs(exp.sum() - 4096) < 1e-6 and exp.min() > 5


def _oracle_alone(o32, st, encs, best_of, depth):
    """(positions, excluded) per draw of sr.SESSION_DRAWS: every window's best_of streams sampled by the oracle alone."""
    out = []
    for T, seed, attempt in sr.SESSION_DRAWS:
        n = ex = 0
        for w, enc in enumerate(encs):
            for j in range(best_of):
                _, a, b = sr.oracle_sample(o32, st, enc, T, seed, w * best_of + j, attempt, depth)
                n, ex = n + a, ex + b
        out.append((T, n, ex))
    return out


def test_the_oracle_alone_stays_inside_the_session_tests_exclusion_cap_micro():
    """The seeds and temperatures of the session tests, sampled by the oracle alone on the micro model over the windows of the
    tests' own audio (sample_ref.windows): at most 5 % of the positions have a top-two key gap inside delta_model."""
    import torch
    from oracle import mel as omel
    from oracle.model import OracleWhisper
    from whisper_burn_amd import synth
    from whisper_burn_amd.tokens import SpecialTokens
    dims = synth.micro_dims(n_state=64, n_head=1, n_layer=1, n_vocab=1031)
    o32 = OracleWhisper(synth.synth_weights(dims, seed=5))
    st = SpecialTokens.for_vocab(1031)
    audio = synth.synth_audio(16000 * 3, 3)
    hop = (len(audio) - 16000) // 3
    encs = []
    for i in range(4):                                   # the 4 x 5 shape's windows: 1 s each, 10 zero frames of padding
        m = omel.prep_audio(torch.from_numpy(audio[i * hop:i * hop + 16000])[None])
        encs.append(o32.forward_encoder(torch.nn.functional.pad(m, (0, 10)))[0].numpy())
    for T, n, ex in _oracle_alone(o32, st, encs, 5, 20):
        assert ex <= 0.05 * n, (T, n, ex)


def test_the_oracle_alone_stays_inside_the_session_tests_exclusion_cap_tiny_en():
    """The same on the tiny.en shape of tests/workloads.py (3 windows of the bench audio, depth 32, best_of 5)."""
    import parity_util as pu
    import workloads
    from oracle.model import OracleWhisper
    from whisper_burn_amd.tokens import SpecialTokens
    wl = workloads.WORKLOADS["tiny_bench"]
    o32 = OracleWhisper(wl.weights())
    st = SpecialTokens.for_vocab(51864)
    encs = [o32.forward_encoder(m)[0].numpy() for m in pu.window_mels(o32, wl.audio())]
    assert len(encs) == 3
    res = _oracle_alone(o32, st, encs, 5, 32)
    print("oracle alone, tiny.en (T, positions, excluded):", res)
    for T, n, ex in res:
        assert ex <= 0.05 * n, (T, n, ex)


def test_header_library_and_rust_shim_name_the_new_functions():
    h = open(os.path.join(ROOT, "include", "whisper_hip.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "whisper-hip", "src", "ffi.rs")).read()
    lib = ctypes.CDLL(os.path.join(PKG, "lib", "libwhisper_hip.so"))
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, h), name
        assert re.search(r"pub\s+fn\s+%s\s*\(" % name, ffi), name
        assert hasattr(lib, name), name
    for name in ("wb_sample_params_default", "wb_fallback_params_default"):
        assert re.search(r"\bvoid\s+%s\s*\(" % name, h) and re.search(r"pub\s+fn\s+%s\s*\(" % name, ffi) and hasattr(lib, name)
