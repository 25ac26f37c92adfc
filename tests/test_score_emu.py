"""CPU: token scoring.

 * score.hip and its host side executed through the hipemu functional model at micro shapes (tests/score_emu_checks.py, one
   subprocess per check): the test hook at the two smallest operator shapes, wb_score_tokens / wb_session_score /
   wb_waveform_to_token_scores / wb_waveform_detect_language against the oracle, every error path;
 * the error bound of the operator test (tests/score_ref.py) passes the f32 NumPy evaluation and rejects each NumPy mutant
   -- target shifted by one position, mask ignored, pad columns included as zeros, splits merged without rescaling to the
   common max -- by at least 10x on the inputs the GPU test uses;
 * the ABI surface: the header declares the new functions, the built library exports them, the Rust shim names them."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import score_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "whisper-burn_amd")
EMU_DIR = os.path.join(PKG, "tools", "hipemu")
EMU_LIB = os.path.join(PKG, "lib", "libwhisper_hip_emu.so")
CLANG = os.environ.get("EMUCXX", "/opt/rocm/lib/llvm/bin/clang++")
NEW = ["wb_score_tokens", "wb_session_score", "wb_waveform_detect_language", "wb_waveform_to_token_scores",
       "wb_logprob_gather"]


@pytest.fixture(scope="module")
def emu_lib():
    if not (os.path.exists(CLANG) or shutil.which(CLANG)):
        pytest.skip("no host clang++ for the hipemu build")
    subprocess.run(["make", "-C", EMU_DIR, "-j", str(min(8, os.cpu_count() or 1)), "all", "ktest"], check=True,
                   stdout=subprocess.DEVNULL)
    return EMU_LIB


@pytest.mark.parametrize("which", ["hook", "entries", "waveform", "errors"])
def test_scoring_under_the_functional_model(emu_lib, which):
    env = dict(os.environ, WHISPER_HIP_LIB=emu_lib, WHISPER_HIP_ALLOW_EMU="1")
    env["PYTHONPATH"] = os.pathsep.join([ROOT, PKG, os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
    env.setdefault("OMP_NUM_THREADS", "2")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "score_emu_checks.py"), which], env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and f"OK {which}" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


CASES = [c for shape in sr.SHAPES for c in sr.make_cases(shape)]
# cases that cannot see a given mutant, whatever the tolerance, named with the reason
NOT_A_PROBE = {
    "mask_ignored": lambda c: c["mask"] is None,                        # no mask to ignore
    "no_rescale": lambda c: c["vs"] == 1 or c["kind"] == "single",      # one split / one finite term: nothing to rescale
    "pad_zeros": lambda c: False,
    "target_shift": lambda c: (c["target"] < 0).all(),                  # the R = 1 call whose only row has no target
}


def _args(c):
    return dict(mask=c["mask"], row_masked=c["row_masked"], target=c["target"], probes=c["probes"])


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_bound_passes_f32_numpy_and_rejects_every_mutant_by_a_decade(case):
    ref, bound = sr.bounds(case)
    f32 = sr.score_ref(case["h"], case["E"], dtype=np.float32, **_args(case))
    assert sr.worst_ratio(f32, ref, bound) <= 1.0
    for mutant, blind in NOT_A_PROBE.items():
        if blind(case):
            continue
        got = sr.score_ref(case["h"], case["E"], mutant=mutant, vs=case["vs"], **_args(case))
        r = sr.worst_ratio(got, ref, bound)
        assert r >= 10.0, f"{mutant}: only {r:.2f}x the bound"


def test_the_cases_cover_what_the_operator_test_promises():
    assert [c[:3] for c in sr.SHAPES] == [(1, 64, 263), (5, 1280, 263), (33, 128, 1031), (130, 384, 1031)]
    assert [sr.n_splits(R, V, s) for R, _, V, s in sr.SHAPES] == [3, 1, 3, 9]
    for shape in sr.SHAPES:
        R, d, V, req = shape
        cases = sr.make_cases(shape)
        rng = sr.split_ranges(V, sr.n_splits(R, V, req))
        assert rng[0][0] == 0 and rng[-1][1] == V and all(a[1] == b[0] for a, b in zip(rng, rng[1:]))
        targets = set(int(t) for c in cases for t in c["target"])
        assert {0, V - 1, -1} <= targets and {lo for lo, _ in rng} <= targets and {hi - 1 for _, hi in rng} <= targets
        assert {c["kind"] for c in cases} >= {"none", "tail", "single"} and (len(rng) == 1 or any(c["kind"] == "split" for c in cases))
        for c in cases:
            pr = c["probes"]
            assert len(pr) != len(set(pr)) and any(i == V - 1 for _, i in pr)                # duplicates, a probe at V - 1
            if c["mask"] is not None and R > 1:
                assert 0 < c["row_masked"].sum() < R                                         # masked and unmasked rows in one call
            if c["kind"] == "split":
                lo, hi = rng[len(rng) // 2]
                assert np.isneginf(c["mask"][lo:hi]).all()


def test_special_tokens_carry_the_language_ids_and_the_no_speech_token(tmp_path):
    from whisper_burn_amd.tokens import LANGUAGES, SpecialTokens, TokenizerAdapter
    ml = SpecialTokens.for_vocab(51865)
    assert len(LANGUAGES) == 98 and ml.language_ids == tuple(range(50259, 50358)) and ml.language == ml.language_ids[0]
    assert ml.no_speech == 50362 and ml.is_special[list(ml.language_ids)].all() and ml.is_special[ml.no_speech]
    en = SpecialTokens.for_vocab(51864)
    assert en.language_ids == () and en.no_speech == 50361
    syn = SpecialTokens.for_vocab(1031)
    assert syn.language_ids == (1017, 1018) and syn.language == 1017 and syn.no_speech == -1
    pytest.importorskip("tokenizers")
    from test_tokenizer_integration import write_synthetic_tokenizer_json
    write_synthetic_tokenizer_json(str(tmp_path / "tokenizer.json"))
    st = TokenizerAdapter.from_file(str(tmp_path / "tokenizer.json")).special_tokens("en")
    assert st.language_ids == syn.language_ids and st.no_speech == -1


def test_cli_auto_without_language_tokens_is_a_clear_error(tmp_path, monkeypatch, capsys):
    """`auto` with a tokenizer that has no language token fails before any model is loaded, and says why."""
    import wave
    pytest.importorskip("tokenizers")
    from tokenizers import Tokenizer, models, pre_tokenizers
    from whisper_burn_amd import transcribe as cli
    monkeypatch.chdir(tmp_path)
    tok = Tokenizer(models.WordLevel(vocab={"a": 0, "<unk>": 1}, unk_token="<unk>"))
    tok.pre_tokenizer = pre_tokenizers.Whitespace()
    tok.add_special_tokens(["<|endoftext|>", "<|startoftranscript|>", "<|transcribe|>", "<|notimestamps|>"])
    tok.save(str(tmp_path / "tokenizer.json"))
    with wave.open(str(tmp_path / "a.wav"), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(np.zeros(16000, dtype="<i2").tobytes())
    assert cli.main(["transcribe", "no-such-model", "a.wav", "auto", "out.txt"]) == 1
    err = capsys.readouterr().err
    assert "no language tokens" in err and "Failed to load whisper model" not in err
    assert not (tmp_path / "out.txt").exists()


def test_header_library_and_rust_shim_name_the_new_functions():
    h = open(os.path.join(ROOT, "include", "whisper_hip.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "whisper-hip", "src", "ffi.rs")).read()
    lib = ctypes.CDLL(os.path.join(PKG, "lib", "libwhisper_hip.so"))
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, h), name
        assert re.search(r"pub\s+fn\s+%s\s*\(" % name, ffi), name
        assert hasattr(lib, name), name
