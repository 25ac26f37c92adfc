"""CPU: one logits role of the persistent kernel that applies the final LayerNorm itself against the final-LN role followed by the
logits role, on the hipemu functional model (`wbk_persist_logits` of lib/libwhisper_hip_ktest_emu.so): the cases of
tests/persist_logits_cases.py, every one in ONE child process that loads the harness library and nothing else of the engine.
Records are compared word for word."""
import json
import os
import shutil
import subprocess
import sys

import pytest

import kernel_cases as kc
import persist_logits_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "whisper-burn_amd")
EMU_DIR = os.path.join(PKG, "tools", "hipemu")
CLANG = os.environ.get("EMUCXX", "/opt/rocm/lib/llvm/bin/clang++")
CASES = mc.cases()


@pytest.fixture(scope="module")
def emu_results():
    if not (os.path.exists(CLANG) or shutil.which(CLANG)):
        pytest.skip("no host clang++ for the hipemu build")
    nj = str(min(8, os.cpu_count() or 1))
    subprocess.run(["make", "-C", EMU_DIR, "-j", nj], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", EMU_DIR, "-j", nj, "ktest"], check=True, stdout=subprocess.DEVNULL)
    env = {k: v for k, v in os.environ.items() if not k.startswith("WHISPER_HIP_") and k != "HIPEMU_CUS"}
    env["PYTHONPATH"] = os.pathsep.join([ROOT, PKG, os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "persist_logits_cases.py"), kc.EMU_LIB], env=env,
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return {r["id"]: r for r in (json.loads(ln[6:]) for ln in p.stdout.splitlines() if ln.startswith("KCASE "))}


def test_the_cases_cover_both_widths_one_and_three_rows_and_a_masked_row():
    ids = {c["id"] for c in CASES}
    assert {f"d{d}-rows{r}-1tile" for d in (128, 384) for r in (1, 3)} <= ids
    assert {f"d{d}-rows3-dead1-1tile" for d in (128, 384)} <= ids


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_records_equal_those_of_the_final_ln_role_and_the_logits_role_on_the_functional_model(emu_results, c):
    r = emu_results[c["id"]]
    print(r)
    assert r["ok"], r["msg"]
