"""CPU: greedy decodes on the hipemu functional model whose windows hold the key counts where the block-parallel softmax of the
fused cross-attention body could lose a key -- 383, 384 and 6 keys in one pass of the functional model's 384-key ring; 385, 511,
512, 513, 745, 768 (and 64) in two -- token-exact against the oracle, through the persistent kernel and through the chain of
one launch per sublayer (WHISPER_HIP_PERSIST=0), on the d = 128 micro model and the d = 384 four-layer model.

tests/cross_softmax_checks.py holds the cases and the seeds; one child process per (decode path, model), side by side (the
functional model runs one fiber at a time); the oracle's rows are computed once in a child of their own."""
import concurrent.futures
import json
import os
import shutil
import subprocess
import sys

import pytest

import cross_softmax_checks as cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "whisper-burn_amd")
EMU_DIR = os.path.join(PKG, "tools", "hipemu")
EMU_LIB = os.path.join(PKG, "lib", "libwhisper_hip_emu.so")
CLANG = os.environ.get("EMUCXX", "/opt/rocm/lib/llvm/bin/clang++")
PATHS = {"persist": {}, "chain": {"WHISPER_HIP_PERSIST": "0"}}


def _child(args, extra):
    env = dict(os.environ)
    env.update({"WHISPER_HIP_LIB": EMU_LIB, "WHISPER_HIP_ALLOW_EMU": "1"})
    env["PYTHONPATH"] = os.pathsep.join([ROOT, PKG, os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
    env.setdefault("OMP_NUM_THREADS", "2")
    env.pop("WHISPER_HIP_PERSIST", None)
    env.update(extra)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "cross_softmax_checks.py")] + args, env=env,
                       capture_output=True, text=True, timeout=1500)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    assert p.returncode == 0 and lines, p.stdout[-2000:] + p.stderr[-4000:]
    return json.loads(lines[-1][7:])


@pytest.fixture(scope="module")
def results():
    if not (os.path.exists(CLANG) or shutil.which(CLANG)):
        pytest.skip("no host clang++ for the hipemu build")
    subprocess.run(["make", "-C", EMU_DIR, "-j", str(min(8, os.cpu_count() or 1))], check=True, stdout=subprocess.DEVNULL)
    with concurrent.futures.ThreadPoolExecutor(max_workers=max(1, min(5, (os.cpu_count() or 2) - 1))) as pool:
        jobs = {(path, model): pool.submit(_child, ["emu", model], extra) for path, extra in PATHS.items() for model in cs.MODELS}
        ref = pool.submit(_child, ["oracle", "emu"], {})
        return ref.result(), {k: f.result() for k, f in jobs.items()}


def test_every_key_count_the_functional_models_rings_can_lose_is_decoded():
    one = {C for lim, Cs, _ in cs.SETS["emu"][1].values() for C in Cs if max(Cs) <= 384}
    two = {C for lim, Cs, _ in cs.SETS["emu"][1].values() for C in Cs if max(Cs) > 384}
    assert one >= {383, 384} and two >= {385, 511, 512, 513, 745, 768}
    assert all(3 <= len(Cs) <= 4 and len(set(Cs)) == len(Cs) for _, Cs, _ in cs.SETS["emu"][1].values()) and cs.DEPTH <= 8


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("model", sorted(cs.MODELS))
@pytest.mark.parametrize("case", sorted(cs.SETS["emu"][1]))
def test_decode_is_token_exact_at_the_softmax_boundaries(results, case, model, path):
    ref, got = results
    key = f"{model}_{case}"
    assert got[(path, model)][key] == ref[key], (path, key, got[(path, model)][key], ref[key])
    assert all(len(r) > 4 for r in ref[key])
