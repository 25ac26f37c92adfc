"""CPU: the self-attention role's QKV weight rounds on the hipemu functional model (whisper-burn_amd/tools/hipemu).

At d = 384 the head's QKV slice is six rounds.  The persistent kernel's `<6,4,1>` instance holds FOUR of them in registers
before its wait (csrc/decode_fused_bodies.h: dec_attn_body, NREG): with the resident region, rounds 0, 1, 4, 5 in registers and
2, 3 in LDS, nothing requested behind the wait; without it (several roles per block, WHISPER_HIP_PERSIST_RESIDENT=0) rounds
0 - 3, and 4, 5 follow into the first two register sets.  Every other instance and the one-launch-per-sublayer kernels keep two.
The products keep their operands and their order, so the tokens are the oracle's in every cell (tests/emu_checks.py asserts the
rows equal to the oracle's inside the child; integers, compared with ==):
  * `persist384` on the full grid, resident (switch unset) and streamed (`0`);
  * `persist384` on 40 blocks (every block holds several roles: the streamed four-round sequence) and on 100 blocks (resident and
    streamed roles side by side in one launch);
  * `persist384x7` (`<6,8,1>`), `persist512`, `greedy` (d = 128): two rounds, as before;
  * `persist384` with WHISPER_HIP_PERSIST=0: the fused kernels, two rounds, the same rows.

Operator level (tests/attn_rounds_cases.py through `wbk_attn_fused` of lib/libwhisper_hip_ktest_emu.so): the one-sublayer kernel
at d = 384 with 2 and with 4 register rounds on the same inputs -- bit-identical planes, cache rows and x_out, each within its
bound of the f64 restatement."""
import concurrent.futures
import json
import os
import shutil
import subprocess
import sys

import pytest

import attn_rounds_cases as ar
import kernel_cases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "whisper-burn_amd")
EMU_DIR = os.path.join(PKG, "tools", "hipemu")
EMU_LIB = os.path.join(PKG, "lib", "libwhisper_hip_emu.so")
CLANG = os.environ.get("EMUCXX", "/opt/rocm/lib/llvm/bin/clang++")

# id -> (check of tests/emu_checks.py, extra environment)
CELLS = {
    "persist384": ("persist384", {}),
    "persist384-resident0": ("persist384", {"WHISPER_HIP_PERSIST_RESIDENT": "0"}),
    "persist384@40": ("persist384", {"HIPEMU_CUS": "40"}),
    "persist384@100": ("persist384", {"HIPEMU_CUS": "100"}),
    "persist384x7@40": ("persist384x7", {"HIPEMU_CUS": "40"}),
    "persist512": ("persist512", {}),
    "greedy": ("greedy", {}),
    "persist384-persist0": ("persist384", {"WHISPER_HIP_PERSIST": "0"}),
}
KCASES = ar.cases()


def _env(extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("WHISPER_HIP_") and k != "HIPEMU_CUS"}
    env["PYTHONPATH"] = os.pathsep.join([ROOT, PKG, os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
    env.setdefault("OMP_NUM_THREADS", "2")
    env.update(extra)
    return env


def _spawn(which, extra):
    return subprocess.run([sys.executable, os.path.join(ROOT, "tests", "emu_checks.py"), which],
                          env=_env(dict(extra, WHISPER_HIP_LIB=EMU_LIB, WHISPER_HIP_ALLOW_EMU="1")), capture_output=True, text=True,
                          timeout=900)


@pytest.fixture(scope="module")
def built():
    if not (os.path.exists(CLANG) or shutil.which(CLANG)):
        pytest.skip("no host clang++ for the hipemu build")
    nj = str(min(8, os.cpu_count() or 1))
    subprocess.run(["make", "-C", EMU_DIR, "-j", nj], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", EMU_DIR, "-j", nj, "ktest"], check=True, stdout=subprocess.DEVNULL)


@pytest.fixture(scope="module")
def jobs(built):
    """Every cell as a process of its own (a switch is read once per process), a few side by side."""
    pool = concurrent.futures.ThreadPoolExecutor(max_workers=max(1, min(6, (os.cpu_count() or 2) - 2)))
    futs = {cid: pool.submit(_spawn, which, extra) for cid, (which, extra) in CELLS.items()}
    yield futs
    for f in futs.values():
        f.cancel()
    pool.shutdown(wait=True)


@pytest.fixture(scope="module")
def emu_results(built):
    """Every operator-level case in ONE child process that loads the harness library and nothing else of the engine."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "attn_rounds_cases.py"), kc.EMU_LIB], env=_env({}),
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return {r["id"]: r for r in (json.loads(ln[6:]) for ln in p.stdout.splitlines() if ln.startswith("KCASE "))}


def test_the_listed_lengths_come_with_one_and_three_rows():
    assert {(c["lens"][0], c["rows"]) for c in KCASES} >= {(n, r) for n in (1, 2, 100, 129) for r in (1, 3)}
    assert all(len(c["lens"]) == c["rows"] and len(set(c["lens"])) == c["rows"] for c in KCASES)


@pytest.mark.parametrize("cid", sorted(CELLS))
def test_tokens_equal_the_oracle_in_every_cell(jobs, cid):
    p = jobs[cid].result()
    assert p.returncode == 0 and f"EMU_CHECK_OK {CELLS[cid][0]}" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]


@pytest.mark.parametrize("c", KCASES, ids=[c["id"] for c in KCASES])
def test_two_and_four_register_rounds_agree_bit_for_bit_on_the_functional_model(emu_results, c):
    r = emu_results[c["id"]]
    print(r)
    assert r["ok"], r.get("msg")
