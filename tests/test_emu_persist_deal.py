"""CPU: the persistent decode kernel under both dealings of the step's tail (WHISPER_HIP_PERSIST_DEAL: unset = merge and
final-LN roles kept off the first-layer attention blocks, `legacy` = the least loaded blocks, `log` = the new rule + one line per
built setup) on the hipemu functional model: every cell token-exact against the oracle (tests/emu_checks.py prints EMU_CHECK_OK
only then), in a process of its own.

Cells: `greedy` (d = 128, one row, 35 blocks), `persist384` (d = 384, 4 rows) on its full grid of 169 blocks and on 40 and 100
blocks (HIPEMU_CUS: several layer roles per block; at 40 every block holds a first-layer attention role, so the new rule falls
back to the least loaded blocks), `persist384x7` (7 rows) on 40.  Where blocks without a first-layer attention role exist
(every cell but the two at 40), the reported merge blocks hold none, and merge(r) sits behind finln(r)."""
import concurrent.futures
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
SWITCH = "WHISPER_HIP_PERSIST_DEAL"
# (check, HIPEMU_CUS, first-layer attention blocks = min(grid, 2 rows heads), rows)
CELLS = [("greedy", "", 4, 1), ("persist384", "", 48, 4), ("persist384", "40", 40, 4), ("persist384", "100", 48, 4),
         ("persist384x7", "40", 40, 7)]
PARAMS = [(which, cus, n_early, rows, value) for which, cus, n_early, rows in CELLS for value in (None, "legacy", "log")]


def _spawn(which, cus, value):
    env = {k: v for k, v in os.environ.items() if k != SWITCH}
    env.update({"WHISPER_HIP_LIB": EMU_LIB, "WHISPER_HIP_ALLOW_EMU": "1"})
    env["PYTHONPATH"] = os.pathsep.join([ROOT, PKG, os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
    env.setdefault("OMP_NUM_THREADS", "2")
    if cus:
        env["HIPEMU_CUS"] = cus
    if value is not None:
        env[SWITCH] = value
    return subprocess.run([sys.executable, os.path.join(ROOT, "tests", "emu_checks.py"), which], env=env, capture_output=True,
                          text=True, timeout=900)


@pytest.fixture(scope="module")
def jobs():
    if not (os.path.exists(CLANG) or shutil.which(CLANG)):
        pytest.skip("no host clang++ for the hipemu build")
    subprocess.run(["make", "-C", EMU_DIR, "-j", str(min(8, os.cpu_count() or 1))], check=True, stdout=subprocess.DEVNULL)
    pool = concurrent.futures.ThreadPoolExecutor(max_workers=max(1, min(6, (os.cpu_count() or 2) - 2)))
    futs = {(which, cus, value): pool.submit(_spawn, which, cus, value) for which, cus, _, _, value in PARAMS}
    yield futs
    for f in futs.values():
        f.cancel()
    pool.shutdown(wait=True)


@pytest.mark.parametrize("which,cus,n_early,rows,value", PARAMS,
                         ids=[f"{p[0]}{'@' + p[1] if p[1] else ''}-{p[4] or 'unset'}" for p in PARAMS])
def test_both_dealings_keep_the_tokens_and_the_new_one_reports_where_the_tail_went(jobs, which, cus, n_early, rows, value):
    p = jobs[(which, cus, value)].result()
    assert p.returncode == 0 and f"EMU_CHECK_OK {which}" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
    lines = re.findall(r"persist deal: merge on blocks ([\d,]+); finln on ([\d,]+); logits blocks (\d+)", p.stderr)
    if value != "log":
        assert not lines, lines                       # (only the logging value prints)
        return
    assert lines, "the persistent kernel did not run (no report line)\n" + p.stderr[-2000:]
    for merge, finln, n_lg in lines:                  # one line per built setup
        merge, finln = [int(b) for b in merge.split(",")], [int(b) for b in finln.split(",")]
        assert len(merge) == len(finln) == rows and int(n_lg) >= 1
        if cus:
            assert max(merge + finln) < int(cus)      # (the grid really was the small one)
        if cus != "40":                               # blocks 0 .. n_early - 1 hold the first-layer attention roles
            assert min(merge) >= n_early and merge == finln, (merge, finln)
