"""CPU: the persistent decode kernel's resident operands under the hipemu functional model (whisper-burn_amd/tools/hipemu).

A block of decode_persist.hip whose role list holds exactly ONE layer role, a self- or cross-attention one, keeps what fits
of that role's step-invariant operands (QKV weight rounds, Wo rows, the window's cached cross V) in LDS for the whole launch
(WHISPER_HIP_PERSIST_RESIDENT, default on; `0`: every block streams them every step; `log`: on, plus one line
`persist resident blocks: N of M` on stderr per launch).  The products keep their operands and their order, so the tokens are
those of the streamed path: tests/emu_checks.py asserts token equality with the oracle for every cell, with the switch at `0`
and at `log`.  From the logged line:
  * every self- / cross-attention role is resident where every block holds one layer role (N = 2 n_layer n_head rows);
  * blocks with several layer roles are left out, on an instance that HAS resident slots: `persist384` (4 rows, d = 384) deals
    144 layer roles; on 40 blocks every block holds several (N = 0, against 96 on the default grid); on 100 blocks the roles
    wrap once -- blocks 0 .. 43 hold two, blocks 44 .. 99 one, and of those one-role blocks 32 hold an attention role -- so
    resident and streamed attention roles run side by side in ONE launch, token-exact (N = 32);
  * the instances that keep the streamed path report N = 0: d >= 384 with the two-pass key ring (prodring30: C = 1500 keys)
    or with 8 rows -- with the resident path compiled in, each spilled a dword more than before (LABLOG)."""
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
EMU_LIB_PROD = os.path.join(PKG, "lib", "libwhisper_hip_emu_prod.so")
CLANG = os.environ.get("EMUCXX", "/opt/rocm/lib/llvm/bin/clang++")
SWITCH = "WHISPER_HIP_PERSIST_RESIDENT"

# check (tests/emu_checks.py), extra environment, library, resident blocks expected with the switch on
#   greedy        d = 128, 2 layers x 2 heads x 1 row                          -> 2 * 2 * 2 * 1 =   8
#   persist384    d = 384, 2 layers x 6 heads x 4 rows                         -> 2 * 2 * 6 * 4 =  96
#   persist384 on 40 blocks: every block holds several of the 144 layer roles  ->                   0
#   persist384 on 100 blocks: role i sits on block i % 100, so blocks 44 .. 99 hold exactly one layer role, role 44 .. 99 of
#                 [layer 0: attn 0..23, cross 24..47, mlp 48..71; layer 1: attn 72..95, cross 96..119, mlp 120..143]:
#                 cross 44..47, mlp 48..71 (never resident), attn 72..95, cross 96..99  -> 4 + 24 + 4 = 32
#   persist384x7  7 rows: the 8-row d = 384 instance keeps the streamed path (and 40 blocks hold several roles each) -> 0
#   persist512    d = 512, 2 layers x 8 heads x 4 rows (192 layer roles, 256 blocks) -> 2 * 2 * 8 * 4 = 128
#   prodring30    d = 384 with the two-pass key ring: the instance keeps the streamed path ->       0
CELLS = [("greedy", {}, "micro", 8), ("persist384", {}, "micro", 96), ("persist384", {"HIPEMU_CUS": "40"}, "micro", 0),
         ("persist384", {"HIPEMU_CUS": "100"}, "micro", 32), ("persist384x7", {"HIPEMU_CUS": "40"}, "micro", 0),
         ("persist512", {}, "micro", 128), ("prodring30", {}, "prod", 0)]
PARAMS = [(which, env, lib, want, value) for which, env, lib, want in CELLS for value in ("0", "log")]


def _spawn(lib, which, extra_env):
    env = dict(os.environ)
    env["WHISPER_HIP_LIB"] = lib
    env["WHISPER_HIP_ALLOW_EMU"] = "1"
    env["PYTHONPATH"] = os.pathsep.join([ROOT, PKG, os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
    env.setdefault("OMP_NUM_THREADS", "2")
    env.update(extra_env)
    return subprocess.run([sys.executable, os.path.join(ROOT, "tests", "emu_checks.py"), which], env=env, capture_output=True,
                          text=True, timeout=900)


def _cus(env):
    return env.get("HIPEMU_CUS", "")


@pytest.fixture(scope="module")
def jobs():
    """Both functional-model libraries, then every cell as a process of its own (a switch is read once per process), a few side
    by side."""
    if not (os.path.exists(CLANG) or shutil.which(CLANG)):
        pytest.skip("no host clang++ for the hipemu build")
    nj = str(min(8, os.cpu_count() or 1))
    subprocess.run(["make", "-C", EMU_DIR, "-j", nj], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", EMU_DIR, "-j", nj, "prod"], check=True, stdout=subprocess.DEVNULL)
    pool = concurrent.futures.ThreadPoolExecutor(max_workers=max(1, min(6, (os.cpu_count() or 2) - 2)))
    libs = {"micro": EMU_LIB, "prod": EMU_LIB_PROD}
    futs = {(which, _cus(env), value): pool.submit(_spawn, libs[lib], which, dict(env, **{SWITCH: value}))
            for which, env, lib, _, value in PARAMS}
    yield futs
    for f in futs.values():
        f.cancel()
    pool.shutdown(wait=True)


@pytest.mark.parametrize("which,env,lib,want,value", PARAMS, ids=[f"{p[0]}{'@' + _cus(p[1]) if _cus(p[1]) else ''}-{p[4]}" for p in PARAMS])
def test_resident_operands_keep_the_tokens_and_cover_the_single_role_blocks(jobs, which, env, lib, want, value):
    p = jobs[(which, _cus(env), value)].result()
    assert p.returncode == 0 and f"EMU_CHECK_OK {which}" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
    lines = re.findall(r"persist resident blocks: (\d+) of (\d+)", p.stderr)
    if value == "0":
        assert not lines, lines                       # (only the logging value prints)
        return
    assert lines, "the persistent kernel did not run (no report line)\n" + p.stderr[-2000:]
    for n, m in lines:                                # one line per persistent launch
        n, m = int(n), int(m)
        assert n == want and n <= m, (which, n, m, want)
    if "HIPEMU_CUS" in env:                           # (the grid really was the small one)
        assert all(int(m) == int(env["HIPEMU_CUS"]) for _, m in lines), lines
