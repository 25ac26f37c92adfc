"""CPU: the persistent decode kernel's step boundary on the hipemu functional model (whisper-burn_amd/tools/hipemu).

First-layer self-attention of step e picks the row's next token itself from the tagged tile records of step e - 1
(csrc/decode_persist.hip, "the step boundary"; csrc/decode_fused_bodies.h: ps_pick_token); WHISPER_HIP_PERSIST_PICK=merge keeps
the old edge (the role waits for the merge role's x row).  Every decode cell runs with the switch unset AND with `merge`, each in
a process of its own; the rows of both are the oracle's (computed here, once per cell) and therefore each other's -- integers,
compared with ==:
  * d384: d = 384, 4 layers, 3 rows (weight seed 480, audio seed 52); the middle row ends with its third token, the others at
    max_depth 8 -- the row-end path and the dead-row path run next to live rows;
  * d384 on 40 and on 100 blocks (HIPEMU_CUS): several roles per block, the streamed form;
  * d512 (the `persist512` model), d128 (d = 128, 2 layers, ONE row);
  * early: two of three rows end on their first generated token;
  * guard_chain of tests/emu_checks.py (the existing fixture whose decoder rows turn NaN): the call fails as it does today and no
    NaN becomes a token id, under either setting.
Operator level (tests/persist_pick_cases.py through `wbk_persist_pick` of lib/libwhisper_hip_ktest_emu.so): the pick alone
against a numpy restatement of `better()` -- n_tiles 1, 2, 406, 513, ties, the best value in the last tile, -inf rows, NaN rows."""
import concurrent.futures
import json
import os
import shutil
import subprocess
import sys

import pytest

import kernel_cases as kc
import persist_pick_cases as pc
import persist_pick_checks as ppc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "whisper-burn_amd")
EMU_DIR = os.path.join(PKG, "tools", "hipemu")
EMU_LIB = os.path.join(PKG, "lib", "libwhisper_hip_emu.so")
CLANG = os.environ.get("EMUCXX", "/opt/rocm/lib/llvm/bin/clang++")
SWITCH = "WHISPER_HIP_PERSIST_PICK"

# id -> (cell of tests/persist_pick_checks.py, extra environment); each runs with the switch unset and with `merge`
DECODE = {
    "d384": ("d384", {}),
    "d384@40": ("d384", {"HIPEMU_CUS": "40"}),
    "d384@100": ("d384", {"HIPEMU_CUS": "100"}),
    "d512": ("d512", {}),
    "d128": ("d128", {}),
    "early": ("early", {}),
}
ARMS = {"pick": {}, "merge": {SWITCH: "merge"}}
KCASES = pc.cases()


def _env(extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("WHISPER_HIP_") and k != "HIPEMU_CUS"}
    env["PYTHONPATH"] = os.pathsep.join([ROOT, PKG, os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
    env.setdefault("OMP_NUM_THREADS", "2")
    env.update(extra)
    return env


def _spawn(script, arg, extra):
    return subprocess.run([sys.executable, os.path.join(ROOT, "tests", script), arg],
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
    """Every (cell, arm) as a process of its own (a switch is read once per process), a few side by side."""
    pool = concurrent.futures.ThreadPoolExecutor(max_workers=max(1, min(6, (os.cpu_count() or 2) - 2)))
    futs = {}
    for cid, (cell, extra) in DECODE.items():
        for arm, sw in ARMS.items():
            futs[(cid, arm)] = pool.submit(_spawn, "persist_pick_checks.py", cell, dict(extra, **sw))
    for arm, sw in ARMS.items():
        futs[("guard_chain", arm)] = pool.submit(_spawn, "emu_checks.py", "guard_chain", sw)
    yield futs
    for f in futs.values():
        f.cancel()
    pool.shutdown(wait=True)


_ORACLE = {}


def _oracle(cell):
    if cell not in _ORACLE:
        _ORACLE[cell] = ppc.oracle_rows(cell)
    return _ORACLE[cell]


def _rows(p):
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])


def test_the_cells_end_their_rows_where_the_docstring_says():
    ref, eot = _oracle("d384")
    assert [len(r) - 4 for r in ref] == [8, 3, 8] and ref[1][-1] == eot, ref
    ref, eot = _oracle("early")
    gen = [len(r) - 4 for r in ref]
    assert len(ref) == 3 and sorted(gen)[:2] == [1, 1] and max(gen) > 3 and all(r[-1] == eot for r in ref if len(r) == 5), ref
    ref, _ = _oracle("d128")
    assert len(ref) == 1 and len(set(ref[0][4:])) >= 4, ref
    ref, eot = _oracle("d512")
    assert len(ref) == 4 and all(len(set(r[4:])) >= 4 for r in ref), ref


@pytest.mark.parametrize("cid", sorted(DECODE))
def test_rows_equal_the_oracle_with_the_pick_and_with_the_merge_edge(jobs, cid):
    ref, _ = _oracle(DECODE[cid][0])
    pick, merge = _rows(jobs[(cid, "pick")].result()), _rows(jobs[(cid, "merge")].result())
    assert pick == ref
    assert merge == ref
    assert pick == merge


@pytest.mark.parametrize("arm", sorted(ARMS))
def test_nan_rows_fail_the_call_as_before_and_never_become_a_token(jobs, arm):
    p = jobs[("guard_chain", arm)].result()
    assert p.returncode == 0 and "EMU_CHECK_OK guard_chain" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]


@pytest.fixture(scope="module")
def emu_results(built):
    """Every operator-level case in ONE child process that loads the harness library and nothing else of the engine."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "persist_pick_cases.py"), kc.EMU_LIB], env=_env({}),
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return {r["id"]: r for r in (json.loads(ln[6:]) for ln in p.stdout.splitlines() if ln.startswith("KCASE "))}


def test_the_pick_cases_cover_the_listed_tile_counts_and_rows():
    ids = {c["id"] for c in KCASES}
    for n in (1, 2, 406, 513):
        assert {f"random-{n}", f"best-in-last-tile-{n}", f"all-neg-inf-{n}", f"nan-among-finite-{n}", f"all-nan-{n}"} <= ids
    assert {f"tie-{n}" for n in (2, 406, 513)} <= ids


@pytest.mark.parametrize("c", KCASES, ids=[c["id"] for c in KCASES])
def test_the_pick_alone_equals_the_numpy_restatement_on_the_functional_model(emu_results, c):
    r = emu_results[c["id"]]
    print(r)
    assert r["ok"], r["msg"]
