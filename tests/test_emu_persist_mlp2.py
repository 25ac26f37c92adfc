"""CPU: the persistent decode kernel's MLP edge on the hipemu functional model (whisper-burn_amd/tools/hipemu).

Default: an MLP role publishes its 64 hidden values per row, sweeps all 4 d of them and finishes 16 columns of the residual row
(csrc/decode_fused_bodies.h: dec_mlp_body, "two phases"); the next layer's self-attention takes the row as a finished stream and
the logits roles apply the final LayerNorm themselves (csrc/decode_persist.hip).  WHISPER_HIP_PERSIST_MLP=planes keeps the old
form: 4 d / 64 partial planes per layer and a final-LN role.  The sums are the same operand for operand, so every decode cell
runs with the switch unset AND with `planes`, each in a process of its own, and the rows of both are the oracle's (computed here,
once per cell) and therefore each other's -- integers, compared with ==:
  * d384: d = 384, 4 layers, 3 rows; the rows generate 8, 3, 8 tokens (the middle one ends: dead rows next to live ones), on the
    full grid and on 40 blocks (HIPEMU_CUS: several roles per block);
  * d128: d = 128, 2 layers, ONE row;
  * early: two of three rows end on their first generated token -- dead rows in both phases of every later MLP role;
  * guard_chain of tests/emu_checks.py (decoder rows turn NaN): the call fails as it does today, under either setting;
  * chain_eot of tests/emu_checks.py (d = 128: 4 d / 64 = 8 MLP roles per layer; 4 windows that end at different steps) with
    the default setting and WHISPER_HIP_PERSIST_DEAL=log, which names the MLP form that ran:
      - on 8 blocks, the smallest grid the two-phase form runs on: every block runs roles of every kind one after another in
        the two-phase form (the kind of cell that caught collective-divergence defects before);
      - on 7 blocks: fewer blocks than MLP roles per layer, where phase 2 would wait for a role further down its own block's
        list -- the host must select the planes form there, so this cell runs NONE of the two-phase code: it checks the choice."""
import concurrent.futures
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

import persist_pick_checks as ppc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "whisper-burn_amd")
EMU_DIR = os.path.join(PKG, "tools", "hipemu")
EMU_LIB = os.path.join(PKG, "lib", "libwhisper_hip_emu.so")
CLANG = os.environ.get("EMUCXX", "/opt/rocm/lib/llvm/bin/clang++")
SWITCH = "WHISPER_HIP_PERSIST_MLP"

# id -> (cell of tests/persist_pick_checks.py, extra environment); each runs with the switch unset and with `planes`
DECODE = {
    "d384": ("d384", {}),
    "d384@40": ("d384", {"HIPEMU_CUS": "40"}),
    "d128": ("d128", {}),
    "early": ("early", {}),
}
ARMS = {"two-phase": {}, "planes": {SWITCH: "planes"}}


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
def jobs():
    """Every (cell, arm) as a process of its own (a switch is read once per process), a few side by side."""
    if not (os.path.exists(CLANG) or shutil.which(CLANG)):
        pytest.skip("no host clang++ for the hipemu build")
    subprocess.run(["make", "-C", EMU_DIR, "-j", str(min(8, os.cpu_count() or 1))], check=True, stdout=subprocess.DEVNULL)
    pool = concurrent.futures.ThreadPoolExecutor(max_workers=max(1, min(6, (os.cpu_count() or 2) - 2)))
    futs = {}
    for cid, (cell, extra) in DECODE.items():
        for arm, sw in ARMS.items():
            futs[(cid, arm)] = pool.submit(_spawn, "persist_pick_checks.py", cell, dict(extra, WHISPER_HIP_PERSIST_DEAL="log", **sw))
    for arm, sw in ARMS.items():
        futs[("guard_chain", arm)] = pool.submit(_spawn, "emu_checks.py", "guard_chain", sw)
    for cus in ("7", "8"):                            # (default setting; the form follows from the grid)
        futs[("chain_eot@" + cus, "default")] = pool.submit(_spawn, "emu_checks.py", "chain_eot",
                                                            {"HIPEMU_CUS": cus, "WHISPER_HIP_PERSIST_DEAL": "log"})
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


@pytest.mark.parametrize("cid", sorted(DECODE))
def test_rows_equal_the_oracle_in_two_phases_and_with_planes(jobs, cid):
    ref, _ = _oracle(DECODE[cid][0])
    two, planes = _rows(jobs[(cid, "two-phase")].result()), _rows(jobs[(cid, "planes")].result())
    for arm in ARMS:                                  # each arm really ran the form it is named after
        forms = re.findall(r"persist deal: .*; mlp form (two-phase|planes)", jobs[(cid, arm)].result().stderr)
        assert forms and set(forms) == {arm}, (arm, forms)
    assert two == ref
    assert planes == ref
    assert two == planes


@pytest.mark.parametrize("arm", sorted(ARMS))
def test_nan_rows_fail_the_call_as_before_and_never_become_a_token(jobs, arm):
    p = jobs[("guard_chain", arm)].result()
    assert p.returncode == 0 and "EMU_CHECK_OK guard_chain" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]


@pytest.mark.parametrize("cus,form", [("8", "two-phase"), ("7", "planes")])
def test_rows_that_end_at_different_steps_on_the_smallest_two_phase_grid_and_one_block_below(jobs, cus, form):
    p = jobs[("chain_eot@" + cus, "default")].result()
    assert p.returncode == 0 and "EMU_CHECK_OK chain_eot" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
    forms = re.findall(r"persist deal: .*; mlp form (two-phase|planes)", p.stderr)
    assert forms and set(forms) == {form}, p.stderr[-2000:]
