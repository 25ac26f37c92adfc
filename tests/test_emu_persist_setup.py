"""CPU: the persistent decode kernel's launch setup, cached on the session, under the hipemu functional model.

The per-layer argument blocks and the dealt role tables of decode_persist.hip are a function of the model, the session's
buffers, W, the grid, the window geometry and the resident switch; csrc/decode_chain.cpp (ps_setup_ensure) keeps them on the
device under a key that names all of it and rebuilds them only when the key changes (WHISPER_HIP_PERSIST_SETUP: unset = on;
`0` = built on every call; `log` = on, plus one line `persist setup: built | reused` on stderr per launch; `0log` = both).

ONE engine -- one pooled session -- decodes six calls on the d = 128 micro model of emu_checks.py `greedy` (max_depth <= 12,
14.9 s windows); tests/persist_setup_checks.py is the child.  Expected lines, and why:
  1  3 windows                                     built    nothing cached yet
  2  the same 3 windows                            reused   same key
  3  2 windows of other audio                      built    W, S, the grid's role count and enc_rows change
  4  3 windows again                               built    the session holds ONE setup, and step 3 replaced it with W = 2's
  5  3 windows, max_depth 12 instead of 8          built    session_reserve sets Lmax = 4 + max_depth + 1: the cached K/V layer
                                                            stride inside the argument blocks changes
  6  as 5 with another special mask and another    reused   both travel by value (PersistArgs::eot) or behind an unchanged
     <|endoftext|>                                          pointer (the mask buffer's contents)
Every call's window rows equal the oracle's, in every run:
  * switch at `log`
  * `log` + WHISPER_HIP_PERSIST_INJECT_FAIL=launch: the first call builds, its launch is refused, the session leaves the
    persistent kernel for good -- one line, and the chain of one launch per sublayer produces the same rows
  * switch at `0` (silent) and at `0log`: six lines, all `built`"""
import concurrent.futures
import json
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
SWITCH = "WHISPER_HIP_PERSIST_SETUP"
STEPS = ["w3", "w3_again", "w2_other", "w3_third", "w3_deeper", "w3_other_tokens"]
WINDOWS = [3, 3, 2, 3, 3, 3]
EXPECT = ["built", "reused", "built", "built", "built", "reused"]
RUNS = {"log": {SWITCH: "log"}, "inject": {SWITCH: "log", "WHISPER_HIP_PERSIST_INJECT_FAIL": "launch"},
        "off": {SWITCH: "0"}, "off_log": {SWITCH: "0log"}}


def _spawn(extra_env):
    env = {k: v for k, v in os.environ.items() if not k.startswith("WHISPER_HIP_")}
    env["WHISPER_HIP_LIB"] = EMU_LIB
    env["WHISPER_HIP_ALLOW_EMU"] = "1"
    env["PYTHONPATH"] = os.pathsep.join([ROOT, PKG, os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
    env.setdefault("OMP_NUM_THREADS", "2")
    env.update(extra_env)
    return subprocess.run([sys.executable, os.path.join(ROOT, "tests", "persist_setup_checks.py"), "emu"], env=env,
                          capture_output=True, text=True, timeout=1800)


@pytest.fixture(scope="module")
def runs():
    if not (os.path.exists(CLANG) or shutil.which(CLANG)):
        pytest.skip("no host clang++ for the hipemu build")
    subprocess.run(["make", "-C", EMU_DIR, "-j", str(min(8, os.cpu_count() or 1))], check=True, stdout=subprocess.DEVNULL)
    with concurrent.futures.ThreadPoolExecutor(max_workers=len(RUNS)) as pool:
        futs = {name: pool.submit(_spawn, env) for name, env in RUNS.items()}
        out = {}
        for name, f in futs.items():
            p = f.result()
            assert p.returncode == 0, (name, p.stdout[-1000:] + p.stderr[-3000:])
            res = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])
            out[name] = (res, re.findall(r"persist setup: (\w+)", p.stderr))
    return out


@pytest.mark.parametrize("run", list(RUNS))
def test_every_call_equals_the_oracle(runs, run):
    res, _ = runs[run]
    assert list(res) == STEPS
    for step, n_win in zip(STEPS, WINDOWS):
        got, ref = res[step]["got"], res[step]["ref"]
        assert len(ref) == n_win and all(len(r) > 4 for r in ref), (step, ref)
        assert got == ref, (run, step, got, ref)
    # (the steps really differ where the table says so: other audio, a deeper decode, other tokens)
    assert res["w3"]["ref"] == res["w3_again"]["ref"] == res["w3_third"]["ref"] != res["w2_other"]["ref"][:3]
    assert max(map(len, res["w3_deeper"]["ref"])) > 4 + 8 and res["w3_deeper"]["ref"] != res["w3_other_tokens"]["ref"]


def test_the_setup_is_reused_exactly_while_its_key_stands(runs):
    assert runs["log"][1] == EXPECT


def test_a_refused_launch_builds_once_and_falls_back(runs):
    assert runs["inject"][1] == ["built"]              # (the session stops trying the persistent kernel)
    assert runs["inject"][0] == runs["log"][0]


def test_switch_off_builds_on_every_call(runs):
    assert runs["off"][1] == []                        # (only a value with `log` prints)
    assert runs["off_log"][1] == ["built"] * len(STEPS)
    assert runs["off"][0] == runs["off_log"][0] == runs["log"][0]
