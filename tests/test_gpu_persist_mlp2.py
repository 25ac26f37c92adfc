"""GPU: the persistent decode kernel with two-phase MLP roles and the final LayerNorm inside the logits roles
(csrc/decode_fused_bodies.h: dec_mlp_body, "two phases"; csrc/decode_persist.hip; WHISPER_HIP_PERSIST_MLP unset) against the
oracle, against the same binary in the old form (`planes`: 4 d / 64 partial planes per layer, a final-LN role) and against the
paths that have no such edge.

Fresh child processes (tests/persist_pick_checks.py), one per cell and setting, each under its own time limit; a child that
failed is not started again:
  * d384 (d = 384, 4 layers, 3 windows, max_depth 8; the middle row ends with its third generated token: dead rows in both
    phases): default, WHISPER_HIP_PERSIST_MLP=planes, WHISPER_HIP_PERSIST_RESIDENT=0, WHISPER_HIP_PERSIST=0 (one launch per
    sublayer: no persistent kernel);
  * d128 (d = 128, 2 layers, one window, max_depth 10): default and `planes`.
The rows of every setting are equal to the oracle's (computed here, once per cell, on the CPU) and to each other."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "whisper-burn_amd")
SETTINGS = {"default": {}, "planes": {"WHISPER_HIP_PERSIST_MLP": "planes"}, "resident0": {"WHISPER_HIP_PERSIST_RESIDENT": "0"},
            "persist0": {"WHISPER_HIP_PERSIST": "0"}}
RUNS = [("d384", s) for s in sorted(SETTINGS)] + [("d128", "default"), ("d128", "planes")]

_CACHE = {}


def _run(cell, name):
    key = (cell, name)
    if isinstance(_CACHE.get(key), str):               # the child failed before: start nothing on the GPU again
        pytest.fail("the child process of this setting failed earlier: " + _CACHE[key])
    if key not in _CACHE:
        env = {k: v for k, v in os.environ.items()
               if not k.startswith("WHISPER_HIP_") or k in ("WHISPER_HIP_LIB", "WHISPER_HIP_ALLOW_EMU")}
        env.update(SETTINGS[name])
        env["PYTHONPATH"] = os.pathsep.join([ROOT, PKG, os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
        try:
            p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "persist_pick_checks.py"), cell], env=env,
                               capture_output=True, text=True, timeout=300)
        except subprocess.TimeoutExpired as e:
            _CACHE[key] = f"no result within {e.timeout} s"
            pytest.fail(_CACHE[key])
        if p.returncode != 0:
            _CACHE[key] = f"exit status {p.returncode}\n" + p.stderr[-3000:]
            pytest.fail(_CACHE[key])
        _CACHE[key] = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])
    return _CACHE[key]


def _oracle(cell):
    if ("oracle", cell) not in _CACHE:
        sys.path[:0] = [p for p in (ROOT, PKG, os.path.join(ROOT, "tests")) if p not in sys.path]
        import persist_pick_checks as ppc
        _CACHE[("oracle", cell)] = ppc.oracle_rows(cell)
    return _CACHE[("oracle", cell)]


def test_the_d384_cell_has_three_windows_and_a_row_that_ends_within_four_tokens():
    ref, eot = _oracle("d384")
    gen = [len(r) - 4 for r in ref]
    assert len(ref) == 3 and min(gen) <= 4 and max(gen) == 8, gen
    assert any(g <= 4 and r[-1] == eot for g, r in zip(gen, ref)), ref


@pytest.mark.gpu
@pytest.mark.parametrize("cell,name", RUNS, ids=[f"{c}-{s}" for c, s in RUNS])
def test_rows_equal_the_oracle_and_each_other(cell, name):
    ref, _ = _oracle(cell)
    got = _run(cell, name)
    assert got == ref
    assert got == _run(cell, "default")
