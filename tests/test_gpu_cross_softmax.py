"""GPU: greedy decodes whose windows hold the key counts where the block-parallel softmax of the fused cross-attention body
could lose a key, token-exact against the oracle: 63, 64, 65, 511, 512, 513, 750 and 6 keys in the default geometry, 768 (one
pass of the 768-key ring) and 769, 1023, 1024, 1025, 1500 (two passes) in the whisper30 geometry (`set_frame_limit`), 3 - 4
windows of different lengths per call, max_depth 8; the d = 128 micro model and the d = 384 four-layer model; through the
persistent kernel and through the chain of one launch per sublayer (WHISPER_HIP_PERSIST=0).

tests/cross_softmax_checks.py holds the cases and the seeds (tests/test_emu_cross_softmax.py is the CPU twin).  One child process
per decode path (the switch is read once per process), one after the other; a child that dies keeps the next from starting.  The
oracle's rows are computed once, on the CPU.  Stand-alone: timeout -k 10 300 python -m pytest -x -q tests/test_gpu_cross_softmax.py -m gpu"""
import json
import os
import subprocess
import sys

import pytest

import cross_softmax_checks as cs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "whisper-burn_amd")
PATHS = {"persist": {}, "chain": {"WHISPER_HIP_PERSIST": "0"}}
_DEAD = []


def _child(args, extra):
    assert not _DEAD, f"not started: the child for {_DEAD[0]} died"
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, PKG, os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
    for k in ("WHISPER_HIP_PERSIST", "WHISPER_HIP_LIB"):
        env.pop(k, None)
    env.update(extra)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "cross_softmax_checks.py")] + args, env=env,
                       capture_output=True, text=True, timeout=240)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    if p.returncode != 0 or not lines:
        _DEAD.append(args + [extra])
    assert p.returncode == 0 and lines, p.stdout[-2000:] + p.stderr[-4000:]
    return json.loads(lines[-1][7:])


@pytest.fixture(scope="module")
def reference():
    return _child(["oracle", "gpu"], {})              # (no engine: the child never opens the GPU)


@pytest.fixture(scope="module")
def decoded():
    return {}


def _rows(decoded, path):
    if path not in decoded:
        decoded[path] = _child(["gpu"], PATHS[path])
    return decoded[path]


def test_every_key_count_audio_can_reach_is_decoded():
    cases = cs.SETS["gpu"][1]
    one = {C for _, Cs, _ in cases.values() for C in Cs if max(Cs) <= 768}
    two = {C for _, Cs, _ in cases.values() for C in Cs if max(Cs) > 768}
    # (1 key and 1536 keys are out of audio's reach: the shortest window has 6, the longest, 3000 frames, 1500)
    assert one >= {63, 64, 65, 511, 512, 513, 750, 768} and two >= {769, 1023, 1024, 1025, 1500}
    assert all(3 <= len(Cs) <= 4 and len(set(Cs)) == len(Cs) for _, Cs, _ in cases.values()) and cs.DEPTH <= 8


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("model", sorted(cs.MODELS))
@pytest.mark.parametrize("case", sorted(cs.SETS["gpu"][1]))
def test_decode_is_token_exact_at_the_softmax_boundaries(reference, decoded, case, model, path):
    got = _rows(decoded, path)
    key = f"{model}_{case}"
    assert got[key] == reference[key], (path, key, got[key], reference[key])
    assert all(len(r) > 4 for r in reference[key])
