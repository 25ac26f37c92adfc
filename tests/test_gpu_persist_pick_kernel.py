"""GPU: the token pick of the persistent kernel's first-layer self-attention role in isolation (ps_pick_token, one block of 512
threads, through `wbk_persist_pick` of lib/libwhisper_hip_ktest.so) against a numpy restatement of `better()`.

Cases (tests/persist_pick_cases.py): n_tiles in {1, 2, 406, 513}; the best value tied between two tiles (the lowest id wins, in
either record order); the best value in the last tile; a row of only -inf; rows holding NaN.  Ids are integers: compared with ==.
tests/test_emu_persist_pick.py runs the same cases on the CPU first.

Safety: the harness refuses (before any launch) a record array that does not hold n_tiles records carrying the tag, so the sweep
never waits; the kernel reads n_tiles x 16 bytes inside the uploaded array and writes one int.  After a failed case nothing more
is launched.  Stand-alone: timeout -k 10 120 python -m pytest -x -q tests/test_gpu_persist_pick_kernel.py -m gpu"""
import os

import pytest

import kernel_cases as kc
import persist_pick_cases as pc

pytestmark = pytest.mark.gpu

CASES = pc.cases()
_FAILED = []


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(kc.GPU_LIB), "build first: make -C whisper-burn_amd/csrc (lib/libwhisper_hip_ktest.so)"
    return pc.load(kc.GPU_LIB)


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_pick_equals_the_numpy_restatement(lib, c):
    if _FAILED:
        pytest.fail("an earlier case failed (" + _FAILED[0] + "): nothing more is launched")
    r = pc.check(lib, c)
    print(r)
    if not r["ok"]:
        _FAILED.append(c["id"])
    assert r["ok"], r["msg"]
