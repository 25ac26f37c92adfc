"""GPU: one logits role of the persistent kernel that applies the final LayerNorm itself against the final-LN role followed by the
logits role (`wbk_persist_logits` of lib/libwhisper_hip_ktest.so, both forms on the same seeded rows): identical tile records.

Cases (tests/persist_logits_cases.py): d = 128 and 384, 1 and 3 rows, with 3 rows one row masked dead, one tile and two tiles.
tests/test_emu_persist_logits_kernel.py runs the same cases on the CPU first.

Safety: the harness checks every array against the shapes before any launch and builds the granule rows itself (every granule
carries the tag the roles wait for); every spin is bounded.  After a failed case nothing more is launched.
Stand-alone: timeout -k 10 120 python -m pytest -x -q tests/test_gpu_persist_logits_kernel.py -m gpu"""
import os

import pytest

import kernel_cases as kc
import persist_logits_cases as mc

pytestmark = pytest.mark.gpu

CASES = mc.cases()
_FAILED = []


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(kc.GPU_LIB), "build first: make -C whisper-burn_amd/csrc (lib/libwhisper_hip_ktest.so)"
    return mc.load(kc.GPU_LIB)


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_records_equal_those_of_the_final_ln_role_and_the_logits_role(lib, c):
    if _FAILED:
        pytest.fail("an earlier case failed (" + _FAILED[0] + "): nothing more is launched")
    r = mc.check(lib, c)
    print(r)
    if not r["ok"]:
        _FAILED.append(c["id"])
    assert r["ok"], r["msg"]
