"""GPU: one layer's MLP roles of the persistent kernel in the two-phase form (4 d / 64 co-resident blocks through
`wbk_persist_mlp2` of lib/libwhisper_hip_ktest.so) against dec_mlp_fused_kernel on the same seeded inputs: bit-identical rows.

Cases (tests/persist_mlp2_cases.py): d = 128 and 384, 1 and 3 rows, with 3 rows one row masked dead.
tests/test_emu_persist_mlp2_kernel.py runs the same cases on the CPU first.

Safety: the harness checks every array against the shapes before any launch and builds the granule inputs itself (every granule
carries the tag the roles wait for, so no sweep waits for anything but the roles' own stores); every spin is bounded.  After a
failed case nothing more is launched.  Stand-alone: timeout -k 10 120 python -m pytest -x -q tests/test_gpu_persist_mlp2_kernel.py -m gpu"""
import os

import pytest

import kernel_cases as kc
import persist_mlp2_cases as mc

pytestmark = pytest.mark.gpu

CASES = mc.cases()
_FAILED = []


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(kc.GPU_LIB), "build first: make -C whisper-burn_amd/csrc (lib/libwhisper_hip_ktest.so)"
    return mc.load(kc.GPU_LIB)


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_two_phase_rows_have_the_bits_of_the_planes_folded(lib, c):
    if _FAILED:
        pytest.fail("an earlier case failed (" + _FAILED[0] + "): nothing more is launched")
    r = mc.check(lib, c)
    print(r)
    if not r["ok"]:
        _FAILED.append(c["id"])
    assert r["ok"], r["msg"]
