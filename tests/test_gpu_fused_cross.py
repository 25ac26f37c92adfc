"""GPU: the fused cross-attention sublayer (launch_dec_cross_fused: dec_cross_fused_kernel<DPL, NP>, the body of the persistent
kernel's cross-attention role) against its f64 restatement, through `wbk_cross_fused` of lib/libwhisper_hip_ktest.so.

Product ring (768 keys per pass): one pass with C in {1, 63, 64, 65, 511, 512, 513, 750, 768}, two passes with C in {769, 1023,
1024, 1025, 1500, 1536}; d = 128 and d = 384, one and three rows with a different C per row, and the two data variants of
tests/fused_cross_cases.py (near-uniform scores; the largest score on a boundary key).  tests/test_emu_fused_cross.py runs the
same generator on the CPU first.

Safety: the harness checks every extent the contract lets the kernel touch before it launches; after a HIP error nothing more is
launched.  Stand-alone: timeout -k 10 300 python -m pytest -x -q tests/test_gpu_fused_cross.py -m gpu"""
import os

import pytest

import fused_cross_cases as fc
import kernel_cases as kc

pytestmark = pytest.mark.gpu

CASES = fc.cases(fc.PROD_RING)


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(kc.GPU_LIB), "build first: make -C whisper-burn_amd/csrc (lib/libwhisper_hip_ktest.so)"
    return fc.load(kc.GPU_LIB)


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_fused_cross_matches_its_f64_restatement(lib, c):
    info = fc.run(lib, c)
    print(info)
