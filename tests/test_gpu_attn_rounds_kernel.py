"""GPU: the fused self-attention sublayer at d = 384 with 2 and with 4 QKV weight rounds held in registers
(launch_dec_attn_fused_rounds: dec_attn_fused_rounds_kernel<NREG>, the body of the persistent kernel's self-attention role), on
the same inputs, through `wbk_attn_fused` of lib/libwhisper_hip_ktest.so.

Lengths 1, 2, 100, 129 and 130 with one and three rows (tests/attn_rounds_cases.py): the plane, the new K / V cache rows and
x_out are bit-identical between the two counts -- same operands, same order -- and each lies within its bound of the f64
restatement.  tests/test_emu_attn_rounds.py runs the same generator on the CPU first.

Safety: the harness checks every extent the contract lets the kernel touch before it launches; after a HIP error nothing more is
launched.  Stand-alone: timeout -k 10 300 python -m pytest -x -q tests/test_gpu_attn_rounds_kernel.py -m gpu"""
import os

import pytest

import attn_rounds_cases as ar
import kernel_cases as kc

pytestmark = pytest.mark.gpu

CASES = ar.cases()


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(kc.GPU_LIB), "build first: make -C whisper-burn_amd/csrc (lib/libwhisper_hip_ktest.so)"
    return ar.load(kc.GPU_LIB)


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_two_and_four_register_rounds_agree_bit_for_bit(lib, c):
    info = ar.run(lib, c)
    print(info)
