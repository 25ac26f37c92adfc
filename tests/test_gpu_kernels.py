"""GPU: every host-callable kernel launcher against a plain f64 restatement of its operator, one operator at a time.

The rest of the suite looks at the kernels through a whole model and `|logits - oracle| < 1e-3`; here each launcher of
csrc/kernels.h / decode.h (launch_gemm_f32, launch_gemm_f16x3 + launch_split_weight_f16, launch_attention / launch_attention_f32,
launch_layernorm / _pieces, launch_embed, launch_dec_skinny_gemm + launch_split_weight_f16_tiles) is called directly through the
test-only harness library (whisper-burn_amd/tools/kernel_harness.cpp -> lib/libwhisper_hip_ktest.so, built by csrc/Makefile) at the
shapes, strides and epilogue combinations where kernels go wrong -- including every dispatcher branch, three of which no model
reaches (K % 32 != 0 ROWS GEMM, causal split-precision attention, scale != 1 inside the attention kernels) -- and compared
elementwise, ALL elements, with tests/kernel_refs.py under bounds that are derived there (f32 unit roundoff, the split's 2^-21,
the f32 NumPy evaluation of the same statement), never tuned against the kernels.  tests/kernel_cases.py holds the cases, the
poison / canary layout and the comparisons; tests/test_kernel_harness_emu.py proves them on the CPU (functional model, NumPy
mutants) before this file is ever run.

Safety: every launch goes through a public launcher with in-contract arguments and in-bounds arrays (the harness checks both
before it launches); refusals are only tested where the launcher returns before launching; after a HIP error nothing more is
launched.  One process, plus one short-lived child per value of the two attention switches (read once per process).
Stand-alone: timeout -k 10 300 python -m pytest -x -q tests/test_gpu_kernels.py -m gpu"""
import json
import os
import subprocess
import sys
import time

import pytest

import kernel_cases as kc
import parity_log

pytestmark = pytest.mark.gpu

CASES = kc.all_cases()
IN_PROCESS = [cid for cid, (c, _) in CASES.items() if not c.get("env")]
BY_ENV = {}
for _cid, (_c, _) in CASES.items():
    if _c.get("env"):
        BY_ENV.setdefault(_c["env"], []).append(_cid)
_CHILD = {}


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(kc.GPU_LIB), "build first: make -C whisper-burn_amd/csrc (lib/libwhisper_hip_ktest.so)"
    t0 = time.time()
    yield kc.load(kc.GPU_LIB)
    parity_log.flush_ratios(file_wall_s=round(time.time() - t0, 1))


def _record(info):
    if "ratio" in info:
        extra = {k: v for k, v in info.items() if k in ("branch", "c_measured", "gelu_ulps", "gelu_torch_worst_ulps", "ksplit")}
        parity_log.record_ratio(info["family"], info["id"], info["ratio"], **extra)


@pytest.mark.parametrize("cid", IN_PROCESS)
def test_kernel_matches_its_f64_restatement(lib, cid):
    c, fn = CASES[cid]
    info = fn(lib, c)
    print(info)
    _record(info)


def _child(lib, env):
    """All cases of one switch value in ONE fresh process (the launchers read their switches into static locals)."""
    if env not in _CHILD:
        assert kc.HIP_ERROR[0] == 0, "not launched: an earlier call returned a HIP error"
        e = dict(os.environ)
        e[env[0]] = env[1]
        p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "kernel_cases.py"), kc.GPU_LIB]
                           + BY_ENV[env], env=e, capture_output=True, text=True, timeout=240)
        if p.returncode != 0:
            kc.HIP_ERROR[0] = p.returncode                              # a child that died: nothing more is launched
        rows = [json.loads(ln[6:]) for ln in p.stdout.splitlines() if ln.startswith("KCASE ")]
        _CHILD[env] = (p.returncode, {r["id"]: r for r in rows}, p.stdout[-2000:] + p.stderr[-2000:])
    return _CHILD[env]


@pytest.mark.parametrize("cid", [cid for ids in BY_ENV.values() for cid in ids])
def test_attention_with_a_switch_off_matches_its_f64_restatement(lib, cid):
    c, _ = CASES[cid]
    rc, rows, tail = _child(lib, c["env"])
    assert rc == 0 and cid in rows, tail
    info = rows[cid]
    print(info)
    assert info["ok"], info.get("msg")
    assert info["branch"] == kc.attn_case_branch(c)
    _record(info)
