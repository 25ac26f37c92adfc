"""CPU: the operator-level kernel tests proven without a GPU.

1. The case generator of tests/test_gpu_kernels.py at the smallest shape of each branch the functional model runs in seconds,
   through lib/libwhisper_hip_ktest_emu.so (tools/kernel_harness.cpp compiled against tools/hipemu): the references, the poison /
   canary layout and the tolerance formulas meet the kernels' own sources here before a GPU minute is spent.
2. Branch coverage: every branch of launch_gemm_f32, launch_gemm_f16x3 and launch_attention / launch_attention_f32 (mirrored in
   tests/kernel_cases.py) is named by at least one case, and so are the required edges.
3. Mutation sensitivity: with NumPy statements of the two arithmetic schemes in the kernels' place, the correct scheme passes
   every case's bound and each mutant -- one cross term dropped, the 2^-11 of the low accumulator forgotten, `kv < q` for
   `kv <= q`, unbiased variance, tanh-GELU -- misses it by at least 10x on the inputs the GPU test uses.

Cases that cannot see a given mutant, whatever the tolerance, are named with the reason (NOT_A_PROBE): a saturated softmax (the
+-80 stress rows are one-hot: an error in the scores does not reach the output) and the LayerNorm cancellation rows (mean 1e4,
spread 1: f32 holds 10 bits of the deviation, the 1 / 2d of an unbiased variance is below that)."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import kernel_cases as kc
import kernel_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "whisper-burn_amd", "tools", "hipemu")
CLANG = os.environ.get("EMUCXX", "/opt/rocm/lib/llvm/bin/clang++")

CASES = kc.all_cases()
EMU_IDS = [cid for cid, (c, _) in CASES.items() if c["emu"]]
GEMM = [(cid, c) for cid, (c, fn) in CASES.items() if fn is kc.run_gemm and c["refuse"] is None and not c["overflow"]]
ATTN = [(cid, c) for cid, (c, fn) in CASES.items() if fn is kc.run_attn and not c.get("bad_ld")]
LN = [(cid, c) for cid, (c, fn) in CASES.items() if fn is kc.run_norm and c["kind"] == "ln"]


# ---- 1. the cases through the functional model -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu_results():
    if not (os.path.exists(CLANG) or shutil.which(CLANG)):
        pytest.skip("no host clang++ for the hipemu build")
    subprocess.run(["make", "-C", EMU_DIR, "-j", str(min(8, os.cpu_count() or 1)), "ktest"], check=True, stdout=subprocess.DEVNULL)
    env = dict(os.environ, WHISPER_HIP_ALLOW_EMU="1")
    for k in ("WHISPER_HIP_ATTN_KVSPLIT", "WHISPER_HIP_ATTN_F16", "WHISPER_HIP_SPLIT_TILE"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "kernel_cases.py"), kc.EMU_LIB] + EMU_IDS, env=env,
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return {r["id"]: r for r in (json.loads(ln[6:]) for ln in p.stdout.splitlines() if ln.startswith("KCASE "))}


@pytest.mark.parametrize("cid", EMU_IDS)
def test_case_passes_on_the_functional_model(emu_results, cid):
    r = emu_results[cid]
    assert r["ok"], r.get("msg")


# ---- 2. coverage -------------------------------------------------------------------------------------------------------------------
def test_every_dispatcher_branch_is_named_by_a_case():
    f32 = {kc.gemm_f32_branch(c["M"], c["N"], c["K"], c["ksplit"], c["mode"] == "conv1") for _, c in GEMM if c["variant"] == "f32"}
    x3 = {kc.gemm_f16x3_branch(c["M"], c["N"], c["K"], c["ksplit"]) for _, c in GEMM if c["variant"] == "f16x3"}
    at = {kc.attn_case_branch(c) for _, c in ATTN}
    assert f32 == kc.GEMM_F32_BRANCHES, kc.GEMM_F32_BRANCHES - f32
    assert x3 == kc.GEMM_F16X3_BRANCHES, kc.GEMM_F16X3_BRANCHES - x3
    assert at == kc.ATTN_BRANCHES, kc.ATTN_BRANCHES - at
    # pieces in (GemmArgs::Ah / Al) is its own template instance of every split-precision tile
    pre = {kc.gemm_f16x3_branch(c["M"], c["N"], c["K"], c["ksplit"]) for _, c in GEMM if c["mode"] == "pre"}
    assert pre >= {"m32_32x128", "64x64", "128x128"}
    # the functional model runs at least one case of every branch it can afford (all but the >= 384-block tiles)
    emu = {kc.gemm_f32_branch(c["M"], c["N"], c["K"], c["ksplit"], c["mode"] == "conv1") for _, c in GEMM
           if c["variant"] == "f32" and c["emu"]}
    assert emu >= kc.GEMM_F32_BRANCHES - {"conv1_128x128", "rows_128x128"}
    assert {kc.attn_case_branch(c) for _, c in ATTN if c["emu"]} >= {"f32_nw2", "f32_kvsplit", "f16x3"}


def test_the_previously_unreached_paths_and_the_required_edges_have_cases():
    # K % 32 != 0 ROWS GEMM; causal split-precision attention; scale != 1 on every attention kernel
    assert any(c["variant"] == "f32" and c["K"] % 32 and c["mode"] != "conv1" for _, c in GEMM)
    assert any(kc.attn_case_branch(c) == "f16x3" and c["causal"] for _, c in ATTN)
    for br in kc.ATTN_BRANCHES:
        assert any(kc.attn_case_branch(c) == br and c["scale"] != 1.0 for _, c in ATTN), br
        assert any(kc.attn_case_branch(c) == br and c["scale"] == 1.0 for _, c in ATTN), br
        if br != "f32_kvsplit":                                        # (the key-split kernel is never chosen for a causal launch)
            assert any(kc.attn_case_branch(c) == br and c["causal"] for _, c in ATTN), br
    for v in ("f32", "f16x3"):
        mine = [c for _, c in GEMM if c["variant"] == v]
        assert {1, 31, 32, 33, 63, 65, 127, 129} <= {c["M"] for c in mine}
        assert {4, 60, 64, 68, 1031} <= {c["N"] for c in mine}
        assert ({32, 96, 1536} | ({16, 48} if v == "f32" else set())) <= {c["K"] for c in mine}
    q = {ql for _, c in ATTN for ql, _ in c["segs"]}
    kv = {kl for _, c in ATTN for _, kl in c["segs"]}
    assert {1, 63, 64, 65, 127, 129, 300} <= q and {1, 31, 32, 33, 63, 65} <= kv
    assert {c["n_head"] for _, c in ATTN} >= {1, 2, 6}
    assert {c["d"] for _, c in LN} == {64, 128, 384, 1280, 260} and {c["M"] for _, c in LN} >= {1, 3, 4, 5, 1001}
    # one child process per switch VALUE, not per case
    assert {c["env"] for _, c in ATTN if c["env"]} == {("WHISPER_HIP_ATTN_KVSPLIT", "0"), ("WHISPER_HIP_ATTN_F16", "0")}


def test_tile_layout_ref_is_the_documented_layout():
    rng = np.random.default_rng(5)
    W = rng.standard_normal((64, 32)).astype(np.float32)
    hi, lo = R.tile_layout_ref(W)
    hb, lb = R.split_f16_bits(W)
    assert hi.shape == (2, 2, 4, 16, 8)
    for k, n in ((0, 0), (37, 21), (63, 31), (8, 16)):
        assert hi[n // 16, k // 32, (k % 32) // 8, n % 16, k % 8] == hb[k, n]
        assert lo[n // 16, k // 32, (k % 32) // 8, n % 16, k % 8] == lb[k, n]
    assert np.abs(R.join_f16(hb, lb) - W.astype(np.float64)).max() <= 2.0 ** -21 * np.abs(W).max()


# ---- 3. mutation sensitivity -------------------------------------------------------------------------------------------------------
NOT_A_PROBE = {
    "drop_cross": lambda c: c.get("stress"),                     # one-hot softmax rows: dS does not reach O
    "unbiased": lambda c: c.get("data") == "cancel",             # f32 holds ~10 bits of (x - mean) there; 1 / 2d is below that
}


def _ratio(fn, c, scheme):
    return fn(None, c, scheme)["ratio"]


@pytest.mark.parametrize("cid", [cid for cid, _ in GEMM])
def test_gemm_bounds_pass_the_correct_scheme_and_fail_every_mutant_by_a_decade(cid):
    c, fn = CASES[cid]
    if c["variant"] == "f32":
        assert _ratio(fn, c, (R.matmul_f32, R.gelu_erf)) <= 1.0
        if c["gelu"]:
            assert _ratio(fn, c, (R.matmul_f32, R.gelu_tanh)) >= 10.0
        return
    assert _ratio(fn, c, (R.matmul_f16x3, R.gelu_erf)) <= 1.0
    for which in ("a_lo", "b_lo"):
        r = _ratio(fn, c, (lambda A, W, w=which: R.matmul_f16x3(A, W, drop_cross=w), R.gelu_erf))
        assert r >= 10.0, f"dropping the {which} cross term reaches only {r:.2f}x the bound"
    r = _ratio(fn, c, (lambda A, W: R.matmul_f16x3(A, W, lo_unscale=1.0), R.gelu_erf))
    assert r >= 10.0, f"forgetting 2^-11 reaches only {r:.2f}x the bound"
    if c["gelu"]:
        assert _ratio(fn, c, (R.matmul_f16x3, R.gelu_tanh)) >= 10.0


@pytest.mark.parametrize("cid", [cid for cid, _ in ATTN])
def test_attention_bounds_pass_the_correct_scheme_and_fail_every_mutant_by_a_decade(cid):
    c, fn = CASES[cid]
    if kc.attn_case_branch(c) == "f16x3":
        assert _ratio(fn, c, R.attention_f16x3) <= 1.0
        muts = {"no 2^-11": dict(lo_unscale=1.0)}
        if not NOT_A_PROBE["drop_cross"](c):
            muts.update({"a_lo dropped": dict(drop_cross="a_lo"), "b_lo dropped": dict(drop_cross="b_lo")})
        if c["causal"]:
            muts["kv < q"] = dict(strict_causal=True)
        for name, kw in muts.items():
            r = _ratio(fn, c, lambda *a, kw=kw: R.attention_f16x3(*a, **kw))
            assert r >= 10.0, f"{name}: only {r:.2f}x the bound"
    else:
        assert _ratio(fn, c, lambda *a: R.attention_ref(*a, dtype=np.float32)[0]) <= 1.0
        if c["causal"]:
            r = _ratio(fn, c, lambda *a: R.attention_ref(*a, dtype=np.float32, strict_causal=True)[0])
            assert r >= 10.0, f"kv < q: only {r:.2f}x the bound"


@pytest.mark.parametrize("cid", [cid for cid, _ in LN])
def test_layernorm_bounds_pass_the_correct_scheme_and_fail_unbiased_variance_by_a_decade(cid):
    c, fn = CASES[cid]
    assert _ratio(fn, c, lambda *a: R.layernorm_ref(*a, dtype=np.float32)) <= 1.0
    if not NOT_A_PROBE["unbiased"](c):
        r = _ratio(fn, c, lambda *a: R.layernorm_ref(*a, dtype=np.float32, unbiased=True))
        assert r >= 10.0, f"unbiased variance: only {r:.2f}x the bound"


def test_harness_library_is_built_with_the_library():
    """`make` in csrc/ -- what __graft_entry__.build() runs -- produces the GPU harness next to the library."""
    assert os.path.exists(kc.GPU_LIB)
