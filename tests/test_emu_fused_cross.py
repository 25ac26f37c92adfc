"""CPU: the fused cross-attention sublayer (launch_dec_cross_fused) against its f64 restatement on the hipemu functional model,
through `wbk_cross_fused` of lib/libwhisper_hip_ktest_emu.so.  The functional model's key ring holds 384 keys per pass, so the
one-pass body runs C in {383, 384} and the two-pass body C in {385, 511, 512, 513, 745, 768}: every boundary of the block-parallel
softmax (512 keys per block round, 64 per lane round, the ring) at d = 128 and d = 384, one and three rows, both data variants
(tests/fused_cross_cases.py)."""
import json
import os
import shutil
import subprocess
import sys

import pytest

import fused_cross_cases as fc
import kernel_cases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "whisper-burn_amd", "tools", "hipemu")
CLANG = os.environ.get("EMUCXX", "/opt/rocm/lib/llvm/bin/clang++")

CASES = fc.cases(fc.EMU_RING)


@pytest.fixture(scope="module")
def emu_results():
    """Every case in ONE child process that loads the harness library and nothing else of the engine (as
    tests/test_kernel_harness_emu.py does: the suite's own process may already hold the gfx950 library, whose launchers carry
    the same names)."""
    if not (os.path.exists(CLANG) or shutil.which(CLANG)):
        pytest.skip("no host clang++ for the hipemu build")
    subprocess.run(["make", "-C", EMU_DIR, "-j", str(min(8, os.cpu_count() or 1)), "ktest"], check=True, stdout=subprocess.DEVNULL)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fused_cross_cases.py"), kc.EMU_LIB, str(fc.EMU_RING)],
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return {r["id"]: r for r in (json.loads(ln[6:]) for ln in p.stdout.splitlines() if ln.startswith("KCASE "))}


def test_every_listed_key_count_has_both_variants_at_both_widths_and_row_counts():
    for ring in (fc.EMU_RING, fc.PROD_RING):
        cs = fc.cases(ring)
        for n_pass in (1, 2):
            for Cn in fc.KEYS[(ring, n_pass)]:
                mine = {(c["d"], c["rows"], c["variant"]) for c in cs if c["n_pass"] == n_pass and c["Cs"][0] == Cn}
                assert mine == {(d, r, v) for d in (128, 384) for r in (1, 3) for v in ("uniform", "peak")}
        assert all(len(set(c["Cs"])) == c["rows"] for c in cs)                       # a different C per row
        # the peak sits on the last key and on every boundary key below it somewhere in the list
        peaks = {fc.peak_key(Cn, r, h) for c in cs for r, Cn in enumerate(reversed(c["Cs"])) for h in range(c["d"] // 64)}
        assert {b for b in fc.BOUNDARY if b < max(max(c["Cs"]) for c in cs) - 1 and b < 2 * ring} <= peaks


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_fused_cross_matches_its_f64_restatement_on_the_functional_model(emu_results, c):
    r = emu_results[c["id"]]
    print(r)
    assert r["ok"], r.get("msg")
