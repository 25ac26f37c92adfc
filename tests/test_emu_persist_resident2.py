"""CPU: the resident region of the persistent decode kernel with its slots packed onto the lanes that hold an operand
(csrc/decode_fused_bodies.h: ResGeom).

The quarter of every wave that loads nothing in the QKV loop (`seg == 3`) and the threads past the out-projection's row groups
(`jg >= G`) no longer own slots, so the bench instance `<6,4,1>` (d = 384, up to 4 rows, one key pass) keeps TWO QKV weight
rounds in LDS instead of one: 2 x 8 slots x 384 lanes x 16 B = 96 KB of its 15 x 8 KB, and 4 Wo rows behind them.

  * wb_persist_resident_geometry (needs no device: the gfx950 library's own constants) pins the geometry: NRND == 2 for
    (384, 3 rows, 750 keys); for every other instance each number is at least what LABLOG.md R11.1's budget table lists
    (RS, resident QKV rounds, Wo rows of the self-attention role, V tiles and Wo rows of the cross-attention role); the three
    instances without a resident path keep none.
  * `persist384` (tests/emu_checks.py: d = 384, 4 rows -- the `<6,4,1>` instance, now with two resident rounds) on the hipemu
    functional model is token-exact against the oracle with WHISPER_HIP_PERSIST_RESIDENT at `0` and at `log`, and reports the
    resident block count of before: 96 of 169."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "whisper-burn_amd")
for _p in (ROOT, PKG):
    if _p not in sys.path:
        sys.path.insert(0, _p)
EMU_DIR = os.path.join(PKG, "tools", "hipemu")
EMU_LIB = os.path.join(PKG, "lib", "libwhisper_hip_emu.so")
CLANG = os.environ.get("EMUCXX", "/opt/rocm/lib/llvm/bin/clang++")

# (n_state, rows, keys) -> (RS, NRND, NWO_A, NVT, NWO_X) of LABLOG.md R11.1, "Budget per instance"
R11 = {(128, 3, 750): (16, 0, 8, 4, 0), (128, 7, 750): (13, 0, 8, 3, 1), (512, 3, 750): (14, 1, 6, 3, 2),
       (128, 3, 1500): (16, 0, 8, 0, 0), (384, 7, 750): (0, 0, 0, 0, 0), (384, 3, 1500): (0, 0, 0, 0, 0),
       (512, 3, 1500): (0, 0, 0, 0, 0)}


def _geometry(d, rows, keys):
    from whisper_burn_amd import _lib
    out = (C.c_int32 * 5)()
    assert _lib.load(_lib.LIB_PATH).wb_persist_resident_geometry(d, rows, keys, out) == 0
    return tuple(out)


def test_the_bench_instance_keeps_two_qkv_rounds_resident():
    rs, nrnd, nwo_a, nvt, nwo_x = _geometry(384, 3, 750)
    assert rs == 15 and nrnd == 2
    assert nvt >= 3 and nwo_x >= 3                    # (the cross-attention role keeps what it had)
    # two packed rounds and the Wo rows fit the region: (16 slots x 384 lanes + rows x 384 threads) float4 <= RS x 512
    assert nwo_a >= 1 and 2 * 8 * 384 + nwo_a * 384 <= rs * 512
    assert _geometry(384, 4, 750) == _geometry(384, 1, 750) == (rs, nrnd, nwo_a, nvt, nwo_x)


@pytest.mark.parametrize("shape", sorted(R11))
def test_no_other_instance_keeps_less_than_before(shape):
    got, want = _geometry(*shape), R11[shape]
    assert all(g >= w for g, w in zip(got, want)), (shape, got, want)
    if want[0] == 0:                                  # the instances that keep the streamed path still do
        assert got == want


def test_a_shape_without_an_instance_is_an_error():
    from whisper_burn_amd import _lib
    out = (C.c_int32 * 5)()
    assert _lib.load(_lib.LIB_PATH).wb_persist_resident_geometry(384, 9, 750, out) != 0


@pytest.fixture(scope="module")
def emu_lib():
    if not (os.path.exists(CLANG) or shutil.which(CLANG)):
        pytest.skip("no host clang++ for the hipemu build")
    subprocess.run(["make", "-C", EMU_DIR, "-j", str(min(8, os.cpu_count() or 1))], check=True, stdout=subprocess.DEVNULL)
    return EMU_LIB


@pytest.mark.parametrize("value", ["0", "log"])
def test_persist384_is_token_exact_with_two_resident_rounds(emu_lib, value):
    env = dict(os.environ)
    env.update({"WHISPER_HIP_LIB": emu_lib, "WHISPER_HIP_ALLOW_EMU": "1", "WHISPER_HIP_PERSIST_RESIDENT": value})
    env["PYTHONPATH"] = os.pathsep.join([ROOT, PKG, os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
    env.setdefault("OMP_NUM_THREADS", "2")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "emu_checks.py"), "persist384"], env=env,
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0 and "EMU_CHECK_OK persist384" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
    lines = re.findall(r"persist resident blocks: (\d+) of (\d+)", p.stderr)
    assert lines == ([] if value == "0" else [("96", "169")]), lines
