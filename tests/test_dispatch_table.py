"""CPU: which kernels the decode-path selection dispatches, per (decode case, runtime-switch setting), against a table recorded
before the selection was gathered into one plan (tests/golden/dispatch_calls.json) -- class names and call counts, every
cell.  Runs the engine's own sources over the hipemu functional model the way tests/test_emu_functional.py does (one
process per cell: a switch is read once per process).  Plus two text-level checks of the switch table (csrc/switches.h)."""
import concurrent.futures
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "whisper-burn_amd")
EMU_DIR = os.path.join(PKG, "tools", "hipemu")
EMU_LIB = os.path.join(PKG, "lib", "libwhisper_hip_emu.so")
CLANG = os.environ.get("EMUCXX", "/opt/rocm/lib/llvm/bin/clang++")
CSRC = os.path.join(PKG, "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "dispatch_calls.json")
CASES = ["greedy", "chain_eot", "chain_eot_batch", "beam_batch", "beam16"]
SETTINGS = [{}, {"FUSE_SUB": "0"}, {"FUSE_X": "0"}, {"FUSE_Q": "0"}, {"FUSE_X": "0", "FUSE_CO": "1"}, {"FUSE16": "0"},
            {"PERSIST": "0"}, {"PERSIST_PREFILL": "0"}, {"BEAM_CHAIN": "0"}, {"CHAIN": "0"}, {"CROSS_STREAM": "0"},
            {"CROSS_STREAM_FUSE": "0"}, {"BATCH_SKINNY": "0"}, {"DECODER_SPLIT": "0"}, {"LOGITS_MFMA": "0"}, {"MLP16_MFMA": "0"}]


@pytest.fixture(scope="module")
def emu_lib():
    if not (os.path.exists(CLANG) or shutil.which(CLANG)):
        pytest.skip("no host clang++ for the hipemu build")
    subprocess.run(["make", "-C", EMU_DIR, "-j", str(min(8, os.cpu_count() or 1))], check=True, stdout=subprocess.DEVNULL)
    return EMU_LIB


def label(setting):
    return " + ".join(f"{k}={v}" for k, v in setting.items()) or "default"


def trace(lib, case, setting):
    """{kernel class: calls} of one cell, from tests/dispatch_trace.py in a process of its own."""
    env = dict(os.environ)
    env.update({"WHISPER_HIP_LIB": lib, "WHISPER_HIP_ALLOW_EMU": "1"})
    env["PYTHONPATH"] = os.pathsep.join([ROOT, PKG, os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
    env.setdefault("OMP_NUM_THREADS", "2")
    env.update({"WHISPER_HIP_" + k: v for k, v in setting.items()})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "dispatch_trace.py"), case], env=env, capture_output=True,
                       text=True, timeout=1800)
    lines = [l for l in p.stdout.splitlines() if l.startswith("DISPATCH ")]
    assert p.returncode == 0 and len(lines) == 1, (case, setting, p.stdout[-1000:] + p.stderr[-3000:])
    return json.loads(lines[0][9:])[case]


def trace_table(lib, workers):
    cells = [(label(s), c, s) for s in SETTINGS for c in CASES]
    with concurrent.futures.ThreadPoolExecutor(max_workers=workers) as pool:
        futs = [pool.submit(trace, lib, c, s) for _, c, s in cells]
        table = {}
        for (lab, c, _), f in zip(cells, futs):
            table.setdefault(lab, {})[c] = f.result()
    return table


def test_every_case_dispatches_the_recorded_kernels_under_every_switch_setting(emu_lib):
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert "commit" in golden["produced_by"]
    got = trace_table(emu_lib, max(1, min(16, (os.cpu_count() or 2) - 2)))
    want = golden["table"]
    assert set(got) == set(want) == {label(s) for s in SETTINGS}
    diff = {(lab, c): (got[lab][c], want[lab][c]) for lab in want for c in CASES if got[lab][c] != want[lab].get(c)}
    assert not diff, diff
    assert all(set(want[lab]) == set(CASES) for lab in want)


def _switch_table_names():
    with open(os.path.join(CSRC, "switches.h")) as f:
        return set(re.findall(r'"(WHISPER_HIP_[A-Z0-9_]+)"', f.read()))


def test_the_environment_is_read_in_one_file():
    hits = []
    for name in sorted(os.listdir(CSRC)):
        if name == "switches.cpp" or not name.endswith((".cpp", ".h", ".hip")):
            continue
        with open(os.path.join(CSRC, name)) as f:
            if 'getenv("WHISPER_HIP_' in f.read():
                hits.append(name)
    assert not hits, hits
    with open(os.path.join(CSRC, "switches.cpp")) as f:
        assert "getenv(" in f.read()


def test_the_switch_table_is_documented_and_covers_the_switches_the_tests_set():
    table = _switch_table_names()
    assert len(table) >= 30
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        doc = f.read()
    start = doc.index("## Runtime switches")
    nxt = doc.find("\n## ", start + 1)
    section = doc[start:nxt if nxt > 0 else len(doc)]
    rows = [l for l in section.splitlines() if l.startswith("| `WHISPER_HIP_")]
    documented = {re.match(r"\| `(WHISPER_HIP_[A-Z0-9_]+)`", l).group(1) for l in rows}
    assert len(rows) == len(documented) and documented == table, sorted(documented ^ table)
    used = set()
    for name in ("test_gpu_switches.py", "test_emu_functional.py"):
        with open(os.path.join(ROOT, "tests", name)) as f:
            used |= set(re.findall(r"WHISPER_HIP_[A-Z0-9_]+", f.read()))
    used -= {"WHISPER_HIP_LIB", "WHISPER_HIP_ALLOW_EMU"}
    assert used <= table, sorted(used - table)


if __name__ == "__main__":      # regenerate the table: python tests/test_dispatch_table.py <emulator library> <commit> <workers>
    out = {"produced_by": f"commit {sys.argv[2]}: tests/dispatch_trace.py over that commit's lib/libwhisper_hip_emu.so",
           "table": trace_table(sys.argv[1], int(sys.argv[3]))}
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
