"""Driven by tests/test_dispatch_table.py in a subprocess with WHISPER_HIP_LIB = lib/libwhisper_hip_emu.so and one setting of
the runtime switches in the environment: runs decode cases of tests/emu_checks.py with per-kernel profiling on and prints,
per case, {kernel class: calls}.  Profiling forces the eager enqueue path -- the function a step graph captures -- so the
counts are a trace of which kernels the decode-path selection picked."""
import contextlib
import io
import json
import sys

import emu_checks
from whisper_burn_amd import _lib

CASES = ["greedy", "chain_eot", "chain_eot_batch", "beam_batch", "beam16"]


def main(cases):
    lib = _lib.load()
    lib.wb_profile_enable(1)
    out = {}
    for which in cases:
        _lib.profile_kernels(reset=True)
        with contextlib.redirect_stdout(io.StringIO()):
            emu_checks.main(which)                   # (asserts token equality with the oracle as it goes)
        out[which] = {k["name"]: k["calls"] for k in _lib.profile_kernels(reset=True)}
    print("DISPATCH " + json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main(sys.argv[1:] or CASES)
