"""GPU: the persistent decode kernel with the merge and final-LN roles dealt off the first-layer attention blocks
(WHISPER_HIP_PERSIST_DEAL unset) against the same binary with the old dealing (`legacy`: merge on the least loaded blocks --
at the bench shape blocks 0, 1, 2, which hold self-attention roles of the first layer) and against the oracle.

Two fresh child processes (tests/persist_deal_checks.py), one per setting, each under its own time limit; a child that failed
is not started again.  Each decodes 3 windows and then 2 windows of other audio on one engine of the d = 128 two-layer micro
model, then 3 short windows on the d = 384 four-layer model (the `<6,4,1>` instance on the full grid: the dealing the
benchmark gets), max_depth 8.  Rows are equal between the two processes and equal to the oracle rows (computed here, once, on
the CPU)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "whisper-burn_amd")
SWITCH = "WHISPER_HIP_PERSIST_DEAL"
CASES = {"d128_w3": 3, "d128_w2_other": 2, "d384_w3": 3}          # call -> windows

_CACHE = {}


def _run(value):
    if isinstance(_CACHE.get(value), str):             # the child failed before: start nothing on the GPU again
        pytest.fail("the child process of this setting failed earlier: " + _CACHE[value])
    if value not in _CACHE:
        env = {k: v for k, v in os.environ.items()
               if not k.startswith("WHISPER_HIP_") or k in ("WHISPER_HIP_LIB", "WHISPER_HIP_ALLOW_EMU")}
        if value is not None:
            env[SWITCH] = value
        env["PYTHONPATH"] = os.pathsep.join([ROOT, PKG, os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
        try:
            p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "persist_deal_checks.py")], env=env,
                               capture_output=True, text=True, timeout=300)
        except subprocess.TimeoutExpired as e:
            _CACHE[value] = f"no result within {e.timeout} s"
            pytest.fail(_CACHE[value])
        if p.returncode != 0:
            _CACHE[value] = f"exit status {p.returncode}\n" + p.stderr[-3000:]
            pytest.fail(_CACHE[value])
        _CACHE[value] = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])
    return _CACHE[value]


def _oracle():
    if "oracle" not in _CACHE:
        sys.path[:0] = [p for p in (ROOT, PKG, os.path.join(ROOT, "tests")) if p not in sys.path]
        import parity_util as pu
        import persist_deal_checks as pdc
        import whisper_burn_amd as wb
        from oracle import transcribe as otr
        from oracle.model import OracleWhisper
        from whisper_burn_amd import synth
        st = pu.ost(wb.SpecialTokens.for_vocab(pdc.N_VOCAB))
        ref = {}
        for name, d, n_head, n_layer, seed in pdc.MODELS:
            o = OracleWhisper(synth.synth_weights(pdc.dims_of(d, n_head, n_layer), seed=seed))
            for call, n_s, aseed in pdc.CALLS[name]:
                ref[f"{name}_{call}"] = [list(map(int, r)) for r in otr.waveform_to_tokens(
                    o, st, synth.synth_audio(n_s, aseed), 16000, 1, pdc.DEPTH, return_windows=True)[1]]
        _CACHE["oracle"] = ref
    return _CACHE["oracle"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_rows_are_equal_under_both_dealings_and_equal_the_oracle(case):
    new, legacy, ref = _run(None), _run("legacy"), _oracle()[case]
    assert len(ref) == CASES[case] and all(len(r) > 4 for r in ref), ref
    assert new[case] == legacy[case]
    assert new[case] == ref
