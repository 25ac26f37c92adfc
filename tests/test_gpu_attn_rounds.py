"""GPU: the persistent decode kernel's self-attention role with four QKV weight rounds in registers at d = 384
(csrc/decode_fused_bodies.h: dec_attn_body, NREG) against the oracle and against the paths that keep two.

Three fresh child processes (tests/attn_rounds_checks.py), one per setting, each under its own time limit; a child that failed
is not started again:
  * default: resident blocks -- rounds 0, 1, 4, 5 in registers, 2, 3 in LDS, no weight load behind the wait;
  * WHISPER_HIP_PERSIST_RESIDENT=0: the streamed form -- rounds 0 - 3 in registers, 4, 5 follow into the first two sets;
  * WHISPER_HIP_PERSIST=0: the one-launch-per-sublayer kernels (two rounds).
The d = 384 four-layer model decodes 3 windows of different lengths, max_depth 8; the middle row ends with its third generated
token.  The rows of the three processes are equal to each other and to the oracle's (computed here, once, on the CPU)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "whisper-burn_amd")
SETTINGS = {"default": {}, "resident0": {"WHISPER_HIP_PERSIST_RESIDENT": "0"}, "persist0": {"WHISPER_HIP_PERSIST": "0"}}

_CACHE = {}


def _run(name):
    if isinstance(_CACHE.get(name), str):              # the child failed before: start nothing on the GPU again
        pytest.fail("the child process of this setting failed earlier: " + _CACHE[name])
    if name not in _CACHE:
        env = {k: v for k, v in os.environ.items()
               if not k.startswith("WHISPER_HIP_") or k in ("WHISPER_HIP_LIB", "WHISPER_HIP_ALLOW_EMU")}
        env.update(SETTINGS[name])
        env["PYTHONPATH"] = os.pathsep.join([ROOT, PKG, os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
        try:
            p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "attn_rounds_checks.py")], env=env,
                               capture_output=True, text=True, timeout=300)
        except subprocess.TimeoutExpired as e:
            _CACHE[name] = f"no result within {e.timeout} s"
            pytest.fail(_CACHE[name])
        if p.returncode != 0:
            _CACHE[name] = f"exit status {p.returncode}\n" + p.stderr[-3000:]
            pytest.fail(_CACHE[name])
        _CACHE[name] = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])
    return _CACHE[name]


def _oracle():
    if "oracle" not in _CACHE:
        sys.path[:0] = [p for p in (ROOT, PKG, os.path.join(ROOT, "tests")) if p not in sys.path]
        import attn_rounds_checks as arc
        import parity_util as pu
        import whisper_burn_amd as wb
        from oracle import transcribe as otr
        from oracle.model import OracleWhisper
        from whisper_burn_amd import synth
        st = pu.ost(wb.SpecialTokens.for_vocab(arc.N_VOCAB))
        o = OracleWhisper(synth.synth_weights(arc.dims(), seed=arc.W_SEED))
        rows = otr.waveform_to_tokens(o, st, synth.synth_audio(arc.N_SAMPLES, arc.A_SEED), 16000, 1, arc.DEPTH, return_windows=True)[1]
        _CACHE["oracle"] = ([list(map(int, r)) for r in rows], int(st.end_of_text))
    return _CACHE["oracle"]


def test_the_case_has_three_windows_and_a_row_that_ends_within_four_tokens():
    ref, eot = _oracle()
    gen = [len(r) - 4 for r in ref]
    assert len(ref) == 3 and min(gen) <= 4 and max(gen) == 8, gen
    assert any(g <= 4 and r[-1] == eot for g, r in zip(gen, ref)), ref


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SETTINGS))
def test_rows_equal_the_oracle_and_each_other(name):
    ref, _ = _oracle()
    got = _run(name)
    assert got == ref
    assert got == _run("default")
