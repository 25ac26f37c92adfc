"""GPU: the persistent decode kernel behind a launch setup cached on the session (WHISPER_HIP_PERSIST_SETUP, default on) against
the same binary with the switch at `0` (argument blocks and role tables built and uploaded on every call) and the oracle.

Two fresh child processes (tests/persist_setup_checks.py gpu), one per setting.  Each decodes, on ONE engine of the d = 128
micro model: 3 windows, the same 3 windows, 2 windows of other audio -- a change of W under a reused session, the smallest
case in which a stale table can go wrong -- then one call of the d = 384 4-layer synthetic model with 3 short windows at
max_depth 8: the bench's own 4-row d = 384 instance of the kernel.  With the cache on, the launch is enqueued behind the
encoder without a synchronisation in between and the host reads error word, control block and token rows from pinned memory
behind one.  Rows are equal between the two processes and equal to the oracle rows (computed here, once, on the CPU)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "whisper-burn_amd")
SWITCH = "WHISPER_HIP_PERSIST_SETUP"
CASES = ["d128_w3", "d128_w3_again", "d128_w2_other", "d384_w3"]
N_WINDOWS = {"d128_w3": 3, "d128_w3_again": 3, "d128_w2_other": 2, "d384_w3": 3}

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
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "persist_setup_checks.py"), "gpu"], env=env,
                           capture_output=True, text=True, timeout=300)
        if p.returncode != 0:
            _CACHE[value] = f"exit status {p.returncode}\n" + p.stderr[-3000:]
            pytest.fail(_CACHE[value])
        _CACHE[value] = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])
    return _CACHE[value]


def _oracle():
    if "oracle" not in _CACHE:
        sys.path[:0] = [p for p in (ROOT, PKG, os.path.join(ROOT, "tests")) if p not in sys.path]
        import parity_util as pu
        import persist_setup_checks as psc
        import whisper_burn_amd as wb
        from oracle import transcribe as otr
        from oracle.model import OracleWhisper
        from whisper_burn_amd import synth
        st = pu.ost(wb.SpecialTokens.for_vocab(2053))
        ref = {}
        for name, d, n_layer, seed in (("d128", 128, 2, 218), ("d384", 384, 4, 474)):
            dims = synth.micro_dims(n_state=d, n_head=d // 64, n_layer=n_layer, n_vocab=2053, n_audio_ctx=400)
            o = OracleWhisper(synth.synth_weights(dims, seed=seed))
            for step, n_s, aseed in psc.GPU_STEPS[name]:
                key = (name, n_s, aseed)
                if key not in ref:
                    ref[key] = [list(map(int, r)) for r in
                                otr.waveform_to_tokens(o, st, synth.synth_audio(n_s, aseed), 16000, 1, 8, return_windows=True)[1]]
                ref[f"{name}_{step}"] = ref[key]
        _CACHE["oracle"] = ref
    return _CACHE["oracle"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_rows_are_equal_with_the_setup_cached_and_rebuilt_and_equal_the_oracle(case):
    on, off, ref = _run(None), _run("0"), _oracle()[case]
    assert len(ref) == N_WINDOWS[case] and all(len(r) > 4 for r in ref), ref
    assert on[case] == off[case]
    assert on[case] == ref
