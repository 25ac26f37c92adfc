"""GPU: the persistent decode kernel with resident operands (WHISPER_HIP_PERSIST_RESIDENT, default on) against the same
binary with the switch at `0` (every block streams its operands every step, the code path of before).

A block of decode_persist.hip whose only layer role is a self- or cross-attention role keeps QKV weight rounds, Wo rows and
the window's cached cross V in LDS for the whole launch.  Every product keeps its operands and its place in the sum, so the
token rows must be IDENTICAL between the two settings -- no tolerance.  One child process per setting (a switch is read once
per process) decodes every case; the results are shared by the tests below.
  (a) the bench clip: tiny.en preset, 3 windows, depth 100 (rows end after 3 / 25 / 100 tokens): identical, and equal to the
      committed oracle rows
  (b) ONE engine decodes clip A, clip B (another seed), clip A again: each equals a fresh engine's result -- V left over
      from an earlier launch would show here (the cached cross K/V changes from decode to decode, the session is reused)
  (c) the d = 128 micro model with 1, 4 and 7 rows (depth 30: its rows end on <|endoftext|> at different steps, so a row that
      has ended runs beside live ones -- asserted) and d = 384 with 2 rows at depth 12 (both rows run to the depth): the
      smallest shapes that reach the 4-row and the 8-row instance and one block per role
  (d) the opt-in 30 s window (C = 1500 keys, two key passes), depth 12: the instance that keeps the streamed path behind the
      same LDS arena; equal to the prefix of the committed depth-100 oracle rows (greedy rows are prefixes of deeper ones)"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "oracle_outputs.npz")
SWITCH = "WHISPER_HIP_PERSIST_RESIDENT"
PROMPT_LEN = 4                                         # <|startoftranscript|> <|en|> <|transcribe|> <|notimestamps|>

CHILD = r"""
import json, sys
sys.path[:0] = [%(root)r, %(pkg)r, %(tests)r]
import whisper_burn_amd as wb
from whisper_burn_amd import synth
import workloads
out = {}
def rows(eng, st, audio, depth):
    return [list(map(int, w)) for w in wb.waveform_to_tokens(eng, st, audio, 16000, 1, depth)[1]]
# (a) + (b): the bench model
wl = workloads.WORKLOADS["tiny_bench"]
w = wl.weights()
eng = wb.Whisper.from_tensors(w)
st = wb.SpecialTokens.for_vocab(eng.dims["n_vocab"])
A, B = wl.audio(), synth.synth_audio(wl.n_samples, wl.audio_seed + 17)
out["bench"] = rows(eng, st, A, wl.depth)
out["reuse"] = [out["bench"], rows(eng, st, B, wl.depth), rows(eng, st, A, wl.depth)]
eng.close()
fresh = []
for clip in (A, B):
    e2 = wb.Whisper.from_tensors(w)
    fresh.append(rows(e2, st, clip, wl.depth))
    e2.close()
out["fresh"] = fresh
# (d): the opt-in 30 s window on the same weights
e3 = wb.Whisper.from_tensors(w)
e3.set_frame_limit(True)
out["whisper30"] = rows(e3, st, workloads.WORKLOADS["tiny_whisper30"].audio(), 12)
e3.close()
# (c): micro models, n_audio_ctx = 400 (windows of 62559 samples, 14559 apart)
for name, d, n_s, depth in (("d128x1", 128, 10000, 30), ("d128x4", 128, 50000, 30), ("d128x7", 128, 96000, 30),
                            ("d384x2", 384, 20000, 12)):
    dims = synth.micro_dims(n_state=d, n_head=d // 64, n_layer=2, n_vocab=2053, n_audio_ctx=400)
    em = wb.Whisper.from_tensors(synth.synth_weights(dims, seed=90 + d))
    out[name] = rows(em, wb.SpecialTokens.for_vocab(2053), synth.synth_audio(n_s, 51), depth)
    em.close()
print("RESULT " + json.dumps(out))
"""

_CACHE = {}


def _run(value):
    if isinstance(_CACHE.get(value), str):             # the child failed before: start nothing on the GPU again
        pytest.fail("the child process of this setting failed earlier: " + _CACHE[value])
    if value not in _CACHE:
        env = {k: v for k, v in os.environ.items()
               if not k.startswith("WHISPER_HIP_") or k in ("WHISPER_HIP_LIB", "WHISPER_HIP_ALLOW_EMU")}
        env[SWITCH] = value
        code = CHILD % {"root": ROOT, "pkg": os.path.join(ROOT, "whisper-burn_amd"), "tests": os.path.join(ROOT, "tests")}
        p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
        if p.returncode != 0:
            _CACHE[value] = f"exit status {p.returncode}\n" + p.stderr[-3000:]
            pytest.fail(_CACHE[value])
        res = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])
        _CACHE[value] = (res, [(int(n), int(m)) for n, m in re.findall(r"persist resident blocks: (\d+) of (\d+)", p.stderr)])
    return _CACHE[value]


def _golden(name):
    g = np.load(GOLD)
    return [g[f"{name}_tokens"][i][:int(g[f"{name}_lens"][i])].tolist() for i in range(len(g[f"{name}_lens"]))]


@pytest.mark.gpu
def test_bench_clip_rows_are_identical_and_equal_the_oracle():
    (on, log), (off, log0) = _run("log"), _run("0")
    assert on["bench"] == off["bench"]
    assert on["bench"] == _golden("tiny_bench")
    assert len({len(r) for r in on["bench"]}) == 3     # (the rows end at three different steps: dead rows beside live ones)
    # the resident path really ran: the first launch is the bench clip's (240 layer roles, 144 of them attention roles)
    assert log and log[0][0] > 0 and not log0, (log[:3], log0[:3])


@pytest.mark.gpu
@pytest.mark.parametrize("value", ["log", "0"])
def test_a_reused_engine_decodes_like_a_fresh_one(value):
    res, _ = _run(value)
    a, b = res["fresh"]
    assert a != b                                      # (two different clips)
    assert res["reuse"] == [a, b, a]


@pytest.mark.gpu
@pytest.mark.parametrize("case,n_rows", [("d128x1", 1), ("d128x4", 4), ("d128x7", 7), ("d384x2", 2)])
def test_micro_models_rows_are_identical(case, n_rows):
    (on, _), (off, _) = _run("log"), _run("0")
    assert len(on[case]) == n_rows and all(len(r) > PROMPT_LEN for r in on[case])
    if case in ("d128x4", "d128x7"):                   # rows end at different steps: a row that has ended beside live ones
        assert len({len(r) for r in on[case]}) >= 2, [len(r) for r in on[case]]
    assert on[case] == off[case]


@pytest.mark.gpu
def test_the_30_s_window_rows_are_identical_and_prefixes_of_the_oracle_rows():
    (on, _), (off, _) = _run("log"), _run("0")
    assert on["whisper30"] == off["whisper30"]
    ref = _golden("tiny_whisper30")
    assert on["whisper30"] == [r[:PROMPT_LEN + 12] for r in ref]
