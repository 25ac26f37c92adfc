"""Child process of tests/test_emu_persist_setup.py and tests/test_gpu_persist_setup.py: ONE engine (so: one pooled session)
decodes a sequence of calls that keep or change what the persistent kernel's launch setup was built from
(csrc/decode_chain.cpp: ps_setup_ensure, WHISPER_HIP_PERSIST_SETUP).  Prints one line `RESULT <json>`: per step the window
rows.  The library's `persist setup: built | reused` lines go to stderr, one per persistent launch.

    python persist_setup_checks.py emu   the d = 128 micro model of emu_checks.py `greedy`, six steps, oracle rows alongside
    python persist_setup_checks.py gpu   the first three of those steps at n_audio_ctx = 400, then the d = 384 4-layer model
                                         (the 4-row d = 384 instance, the bench's) with 3 short windows at depth 8"""
import dataclasses
import json
import sys

import numpy as np

import whisper_burn_amd as wb
from whisper_burn_amd import synth


def other_tokens(st, n_vocab):
    """Another special mask (the first 64 ordinary ids are masked too) and another <|endoftext|> with the same geometry."""
    mask = np.array(st.is_special, dtype=np.uint8).copy()
    mask[:64] = 1
    return dataclasses.replace(st, end_of_text=n_vocab - 20, is_special=mask)


def emu_steps(n_vocab):
    """(name, seconds, audio seed, max_depth, other tokens?) -- 14.9 s windows: 28 s = 3 windows, 17 s = 2"""
    return [("w3", 28, 7, 8, False), ("w3_again", 28, 7, 8, False), ("w2_other", 17, 11, 8, False), ("w3_third", 28, 7, 8, False),
            ("w3_deeper", 28, 7, 12, False), ("w3_other_tokens", 28, 7, 12, True)]


def rows(eng, st, audio, depth):
    return [list(map(int, w)) for w in wb.waveform_to_tokens(eng, st, audio, 16000, 1, depth)[1]]


def main(mode):
    out = {}
    if mode == "emu":
        import parity_util as pu
        from oracle import transcribe as otr
        from oracle.model import OracleWhisper
        dims = synth.micro_dims(n_state=128, n_head=2, n_layer=2, n_vocab=1031)
        w = synth.synth_weights(dims, seed=4242)
        eng, o = wb.Whisper.from_tensors(w), OracleWhisper(w)
        st = wb.SpecialTokens.for_vocab(1031)
        refs = {}
        for name, secs, seed, depth, other in emu_steps(1031):
            a = synth.synth_audio(16000 * secs, seed)
            s = other_tokens(st, 1031) if other else st
            key = (secs, seed, depth, other)
            if key not in refs:
                refs[key] = [list(map(int, r)) for r in
                             otr.waveform_to_tokens(o, pu.ost(s), a, 16000, 1, depth, return_windows=True)[1]]
            out[name] = {"got": rows(eng, s, a, depth), "ref": refs[key]}
        eng.close()
    else:
        for name, dims, seed in (("d128", synth.micro_dims(n_state=128, n_head=2, n_layer=2, n_vocab=2053, n_audio_ctx=400), 218),
                                 ("d384", synth.micro_dims(n_state=384, n_head=6, n_layer=4, n_vocab=2053, n_audio_ctx=400), 474)):
            eng = wb.Whisper.from_tensors(synth.synth_weights(dims, seed=seed))
            st = wb.SpecialTokens.for_vocab(2053)
            for step, n_s, aseed in GPU_STEPS[name]:
                out[f"{name}_{step}"] = rows(eng, st, synth.synth_audio(n_s, aseed), 8)
            eng.close()
    print("RESULT " + json.dumps(out))


# n_audio_ctx = 400: windows of 62559 samples, 14559 apart -- 40000 samples = 3 windows, 25000 = 2
GPU_STEPS = {"d128": [("w3", 40000, 51), ("w3_again", 40000, 51), ("w2_other", 25000, 52)], "d384": [("w3", 40000, 51)]}

if __name__ == "__main__":
    main(sys.argv[1])
