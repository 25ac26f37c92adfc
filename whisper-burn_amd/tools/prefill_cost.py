"""Cost of the prompt prefill (LABLOG R19.1): tiny.en bench windows, W = 1 (the seek loop's shape) and
W = 3, prompts of n = 3, 16, 64 and 226 tokens, one MI355X.  Wall time of the greedy decode_timestamps at depth 100 behind the
prompt and of the prefill of its first n - 1 tokens alone, each the median of 5 calls on a rewound session.

    python whisper-burn_amd/tools/prefill_cost.py [pass|steps] [repeats]

`pass`: prefill mode 1 (one teacher-forced pass); `steps`: mode 0, and the prefill alone as n - 1 Session.step calls -- what a
tree without the pass does, so the same file measures the parent commit (it falls back to `steps` where Session has no
set_prefill; PREFILL_COST_ROOT=<checkout> makes this file import that checkout's package and library).  Run it once under `rocprofv3 --kernel-trace --stats` for the per-launch times."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.environ.get("PREFILL_COST_ROOT") or os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "whisper-burn_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import whisper_burn_amd as wb          # noqa: E402
from whisper_burn_amd import synth     # noqa: E402
from whisper_burn_amd.tokens import default_suppress   # noqa: E402


def main():
    arm = sys.argv[1] if len(sys.argv) > 1 else "pass"
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    if not hasattr(wb.Session, "set_prefill"):
        arm = "steps"
    eng = wb.Whisper.from_tensors(synth.synth_preset("tiny.en"))
    st = wb.SpecialTokens.for_vocab(51864)
    audio = synth.synth_audio(480000, synth.BENCH_AUDIO_SEED)
    depth = 100
    p1 = wb.decode_params(st, 1, depth)
    wlen = wb.max_waveform_samples(eng.max_mel_frames() - p1.padding)
    starts, lens = wb.window_extents(len(audio), 16000, wlen, p1.overlap_seconds)
    sup, sup1 = default_suppress(st)
    tp = wb.TimestampParams(st.timestamp_begin, st.n_timestamps)
    ids = [int(t) for t in np.random.default_rng(3).integers(1000, 40000, 256)]
    base = [st.start_of_transcript, st.language, st.transcribe]
    out = {"arm": arm}
    for W in (1, 3):
        sess = wb.Session.begin(eng, audio, starts[:W], lens[:W], max_beams=1)
        sess.set_suppress(sup, sup1)
        if arm == "pass":
            sess.set_prefill(1)
        for n in (3, 16, 64, 226):
            prompt = base if n == 3 else [st.start_of_prev] + ids[:n - 4] + base
            assert len(prompt) == n

            def prefill_alone():
                if arm == "pass":
                    sess.prefill(prompt[:-1])
                else:
                    for t, tok in enumerate(prompt[:-1]):
                        sess.step([tok] * W, [-1] * W if t == 0 else list(range(W)), list(range(W)), k=0)

            res = {}
            for name, fn in (("decode", lambda: sess.decode_timestamps(p1, tp, prompt=prompt)), ("prefill", prefill_alone)):
                fn(); sess.rewind()                                   # warm-up: captures, workspace growth
                wall = []
                for _ in range(repeats):
                    t0 = time.perf_counter()
                    r = fn()
                    wall.append(time.perf_counter() - t0)
                    if name == "decode":
                        res["generated"] = max(len(row) for row in r[0]) - n
                    sess.rewind()
                res[name + "_ms"] = statistics.median(wall) * 1e3
                res[name + "_spread_ms"] = (max(wall) - min(wall)) * 1e3
            out[f"W{W}_n{n}"] = res
            print(f"W{W} n{n}", json.dumps(res), flush=True)
        sess.close()
    eng.close()
    print("PREFILL_COST " + json.dumps(out))


if __name__ == "__main__":
    main()
