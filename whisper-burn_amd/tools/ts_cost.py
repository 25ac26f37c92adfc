"""Cost of the timestamp-rules kernel next to the sampling kernel (LABLOG R16.1): tiny.en bench windows (3 windows, depth 100),
one MI355X.  Kernel time per launch from wb_profile_kernels (eager launches) at 3 and 15 rows for dec_ts_update_kernel and
dec_sample_update_kernel on the same session and rows; wall time per step on replayed graphs for a timestamp-greedy decode, a
sampled decode and the graph-chained greedy decode.  Run with WHISPER_HIP_PERSIST=0 (the chained greedy step is the comparison).

    WHISPER_HIP_PERSIST=0 python whisper-burn_amd/tools/ts_cost.py"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "whisper-burn_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import whisper_burn_amd as wb          # noqa: E402
from whisper_burn_amd import _lib, synth   # noqa: E402
from whisper_burn_amd.tokens import default_suppress   # noqa: E402


def main():
    weights = synth.synth_preset("tiny.en")
    eng = wb.Whisper.from_tensors(weights)
    st = wb.SpecialTokens.for_vocab(51864)
    audio = synth.synth_audio(480000, synth.BENCH_AUDIO_SEED)
    p = wb.decode_params(st, 1, 100)
    wlen = wb.max_waveform_samples(eng.max_mel_frames() - p.padding)
    starts, lens = wb.window_extents(len(audio), 16000, wlen, p.overlap_seconds)
    sup, sup1 = default_suppress(st)
    lib = _lib.load()
    out = {}
    for bo in (1, 5):
        sess = wb.Session.begin(eng, audio, starts, lens, max_beams=bo)
        sess.set_special_mask(st.is_special)
        sess.set_suppress(sup, sup1)
        R = len(starts) * bo
        tpar = lambda T: wb.TimestampParams(st.timestamp_begin, st.n_timestamps, temperature=T, best_of=bo, seed=7)
        runs = {"ts_greedy": (lambda: sess.decode_timestamps(p, tpar(0.0))) if bo == 1 else None,
                "ts_T1": lambda: sess.decode_timestamps(p, tpar(1.0)),
                "sample_T1": lambda: sess.decode_sample(p, wb.SampleParams(1.0, bo, 7, 0)),
                "greedy_chain": (lambda: sess.decode(p)) if bo == 1 else None}
        for name, fn in runs.items():
            if fn is None:
                continue
            fn(); sess.rewind()                                   # warm-up: captures
            wall, steps = [], 0
            for _ in range(5):
                t0 = time.perf_counter()
                rows = fn()
                wall.append(time.perf_counter() - t0)
                rows = rows[0] if isinstance(rows, tuple) else rows
                steps = max(len(r) for r in rows) - 1             # prefill steps + generated positions of the longest row
                if name != "greedy_chain":                        # ... of the longest SAMPLE: the call runs until every row has ended
                    n_prompt = 3 if name.startswith("ts") else 4
                    steps = n_prompt - 1 + max(len(g) for w in sess.last_samples(bo, p.max_depth) for g in w)
                sess.rewind()
            rec = dict(rows=R, steps=steps, wall_ms=statistics.median(wall) * 1e3, wall_us_per_step=statistics.median(wall) * 1e6 / steps)
            if name != "greedy_chain":
                lib.wb_profile_enable(1)
                _lib.profile_kernels(reset=True)
                fn(); sess.rewind()
                ks = _lib.profile_kernels(reset=True)
                lib.wb_profile_enable(0)
                for k in ks:
                    if k["name"].startswith(("dec_ts_update", "dec_sample_update")):
                        rec["kernel"] = k["name"].split(" ")[0]
                        rec["kernel_us_per_launch"] = k["total_ms"] * 1e3 / k["calls"]
                        rec["kernel_launches"] = k["calls"]
                rec["tagged_us_per_step"] = sum(k["total_ms"] for k in ks if not k["name"].startswith("dec_prepare")) * 1e3 / max(
                    rec.get("kernel_launches", 1), 1)
            out[f"{name}_{R}rows"] = rec
            print(name, R, json.dumps(rec), flush=True)
        sess.close()
    eng.close()
    print("TS_COST " + json.dumps(out))


if __name__ == "__main__":
    main()
