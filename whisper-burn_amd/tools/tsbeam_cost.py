"""Cost of beam search under the timestamp rules (LABLOG R18): tiny.en bench windows (3 windows, depth
100), one MI355X.  Wall time per decode step on replayed graphs for a beam-5 timestamp decode (15 rows at most), the beam.rs-mode
beam-5 decode under <|notimestamps|>, the greedy timestamp decode (3 rows) and the best-of-5 sampled timestamp decode (15 rows).
Run it plainly for the wall times and once under `rocprofv3 --kernel-trace --stats` for the per-launch times of
dec_tsbeam_rows_kernel / dec_tsbeam_update_kernel next to dec_ts_update_kernel / dec_beam_update_kernel.

    python whisper-burn_amd/tools/tsbeam_cost.py [repeats]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "whisper-burn_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import whisper_burn_amd as wb          # noqa: E402
from whisper_burn_amd import synth     # noqa: E402
from whisper_burn_amd.tokens import default_suppress   # noqa: E402


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    eng = wb.Whisper.from_tensors(synth.synth_preset("tiny.en"))
    st = wb.SpecialTokens.for_vocab(51864)
    audio = synth.synth_audio(480000, synth.BENCH_AUDIO_SEED)
    depth = 100
    p1, p5 = wb.decode_params(st, 1, depth), wb.decode_params(st, 5, depth)
    wlen = wb.max_waveform_samples(eng.max_mel_frames() - p1.padding)
    starts, lens = wb.window_extents(len(audio), 16000, wlen, p1.overlap_seconds)
    sup, sup1 = default_suppress(st)
    tpar = lambda T, bo: wb.TimestampParams(st.timestamp_begin, st.n_timestamps, temperature=T, best_of=bo, seed=7)
    out = {}
    for mb in (1, 5):
        sess = wb.Session.begin(eng, audio, starts, lens, max_beams=mb)
        sess.set_special_mask(st.is_special)
        sess.set_suppress(sup, sup1)

        def steps_ts_beam():
            return 2 + max(len(t) for t in sess.last_beam_trace(depth))

        def steps_samples():
            return 2 + max(len(g) for w in sess.last_samples(mb, depth) for g in w)

        runs = ({"ts_greedy": (lambda: sess.decode_timestamps(p1, tpar(0.0, 1)), steps_samples)} if mb == 1 else
                {"ts_beam5": (lambda: sess.decode_timestamps_beam(p1, tpar(0.0, 1), wb.BeamParams(5)), steps_ts_beam),
                 "beam_rs_beam5": (lambda: sess.decode(p5), None),
                 "ts_best_of_5_T1": (lambda: sess.decode_timestamps(p1, tpar(1.0, 5)), steps_samples)})
        for name, (fn, steps_of) in runs.items():
            fn(); sess.rewind()                                   # warm-up: captures
            wall, steps = [], 0
            for _ in range(repeats):
                t0 = time.perf_counter()
                rows = fn()
                wall.append(time.perf_counter() - t0)
                rows = rows[0] if isinstance(rows, tuple) else rows
                steps = steps_of() if steps_of else max(len(r) for r in rows) - 1
                sess.rewind()
            med = statistics.median(wall)
            out[name] = dict(windows=len(starts), max_rows=len(starts) * mb, steps=steps, wall_ms=med * 1e3, wall_us_per_step=med * 1e6 / steps)
            print(name, json.dumps(out[name]), flush=True)
        sess.close()
    eng.close()
    print("TSBEAM_COST " + json.dumps(out))


if __name__ == "__main__":
    main()
