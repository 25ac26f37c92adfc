"""Driven by tests/test_tsbeam_emu.py in a subprocess with WHISPER_HIP_LIB = lib/libwhisper_hip_emu.so: tsbeam.hip and its host side
executed through the hipemu functional model at micro shapes, compared with tests/tsbeam_ref.py and the oracle.  A check of the
kernel sources' logic on a machine without a GPU; tests/test_gpu_tsbeam_kernel.py / test_gpu_tsbeam.py are the parity tests
proper."""
import sys

import numpy as np

import tsbeam_ref as tb
import tsrules_ref as tr
import whisper_burn_amd as wb
from oracle.model import OracleWhisper
from whisper_burn_amd import _lib


def _micro():
    weights = tr.fixture()[0]
    return weights, wb.Whisper.from_tensors(weights)


def check_rows():
    rec = []
    for shape in tr.SHAPES[:2]:
        for case in tr.make_cases(shape):
            ref = tb.rows_reference(case)
            for k in tb.ROW_KS:
                tb.check_rows_case(case, k, record=rec, ref=ref)
    print("rows:", len(rec), "(case, k) pairs,", sum(r[2] for r in rec), "rows with fewer than k allowed ids")
    assert sum(r[2] for r in rec) > 0
    tb.check_rows_determinism(tr.make_cases(tr.SHAPES[1])[0])


def check_script():
    for c in tb.SCRIPT_CASES:
        ref = tb.check_script_case(*c)
        print("scripted", c, [len(r["trace"]) for r in ref], [len(r["cands"]) for r in ref])


def check_session(W, B, patience):
    weights, eng = _micro()
    rec = []
    tb.check_session_shape(eng, OracleWhisper(weights), W, B, patience, record=rec)
    print("session (B, patience, window-steps, excluded):", W, rec)
    eng.close()


def check_greedy_and_segments():
    _, eng = _micro()
    tb.check_beam1_is_greedy(eng)
    eng.close()
    eng = tr.short_context_engine()
    segs, seeks = tb.check_seek_loop_beam(eng)
    print("seek loop (beam 3): seeks", seeks, "segments", len(segs))
    eng.close()


def check_errors():
    weights, eng = _micro()
    _, st, audio, R, sup, prompt = tr.fixture()
    lib = _lib.load()
    lib.wb_profile_enable(1)

    def status(fn):
        try:
            fn()
        except wb.WbError as e:
            return e.status
        return 0

    sess = tr.fixture_session(eng, audio, 2, 3)
    _lib.profile_kernels(reset=True)
    p = wb.decode_params(st, 1, 6)
    tp = lambda **kw: wb.TimestampParams(**{**dict(timestamp_begin=R["tb"], n_timestamps=R["n_ts"]), **kw})
    run = lambda t=None, b=None, **kw: sess.decode_timestamps_beam(p, t or tp(), b or wb.BeamParams(3), **kw)
    assert status(run) == -6                                                             # set_suppress not called
    sess.set_suppress(sup)
    assert status(lambda: run(tp(temperature=0.5))) == -1                                # temperature other than 0
    assert status(lambda: run(tp(temperature=0.5, best_of=2))) == -1
    assert status(lambda: run(tp(best_of=2))) == -1                                      # best_of other than 1
    for B in (0, -1, 8, 4):                                                              # outside [1, 7]; above max_beams = 3
        assert status(lambda: run(b=wb.BeamParams(B))) == -1, B
    for pat in (0.5, float("nan"), float("inf"), 6.0):                                   # < 1, not finite, C = 18 > 16
        assert status(lambda: run(b=wb.BeamParams(3, pat))) == -1, pat
    for lp in (float("nan"), float("inf")):
        assert status(lambda: run(b=wb.BeamParams(3, 1.0, lp))) == -1, lp
    assert status(lambda: run(tp(timestamp_begin=tr.FIX_V - 10))) == -1                  # the timestamp checks of decode_timestamps
    small = np.zeros((2, 8), dtype=np.int32)
    assert status(lambda: run(out_tokens=small, out_lens=np.zeros(2, np.int32))) == -1
    assert status(lambda: run(prompt=[tr.FIX_V, 1])) == -1
    assert status(lambda: sess.last_beams(6)) == -6                                      # no beam search has run
    assert _lib.profile_kernels(reset=True) == [], "an error case launched a kernel"
    assert status(run) == 0
    names = {k["name"].split(" ")[0] for k in _lib.profile_kernels(reset=True)}
    assert {"dec_tsbeam_rows", "dec_tsbeam_update"} <= names and "dec_ts_update" not in names and "dec_beam_update" not in names, names
    assert status(run) == -6                                                             # not at step 0
    sess.rewind()
    assert status(lambda: run(b=wb.BeamParams(3, 5.0))) == 0                             # C = 15
    sess.close()
    _lib.profile_kernels(reset=True)
    case = tr.make_cases(tr.SHAPES[0])[0]
    Rl = case["rules"]
    h = np.array([tr.history(Rl, g) for g in case["gens"]], dtype=np.int32).reshape(case["R"], 4)
    ctp = wb.TimestampParams(Rl["tb"], Rl["n_ts"], Rl["max_init"], Rl["max_ts"])
    for k, eot in ((0, case["eot"]), (9, case["eot"]), (3, case["V"])):
        assert status(lambda: wb.timestamp_beam_rows(case["logits"], ctp, h[:, 0], h[:, 1], h[:, 2], h[:, 3], eot, k, V=case["V"])) == -1
    Rs, eot, ssup = tb.script_setup()
    fill = lambda *a: np.zeros((len(a[1]), tb.SCRIPT_V), dtype=np.float32)
    stp = wb.TimestampParams(Rs["tb"], Rs["n_ts"])
    for bp in (wb.BeamParams(8), wb.BeamParams(3, 0.5)):
        assert status(lambda: wb.timestamp_beam_search_device(fill, stp, bp, 2, tb.SCRIPT_V, eot, 4)) == -1
    assert status(lambda: wb.waveform_to_segments(eng, st, audio, 16000, params=p, timestamps=tp(), suppress=sup, prompt=prompt,
                                                  beam=wb.BeamParams(8))) == -1
    assert status(lambda: wb.waveform_to_segments(eng, st, audio, 16000, params=p, timestamps=tp(temperature=1.0), suppress=sup,
                                                  prompt=prompt, beam=wb.BeamParams(3))) == -1
    assert _lib.profile_kernels(reset=True) == [], "an error case launched a kernel"
    # a NaN row of the scripted hook fails the call
    nan_fill = lambda step, win, *_: np.full((len(win), tb.SCRIPT_V), np.nan, dtype=np.float32)
    assert status(lambda: wb.timestamp_beam_search_device(nan_fill, stp, wb.BeamParams(2), 2, tb.SCRIPT_V, eot, 4, suppress=ssup)) == -6
    lib.wb_profile_enable(0)
    eng.close()


if __name__ == "__main__":
    assert b"hipemu" in _lib.load().wb_version()
    which = sys.argv[1]
    if which.startswith("session"):
        _, W, B, pat = which.split("_")
        check_session(int(W), int(B), float(pat))
    else:
        {"rows": check_rows, "script": check_script, "greedy_segments": check_greedy_and_segments, "errors": check_errors}[which]()
    print("OK", which)
