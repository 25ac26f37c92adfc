"""Driven by tests/test_tsrules_emu.py in a subprocess with WHISPER_HIP_LIB = lib/libwhisper_hip_emu.so: tsrules.hip and its host
side executed through the hipemu functional model at micro shapes, compared with tests/tsrules_ref.py and the oracle.  A check
of the kernel sources' logic on a machine without a GPU; tests/test_gpu_tsrules_kernel.py / test_gpu_tsrules.py are the parity
tests proper."""
import sys

import numpy as np

import tsrules_ref as tr
import whisper_burn_amd as wb
from oracle.model import OracleWhisper
from whisper_burn_amd import _lib


def _micro():
    weights = tr.fixture()[0]
    return weights, wb.Whisper.from_tensors(weights)


def check_hook():
    rec = []
    for shape in tr.SHAPES[:2]:
        for case in tr.make_cases(shape):
            tr.check_hook_case(case, record=rec)
    for shape in tr.SHAPES[2:]:                 # the larger shapes: two cases each (more than one prefetch batch; the real vocabulary)
        for case in tr.make_cases(shape)[:2]:
            tr.check_hook_case(case, record=rec)
    print("hook (case, excluded, largest error / bound):", rec)
    for case in (tr.make_cases(tr.SHAPES[1])[1], tr.make_cases(tr.SHAPES[1])[2]):
        tr.check_hook_determinism(case)
    for shape in tr.SHAPES[:2]:
        tr.check_hook_no_admissible_id([c for c in tr.make_cases(shape) if c["kind"] == "one_text"][0])


def check_session(W, best_of):
    weights, eng = _micro()
    rec = []
    tr.check_session_shape(eng, OracleWhisper(weights), W, best_of, record=rec)
    print("session", W, best_of, rec)
    eng.close()


def check_rules_off():
    _, eng = _micro()
    tr.check_rules_off(eng)
    eng.close()


def check_segments():
    tr.check_segments_hook()
    eng = tr.short_context_engine()
    segs, seeks = tr.check_seek_loop(eng)
    print("seek loop: seeks", seeks, "segments", len(segs))
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

    V = tr.FIX_V
    sess = tr.fixture_session(eng, audio, 2, 3)
    _lib.profile_kernels(reset=True)
    p = wb.decode_params(st, 1, 6)
    ok = lambda **kw: wb.TimestampParams(**{**dict(timestamp_begin=R["tb"], n_timestamps=R["n_ts"]), **kw})
    assert status(lambda: sess.decode_timestamps(p, ok())) == -6                          # set_suppress not called
    sess.set_suppress(sup)
    for T in (-1.0, float("nan"), float("inf"), 1e-42):          # (1e-42: a subnormal, 1 / T is not finite)
        assert status(lambda: sess.decode_timestamps(p, ok(temperature=T, best_of=2))) == -1, T
    assert status(lambda: sess.decode_timestamps(p, ok(temperature=0.0, best_of=2))) == -1   # best_of > 1 needs a temperature
    assert status(lambda: sess.decode_timestamps(p, ok(temperature=1.0, best_of=0))) == -1   # best_of outside 1 .. max_beams
    assert status(lambda: sess.decode_timestamps(p, ok(temperature=1.0, best_of=4))) == -1
    assert status(lambda: sess.decode_timestamps(p, ok(attempt=-1))) == -1
    assert status(lambda: sess.decode_timestamps(p, ok(timestamp_begin=V - 10))) == -1       # the range leaves [0, V)
    assert status(lambda: sess.decode_timestamps(p, ok(timestamp_begin=-1))) == -1
    assert status(lambda: sess.decode_timestamps(p, ok(n_timestamps=-1))) == -1
    assert status(lambda: sess.decode_timestamps(p, ok(timestamp_begin=st.end_of_text - 3, n_timestamps=8))) == -1   # eot inside T
    assert status(lambda: sess.decode_timestamps(p, ok(max_initial_timestamp_index=-2))) == -1
    small = np.zeros((2, 8), dtype=np.int32)
    assert status(lambda: sess.decode_timestamps(p, ok(), out_tokens=small, out_lens=np.zeros(2, np.int32))) == -1
    assert status(lambda: sess.decode_timestamps(p, ok(), prompt=[V, 1])) == -1
    assert _lib.profile_kernels(reset=True) == [], "an error case launched a kernel"
    assert status(lambda: sess.decode_timestamps(p, ok())) == 0
    names = {k["name"].split(" ")[0] for k in _lib.profile_kernels(reset=True)}
    assert "dec_ts_update" in names and "dec_sample_update" not in names, names
    assert status(lambda: sess.decode_timestamps(p, ok())) == -6                          # not at step 0
    sess.rewind()
    assert status(lambda: sess.decode_timestamps(p, ok())) == 0
    sess.close()
    _lib.profile_kernels(reset=True)
    # the hook's own argument checks
    case = tr.make_cases(tr.SHAPES[0])[0]
    for key, val in (("T", -1.0), ("eot", case["V"]), ("eot", case["rules"]["tb"]), ("attempt", -1)):
        c = dict(case); c[key] = val
        assert status(lambda: tr.run_hook(c)) == -1, key
    c = dict(case); c["rules"] = dict(case["rules"], tb=case["V"] - 1, n_ts=5)
    assert status(lambda: tr.run_hook(c)) == -1
    # the segment slicer's and the seek loop's
    assert status(lambda: wb.segments_from_tokens([1, 2], wb.TimestampParams(100, 51), 99, -1)) == -1
    assert status(lambda: wb.waveform_to_segments(eng, st, audio, 16000, params=p, timestamps=ok(seconds_per_timestamp=0.0),
                                                  suppress=sup, prompt=prompt)) == -1
    assert status(lambda: wb.waveform_to_segments(eng, st, audio, 16000, params=p, timestamps=ok(temperature=-1.0), suppress=sup,
                                                  prompt=prompt)) == -1
    assert status(lambda: wb.waveform_to_segments(eng, st, audio, 16000, params=p, timestamps=ok(timestamp_begin=V - 10), suppress=sup,
                                                  prompt=prompt)) == -1
    assert status(lambda: wb.waveform_to_segments(eng, st, audio, 16000, params=p, timestamps=ok(temperature=0.0, best_of=2),
                                                  suppress=sup, prompt=prompt)) == -1
    assert _lib.profile_kernels(reset=True) == [], "an error case launched a kernel"
    lib.wb_profile_enable(0)
    eng.close()


if __name__ == "__main__":
    assert b"hipemu" in _lib.load().wb_version()
    which = sys.argv[1]
    if which.startswith("session"):
        _, W, bo = which.split("_")
        check_session(int(W), int(bo))
    else:
        {"hook": check_hook, "rules_off": check_rules_off, "segments": check_segments, "errors": check_errors}[which]()
    print("OK", which)
