"""Driven by tests/test_sample_emu.py in a subprocess with WHISPER_HIP_LIB = lib/libwhisper_hip_emu.so: sample.hip and its host
side executed through the hipemu functional model at micro shapes, compared with tests/sample_ref.py and the oracle.  A check
of the kernel sources' logic on a machine without a GPU; tests/test_gpu_sample_kernel.py / test_gpu_sample.py are the parity
tests proper."""
import sys

import numpy as np

import sample_ref as sr
import whisper_burn_amd as wb
from oracle.model import OracleWhisper
from whisper_burn_amd import _lib, synth

V = 1031


def _micro():
    dims = synth.micro_dims(n_state=64, n_head=1, n_layer=1, n_vocab=V)
    weights = synth.synth_weights(dims, seed=5)
    return weights, wb.Whisper.from_tensors(weights)


def check_hook():
    for shape in sr.SHAPES[:2]:
        for case in sr.make_cases(shape):
            sr.check_hook_case(case)
    for shape in sr.SHAPES[2:]:                 # the larger shapes: one case each (more than one prefetch batch; the real vocabulary)
        sr.check_hook_case(sr.make_cases(shape)[0])
    case = sr.make_cases(sr.SHAPES[1])[0]
    a, b = sr.run_hook(case), sr.run_hook(case)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))
    # the same rows reversed, and alone: the same tokens exactly
    rev = sr.run_hook(case, rows=np.arange(case["R"])[::-1])
    assert np.array_equal(rev[0][::-1], a[0]) and np.array_equal(rev[1][::-1].view(np.int32), a[1].view(np.int32))
    for r in range(case["R"]):
        one = sr.run_hook(case, rows=[r])
        assert one[0][0] == a[0][r] and one[1][0] == a[1][r]
    # a NaN logit: the row ends on eot with the error word raised, the others are as before
    bad = dict(case); bad["logits"] = case["logits"].copy(); bad["logits"][2, 17] = np.nan
    tok, lp, err = sr.run_hook(bad)
    assert err == 1 and tok[2] == case["eot"] and np.array_equal(np.delete(tok, 2), np.delete(a[0], 2))


def check_session(W, best_of):
    weights, eng = _micro()
    o32 = OracleWhisper(weights)
    st = wb.SpecialTokens.for_vocab(V)
    audio = synth.synth_audio(16000 * 3, 3)
    starts, lens = sr.windows(eng, audio, W)
    sess = wb.Session.begin(eng, audio, starts, lens, max_beams=max(best_of, 1))
    sess.set_special_mask(st.is_special)
    p = wb.decode_params(st, 1, 20)
    rec = []
    (T1, seed1, att1), (T2, seed2, att2) = sr.SESSION_DRAWS
    r1 = sr.check_sampled_session(sess, o32, st, p, T1, seed1, att1, best_of, record=rec)
    sr.check_sums_against_score(sess, st, p, best_of, r1[1])
    n_graphs, n_cap = sess.graph_count(), sess.graph_captures()
    assert n_graphs >= 1 and n_cap >= n_graphs
    sess.rewind()
    r2 = sr.check_sampled_session(sess, o32, st, p, T1, seed1, att1, best_of)       # again: bit-identical
    assert r1[0] == r2[0] and np.array_equal(r1[1], r2[1]) and np.array_equal(r1[2], r2[2])
    sess.rewind()
    sr.check_sampled_session(sess, o32, st, p, T2, seed2, att2, best_of, record=rec)   # another temperature, seed, attempt:
    assert sess.graph_count() == n_graphs and sess.graph_captures() == n_cap         # ... replays the captured graphs: no capture
    sess.rewind()
    r4 = sr.check_sampled_session(sess, o32, st, p, T1, seed1 + 1, att1, best_of)
    assert r4[0] != r1[0]                                                            # another seed: other rows
    # active windows: the others' output is untouched
    sess.rewind()
    act = np.ones(W, dtype=np.uint8); act[1] = 0
    ids = [7 * w + 100 for w in range(W)]
    sr.check_sampled_session(sess, o32, st, p, T1, seed1, att1, best_of, stream_ids=ids, active=act)
    print("session", W, best_of, rec)
    sess.close()
    eng.close()


def check_fallback():
    # (short windows, so that a few seconds of audio hold several of them)
    dims = synth.micro_dims(n_state=64, n_head=1, n_layer=1, n_vocab=V, n_audio_ctx=400)
    eng = wb.Whisper.from_tensors(synth.synth_weights(dims, seed=5))
    st = wb.SpecialTokens.for_vocab(V)
    audio = synth.synth_audio(16000 * 11, 3)
    p = wb.decode_params(st, 1, 6, overlap_seconds=1)
    wlen = wb.max_waveform_samples(eng.max_mel_frames() - p.padding)
    assert len(wb.window_extents(len(audio), 16000, wlen, p.overlap_seconds)[0]) >= 4
    sr.check_fallback_scenarios(eng, st, audio, p)
    eng.close()


def check_errors():
    weights, eng = _micro()
    st = wb.SpecialTokens.for_vocab(V)
    audio = synth.synth_audio(16000 * 3, 3)
    starts, lens = sr.windows(eng, audio, 2)
    lib = _lib.load()
    lib.wb_profile_enable(1)

    def status(fn):
        try:
            fn()
        except wb.WbError as e:
            return e.status
        return 0

    sess = wb.Session.begin(eng, audio, starts, lens, max_beams=3)
    _lib.profile_kernels(reset=True)
    p = wb.decode_params(st, 1, 6)
    assert status(lambda: sess.decode_sample(p, wb.SampleParams(1.0, 2, 0, 0))) == -6            # the mask is needed and not set
    sess.set_special_mask(st.is_special)
    for T in (0.0, -1.0, float("nan"), float("inf"), 1e-42):      # (1e-42: a subnormal, 1 / T is not finite)
        assert status(lambda: sess.decode_sample(p, wb.SampleParams(T, 2, 0, 0))) == -1, T
    assert status(lambda: sess.decode_sample(p, wb.SampleParams(1.0, 0, 0, 0))) == -1            # best_of outside 1 .. max_beams
    assert status(lambda: sess.decode_sample(p, wb.SampleParams(1.0, 4, 0, 0))) == -1
    assert status(lambda: sess.decode_sample(p, wb.SampleParams(1.0, 2, 0, -1))) == -1
    small = np.zeros((2, 9), dtype=np.int32)
    assert status(lambda: sess.decode_sample(p, wb.SampleParams(1.0, 2, 0, 0), out_tokens=small, out_lens=np.zeros(2, np.int32))) == -1
    assert status(lambda: sess.decode_sample(p, wb.SampleParams(1.0, 2, 0, 0), prompt=[V, 1])) == -1
    assert status(lambda: sess.last_samples(2, 6)) == -6                                         # no sampling call yet
    assert _lib.profile_kernels(reset=True) == [], "an error case launched a kernel"
    assert status(lambda: sess.decode_sample(p, wb.SampleParams(1.0, 2, 0, 0))) == 0
    names = {k["name"].split(" ")[0] for k in _lib.profile_kernels(reset=True)}
    assert "dec_sample_update" in names, names
    assert status(lambda: sess.decode_sample(p, wb.SampleParams(1.0, 2, 0, 0))) == -6            # not at step 0
    sess.rewind()
    assert status(lambda: sess.decode_sample(p, wb.SampleParams(1.0, 2, 0, 0))) == 0
    sess.close()
    _lib.profile_kernels(reset=True)
    # the hook's own argument checks
    case = sr.make_cases(sr.SHAPES[0])[0]
    for key, val in (("T", 0.0), ("eot", case["V"]), ("attempt", -1)):
        c = dict(case); c[key] = val
        assert status(lambda: sr.run_hook(c)) == -1, key
    # the fallback driver's
    for kw in (dict(temperatures=[0.2, 0.4]), dict(temperatures=[0.0, -0.5]), dict(best_of=0), dict(best_of=9), dict(tok_no_speech=V)):
        assert status(lambda: wb.waveform_to_tokens_fallback(eng, st, audio, 16000, 1, 6, fallback=wb.FallbackParams(**kw))) == -1, kw
    assert _lib.profile_kernels(reset=True) == [], "an error case launched a kernel"
    lib.wb_profile_enable(0)
    eng.close()


def check_decide():
    nan, inf = float("nan"), float("inf")
    lib = _lib.load()
    import ctypes as C
    import itertools
    n = 0
    for lp_t, ns_t, cr_t, nsp_tok in itertools.product((-1.0, nan), (0.6, nan), (2.4, nan), (-1, 7)):
        fp = wb.FallbackParams(None, None, None if lp_t != lp_t else lp_t, None if ns_t != ns_t else ns_t,
                               None if cr_t != cr_t else cr_t, 0, nsp_tok)
        d = dict(logprob_threshold=lp_t, no_speech_threshold=ns_t, compression_ratio_threshold=cr_t, tok_no_speech=nsp_tok)
        for avg, nsp, ratio in itertools.product((-2.0, -1.0, -0.5, nan, -inf), (0.1, 0.6, 0.9, nan), (1.0, 2.4, 3.0, nan)):
            f32 = lambda v: float(np.float32(v))
            want = sr.fallback_decide_ref({k: (f32(v) if isinstance(v, float) else v) for k, v in d.items()}, f32(avg), f32(nsp), f32(ratio))
            assert wb.fallback_decide(fp, avg, nsp, ratio) == want, (d, avg, nsp, ratio, want)
            n += 1
    # Whisper's defaults, case by case
    fp = wb.FallbackParams(tok_no_speech=7)
    assert wb.fallback_decide(fp, -0.5, 0.1, 1.5) == 0 and wb.fallback_decide(fp, -1.5, 0.1, 1.5) == 1
    assert wb.fallback_decide(fp, -0.5, 0.1, 2.5) == 1 and wb.fallback_decide(fp, -1.5, 0.9, 1.5) == 2
    assert wb.fallback_decide(fp, -0.5, 0.9, 1.5) == 0 and wb.fallback_decide(fp, -0.5, 0.9, 2.5) == 0
    assert wb.fallback_decide(fp, nan, 0.1, 1.5) == 1 and wb.fallback_decide(fp, -0.5, nan, 1.5) == 1
    assert n == 16 * 80 and lib.wb_fallback_decide(None, 0.0, 0.0, 0.0) == 0
    assert abs(wb.compression_ratio("ab" * 200) - 400 / len(__import__("zlib").compress(b"ab" * 200))) < 1e-12


if __name__ == "__main__":
    assert b"hipemu" in _lib.load().wb_version()
    which = sys.argv[1]
    if which.startswith("session"):
        _, W, bo = which.split("_")
        check_session(int(W), int(bo))
    else:
        {"hook": check_hook, "fallback": check_fallback, "errors": check_errors, "decide": check_decide}[which]()
    print("OK", which)
