"""Driven by tests/test_align_emu.py in a subprocess with WHISPER_HIP_LIB = lib/libwhisper_hip_emu.so: align.hip and its
host side executed through the hipemu functional model at micro shapes, compared with tests/align_ref.py.  A check of the
kernel sources' logic on a machine without a GPU; tests/test_gpu_align.py is the parity test proper."""
import sys

import numpy as np
import torch

import align_ref as ar
import whisper_burn_amd as wb
from whisper_burn_amd import _lib, synth


def _micro():
    dims = synth.micro_dims(n_state=128, n_head=2, n_layer=2, n_vocab=1031)
    weights = synth.synth_weights(dims, seed=77)
    return weights, wb.Whisper.from_tensors(weights)


def _enc(model32, C, seed):
    """An encoder output of C positions: the oracle's own, from a short synthetic mel (so that the values are realistic)."""
    g = np.random.default_rng(seed)
    mel = torch.from_numpy(g.standard_normal((1, 80, 2 * C)).astype(np.float32) * 0.5)
    return model32.forward_encoder(mel)[0].numpy()


def check_matrix_and_dtw():
    weights, eng = _micro()
    o32 = ar.AlignOracle(weights)
    o64 = ar.AlignOracle(weights, dtype=torch.float64)
    g = np.random.default_rng(5)
    # two rows of different len and C in ONE call of the session-free entry point needs equal C: rows of different C go
    # through separate calls here and through one session in the GPU test; different len in one call
    cases = [dict(C=48, lens=[12, 9], heads=None, fw=7, n_prefix=4, drop_last=1),
             dict(C=48, lens=[12, 9], heads=[(1, 1), (0, 0), (1, 0)], fw=3, n_prefix=2, drop_last=0),
             dict(C=37, lens=[7, 11], heads=[(0, 1)], fw=1, n_prefix=4, drop_last=1),
             dict(C=3, lens=[6, 6], heads=None, fw=7, n_prefix=1, drop_last=1)]       # C <= fw // 2: filter skipped
    for ci, c in enumerate(cases):
        C, lens = c["C"], c["lens"]
        L = max(lens)
        enc = np.stack([_enc(o32, C, 100 + ci * 10 + i) for i in range(len(lens))])
        toks = np.zeros((len(lens), L), dtype=np.int32)
        for i, n in enumerate(lens):
            toks[i, :n] = g.integers(0, 1031, n)
        pos, mat = eng.align_tokens(toks, enc, lens=lens, heads=c["heads"], n_prefix=c["n_prefix"],
                                    drop_last=c["drop_last"], filter_width=c["fw"], return_matrix=True)
        for i, n in enumerate(lens):
            m32 = ar.alignment_matrix(o32, toks[i, :n], enc[i], c["heads"], c["fw"]).numpy()
            m64 = ar.alignment_matrix(o64, toks[i, :n], enc[i], c["heads"], c["fw"]).numpy()
            d32 = float(np.abs(m32 - m64).max())
            err = float(np.abs(mat[i, :n] - m64).max())
            print(f"case {ci} row {i}: len {n} C {C} d32 {d32:.3e} err {err:.3e} ratio {err / d32:.2f}")
            assert err <= 4 * d32, (ci, i, err, d32)
            assert not mat[i, n:].any()
            ref = ar.start_positions(mat[i, :n], c["n_prefix"], c["drop_last"])
            assert np.array_equal(pos[i, :n], ref), (ci, i, pos[i, :n], ref)
            assert (pos[i, n:] == -1).all()
        # bit-identical on a second call
        pos2, mat2 = eng.align_tokens(toks, enc, lens=lens, heads=c["heads"], n_prefix=c["n_prefix"],
                                      drop_last=c["drop_last"], filter_width=c["fw"], return_matrix=True)
        assert np.array_equal(pos, pos2) and np.array_equal(mat.view(np.int32), mat2.view(np.int32))
    eng.close()


def check_dtw():
    g = np.random.default_rng(11)
    for (N, C) in [(1, 1), (1, 9), (7, 1), (5, 23), (12, 48), (20, 6), (70, 33)]:
        for kind in ("float", "ties"):
            x = g.standard_normal((N, C)).astype(np.float32) if kind == "float" else \
                g.integers(-2, 3, (N, C)).astype(np.float32)
            got = wb.dtw_start_positions(x)
            ref = ar.dtw_start_positions(x)
            assert np.array_equal(got, ref), (N, C, kind, got, ref)
    x = np.zeros((6, 10), dtype=np.float32)                  # every comparison a tie
    assert np.array_equal(wb.dtw_start_positions(x), ar.dtw_start_positions(x))


def check_errors():
    weights, eng = _micro()
    o32 = ar.AlignOracle(weights)
    enc = _enc(o32, 16, 1)[None]
    toks = np.arange(8, dtype=np.int32)[None]
    lib = _lib.load()
    lib.wb_profile_enable(1)
    _lib.profile_kernels(reset=True)

    def status(**kw):
        a = dict(lens=None, heads=None, n_prefix=4, drop_last=1, filter_width=7)
        a.update(kw)
        try:
            eng.align_tokens(kw.pop("tokens", toks), enc, **a)
        except wb.WbError as e:
            return e.status
        return 0

    assert status(heads=[(2, 0)]) == -1 and status(heads=[(0, 2)]) == -1 and status(heads=[(-1, 0)]) == -1
    assert status(heads=[(1, 0), (1, 0), (1, 1)]) == -1 and status(heads=[(0, 1), (1, 1), (0, 1)]) == -1   # listed twice
    assert status(filter_width=4) == -1 and status(filter_width=17) == -1 and status(filter_width=0) == -1
    assert status(n_prefix=7, drop_last=1) == -1 and status(n_prefix=8, drop_last=0) == -1
    long = np.zeros((1, 449), dtype=np.int32)
    try:
        eng.align_tokens(long, enc)
        raise AssertionError("len > n_text_ctx accepted")
    except wb.WbError as e:
        assert e.status == -2
    assert _lib.profile_kernels(reset=True) == [], "an error case launched a kernel"
    assert status() == 0
    names = {k["name"].split(" ")[0]: k["calls"] for k in _lib.profile_kernels(reset=True)}
    assert names == {"align_row_stats": 1, "align_accumulate": 1, "align_dtw": 1}, names   # default heads: layer 1 only
    lib.wb_profile_enable(0)
    eng.close()


def check_stitch_times():
    g = np.random.default_rng(3)
    for trial in range(200):
        W = int(g.integers(1, 5))
        stride = 24
        rows, times = [], []
        prev_tail = []
        for w in range(W):
            n = int(g.integers(1, 20))
            r = g.integers(0, 6, n).tolist()
            if prev_tail and g.random() < 0.7:                # an overlap with the previous window's tail
                k = int(g.integers(1, min(len(prev_tail), n) + 1))
                r[:k] = prev_tail[-k:]
            rows.append(r)
            times.append((g.random(n) * 100).astype(np.float32).tolist())
            prev_tail = r
        wt = np.zeros((W, stride), dtype=np.int32)
        tm = np.full((W, stride), np.nan, dtype=np.float32)
        for w in range(W):
            wt[w, :len(rows[w])] = rows[w]
            tm[w, :len(rows[w])] = times[w]
        lens = np.array([len(r) for r in rows], dtype=np.int32)
        toks, tt = wb.stitch_windows(wt, lens, times=tm)
        rt, rtt = ar.stitch_with_times(rows, times)
        assert toks == rt and np.array_equal(tt, np.asarray(rtt, dtype=np.float32)), trial
        assert toks == wb.stitch_windows(wt, lens)


def check_short_rows():
    """Rows as decoded that leave no DTW row (max_depth 0: the prompt alone) get NaN times; the transcription is the one
    wb_waveform_to_tokens returns.  The public alignment entries still refuse such a row."""
    weights, eng = _micro()
    st = wb.SpecialTokens.for_vocab(1031)
    audio = synth.synth_audio(16000 * 2, 3)
    for depth in (0, 1, 3):
        p = wb.decode_params(st, 1, depth)
        full, wins = wb.waveform_to_tokens(eng, st, audio, 16000, params=p)
        toks, times, wtoks, wtimes = wb.waveform_to_token_times(eng, st, audio, 16000, params=wb.decode_params(st, 1, depth))
        assert toks == full and wtoks == wins and len(times) == len(toks)
        for row, t in zip(wins, wtimes):
            n_dtw = len(row) - 4 - (row[-1] == st.end_of_text)
            assert len(row) == 4 + depth or row[-1] == st.end_of_text
            assert int((~np.isnan(t)).sum()) == max(n_dtw, 0) and np.isnan(t[:4]).all(), (depth, row, t)
    eng.close()


def check_harness():
    """The launchers on their own, through the kernel test harness: row statistics and the accumulated matrix against NumPy
    (f64) on random Q / K with padded leading dimensions, a head subset, rows of different len / C; the DTW launcher."""
    import ctypes as C
    import os
    kt = C.CDLL(os.environ["WHISPER_HIP_KTEST_LIB"])

    class Buf(C.Structure):
        _fields_ = [("host", C.c_void_p), ("bytes", C.c_int64), ("off", C.c_int64)]

    class Align(C.Structure):
        _fields_ = [(n, Buf) for n in ("Q", "K", "segs", "heads", "stats", "M")] + \
                   [(n, C.c_int64) for n in ("ldq", "ldkv", "n_q_rows", "n_kv_rows", "n_rows", "max_len", "n_heads",
                                             "n_model_heads", "ld_stats", "ld_row", "ldm", "filter_width", "first",
                                             "n_total", "stages")]

    class Dtw(C.Structure):
        _fields_ = [("X", Buf), ("out", Buf)] + [(n, C.c_int64) for n in ("N", "C", "ldx", "negate")]

    def buf(a):
        return Buf(a.ctypes.data, a.nbytes, 0)

    g = np.random.default_rng(21)
    H, ldq, ldkv = 3, 3 * 64 + 4, 2 * 3 * 64
    lens, Cs = [37, 5], [70, 9]
    L, maxC = max(lens), max(Cs)
    Q = g.standard_normal((len(lens) * L, ldq)).astype(np.float32) * 0.6
    K = g.standard_normal((sum(Cs), ldkv)).astype(np.float32) * 0.6
    segs = np.array([[0, lens[0], 0, Cs[0]], [L, lens[1], Cs[0], Cs[1]]], dtype=np.int32)
    heads = np.array([2, 0], dtype=np.int32)
    for fw in (1, 3, 7):
        stats = np.full((len(heads), len(lens), L, 2), np.nan, dtype=np.float32)
        M = np.full((len(lens), L, maxC), np.nan, dtype=np.float32)
        a = Align(buf(Q), buf(K), buf(segs), buf(heads), buf(stats), buf(M), ldq, ldkv, Q.shape[0], K.shape[0], len(lens), L,
                  len(heads), H, L, L, maxC, fw, 1, len(heads), 3)
        assert kt.wbk_align(C.byref(a)) == 0
        for r, (n, Cr) in enumerate(zip(lens, Cs)):
            acc = 0
            for hi, h in enumerate(heads):
                q = Q[segs[r, 0]:segs[r, 0] + n, h * 64:h * 64 + 64].astype(np.float64)
                k = K[segs[r, 2]:segs[r, 2] + Cr, h * 64:h * 64 + 64].astype(np.float64)
                s = q @ k.T
                mx = s.max(1)
                assert np.abs(stats[hi, r, :n, 0] - mx).max() < 1e-4
                sm = np.exp(s - mx[:, None]).sum(1)
                assert np.abs(stats[hi, r, :n, 1] / sm - 1).max() < 1e-5
                w = torch.from_numpy(np.exp(s - mx[:, None]) / sm[:, None])
                z = (w - w.mean(0, keepdim=True)) / torch.sqrt(((w - w.mean(0, keepdim=True)) ** 2).mean(0, keepdim=True))
                acc = acc + ar.median_filter(z, fw)
            ref = (acc / len(heads)).numpy()
            assert np.abs(M[r, :n, :Cr] - ref).max() < 2e-5, (fw, r, np.abs(M[r, :n, :Cr] - ref).max())
            assert np.isnan(M[r, n:]).all() and np.isnan(M[r, :, Cr:]).all()       # nothing written outside the row
    bad = Align(buf(Q), buf(K), buf(segs), buf(heads), buf(stats), buf(M), ldq, ldkv, Q.shape[0], K.shape[0], len(lens), L,
                len(heads), H, L, L, maxC, 4, 1, len(heads), 3)
    assert kt.wbk_align(C.byref(bad)) == -2                                        # even filter width: refused, no launch
    for (N, Cc) in [(1, 1), (9, 30), (30, 9)]:
        X = g.integers(-2, 3, (N, Cc + 3)).astype(np.float32)
        out = np.full(N, -7, dtype=np.int32)
        d = Dtw(buf(X), buf(out), N, Cc, Cc + 3, 1)
        assert kt.wbk_align_dtw(C.byref(d)) == 0
        assert np.array_equal(out, ar.dtw_start_positions(-X[:, :Cc]))


if __name__ == "__main__":
    assert b"hipemu" in _lib.load().wb_version()
    {"matrix": check_matrix_and_dtw, "dtw": check_dtw, "errors": check_errors, "stitch": check_stitch_times,
     "harness": check_harness, "short_rows": check_short_rows}[sys.argv[1]]()
    print("OK", sys.argv[1])
