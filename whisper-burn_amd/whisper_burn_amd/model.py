"""Host-side mirror of the reference interface for the hot path, over the C ABI.

Same names, argument meaning and error behaviour as the reference seams
(/root/reference/src/audio.rs:34 prep_audio, src/model/mod.rs:47-71 Whisper::{forward,
forward_encoder, forward_decoder, encoder_ctx_size, decoder_ctx_size},
src/transcribe.rs:23-29 waveform_to_text), so the parity tests read like tests of the
reference would.  Shape-contract violations the reference `assert!`s on raise
`ShapeError` (a WbError with status WB_ERR_SHAPE).  All arithmetic happens in
libwhisper_hip.so; this file only marshals NumPy arrays.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import WbBeamParams, WbDecodeParams, WbDims, WbError, WbFallbackParams, WbSampleParams, WbTimestampParams, check
from .tokens import SpecialTokens

WB_F32, WB_BF16 = 0, 1
WB_ERR_ARG = -1
WB_ERR_SHAPE = -2


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


def _i32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.int32)


def _fp(a: np.ndarray):
    return a.ctypes.data_as(_lib.c_float_p)


def _ip(a: np.ndarray):
    return a.ctypes.data_as(_lib.c_int32_p)


def _heads_arg(heads):
    """(layer, head) pairs -> (int32 array or None, count) for the alignment entry points (None: the default set)."""
    if heads is None:
        return None, 0
    h = _i32(np.asarray(heads, dtype=np.int32).reshape(-1, 2))
    return h, len(h)


def _rows_arg(tokens, lens):
    """token rows (a 2-D array + lens, or a list of rows of different lengths) -> (int32 [n, L], int32 [n])."""
    if lens is None and not isinstance(tokens, np.ndarray):
        rows = [list(r) for r in tokens]
        lens = [len(r) for r in rows]
        L = max(lens)
        tokens = np.zeros((len(rows), L), dtype=np.int32)
        for i, r in enumerate(rows):
            tokens[i, :len(r)] = r
    tokens = _i32(tokens)
    lens = _i32(lens if lens is not None else [tokens.shape[1]] * tokens.shape[0])
    return tokens, lens


def dtw_start_positions(x, device: int = 0) -> np.ndarray:
    """DTW (device) over a cost matrix x [N, C] f32: the column of the first path cell of every row."""
    x = _f32(x)
    N, Cc = x.shape
    out = np.zeros(N, dtype=np.int32)
    check(_lib.load().wb_dtw_start_positions(device, _fp(x), N, Cc, _ip(out)))
    return out


def _u8p(a: Optional[np.ndarray]):
    return a.ctypes.data_as(_lib.c_uint8_p) if a is not None else None


def logprob_gather(h, E, target=None, mask=None, row_masked=None, probes=None, v_splits: int = 0, device: int = 0):
    """The fused scoring kernels alone (wb_logprob_gather, a test hook): h [R, d], E [V, d] -> (logprob [R], lse [R],
    probe_lp [n_probe]).  mask [V] of 0 / -inf applies to the rows with row_masked != 0; target[r] = -1: none;
    probes: (row, id) pairs, scored unmasked."""
    h, E = _f32(h), _f32(E)
    R, d = h.shape
    V = E.shape[0]
    assert E.shape[1] == d
    tg = _i32(target) if target is not None else None
    mk = _f32(mask) if mask is not None else None
    rm = np.ascontiguousarray(row_masked, dtype=np.uint8) if row_masked is not None else None
    pr = _i32(np.asarray(probes, dtype=np.int32).reshape(-1, 2)) if probes is not None and len(probes) else None
    n_probe = len(pr) if pr is not None else 0
    prow = _i32(pr[:, 0]) if pr is not None else None
    pid = _i32(pr[:, 1]) if pr is not None else None
    lp = np.full(R, np.nan, dtype=np.float32)
    lse = np.full(R, np.nan, dtype=np.float32)
    plp = np.full(max(n_probe, 1), np.nan, dtype=np.float32)
    check(_lib.load().wb_logprob_gather(device, _fp(h), R, d, _fp(E), V, _fp(mk) if mk is not None else None, _u8p(rm),
                                        _ip(tg) if tg is not None else None, _ip(prow) if pr is not None else None,
                                        _ip(pid) if pr is not None else None, n_probe, v_splits, _fp(lp), _fp(lse),
                                        _fp(plp)))
    return lp, lse, plp[:n_probe]


def sample_rows(logits, row_stats, temperature: float, seed: int, attempt, stream, position, eot: int, V: Optional[int] = None,
                mask=None, row_masked=None, device: int = 0):
    """The Gumbel-max draw alone (wb_sample_rows, a test hook): logits [R, ld] of which the first V columns are the row,
    row_stats [R, 2] = (row maximum, log-sum-exp) under the row's mask -> (token [R], logprob [R], error word)."""
    x = _f32(logits)
    R, ld = x.shape
    V = ld if V is None else V
    stt = _f32(row_stats)
    sid, pos = _i32(stream), _i32(position)
    assert stt.shape == (R, 2) and sid.shape == (R,) and pos.shape == (R,)
    mk = _f32(mask) if mask is not None else None
    rm = np.ascontiguousarray(row_masked, dtype=np.uint8) if row_masked is not None else None
    tok = np.full(R, -1, dtype=np.int32)
    lp = np.full(R, np.nan, dtype=np.float32)
    err = np.full(1, -1, dtype=np.int32)
    check(_lib.load().wb_sample_rows(device, _fp(x), R, ld, V, _fp(mk) if mk is not None else None, _u8p(rm), _fp(stt),
                                     float(temperature), int(seed), int(attempt), _ip(sid), _ip(pos), int(eot), _ip(tok),
                                     _fp(lp), _ip(err)))
    return tok, lp, int(err[0])


def SampleParams(temperature: float = 1.0, best_of: int = 5, seed: int = 0, attempt: int = 0) -> WbSampleParams:
    """wb_sample_params: one sampled decode at `temperature`, best of `best_of` per window."""
    p = WbSampleParams()
    _lib.load().wb_sample_params_default(C.byref(p))
    p.temperature, p.best_of, p.seed, p.attempt = temperature, best_of, seed, attempt
    return p


def TimestampParams(timestamp_begin: int = 0, n_timestamps: int = 0, max_initial_timestamp_index: int = 50,
                    max_timestamp_index: int = -1, seconds_per_timestamp: float = 0.02, temperature: float = 0.0,
                    best_of: int = 1, seed: int = 0, attempt: int = 0) -> WbTimestampParams:
    """wb_timestamp_params: the timestamp range [timestamp_begin, timestamp_begin + n_timestamps), the two index limits (-1:
    none) and the pick (temperature 0: greedy; > 0: the sampling draw, best of `best_of`)."""
    p = WbTimestampParams()
    _lib.load().wb_timestamp_params_default(C.byref(p))
    p.tok_timestamp_begin, p.n_timestamps = int(timestamp_begin), int(n_timestamps)
    p.max_initial_timestamp_index, p.max_timestamp_index = int(max_initial_timestamp_index), int(max_timestamp_index)
    p.seconds_per_timestamp, p.temperature, p.best_of, p.seed, p.attempt = seconds_per_timestamp, temperature, best_of, seed, attempt
    return p


def BeamParams(beam_size: int = 5, patience: float = 1.0, length_penalty: float = -1.0) -> WbBeamParams:
    """wb_beam_params: beam search under the timestamp rules -- beam_size live beams, a finished store of
    round(beam_size * patience) candidates, ranking by score / n_text (length_penalty < 0) or Google NMT's penalty."""
    p = WbBeamParams()
    _lib.load().wb_beam_params_default(C.byref(p))
    p.beam_size, p.patience, p.length_penalty = int(beam_size), patience, length_penalty
    return p


BEAM_STORE_CAP = 16     # most finalized candidates of a window (wb_session_last_beams)


def _beams_out(W: int, depth: int):
    cap, stride = BEAM_STORE_CAP, max(depth, 1)
    return (np.zeros((W, cap, stride), dtype=np.int32), np.zeros((W, cap), dtype=np.int32), np.zeros((W, cap), dtype=np.float64),
            np.zeros((W, cap), dtype=np.float64), np.zeros(W, dtype=np.int32))


def _beams_list(toks, lens, scores, ranks, n):
    return [None if n[w] < 0 else [dict(tokens=toks[w, i, :lens[w, i]].tolist(), score=float(scores[w, i]), rank=float(ranks[w, i]))
                                   for i in range(n[w])] for w in range(len(n))]


def _trace_out(W: int, depth: int):
    T = max(depth, 1)
    return (np.zeros(W, dtype=np.int32), np.zeros((T, W), dtype=np.int32), np.zeros((T, W), dtype=np.int32),
            np.zeros((T, W, 8), dtype=np.int32), np.zeros((T, W, 8), dtype=np.int32), np.zeros((T, W, 8), dtype=np.float64))


def _trace_list(n_steps, n_live, n_fin, toks, pars, scores):
    return [[dict(finished=int(n_fin[t, w]), beams=[(int(toks[t, w, q]), int(pars[t, w, q]), float(scores[t, w, q]))
                                                     for q in range(n_live[t, w])]) for t in range(n_steps[w])]
            for w in range(len(n_steps))]


def timestamp_beam_rows(logits, tp: WbTimestampParams, n_gen, prev1, prev2, last_ts, eot: int, k: int, V: Optional[int] = None,
                        suppress=None, suppress_first=None, device: int = 0):
    """The candidates of the beam search's rows kernel alone (wb_timestamp_beam_rows, a test hook): timestamp_rows' inputs at
    temperature 0 plus k.  Returns (ids [R, k], logprobs [R, k], count [R], forced [R], stats [R, 2], error word); entries
    past a row's count keep their fill (-1 / nan)."""
    x = _f32(logits)
    R, ld = x.shape
    V = ld if V is None else V
    cols = [_i32(c) for c in (n_gen, prev1, prev2, last_ts)]
    assert all(c.shape == (R,) for c in cols)
    sup, sup1 = _u8v(suppress, V), _u8v(suppress_first, V)
    kk = max(int(k), 1)
    ids = np.full((R, kk), -1, dtype=np.int32)
    lp = np.full((R, kk), np.nan, dtype=np.float32)
    count = np.full(R, -1, dtype=np.int32)
    forced = np.full(R, -1, dtype=np.int32)
    stats = np.full((R, 2), np.nan, dtype=np.float32)
    err = np.full(1, -1, dtype=np.int32)
    check(_lib.load().wb_timestamp_beam_rows(device, _fp(x), R, ld, V, _u8p(sup), _u8p(sup1), tp.tok_timestamp_begin, tp.n_timestamps,
                                             tp.max_initial_timestamp_index, tp.max_timestamp_index, *[_ip(c) for c in cols],
                                             int(eot), int(k), _ip(ids), _fp(lp), _ip(count), _ip(forced), _fp(stats), _ip(err)))
    return ids, lp, count, forced, stats, int(err[0])


def timestamp_beam_search_device(fill, tp: WbTimestampParams, bp: WbBeamParams, n_windows: int, V: int, eot: int, max_depth: int,
                                 suppress=None, suppress_first=None, device: int = 0):
    """Both kernels of the beam search under the timestamp rules without a model (wb_timestamp_beam_search_device, a test
    hook).  fill(step, window [n], beam [n], token [n], parent [n]) -> logits [n, V] of the live rows.  Returns (beams, best,
    trace) as Session.last_beams / the index of the returned candidate per window / Session.last_beam_trace."""
    W = int(n_windows)
    error = []

    def cb(_user, step, n, win, beam, tok, par, out):
        try:
            arr = lambda p: np.ctypeslib.as_array(p, shape=(n,)).copy()
            x = np.ascontiguousarray(fill(int(step), arr(win), arr(beam), arr(tok), arr(par)), dtype=np.float32)
            assert x.shape == (n, V), x.shape
            np.ctypeslib.as_array(out, shape=(n, V))[:] = x
            return 0
        except Exception as e:  # noqa: BLE001 - reported through the status
            error.append(e)
            return -1

    fn = _lib.TSBEAM_LOGITS_FN(cb)
    sup, sup1 = _u8v(suppress, V), _u8v(suppress_first, V)
    toks, lens, scores, ranks, n = _beams_out(W, max_depth)
    best = np.zeros(W, dtype=np.int32)
    tr = _trace_out(W, max_depth)
    try:
        check(_lib.load().wb_timestamp_beam_search_device(device, C.byref(tp), C.byref(bp), W, V, _u8p(sup), _u8p(sup1), int(eot),
                                                          int(max_depth), C.cast(fn, C.c_void_p), None, _ip(toks), toks.shape[2],
                                                          _ip(lens), scores.ctypes.data_as(_lib.c_double_p),
                                                          ranks.ctypes.data_as(_lib.c_double_p), _ip(n), _ip(best), _ip(tr[0]),
                                                          _ip(tr[1]), _ip(tr[2]), _ip(tr[3]), _ip(tr[4]),
                                                          tr[5].ctypes.data_as(_lib.c_double_p)))
    except WbError:
        if error:
            raise error[0]
        raise
    return _beams_list(toks, lens, scores, ranks, n), best.tolist(), _trace_list(*tr)


def _u8v(a, V: int) -> Optional[np.ndarray]:
    if a is None:
        return None
    a = np.ascontiguousarray(np.asarray(a) != 0, dtype=np.uint8)
    assert a.shape == (V,), (a.shape, V)
    return a


def timestamp_rows(logits, tp: WbTimestampParams, n_gen, prev1, prev2, last_ts, stream, position, eot: int,
                   V: Optional[int] = None, suppress=None, suppress_first=None, device: int = 0):
    """The timestamp rules + pick alone (wb_timestamp_rows, a test hook): logits [R, ld] of which the first V columns are the
    row; per row n_gen = len(gen), prev1 / prev2 = gen[-1] / gen[-2], last_ts = the last generated timestamp or -1.
    Returns (token [R], logprob [R], forced [R], stats [R, 2] = (ts_lse, mN), error word)."""
    x = _f32(logits)
    R, ld = x.shape
    V = ld if V is None else V
    cols = [_i32(c) for c in (n_gen, prev1, prev2, last_ts, stream, position)]
    assert all(c.shape == (R,) for c in cols)
    sup, sup1 = _u8v(suppress, V), _u8v(suppress_first, V)
    tok = np.full(R, -1, dtype=np.int32)
    lp = np.full(R, np.nan, dtype=np.float32)
    forced = np.full(R, -1, dtype=np.int32)
    stats = np.full((R, 2), np.nan, dtype=np.float32)
    err = np.full(1, -1, dtype=np.int32)
    check(_lib.load().wb_timestamp_rows(device, _fp(x), R, ld, V, _u8p(sup), _u8p(sup1), tp.tok_timestamp_begin, tp.n_timestamps,
                                        tp.max_initial_timestamp_index, tp.max_timestamp_index, float(tp.temperature),
                                        int(tp.seed), int(tp.attempt), *[_ip(c) for c in cols], int(eot), _ip(tok), _fp(lp),
                                        _ip(forced), _fp(stats), _ip(err)))
    return tok, lp, forced, stats, int(err[0])


def prefill_store(qkv, nA: int, n: int, d: int, S: int, Lmax: int, Kc, Vc, tabs, device: int = 0):
    """The store kernel of the one-pass prompt prefill alone (wb_prefill_store, a test hook): qkv [nA * n, ld]; Kc / Vc
    [Lmax * S, d] f32 and tabs [2, S, Lmax] i32 are updated in place."""
    q = _f32(qkv)
    assert q.ndim == 2 and q.shape[0] == nA * n
    for a, shape, dt in ((Kc, (Lmax * S, d), np.float32), (Vc, (Lmax * S, d), np.float32), (tabs, (2, S, Lmax), np.int32)):
        assert a.dtype == dt and a.flags.c_contiguous and a.shape == shape, (a.dtype, a.shape, shape)
    check(_lib.load().wb_prefill_store(device, _fp(q), nA, n, d, q.shape[1], S, Lmax, _fp(Kc), _fp(Vc), _ip(tabs)))


def segments_from_tokens(tokens, tp: WbTimestampParams, eot: int, window_index: int):
    """Whisper transcribe()'s slicing of one window's generated tokens (wb_segments_from_tokens, host only): a list of
    dict(begin, end, start, end_time) -- token index range and seconds relative to the window -- and the advance index."""
    t = _i32(list(tokens))
    cap = len(t) + 1
    sb, se = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int32)
    t0, t1 = np.zeros(cap, dtype=np.float32), np.zeros(cap, dtype=np.float32)
    k, adv = C.c_int32(0), C.c_int32(0)
    check(_lib.load().wb_segments_from_tokens(_ip(t) if len(t) else None, len(t), tp.tok_timestamp_begin, tp.n_timestamps, int(eot),
                                              int(window_index), float(tp.seconds_per_timestamp), _ip(sb), _ip(se), _fp(t0),
                                              _fp(t1), cap, C.byref(k), C.byref(adv)))
    return [dict(begin=int(sb[i]), end=int(se[i]), start=float(t0[i]), end_time=float(t1[i])) for i in range(k.value)], int(adv.value)


def waveform_to_segments(whisper: "Whisper", st: SpecialTokens, waveform, sample_rate: int = 16000, params=None,
                         timestamps: Optional[WbTimestampParams] = None, suppress=None, suppress_first=None, prompt=None,
                         beam: Optional[WbBeamParams] = None, condition_on_previous_text: bool = False, initial_prompt=None,
                         max_prompt_tokens: int = -1, return_windows: bool = False):
    """Long-form transcription by timestamps (wb_waveform_to_segments): the window moves by the last decoded timestamp.
    Returns (segments, tokens, n_windows): segments = dict(start, end, tokens) with absolute seconds and the segment's
    non-timestamp tokens; tokens = their concatenation.  beam: BeamParams -- every window by beam search under the rules
    (wb_waveform_to_segments_beam); None: greedy / best-of-n as `timestamps` says.
    condition_on_previous_text / initial_prompt (token ids) / max_prompt_tokens (-1: n_text_ctx / 2 - 1): every window's prompt
    carries [<|startofprev|>] + the tail of the text before it (wb_waveform_to_segments_conditioned states the rule); such
    prompts are prefilled by one pass.  return_windows: a fourth result dict(seek, prompt_len), one entry per window."""
    from .tokens import default_suppress
    wav = _f32(waveform).reshape(-1)
    p = params if params is not None else decode_params(st)
    tp = timestamps if timestamps is not None else TimestampParams(st.timestamp_begin, st.n_timestamps)
    V = whisper.dims["n_vocab"]
    if suppress is None:
        suppress, d1 = default_suppress(st)
        suppress_first = d1 if suppress_first is None else suppress_first
    sup, sup1 = _u8v(suppress, V), _u8v(suppress_first, V)
    pr = _i32([st.start_of_transcript, st.language, st.transcribe] if prompt is None else list(prompt))
    wlen = max_waveform_samples(whisper.max_mel_frames() - p.padding)
    # (capacity: a window advances by at least one timestamp unit -- or wholly -- and a tail below 400 samples is not decoded)
    spts = max(1, int(tp.seconds_per_timestamp * sample_rate))
    n_win_max = max(len(wav) // 400, len(wav) // spts) + 2
    seg_cap = n_win_max * (p.max_depth + 1)
    text_cap = n_win_max * max(p.max_depth, 1)
    t0, t1 = np.zeros(seg_cap, dtype=np.float32), np.zeros(seg_cap, dtype=np.float32)
    b, e = np.zeros(seg_cap, dtype=np.int32), np.zeros(seg_cap, dtype=np.int32)
    text = np.zeros(text_cap, dtype=np.int32)
    ns, nw, nt = C.c_int32(0), C.c_int32(0), C.c_int64(0)
    tail = (_u8p(sup), _u8p(sup1), _ip(pr), len(pr), _fp(t0), _fp(t1), _ip(b), _ip(e), seg_cap, C.byref(ns), _ip(text), text_cap,
            C.byref(nt), C.byref(nw))
    init = _i32([] if initial_prompt is None else list(initial_prompt))
    if condition_on_previous_text or len(init) or return_windows:
        win_seek, win_plen = np.zeros(n_win_max, dtype=np.int64), np.zeros(n_win_max, dtype=np.int32)
        # (return_windows alone: no history can form, <|startofprev|> is never used -- a tokenizer without one still gets its windows)
        sop = int(st.start_of_prev) if (condition_on_previous_text or len(init)) else max(int(st.start_of_prev), 0)
        check(_lib.load().wb_waveform_to_segments_conditioned(
            whisper._h, _fp(wav), len(wav), sample_rate, C.byref(p), C.byref(tp), C.byref(beam) if beam is not None else None,
            *tail[:4], sop, int(bool(condition_on_previous_text)), int(max_prompt_tokens),
            _ip(init) if len(init) else None, len(init), *tail[4:], win_seek.ctypes.data_as(_lib.c_int64_p), _ip(win_plen),
            n_win_max))
        toks = text[:nt.value].tolist()
        segs = [dict(start=float(t0[i]), end=float(t1[i]), tokens=toks[b[i]:e[i]]) for i in range(ns.value)]
        if not return_windows:
            return segs, toks, int(nw.value)
        return segs, toks, int(nw.value), dict(seek=win_seek[:nw.value].tolist(), prompt_len=win_plen[:nw.value].tolist())
    if beam is None:
        check(_lib.load().wb_waveform_to_segments(whisper._h, _fp(wav), len(wav), sample_rate, C.byref(p), C.byref(tp), *tail))
    else:
        check(_lib.load().wb_waveform_to_segments_beam(whisper._h, _fp(wav), len(wav), sample_rate, C.byref(p), C.byref(tp),
                                                       C.byref(beam), *tail))
    toks = text[:nt.value].tolist()
    segs = [dict(start=float(t0[i]), end=float(t1[i]), tokens=toks[b[i]:e[i]]) for i in range(ns.value)]
    return segs, toks, int(nw.value)


def FallbackParams(temperatures=None, best_of: Optional[int] = None, logprob_threshold: Optional[float] = -1.0,
                   no_speech_threshold: Optional[float] = 0.6, compression_ratio_threshold: Optional[float] = 2.4,
                   seed: int = 0, tok_no_speech: int = -1) -> WbFallbackParams:
    """wb_fallback_params with Whisper's defaults; None for a threshold switches its rule off."""
    p = WbFallbackParams()
    _lib.load().wb_fallback_params_default(C.byref(p))
    if temperatures is not None:
        ts = [float(t) for t in temperatures]
        if not 1 <= len(ts) <= 8:
            raise ValueError("fallback: 1 .. 8 temperatures")
        for i in range(8):
            p.temperatures[i] = ts[i] if i < len(ts) else 0.0
        p.n_temperatures = len(ts)
    if best_of is not None:
        p.best_of = best_of
    nan = float("nan")
    p.logprob_threshold = nan if logprob_threshold is None else logprob_threshold
    p.no_speech_threshold = nan if no_speech_threshold is None else no_speech_threshold
    p.compression_ratio_threshold = nan if compression_ratio_threshold is None else compression_ratio_threshold
    p.seed, p.tok_no_speech = seed, tok_no_speech
    return p


FALLBACK_ACCEPT, FALLBACK_RETRY, FALLBACK_NO_SPEECH = 0, 1, 2


def fallback_decide(params: WbFallbackParams, avg_logprob: float, no_speech_prob: float, ratio: float) -> int:
    """Whisper's accept (0) / retry (1) / no speech (2) decision for one window (wb_fallback_decide, host only)."""
    return int(_lib.load().wb_fallback_decide(C.byref(params), float(avg_logprob), float(no_speech_prob), float(ratio)))


def compression_ratio(text: str) -> float:
    """Whisper's compression ratio: len(utf8) / len(zlib.compress(utf8))."""
    import zlib
    b = text.encode("utf-8")
    return len(b) / len(zlib.compress(b))


def ratio_from_tokenizer(bpe):
    """The `ratio` callback of waveform_to_tokens_fallback from a tokenizer adapter (`decode(tokens, skip_special) -> str`)."""
    def ratio(tokens: List[int]) -> float:
        return compression_ratio(bpe.decode(list(tokens), True))
    return ratio


def waveform_to_tokens_fallback(whisper: "Whisper", st: SpecialTokens, waveform, sample_rate: int = 16000,
                                beam_size: int = 5, max_depth: int = 100, win_begin: int = 0, win_end: int = -1,
                                params: Optional[WbDecodeParams] = None, fallback: Optional[WbFallbackParams] = None,
                                ratio=None):
    """waveform_to_tokens with Whisper's decode fallback (wb_waveform_to_tokens_fallback): a window whose decode fails
    the thresholds is decoded again by sampling at the next temperature, on the same session; silent windows are left out
    of the stitched stream.  ratio: callable(list of generated token ids) -> compression ratio, or None (rule off).

    Returns a dict: tokens (stitched), win_tokens, and per local window temperature, status (0 accepted, 1 failed every
    temperature, 2 no speech), avg_logprob, no_speech_prob, ratio, attempts."""
    lib = _lib.load()
    wav = _f32(waveform).reshape(-1)
    p = params or decode_params(st, beam_size, max_depth)
    fp = fallback or FallbackParams(tok_no_speech=st.no_speech)
    wlen = max_waveform_samples(whisper.max_mel_frames() - p.padding)
    starts, _ = window_extents(len(wav), sample_rate, wlen, p.overlap_seconds)
    if win_end < 0:
        win_end = len(starts)
    n_local = max(0, win_end - win_begin)
    nw = max(n_local, 1)
    stride = 4 + p.max_depth + 4
    win_tokens = np.zeros((nw, stride), dtype=np.int32)
    win_lens = np.zeros(nw, dtype=np.int32)
    cap = nw * stride
    stitched = np.zeros(cap, dtype=np.int32)
    n_st = C.c_int64(0)
    temp = np.full(nw, np.nan, dtype=np.float32)
    status = np.full(nw, -1, dtype=np.int32)
    avg = np.full(nw, np.nan, dtype=np.float32)
    nsp = np.full(nw, np.nan, dtype=np.float32)
    rat = np.full(nw, np.nan, dtype=np.float32)
    att = np.zeros(nw, dtype=np.int32)
    mask = special_mask_bytes(whisper, st.is_special)
    failure = []

    def _ratio(_user, toks, n):
        try:
            return float(ratio([int(toks[i]) for i in range(n)]))
        except Exception as e:  # nothing unwinds across the C boundary
            failure.append(e)
            return float("nan")
    cb = _lib.RATIO_FN(_ratio) if ratio is not None else None
    check(lib.wb_waveform_to_tokens_fallback(whisper._h, _fp(wav), len(wav), sample_rate, C.byref(p),
                                             mask.ctypes.data_as(_lib.c_uint8_p), win_begin, win_end, _ip(win_tokens), stride,
                                             _ip(win_lens), _ip(stitched), cap, C.byref(n_st), C.byref(fp),
                                             C.cast(cb, C.c_void_p) if cb is not None else None, None, _fp(temp),
                                             _ip(status), _fp(avg), _fp(nsp), _fp(rat), _ip(att)))
    if failure:
        raise failure[0]
    n = n_local
    return dict(tokens=stitched[:n_st.value].tolist(), win_tokens=[win_tokens[i, :win_lens[i]].tolist() for i in range(n)],
                temperature=temp[:n].copy(), status=status[:n].copy(), avg_logprob=avg[:n].copy(),
                no_speech_prob=nsp[:n].copy(), ratio=rat[:n].copy(), attempts=att[:n].copy())


def special_mask_bytes(whisper: "Whisper", is_special) -> np.ndarray:
    """uint8 [n_vocab] for the C side, which reads exactly n_vocab bytes.  The reference adds a [vocab_size] mask to
    [.., n_vocab] logits (transcribe.rs:243-275) and panics when the tokenizer's vocabulary and the model's differ; a
    shorter buffer here would be an out-of-bounds host read."""
    m = np.ascontiguousarray(is_special, dtype=np.uint8).reshape(-1)
    if m.shape[0] != whisper.dims["n_vocab"]:
        raise WbError(WB_ERR_SHAPE, f"special-token mask has {m.shape[0]} entries but the model's vocabulary has "
                                    f"{whisper.dims['n_vocab']} (tokenizer / checkpoint mismatch)")
    return m


def max_waveform_samples(n_frame_max: int) -> int:
    """audio.rs:12-17."""
    return int(_lib.load().wb_max_waveform_samples(int(n_frame_max)))


FRONTENDS = {"fft": 0, "reference": 1}


def frontend_id(frontend: str) -> int:
    """"fft" (K1, the default) -> 0, "reference" (the reference's dense f32 DFT recipe) -> 1."""
    if frontend not in FRONTENDS:
        raise ValueError(f"frontend {frontend!r}: one of {sorted(FRONTENDS)}")
    return FRONTENDS[frontend]


def mel_dft_table() -> np.ndarray:
    """The [402, 400] DFT operand of the reference-recipe frontend (host only, no GPU): row 2k = cos(b[k]) * w,
    row 2k+1 = sin(b[k]) * (-w), audio.rs:348-364."""
    t = np.empty((402, 400), dtype=np.float32)
    check(_lib.load().wb_mel_dft_table(_fp(t)))
    return t


def mel_filterbank(sample_rate: float = 16000.0, n_mels: int = 80) -> np.ndarray:
    """The dense [n_mels, 201] filterbank the frontend kernels use (host only, no GPU; wb_mel_filterbank): 80 rows in the
    reference's f32 op order, 128 rows (large-v3 and later) designed in f64 and rounded once."""
    f = np.empty((max(int(n_mels), 1), 201), dtype=np.float32)
    check(_lib.load().wb_mel_filterbank(float(sample_rate), int(n_mels), _fp(f)))
    return f


def prep_audio(waveform, sample_rate: float = 16000.0, device: int = 0, frontend: str = "fft",
               n_mels: int = 80) -> np.ndarray:
    """audio.rs:34: waveform [n_batch, n_samples] -> log-mel [n_batch, n_mels, n_samples // 160].
    frontend="reference" computes the reference's own recipe (dense f32 DFT, wb_prep_audio_frontend); it has 80 rows only.
    n_mels=128 is the frontend of large-v3 and later (wb_prep_audio_mels)."""
    lib = _lib.load()
    fid = frontend_id(frontend)
    if n_mels != 80 and fid != 0:
        raise WbError(WB_ERR_ARG, "the reference recipe has 80 mel rows only")
    w = _f32(waveform)
    if w.ndim == 1:
        w = w[None]
    out = []
    for row in w:
        n = row.shape[0]
        mel = np.empty((max(int(n_mels), 1), max(n // 160, 0)), dtype=np.float32)
        nf = C.c_int64(0)
        if n_mels == 80:
            check(lib.wb_prep_audio_frontend(device, _fp(row), n, float(sample_rate), _fp(mel), C.byref(nf), fid))
        else:
            check(lib.wb_prep_audio_mels(device, _fp(row), n, float(sample_rate), int(n_mels), _fp(mel), C.byref(nf)))
        out.append(mel)
    return np.stack(out)


def burn_record_tensors(mpk_gz_path: str, cfg_path: Optional[str] = None) -> Dict[str, np.ndarray]:
    """The tensors of a converted model file under their dump-directory names (host only, no GPU)."""
    out: Dict[str, np.ndarray] = {}

    def cb(_user, name, data, shape, rank):
        shp = tuple(int(shape[i]) for i in range(rank))
        n = int(np.prod(shp)) if shp else 1
        out[name.decode()] = np.ctypeslib.as_array(data, shape=(n,)).copy().reshape(shp)
        return 0

    fn = _lib.TENSOR_FN(cb)
    check(_lib.load().wb_burn_record_read(mpk_gz_path.encode(), cfg_path.encode() if cfg_path else None, fn, None))
    return out


def load_audio_waveform(path: str, any_rate: bool = False):
    """bin/transcribe/main.rs:31-55: (f32 samples, sample_rate); 16 kHz mono only, like the reference, unless
    `any_rate` (then the caller resamples: `resample`)."""
    lib = _lib.load()
    n, sr = C.c_int64(0), C.c_int32(0)
    check(lib.wb_wav_info(path.encode(), C.byref(n), C.byref(sr), None, None, None))
    out = np.empty(int(n.value), dtype=np.float32)
    got = C.c_int64(0)
    read = lib.wb_wav_read_f32_any_rate if any_rate else lib.wb_wav_read_f32
    check(read(path.encode(), _fp(out), int(n.value), C.byref(got)))
    return out[:int(got.value)], int(sr.value)


def resample_filter(rate_in: int, rate_out: int = 16000):
    """(taps f32 [20*max(up,down)+1], up, down) of the device resampler (host only)."""
    lib = _lib.load()
    n, up, down = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    check(lib.wb_resample_filter(rate_in, rate_out, None, 0, C.byref(n), C.byref(up), C.byref(down)))
    taps = np.empty(int(n.value), dtype=np.float32)
    check(lib.wb_resample_filter(rate_in, rate_out, _fp(taps), int(n.value), None, None, None))
    return taps, int(up.value), int(down.value)


def resample(pcm, rate_in: int, rate_out: int = 16000, device: int = 0) -> np.ndarray:
    """Polyphase resampling on the GPU (wb_resample_dev): f32 [n] -> f32 [ceil(n*rate_out/rate_in)]."""
    import torch
    lib = _lib.load()
    x = torch.as_tensor(np.ascontiguousarray(pcm, dtype=np.float32)).to(f"cuda:{device}")
    n_out = int(lib.wb_resample_len(x.numel(), rate_in, rate_out))
    if n_out < 0:
        raise ValueError(f"unsupported sample-rate pair {rate_in} -> {rate_out}")
    y = torch.empty(max(n_out, 1), dtype=torch.float32, device=x.device)
    torch.cuda.synchronize(x.device)
    got = C.c_int64(0)
    check(lib.wb_resample_dev(device, C.c_void_p(x.data_ptr()), x.numel(), rate_in, rate_out, C.c_void_p(y.data_ptr()),
                              y.numel(), C.byref(got)))
    return y[:int(got.value)].cpu().numpy()


def wav_info(path: str) -> dict:
    lib = _lib.load()
    n, sr, ch, bits, fl = C.c_int64(0), C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
    check(lib.wb_wav_info(path.encode(), C.byref(n), C.byref(sr), C.byref(ch), C.byref(bits), C.byref(fl)))
    return dict(n_samples=int(n.value), sample_rate=int(sr.value), channels=int(ch.value), bits=int(bits.value),
                is_float=bool(fl.value))


def pcm_s16_to_f32_dev(src_ptr: int, n: int, dst_ptr: int, device: int = 0) -> None:
    """main.rs:45-52 on the device: dst[i] = src[i] / 32767."""
    check(_lib.load().wb_pcm_s16_to_f32_dev(device, C.c_void_p(src_ptr), n, C.c_void_p(dst_ptr)))


def waveform_to_mels_dev(pcm_ptr: int, n_samples: int, starts, lens, mel_ptr: int, win_stride: int, row_stride: int,
                         sample_rate: float = 16000.0, clip_frames: int = 1490, padding: int = 10, device: int = 0,
                         iters: int = 1, frontend: str = "fft", n_mels: int = 80):
    """transcribe.rs:114-138 + :171-177 for a batch of windows, device pointers in and out; window w is written as
    [n_mels, row_stride].  Returns (frames per window, HIP-event milliseconds of all `iters` passes).  frontend, n_mels:
    as `prep_audio`."""
    fid = frontend_id(frontend)
    lib = _lib.load()
    st = np.ascontiguousarray(starts, dtype=np.int64)
    ln = np.ascontiguousarray(lens, dtype=np.int64)
    frames = np.zeros(len(st), dtype=np.int32)
    ms = C.c_double(0.0)
    if n_mels != 80:
        check(lib.wb_waveform_to_mels_dev_mels(device, C.c_void_p(pcm_ptr), n_samples, float(sample_rate),
                                               st.ctypes.data_as(_lib.c_int64_p), ln.ctypes.data_as(_lib.c_int64_p),
                                               len(st), clip_frames, padding, C.c_void_p(mel_ptr), win_stride,
                                               row_stride, frames.ctypes.data_as(_lib.c_int32_p), iters, C.byref(ms),
                                               int(n_mels), fid))
        return frames, float(ms.value)
    check(lib.wb_waveform_to_mels_dev_frontend(device, C.c_void_p(pcm_ptr), n_samples, float(sample_rate),
                                               st.ctypes.data_as(_lib.c_int64_p), ln.ctypes.data_as(_lib.c_int64_p),
                                               len(st), clip_frames, padding, C.c_void_p(mel_ptr), win_stride,
                                               row_stride, frames.ctypes.data_as(_lib.c_int32_p), iters, C.byref(ms),
                                               fid))
    return frames, float(ms.value)


class Whisper:
    """mod.rs:41-71 `Whisper<B>` on one MI355X."""

    def __init__(self, handle, device: int):
        self._h = handle
        self.device = device
        d = WbDims()
        check(_lib.load().wb_model_dims(self._h, C.byref(d)))
        self.dims = {k: int(getattr(d, k)) for k, _ in WbDims._fields_}

    # -- construction -----------------------------------------------------------------
    @staticmethod
    def load_dump_dir(path: str, device: int = 0, compute_dtype: int = WB_F32) -> "Whisper":
        """load_whisper(path), load.rs:295-310."""
        h = C.c_void_p()
        check(_lib.load().wb_model_load_dump_dir(path.encode(), device, compute_dtype, C.byref(h)))
        return Whisper(h, device)

    @staticmethod
    def load_burn_record(mpk_gz_path: str, cfg_path: Optional[str] = None, device: int = 0,
                         compute_dtype: int = WB_F32) -> "Whisper":
        """load_whisper_model_file, bin/transcribe/main.rs:63-70 (+ the .cfg of :116-123)."""
        h = C.c_void_p()
        check(_lib.load().wb_model_load_burn_record(mpk_gz_path.encode(), cfg_path.encode() if cfg_path else None,
                                                    device, compute_dtype, C.byref(h)))
        return Whisper(h, device)

    @staticmethod
    def from_tensors(weights: Dict[str, np.ndarray], device: int = 0, compute_dtype: int = WB_F32) -> "Whisper":
        names = list(weights)
        arrs = [_f32(weights[k]) for k in names]
        n = len(names)
        c_names = (C.c_char_p * n)(*[k.encode() for k in names])
        c_data = (_lib.c_float_p * n)(*[_fp(a) for a in arrs])
        shp = [np.asarray(a.shape if a.ndim else (1,), dtype=np.int64) for a in arrs]
        c_shapes = (_lib.c_int64_p * n)(*[s.ctypes.data_as(_lib.c_int64_p) for s in shp])
        c_ranks = (C.c_int32 * n)(*[len(s) for s in shp])
        h = C.c_void_p()
        check(_lib.load().wb_model_load_tensors(c_names, c_data, c_shapes, c_ranks, n, device, compute_dtype,
                                                C.byref(h)))
        return Whisper(h, device)

    def close(self):
        if self._h:
            _lib.load().wb_model_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_layernorm_variant(self, eps_inside_sqrt: bool):
        check(_lib.load().wb_model_set_ln_variant(self._h, int(eps_inside_sqrt)))

    def set_frame_limit(self, whisper_geometry: bool):
        """False (default): a window holds at most n_audio_ctx MEL FRAMES, as the reference asserts (mod.rs:236-241).
        True: at most n_audio_ctx encoder positions = 2 n_audio_ctx frames -- Whisper's own 30 s window (the "perf
        geometry" T = 3000, C = 1500 of SURVEY 8d config 2b); the reference panics on such a window."""
        check(_lib.load().wb_model_set_frame_limit(self._h, int(bool(whisper_geometry))))
        self._frame_limit_x2 = bool(whisper_geometry)

    def set_frontend(self, name: str):
        """Log-mel frontend of every PCM entry point of this model (wb_model_set_frontend): "fft" (K1, default) or
        "reference" (the reference's own recipe, audio.rs:284-367: dense f32 DFT against its f32 angle table)."""
        check(_lib.load().wb_model_set_frontend(self._h, frontend_id(name)))

    @property
    def frontend(self) -> str:
        """The current log-mel frontend: "fft" or "reference"."""
        v = _lib.load().wb_model_frontend(self._h)
        if v < 0:
            check(v)
        return ("fft", "reference")[v]

    def encoder_gemm(self) -> str:
        """Arithmetic of the encoder-side Linear layers: "f32" (exact-f32 MFMA), "f16x3" (split precision: three fp16 MFMAs
        per product, f32-grade; the default)."""
        return ("f32", "f16x3")[_lib.load().wb_model_encoder_gemm(self._h)]

    def decoder_gemm(self) -> str:
        """Arithmetic of the decoder's Linear layers in batch mode: "f16x3" (split precision on fp16 weight tiles; default)
        or "f32" (exact-f32 MFMA; also after a decoder range guard has tripped -- wb_model_decoder_gemm)."""
        return ("f32", "f16x3")[_lib.load().wb_model_decoder_gemm(self._h)]

    def max_mel_frames(self) -> int:
        """Mel frames one window may hold (what transcribe.rs:32 calls n_ctx_max_encoder)."""
        return self.dims["n_audio_ctx"] * (2 if getattr(self, "_frame_limit_x2", False) else 1)

    # -- mod.rs:47-71 -------------------------------------------------------------------
    def encoder_ctx_size(self) -> int:
        return self.dims["n_audio_ctx"]

    def decoder_ctx_size(self) -> int:
        return self.dims["n_text_ctx"]

    def forward_encoder(self, mel) -> np.ndarray:
        """[B, 80, T] -> [B, C, d]."""
        mel = _f32(mel)
        B, n_mels, T = mel.shape
        if n_mels != self.dims["n_mels"]:     # mod.rs:231-235
            raise WbError(WB_ERR_SHAPE, f"Audio mel spectrum size must be {self.dims['n_mels']}.")
        out = np.empty((B, (T - 1) // 2 + 1 if T > 0 else 0, self.dims["n_audio_state"]), dtype=np.float32)
        check(_lib.load().wb_forward_encoder(self._h, _fp(mel), B, T, _fp(out)))
        return out

    def forward_decoder(self, tokens, encoder_output) -> np.ndarray:
        """tokens [n, L] int, encoder_output [n, C, d] -> logits [n, L, V]."""
        tokens = _i32(tokens)
        enc = _f32(encoder_output)
        n, L = tokens.shape
        assert enc.shape[0] == n and enc.shape[2] == self.dims["n_text_state"]
        logits = np.empty((n, L, self.dims["n_vocab"]), dtype=np.float32)
        check(_lib.load().wb_forward_decoder(self._h, _ip(tokens), n, L, _fp(enc), enc.shape[1], _fp(logits)))
        return logits

    def align_tokens(self, tokens, encoder_output, lens=None, heads=None, n_prefix: int = 4, drop_last: int = 1,
                     filter_width: int = 7, return_matrix: bool = False):
        """Token start positions from the cross-attention weights (wb_align_tokens): tokens [n, L] (+ lens) or a list
        of rows, encoder_output [n, C, d] -> start_pos [n, L] (-1 where a token is not aligned) and, on request, the
        token x position matrix [n, L, C].  heads: (layer, head) pairs; None = the upper half of the decoder."""
        tokens, lens = _rows_arg(tokens, lens)
        enc = _f32(encoder_output)
        n, L = tokens.shape
        assert enc.shape[0] == n and enc.shape[2] == self.dims["n_text_state"]
        h, nh = _heads_arg(heads)
        pos = np.full((n, L), -1, dtype=np.int32)
        mat = np.zeros((n, L, enc.shape[1]), dtype=np.float32) if return_matrix else None
        check(_lib.load().wb_align_tokens(self._h, _ip(tokens), n, L, _ip(lens), _fp(enc), enc.shape[1],
                                          _ip(h) if h is not None else None, nh, n_prefix, drop_last, filter_width,
                                          _ip(pos), _fp(mat) if mat is not None else None))
        return (pos, mat) if return_matrix else pos

    def score_tokens(self, tokens, encoder_output, lens=None, is_special=None, mask_until_len: int = 0,
                     probe_ids=None, probe_pos: int = 0):
        """Per-token log-probabilities of finished rows (wb_score_tokens): tokens [n, L] (+ lens) or a list of rows,
        encoder_output [n, C, d] -> token_logprobs [n, L]: entry l = log-prob of tokens[l] given tokens[:l] (NaN at entry
        0 and past a row's len), under the special mask `is_special` while l <= mask_until_len.  With probe_ids also
        returns probe_logprobs [n, n_probe]: the unmasked log-probs of those ids at position probe_pos."""
        tokens, lens = _rows_arg(tokens, lens)
        enc = _f32(encoder_output)
        n, L = tokens.shape
        assert enc.shape[0] == n and enc.shape[2] == self.dims["n_text_state"]
        mk = special_mask_bytes(self, is_special) if is_special is not None else None
        pid = _i32(probe_ids) if probe_ids is not None else None
        npb = len(pid) if pid is not None else 0
        lp = np.full((n, L), np.nan, dtype=np.float32)
        plp = np.full((n, max(npb, 1)), np.nan, dtype=np.float32)
        check(_lib.load().wb_score_tokens(self._h, _ip(tokens), n, L, _ip(lens), _fp(enc), enc.shape[1], _u8p(mk),
                                          mask_until_len, _ip(pid) if pid is not None else None, npb, probe_pos,
                                          _fp(lp), _fp(plp) if npb else None))
        return (lp, plp[:, :npb]) if pid is not None else lp

    def forward(self, mel, tokens) -> np.ndarray:
        mel = _f32(mel)
        tokens = _i32(tokens)
        B, _, T = mel.shape
        logits = np.empty((B, tokens.shape[1], self.dims["n_vocab"]), dtype=np.float32)
        check(_lib.load().wb_forward(self._h, _fp(mel), B, T, _ip(tokens), tokens.shape[1], _fp(logits)))
        return logits


def decode_params(st: SpecialTokens, beam_size: int = 5, max_depth: int = 100, **kw) -> WbDecodeParams:
    """The constants transcribe.rs hard-codes (beam 5 x depth 100, padding 10, 3 s overlap, (40, 3) stitch)."""
    p = WbDecodeParams()
    _lib.load().wb_decode_params_default(C.byref(p))
    p.beam_size, p.max_depth = beam_size, max_depth
    p.tok_start_of_transcript, p.tok_language = st.start_of_transcript, st.language
    p.tok_transcribe, p.tok_no_timestamps, p.tok_end_of_text = st.transcribe, st.no_timestamps, st.end_of_text
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def window_extents(n_samples: int, sample_rate: int, window_len: int, overlap_seconds: int = 3):
    """transcribe.rs:120-128."""
    lib = _lib.load()
    n = int(lib.wb_window_extents(n_samples, sample_rate, window_len, overlap_seconds, None, None, 0))
    starts = np.zeros(n, dtype=np.int64)
    lens = np.zeros(n, dtype=np.int64)
    lib.wb_window_extents(n_samples, sample_rate, window_len, overlap_seconds,
                          starts.ctypes.data_as(_lib.c_int64_p), lens.ctypes.data_as(_lib.c_int64_p), n)
    return starts, lens


def find_chunk_overlap(prev_tokens: Sequence[int], curr_tokens: Sequence[int], max_n_offsets: int,
                       min_n_overlaps: int) -> Optional[Tuple[int, int]]:
    """transcribe.rs:76-110."""
    p, c = _i32(list(prev_tokens)), _i32(list(curr_tokens))
    pi, ci = C.c_int64(0), C.c_int64(0)
    r = _lib.load().wb_find_chunk_overlap(_ip(p), len(p), _ip(c), len(c), max_n_offsets, min_n_overlaps,
                                          C.byref(pi), C.byref(ci))
    return (int(pi.value), int(ci.value)) if r == 1 else None


def stitch_windows(win_tokens: np.ndarray, win_lens: np.ndarray, max_n_offsets: int = 40,
                   min_n_overlaps: int = 3, times: Optional[np.ndarray] = None):
    """Fold transcribe.rs:56-63 over per-window token rows in window order.  With `times` (a float per token, same
    shape as win_tokens) returns (tokens, times): a stitched token keeps the value of the window it was taken from."""
    wt, wl = _i32(win_tokens), _i32(win_lens)
    cap = int(wl.sum()) + 1
    out = np.zeros(cap, dtype=np.int32)
    n_out = C.c_int64(0)
    if times is not None:
        tm = _f32(times)
        assert tm.shape == wt.shape
        out_t = np.zeros(cap, dtype=np.float32)
        check(_lib.load().wb_stitch_windows_times(_ip(wt), wt.shape[1] if wt.ndim == 2 else 0, _ip(wl), len(wl),
                                                  max_n_offsets, min_n_overlaps, _ip(out), cap, C.byref(n_out),
                                                  _fp(tm), _fp(out_t)))
        return out[:n_out.value].tolist(), out_t[:n_out.value].copy()
    check(_lib.load().wb_stitch_windows(_ip(wt), wt.shape[1] if wt.ndim == 2 else 0, _ip(wl), len(wl),
                                        max_n_offsets, min_n_overlaps, _ip(out), cap, C.byref(n_out)))
    return out[:n_out.value].tolist()


def waveform_to_tokens(whisper: Whisper, st: SpecialTokens, waveform, sample_rate: int = 16000,
                       beam_size: int = 5, max_depth: int = 100, win_begin: int = 0, win_end: int = -1,
                       params: Optional[WbDecodeParams] = None, device_ptr: Optional[int] = None,
                       n_samples: Optional[int] = None):
    """waveform_to_text (transcribe.rs:23-74) without the tokenizer.

    Returns (stitched token ids of the local windows, per-window token lists).  [win_begin, win_end)
    selects the windows this process decodes (multi-GPU sharding); default all.
    With `device_ptr` (+ `n_samples`) the waveform is read in place from device memory
    (wb_waveform_to_tokens_dev) and `waveform` is ignored."""
    lib = _lib.load()
    if device_ptr is None:
        wav = _f32(waveform).reshape(-1)
        n_samples = len(wav)
    p = params or decode_params(st, beam_size, max_depth)
    wlen = max_waveform_samples(whisper.max_mel_frames() - p.padding)
    starts, _ = window_extents(n_samples, sample_rate, wlen, p.overlap_seconds)
    n_win = len(starts)
    if win_end < 0:
        win_end = n_win
    n_local = max(0, win_end - win_begin)
    stride = 4 + p.max_depth + 4
    win_tokens = np.zeros((max(n_local, 1), stride), dtype=np.int32)
    win_lens = np.zeros(max(n_local, 1), dtype=np.int32)
    cap = max(n_local, 1) * stride
    stitched = np.zeros(cap, dtype=np.int32)
    n_st = C.c_int64(0)
    mask = special_mask_bytes(whisper, st.is_special)
    if device_ptr is None:
        check(lib.wb_waveform_to_tokens(whisper._h, _fp(wav), n_samples, sample_rate, C.byref(p),
                                        mask.ctypes.data_as(_lib.c_uint8_p), win_begin, win_end, _ip(win_tokens),
                                        stride, _ip(win_lens), _ip(stitched), cap, C.byref(n_st)))
    else:
        check(lib.wb_waveform_to_tokens_dev(whisper._h, C.c_void_p(device_ptr), n_samples, sample_rate, C.byref(p),
                                            mask.ctypes.data_as(_lib.c_uint8_p), win_begin, win_end,
                                            _ip(win_tokens), stride, _ip(win_lens), _ip(stitched), cap,
                                            C.byref(n_st)))
    per_window = [win_tokens[i, :win_lens[i]].tolist() for i in range(n_local)]
    return stitched[:n_st.value].tolist(), per_window


def waveform_to_token_times(whisper: Whisper, st: SpecialTokens, waveform, sample_rate: int = 16000,
                            beam_size: int = 5, max_depth: int = 100, params: Optional[WbDecodeParams] = None,
                            heads=None, filter_width: int = 7):
    """waveform_to_tokens + token start times (wb_waveform_to_token_times).

    Returns (stitched tokens, stitched times [s], per-window token lists, per-window time arrays); a time is NaN for
    the prompt tokens and a final <|endoftext|> of the window the token came from."""
    lib = _lib.load()
    wav = _f32(waveform).reshape(-1)
    p = params or decode_params(st, beam_size, max_depth)
    wlen = max_waveform_samples(whisper.max_mel_frames() - p.padding)
    starts, _ = window_extents(len(wav), sample_rate, wlen, p.overlap_seconds)
    n_win = max(len(starts), 1)
    stride = 4 + p.max_depth + 4
    win_tokens = np.zeros((n_win, stride), dtype=np.int32)
    win_lens = np.zeros(n_win, dtype=np.int32)
    win_times = np.full((n_win, stride), np.nan, dtype=np.float32)
    cap = n_win * stride
    stitched = np.zeros(cap, dtype=np.int32)
    stitched_t = np.full(cap, np.nan, dtype=np.float32)
    n_st = C.c_int64(0)
    mask = special_mask_bytes(whisper, st.is_special)
    h, nh = _heads_arg(heads)
    check(lib.wb_waveform_to_token_times(whisper._h, _fp(wav), len(wav), sample_rate, C.byref(p),
                                         mask.ctypes.data_as(_lib.c_uint8_p), 0, -1, _ip(win_tokens), stride,
                                         _ip(win_lens), _ip(stitched), cap, C.byref(n_st),
                                         _ip(h) if h is not None else None, nh, filter_width, _fp(win_times),
                                         _fp(stitched_t)))
    n = len(starts)
    return (stitched[:n_st.value].tolist(), stitched_t[:n_st.value].copy(),
            [win_tokens[i, :win_lens[i]].tolist() for i in range(n)],
            [win_times[i, :win_lens[i]].copy() for i in range(n)])


def waveform_to_token_scores(whisper: Whisper, st: SpecialTokens, waveform, sample_rate: int = 16000,
                             beam_size: int = 5, max_depth: int = 100, params: Optional[WbDecodeParams] = None,
                             no_speech: Optional[int] = None):
    """waveform_to_tokens + token log-probabilities (wb_waveform_to_token_scores).

    Returns a dict: tokens / logprobs (the stitched stream), win_tokens / win_logprobs (per window; NaN at entry 0),
    avg_logprob [n_windows] (mean over the generated tokens of the window) and no_speech_prob [n_windows] (NaN when the
    vocabulary has no no-speech token: `no_speech`, default st.no_speech, is -1)."""
    lib = _lib.load()
    if no_speech is None:
        no_speech = st.no_speech
    wav = _f32(waveform).reshape(-1)
    p = params or decode_params(st, beam_size, max_depth)
    wlen = max_waveform_samples(whisper.max_mel_frames() - p.padding)
    starts, _ = window_extents(len(wav), sample_rate, wlen, p.overlap_seconds)
    n = len(starts)
    n_win = max(n, 1)
    stride = 4 + p.max_depth + 4
    win_tokens = np.zeros((n_win, stride), dtype=np.int32)
    win_lens = np.zeros(n_win, dtype=np.int32)
    win_lp = np.full((n_win, stride), np.nan, dtype=np.float32)
    cap = n_win * stride
    stitched = np.zeros(cap, dtype=np.int32)
    stitched_lp = np.full(cap, np.nan, dtype=np.float32)
    avg = np.full(n_win, np.nan, dtype=np.float32)
    nsp = np.full(n_win, np.nan, dtype=np.float32)
    n_st = C.c_int64(0)
    mask = special_mask_bytes(whisper, st.is_special)
    check(lib.wb_waveform_to_token_scores(whisper._h, _fp(wav), len(wav), sample_rate, C.byref(p),
                                          mask.ctypes.data_as(_lib.c_uint8_p), 0, -1, _ip(win_tokens), stride,
                                          _ip(win_lens), _ip(stitched), cap, C.byref(n_st), int(no_speech), _fp(win_lp),
                                          _fp(stitched_lp), _fp(avg), _fp(nsp)))
    return dict(tokens=stitched[:n_st.value].tolist(), logprobs=stitched_lp[:n_st.value].copy(),
                win_tokens=[win_tokens[i, :win_lens[i]].tolist() for i in range(n)],
                win_logprobs=[win_lp[i, :win_lens[i]].copy() for i in range(n)],
                avg_logprob=avg[:n].copy(), no_speech_prob=nsp[:n].copy())


def detect_language(whisper: Whisper, st_or_ids, waveform, sample_rate: int = 16000, sot: Optional[int] = None,
                    padding: int = 10, max_windows: int = 1):
    """Whisper's detect_language over the first `max_windows` windows (0: all; wb_waveform_detect_language).
    st_or_ids: a SpecialTokens (its `language_ids` and start_of_transcript are used), or a sequence of language token
    ids (then `sot` is required).  Returns (best index into the ids, mean_probs [n_lang], win_probs [W, n_lang])."""
    if hasattr(st_or_ids, "start_of_transcript"):
        ids = st_or_ids.language_ids
        if len(ids) == 0:
            raise ValueError("the tokenizer has no language tokens: language detection needs a multilingual vocabulary")
        sot = st_or_ids.start_of_transcript if sot is None else sot
    else:
        ids = st_or_ids
    if sot is None:
        raise ValueError("detect_language: sot (the start-of-transcript id) is required with a plain id list")
    ids = _i32(list(ids))
    wav = _f32(waveform).reshape(-1)
    wlen = max_waveform_samples(whisper.max_mel_frames() - padding)
    dp = WbDecodeParams()
    _lib.load().wb_decode_params_default(C.byref(dp))        # the C side cuts its windows with the default overlap
    starts, _ = window_extents(len(wav), sample_rate, wlen, dp.overlap_seconds)
    W = len(starts) if max_windows <= 0 else min(max_windows, len(starts))
    win = np.zeros((max(W, 1), len(ids)), dtype=np.float32)
    mean = np.zeros(len(ids), dtype=np.float32)
    best = C.c_int32(-1)
    check(_lib.load().wb_waveform_detect_language(whisper._h, _fp(wav), len(wav), sample_rate, padding, int(sot), _ip(ids),
                                                  len(ids), max_windows, _fp(win), _fp(mean), C.byref(best)))
    return int(best.value), mean, win[:W]


def waveform_to_text(whisper: Whisper, bpe, lang, waveform, sample_rate: int = 16000):
    """transcribe.rs:23-29 shape: returns (text, tokens).  `bpe` must offer
    `special_tokens(lang) -> SpecialTokens` and `decode(tokens, skip_special) -> str`
    (the tokenizer stays outside the engine; none ships in this environment)."""
    st = bpe.special_tokens(lang)
    tokens, _ = waveform_to_tokens(whisper, st, waveform, sample_rate)
    return bpe.decode(tokens, True), tokens


class Session:
    """KV-cached decode session over a batch of windows (include/whisper_hip.h, wb_session_*).

    New relative to the reference, which has no KV cache (transcribe.rs:270); result-equivalent
    to running `beamsearch_next` (transcribe.rs:253-307) on the same beams."""

    def __init__(self, whisper: Whisper, handle, n_windows: int):
        self._w = whisper
        self._h = handle
        self.n_windows = n_windows

    @staticmethod
    def begin(whisper: Whisper, waveform, starts, lens, max_beams: int = 5, padding: int = 10) -> "Session":
        wav = _f32(waveform).reshape(-1)
        st = np.ascontiguousarray(starts, dtype=np.int64)
        ln = np.ascontiguousarray(lens, dtype=np.int64)
        h = C.c_void_p()
        check(_lib.load().wb_session_begin(whisper._h, _fp(wav), len(wav), st.ctypes.data_as(_lib.c_int64_p),
                                           ln.ctypes.data_as(_lib.c_int64_p), len(st), max_beams, padding,
                                           C.byref(h)))
        return Session(whisper, h, len(st))

    @staticmethod
    def begin_mel(whisper: Whisper, mels: Sequence[np.ndarray], max_beams: int = 5, padding: int = 10) -> "Session":
        mels = [_f32(m) for m in mels]
        T = _i32([m.shape[1] for m in mels])
        flat = np.concatenate([m.reshape(-1) for m in mels])
        h = C.c_void_p()
        check(_lib.load().wb_session_begin_mel(whisper._h, _fp(flat), _ip(T), len(mels), max_beams, padding,
                                               C.byref(h)))
        return Session(whisper, h, len(mels))

    def set_special_mask(self, is_special) -> None:
        m = special_mask_bytes(self._w, is_special)
        check(_lib.load().wb_session_set_special_mask(self._h, m.ctypes.data_as(_lib.c_uint8_p)))

    def step(self, new_tokens, parent, window, apply_special_mask: bool = False, k: int = 5):
        t, p, w = _i32(new_tokens), _i32(parent), _i32(window)
        n = len(t)
        ids = np.zeros((n, max(k, 1)), dtype=np.int32)
        lps = np.zeros((n, max(k, 1)), dtype=np.float32)
        check(_lib.load().wb_session_step(self._h, _ip(t), _ip(p), _ip(w), n, int(apply_special_mask), k,
                                          _ip(ids), _fp(lps)))
        return (ids[:, :k], lps[:, :k]) if k > 0 else (None, None)

    def last_logprobs(self, slot: int) -> np.ndarray:
        out = np.empty(self._w.dims["n_vocab"], dtype=np.float32)
        check(_lib.load().wb_session_last_logprobs(self._h, slot, _fp(out)))
        return out

    def encoder_output(self, w: int) -> np.ndarray:
        c = C.c_int32(0)
        check(_lib.load().wb_session_encoder_output(self._h, w, None, C.byref(c)))
        out = np.empty((c.value, self._w.dims["n_audio_state"]), dtype=np.float32)
        check(_lib.load().wb_session_encoder_output(self._h, w, _fp(out), C.byref(c)))
        return out

    def decode(self, params: WbDecodeParams) -> List[List[int]]:
        stride = 4 + params.max_depth + 4
        toks = np.zeros((self.n_windows, stride), dtype=np.int32)
        lens = np.zeros(self.n_windows, dtype=np.int32)
        check(_lib.load().wb_session_decode(self._h, C.byref(params), _ip(toks), stride, _ip(lens)))
        return [toks[i, :lens[i]].tolist() for i in range(self.n_windows)]

    def decode_prompt(self, params: WbDecodeParams, prompt) -> List[List[int]]:
        """Session.decode behind a caller's prompt (wb_session_decode_prompt): the host-driven beam search of params.beam_size."""
        pr = _i32(list(prompt))
        stride = len(pr) + params.max_depth + 4
        toks = np.zeros((self.n_windows, stride), dtype=np.int32)
        lens = np.zeros(self.n_windows, dtype=np.int32)
        check(_lib.load().wb_session_decode_prompt(self._h, C.byref(params), _ip(pr), len(pr), _ip(toks), stride, _ip(lens)))
        return [toks[i, :lens[i]].tolist() for i in range(self.n_windows)]

    def set_prefill(self, mode: int) -> None:
        """How the decode calls feed a prompt to the self-KV cache (wb_session_set_prefill): 0 one step per token (default),
        1 one teacher-forced pass over all prompt positions."""
        check(_lib.load().wb_session_set_prefill(self._h, int(mode)))

    def prefill(self, tokens, active=None) -> None:
        """The one-pass prompt prefill alone (wb_session_prefill), on a fresh or rewound session: the same `tokens` for every
        active window (active [W] of 0 / 1, default all); step() continues behind it with parent = index among the active."""
        t = _i32(list(tokens))
        act = np.ascontiguousarray(active, dtype=np.uint8) if active is not None else None
        check(_lib.load().wb_session_prefill(self._h, _ip(t) if len(t) else None, len(t), _u8p(act)))

    def self_kv(self, layer: int, slot: int, n_pos: int):
        """Cached self-attention K (pre-scaled) and V of a live slot, [n_pos, d] each (wb_session_self_kv, a test hook)."""
        d = self._w.dims["n_text_state"]
        K, V = np.full((n_pos, d), np.nan, dtype=np.float32), np.full((n_pos, d), np.nan, dtype=np.float32)
        check(_lib.load().wb_session_self_kv(self._h, int(layer), int(slot), int(n_pos), _fp(K), _fp(V)))
        return K, V

    def rewind(self) -> None:
        """Back to step 0 over the same encoded windows (wb_session_rewind): another decode costs decode steps only."""
        check(_lib.load().wb_session_rewind(self._h))

    def graph_count(self) -> int:
        """Captured step graphs the session holds (debug)."""
        return int(_lib.load().wb_session_graph_count(self._h))

    def graph_captures(self) -> int:
        """Step graphs captured over the session's life (debug): unchanged by a call that only replays."""
        return int(_lib.load().wb_session_graph_captures(self._h))

    def decode_sample(self, params: WbDecodeParams, sample: WbSampleParams, prompt=None, active=None, stream_ids=None,
                      out_tokens: Optional[np.ndarray] = None, out_lens: Optional[np.ndarray] = None):
        """best_of sampled sequences per window at sample.temperature (wb_session_decode_sample), on a fresh or rewound
        session.  prompt: default the four-token prompt of `params`; active [W]: windows to decode (default all);
        stream_ids [W]: base stream of each window (default w * best_of); out_tokens / out_lens: arrays to write into
        (rows of inactive windows stay as they are).  Returns (rows, sum_logprob [W, best_of] f64, best [W])."""
        W, bo = self.n_windows, int(sample.best_of)
        pr = _i32([params.tok_start_of_transcript, params.tok_language, params.tok_transcribe, params.tok_no_timestamps]
                  if prompt is None else list(prompt))
        stride = len(pr) + params.max_depth + 4
        toks = out_tokens if out_tokens is not None else np.zeros((W, stride), dtype=np.int32)
        lens = out_lens if out_lens is not None else np.zeros(W, dtype=np.int32)
        assert toks.dtype == np.int32 and toks.flags.c_contiguous and toks.shape[0] == W and lens.dtype == np.int32
        act = np.ascontiguousarray(active, dtype=np.uint8) if active is not None else None
        sid = _i32(stream_ids) if stream_ids is not None else None
        sums = np.full((W, max(bo, 1)), np.nan, dtype=np.float64)
        best = np.full(W, -1, dtype=np.int32)
        check(_lib.load().wb_session_decode_sample(self._h, C.byref(params), C.byref(sample), _ip(pr), len(pr), _u8p(act),
                                                   _ip(sid) if sid is not None else None, _ip(toks), toks.shape[1], _ip(lens),
                                                   sums.ctypes.data_as(_lib.c_double_p), _ip(best)))
        return [toks[i, :lens[i]].tolist() for i in range(W)], sums, best

    def set_suppress(self, suppress, suppress_first=None) -> None:
        """The static masks of timestamp decoding (wb_session_set_suppress): [V] of 0 / 1 each."""
        V = self._w.dims["n_vocab"]
        check(_lib.load().wb_session_set_suppress(self._h, _u8p(_u8v(suppress, V)), _u8p(_u8v(suppress_first, V))))

    def decode_timestamps(self, params: WbDecodeParams, timestamps: WbTimestampParams, prompt=None, active=None,
                          stream_ids=None, out_tokens: Optional[np.ndarray] = None, out_lens: Optional[np.ndarray] = None):
        """Decoding under the timestamp rules (wb_session_decode_timestamps), on a fresh or rewound session after
        set_suppress.  prompt: default [sot, language, transcribe] of `params`; the other arguments and the result as
        decode_sample: (rows, sum_logprob [W, best_of] f64, best [W])."""
        W, bo = self.n_windows, int(timestamps.best_of)
        pr = _i32([params.tok_start_of_transcript, params.tok_language, params.tok_transcribe] if prompt is None else list(prompt))
        stride = len(pr) + params.max_depth + 4
        toks = out_tokens if out_tokens is not None else np.zeros((W, stride), dtype=np.int32)
        lens = out_lens if out_lens is not None else np.zeros(W, dtype=np.int32)
        assert toks.dtype == np.int32 and toks.flags.c_contiguous and toks.shape[0] == W and lens.dtype == np.int32
        act = np.ascontiguousarray(active, dtype=np.uint8) if active is not None else None
        sid = _i32(stream_ids) if stream_ids is not None else None
        sums = np.full((W, max(bo, 1)), np.nan, dtype=np.float64)
        best = np.full(W, -1, dtype=np.int32)
        check(_lib.load().wb_session_decode_timestamps(self._h, C.byref(params), C.byref(timestamps), _ip(pr), len(pr), _u8p(act),
                                                       _ip(sid) if sid is not None else None, _ip(toks), toks.shape[1],
                                                       _ip(lens), sums.ctypes.data_as(_lib.c_double_p), _ip(best)))
        return [toks[i, :lens[i]].tolist() for i in range(W)], sums, best

    def decode_timestamps_beam(self, params: WbDecodeParams, timestamps: WbTimestampParams, beam: WbBeamParams, prompt=None,
                               active=None, out_tokens: Optional[np.ndarray] = None, out_lens: Optional[np.ndarray] = None):
        """Beam search under the timestamp rules (wb_session_decode_timestamps_beam), on a fresh or rewound session after
        set_suppress.  prompt / active / out_tokens / out_lens as decode_timestamps.  Returns (rows, score [W] f64 -- the
        best candidate's cumulative log-prob, nan for inactive windows --, n_candidates [W], -1 for inactive windows)."""
        W = self.n_windows
        pr = _i32([params.tok_start_of_transcript, params.tok_language, params.tok_transcribe] if prompt is None else list(prompt))
        stride = len(pr) + params.max_depth + 4
        toks = out_tokens if out_tokens is not None else np.zeros((W, stride), dtype=np.int32)
        lens = out_lens if out_lens is not None else np.zeros(W, dtype=np.int32)
        assert toks.dtype == np.int32 and toks.flags.c_contiguous and toks.shape[0] == W and lens.dtype == np.int32
        act = np.ascontiguousarray(active, dtype=np.uint8) if active is not None else None
        score = np.full(W, np.nan, dtype=np.float64)
        ncand = np.full(W, -1, dtype=np.int32)
        check(_lib.load().wb_session_decode_timestamps_beam(self._h, C.byref(params), C.byref(timestamps), C.byref(beam), _ip(pr),
                                                            len(pr), _u8p(act), _ip(toks), toks.shape[1], _ip(lens),
                                                            score.ctypes.data_as(_lib.c_double_p), _ip(ncand)))
        return [toks[i, :lens[i]].tolist() for i in range(W)], score, ncand

    def last_beams(self, max_depth: int):
        """Every finalized candidate of the last decode_timestamps_beam (wb_session_last_beams), in store order: per window a
        list of dict(tokens -- generated, no prompt --, score, rank); None for the windows that were not active."""
        toks, lens, scores, ranks, n = _beams_out(self.n_windows, max_depth)
        check(_lib.load().wb_session_last_beams(self._h, toks.shape[1], _ip(toks), toks.shape[2], _ip(lens),
                                                scores.ctypes.data_as(_lib.c_double_p), ranks.ctypes.data_as(_lib.c_double_p), _ip(n)))
        return _beams_list(toks, lens, scores, ranks, n)

    def last_beam_trace(self, max_depth: int):
        """The trace of the last decode_timestamps_beam (wb_session_last_beam_trace): per window a list of steps, each
        dict(finished = candidates newly finished in the step, beams = [(token, parent beam index, f64 score)] of the live
        beams behind it)."""
        tr = _trace_out(self.n_windows, max_depth)
        check(_lib.load().wb_session_last_beam_trace(self._h, tr[1].shape[0], _ip(tr[0]), _ip(tr[1]), _ip(tr[2]), _ip(tr[3]),
                                                     _ip(tr[4]), tr[5].ctypes.data_as(_lib.c_double_p)))
        return _trace_list(*tr)

    def last_samples(self, best_of: int, max_depth: int) -> List[List[Optional[List[int]]]]:
        """Every sample of the last decode_sample (wb_session_last_samples): [W][best_of] lists of generated tokens (without
        the prompt); None for the windows that were not active."""
        W = self.n_windows
        toks = np.zeros((W * best_of, max(max_depth, 1)), dtype=np.int32)
        lens = np.zeros(W * best_of, dtype=np.int32)
        check(_lib.load().wb_session_last_samples(self._h, _ip(toks), toks.shape[1], _ip(lens)))
        return [[toks[w * best_of + j, :lens[w * best_of + j]].tolist() if lens[w * best_of + j] >= 0 else None
                 for j in range(best_of)] for w in range(W)]

    def align(self, tokens, lens=None, heads=None, n_prefix: int = 4, drop_last: int = 1, filter_width: int = 7,
              return_matrix: bool = False):
        """Token start positions of one row per window (wb_session_align), on the session's encoder output and cached
        cross-attention K: start_pos [W, L] (-1 where a token is not aligned) and, on request, the matrix [W, L, maxC]."""
        tokens, lens = _rows_arg(tokens, lens)
        W, L = tokens.shape
        assert W == self.n_windows
        h, nh = _heads_arg(heads)
        pos = np.full((W, L), -1, dtype=np.int32)
        mat = None
        if return_matrix:
            c = C.c_int32(0)
            maxC = 0
            for w in range(W):
                check(_lib.load().wb_session_encoder_output(self._h, w, None, C.byref(c)))
                maxC = max(maxC, c.value)
            mat = np.zeros((W, L, maxC), dtype=np.float32)
        check(_lib.load().wb_session_align(self._h, _ip(tokens), L, _ip(lens), _ip(h) if h is not None else None, nh,
                                           n_prefix, drop_last, filter_width, _ip(pos),
                                           _fp(mat) if mat is not None else None))
        return (pos, mat) if return_matrix else pos

    def score(self, tokens, lens=None, mask_until_len: int = 0, probe_ids=None, probe_pos: int = 0):
        """Per-token log-probabilities of one row per window (wb_session_score) on the session's cached cross K/V:
        token_logprobs [W, L] as Whisper.score_tokens; the mask is the one of set_special_mask.  With probe_ids also
        returns probe_logprobs [W, n_probe] (unmasked, at position probe_pos)."""
        tokens, lens = _rows_arg(tokens, lens)
        W, L = tokens.shape
        assert W == self.n_windows
        pid = _i32(probe_ids) if probe_ids is not None else None
        npb = len(pid) if pid is not None else 0
        lp = np.full((W, L), np.nan, dtype=np.float32)
        plp = np.full((W, max(npb, 1)), np.nan, dtype=np.float32)
        check(_lib.load().wb_session_score(self._h, _ip(tokens), L, _ip(lens), mask_until_len,
                                           _ip(pid) if pid is not None else None, npb, probe_pos, _fp(lp),
                                           _fp(plp) if npb else None))
        return (lp, plp[:, :npb]) if pid is not None else lp

    def detect_language(self, sot: int, lang_ids):
        """Language probabilities of every window of the session: softmax over `lang_ids` of the distribution after
        [sot] (Whisper's detect_language) -> (argmax of the mean over the windows, mean_probs, win_probs [W, n_lang])."""
        ids = _i32(list(lang_ids))
        _, plp = self.score(np.full((self.n_windows, 1), sot, dtype=np.int32), probe_ids=ids, probe_pos=0)
        z = plp.astype(np.float64)
        e = np.exp(z - z.max(axis=1, keepdims=True))
        win = e / e.sum(axis=1, keepdims=True)
        mean = win.mean(axis=0)
        return int(np.argmax(mean)), mean.astype(np.float32), win.astype(np.float32)

    def close(self):
        if self._h:
            _lib.load().wb_session_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
