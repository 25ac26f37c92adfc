"""Temperature sampling restated in NumPy (the checker side of csrc/sample.hip and wb_sample_rows), written from the contract in
include/whisper_hip.h: Philox4x32-10 with its known answers, the uniform, the Gumbel keys in f64, the exclusion rule of the
parity tests and the inputs of the operator test."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)
I31 = 2 ** 31 - 1

# (counter, key, output): the known answers of the generator
KAT = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
        (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 over arrays (broadcast): four uint32 output words, as uint64 arrays below 2^32."""
    c0, c1, c2, c3 = [np.asarray(c, dtype=np.uint64) & MASK32 for c in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = np.uint64(k0 & 0xFFFFFFFF), np.uint64(k1 & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ k0
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ k1
        c1, c3, c0, c2 = p1 & MASK32, p0 & MASK32, n0, n2
        k0, k1 = (k0 + np.uint64(W0)) & MASK32, (k1 + np.uint64(W1)) & MASK32
    return c0, c1, c2, c3


def words(V, seed, stream, attempt, position):
    """The uint32 word of every vocabulary id: output (v & 3) under counter (v >> 2, position, stream, attempt)."""
    g = np.arange((V + 3) // 4, dtype=np.uint64)
    out = philox4x32_10(g, int(position) & 0xFFFFFFFF, int(stream) & 0xFFFFFFFF, int(attempt) & 0xFFFFFFFF,
                        int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    return np.stack(out, axis=1).reshape(-1)[:V]


def uniform(w):
    """((word >> 9) + 0.5) 2^-23: exact in f32, inside [2^-24, 1 - 2^-24]."""
    return ((np.asarray(w, dtype=np.uint64) >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def gumbel(w):
    return -np.log(-np.log(uniform(w)))


def row_stats(x, mask=None):
    """(M, lse) of a row under its mask, as f32 from an f64 evaluation -- what a logits tail leaves in row_stats."""
    v = np.asarray(x, dtype=np.float64) + (0.0 if mask is None else np.asarray(mask, dtype=np.float64))
    M = v.max()
    with np.errstate(divide="ignore"):
        lse = np.log(np.exp(v - M).sum())
    return np.float32(M), np.float32(lse)


def keys(x, mask, M, T, seed, stream, attempt, position):
    """The f64 keys (x + mask - M) / T + g of a row; a masked id has key -inf.  T is the caller's f32 temperature: the device
    multiplies by the f32 1 / T, and so does this."""
    inv_t = float(np.float32(1.0) / np.float32(T))
    v = np.asarray(x, dtype=np.float64) + (0.0 if mask is None else np.asarray(mask, dtype=np.float64))
    return (v - float(M)) * inv_t + gumbel(words(len(v), seed, stream, attempt, position))


def delta_op(A, T):
    """Key error of the device draw: each key carries at most about 2^-22 (|x - M| / T + |g| + 1) from two one-ulp logf and
    three f32 roundings, |g| <= 16.64; doubled for the pair and doubled again as margin."""
    return 2.0 ** -20 * (A / float(T) + 18.0)


def draw(x, mask, M, lse, T, seed, stream, attempt, position):
    """f64 restatement of one draw: dict(token, logprob, gap = top-two key gap, A = largest finite |x + mask - M|)."""
    k = keys(x, mask, M, T, seed, stream, attempt, position)
    order = np.lexsort((np.arange(len(k)), -k))          # key descending, id ascending
    tok = int(order[0])
    gap = float(k[order[0]] - k[order[1]]) if len(k) > 1 else np.inf
    v = np.asarray(x, dtype=np.float64) + (0.0 if mask is None else np.asarray(mask, dtype=np.float64))
    t = v - float(M)
    A = float(np.abs(t[np.isfinite(t)]).max())
    return dict(token=tok, logprob=float(t[tok] - float(lse)), gap=gap, A=A, t_tok=float(t[tok]))


def logprob_bound(d):
    """(x + mask - M) - lse in f32 from f32 inputs: two roundings."""
    return 2.0 ** -22 * (abs(d["t_tok"]) + abs(d["logprob"])) + 1e-30


# ---- the operator test's inputs ------------------------------------------------------------------------------------------------
SHAPES = [(1, 263), (5, 1031), (33, 7001), (3, 51865)]
TEMPS = [0.2, 1.0]
PAD = 5                       # extra columns of the logits rows, poisoned with NaN


def make_cases(shape, seed=0):
    """Cases of one (R, V): kinds `mixed` (a tail mask on every other row), `single` (the mask leaves one id), `heavy` (the mask
    leaves one id in ten), each at both temperatures; streams / positions / attempts at 0 and 2^31 - 1."""
    R, V = shape
    out = []
    for ti, T in enumerate(TEMPS):
        for ki, kind in enumerate(("mixed", "single", "heavy")):
            g = np.random.default_rng([seed, R, V, ti, ki])
            x = (g.standard_normal((R, V)) * 3.0).astype(np.float32)
            mask = np.zeros(V, dtype=np.float32)
            if kind == "mixed":
                mask[V - max(V // 10, 2):] = -np.inf
                rm = (np.arange(R) % 2 == 0) if R > 1 else np.ones(1, dtype=bool)
            elif kind == "single":
                mask[:] = -np.inf
                mask[int(g.integers(0, V))] = 0.0
                rm = (np.arange(R) % 2 == 1) if R > 1 else np.ones(1, dtype=bool)
            else:
                mask[g.random(V) < 0.9] = -np.inf
                mask[V - 1] = 0.0
                rm = (np.arange(R) % 3 != 1) if R > 1 else np.ones(1, dtype=bool)
            stream = g.integers(0, I31, R).astype(np.int64)
            position = g.integers(0, 448, R).astype(np.int64)
            stream[0] = 0 if ki != 1 else I31
            position[0] = I31 if ki != 1 else 0
            if R > 1:
                stream[1], position[1] = I31, I31
            if R > 2:
                stream[2], position[2] = 0, 0
            logits = np.full((R, V + PAD), np.nan, dtype=np.float32)
            logits[:, :V] = x
            stats = np.array([row_stats(x[r], mask if rm[r] else None) for r in range(R)], dtype=np.float32)
            out.append(dict(name=f"R{R}_V{V}_T{T}_{kind}", kind=kind, R=R, V=V, T=T, logits=logits, mask=mask,
                            row_masked=rm.astype(np.uint8), stats=stats, seed=int(g.integers(0, 2 ** 63)) | (1 << 40),
                            attempt=(0, I31, 3)[ki], stream=stream.astype(np.int32), position=position.astype(np.int32),
                            eot=V - 2))
    return out


def reference(case):
    """The f64 draws of a case: a list of draw() dicts, one per row."""
    V = case["V"]
    return [draw(case["logits"][r, :V], case["mask"] if case["row_masked"][r] else None, case["stats"][r, 0], case["stats"][r, 1],
                 case["T"], case["seed"], int(case["stream"][r]), case["attempt"], int(case["position"][r]))
            for r in range(case["R"])]


def excluded(ref, T):
    """Rows whose f64 top-two key gap does not exceed delta_op: the device may pick either id there."""
    return np.array([not (d["gap"] > delta_op(d["A"], T)) for d in ref])


def run_hook(case, rows=None, device=0):
    import whisper_burn_amd as wb
    sel = np.arange(case["R"]) if rows is None else np.asarray(rows)
    return wb.sample_rows(case["logits"][sel], case["stats"][sel], case["T"], case["seed"], case["attempt"], case["stream"][sel],
                          case["position"][sel], case["eot"], V=case["V"], mask=case["mask"],
                          row_masked=case["row_masked"][sel] if case["row_masked"] is not None else None, device=device)


def check_hook_case(case, ref=None, record=None):
    """The hook against the f64 restatement: the token wherever the gap exceeds delta_op (at most 1 % of the draws may be
    excluded), the recorded log-prob of every agreed token within the two-rounding bound, no error word."""
    ref = ref or reference(case)
    tok, lp, err = run_hook(case)
    ex = excluded(ref, case["T"])
    if record is not None:
        record.append((case["name"], int(ex.sum()), [int(t) for t in tok[:4]]))
    assert err == 0, case["name"]
    assert ex.sum() <= 0.01 * case["R"], (case["name"], int(ex.sum()))
    for r, d in enumerate(ref):
        if ex[r]:
            continue
        assert tok[r] == d["token"], (case["name"], r, int(tok[r]), d["token"], d["gap"])
        assert abs(float(lp[r]) - d["logprob"]) <= logprob_bound(d), (case["name"], r, float(lp[r]), d["logprob"])
        if case["kind"] == "single" and case["row_masked"][r]:
            assert tok[r] == int(np.flatnonzero(case["mask"] == 0)[0]) and abs(float(lp[r])) <= logprob_bound(d)
    return tok, lp


def chi_square_case(n_streams=4096, T=0.5, seed=77):
    """One 8-id row drawn on n_streams streams: (case, expected counts under softmax(x / T))."""
    x = np.array([0.3, -0.6, 0.5, 0.0, -0.2, 0.7, -0.9, 0.4], dtype=np.float32)
    V = len(x)
    logits = np.full((n_streams, V + PAD), np.nan, dtype=np.float32)
    logits[:, :V] = x
    st = np.tile(np.array(row_stats(x), dtype=np.float32), (n_streams, 1))
    case = dict(name="chi", kind="chi", R=n_streams, V=V, T=T, logits=logits, mask=None, row_masked=None, stats=st, seed=seed,
                attempt=1, stream=np.arange(n_streams, dtype=np.int32), position=np.full(n_streams, 7, dtype=np.int32), eot=V - 1)
    z = x.astype(np.float64) / T
    p = np.exp(z - z.max())
    return case, n_streams * p / p.sum()


# chi-square, 7 degrees of freedom: the 1 - 1e-6 quantile
CHI2_7_1M6 = 40.52


# ---- the model entries against the oracle --------------------------------------------------------------------------------------
def oracle_row_check(oracle, is_special, enc, row, P, mask_until_len, T, seed, stream, attempt, eot):
    """A sampled row against ONE teacher-forced pass of the oracle over it: for every generated position the oracle's f32 logits
    give the Gumbel-max argmax for the same counters.  Returns (positions, excluded, mismatches, sum of the oracle log-probs of
    the row's tokens): a position is excluded when the oracle's top-two key gap is at most delta_model = 2e-3 / T + delta_op
    (the 1e-3 log-prob gate of DESIGN.md section 5, once per candidate)."""
    import torch
    toks = torch.tensor([list(row)], dtype=torch.long)
    logits = oracle.forward_decoder(toks, torch.as_tensor(np.asarray(enc))[None])[0].double().numpy()
    maskv = np.where(np.asarray(is_special).astype(bool), -np.inf, 0.0)
    n = ex = bad = 0
    total = 0.0
    for l in range(P, len(row)):
        x = logits[l - 1]
        mk = maskv if l <= mask_until_len else None
        M, lse = row_stats(x, mk)
        v = x + (0.0 if mk is None else mk)
        lse64 = np.log(np.exp(v - v.max()).sum()) + v.max()
        total += float(v[row[l]] - lse64)
        d = draw(x, mk, M, lse, T, seed, stream, attempt, l)
        n += 1
        if not (d["gap"] > 2e-3 / T + delta_op(d["A"], T)):
            ex += 1
        elif d["token"] != row[l]:
            bad += 1
    return n, ex, bad, total


# (temperature, seed, attempt) of the session tests' draws
SESSION_DRAWS = [(1.0, 1234, 2), (0.2, 99, 1)]


# ---- shared by the functional-model checks and the GPU tests ---------------------------------------------------------------------
def windows(eng, audio, W, win_len=16000):
    """W overlapping windows of `win_len` samples cut from `audio` (explicit extents: the sessions of the tests)."""
    import whisper_burn_amd as wb
    win_len = min(win_len, wb.max_waveform_samples(eng.max_mel_frames() - 10))
    hop = max(1, (len(audio) - win_len) // max(W - 1, 1))
    starts = np.array([min(i * hop, len(audio) - win_len) for i in range(W)], dtype=np.int64)
    return starts, np.full(W, win_len, dtype=np.int64)


def n_text(gen, eot):
    return len(gen) - (1 if gen and gen[-1] == eot else 0)


def check_sampled_session(sess, oracle, st, params, T, seed, attempt, best_of, stream_ids=None, active=None, max_excluded=0.05,
                          record=None):
    """One decode_sample on a rewound / fresh session against the teacher-forced oracle: every sample of every active window
    (wb_session_last_samples) token by token outside the exclusion rule, its f64 sum against the oracle's log-probs within
    1e-3 per token, the returned row = the sample of out_best = the first argmax of sum / n_text.  Returns (rows, sums, best)."""
    import whisper_burn_amd as wb
    W = sess.n_windows
    prompt = [st.start_of_transcript, st.language, st.transcribe, st.no_timestamps]
    rows, sums, best = sess.decode_sample(params, wb.SampleParams(T, best_of, seed, attempt), stream_ids=stream_ids, active=active)
    gens = sess.last_samples(best_of, params.max_depth)
    n = ex = bad = 0
    for w in range(W):
        if active is not None and not active[w]:
            assert gens[w][0] is None and rows[w] == [] and np.isnan(sums[w]).all() and best[w] == -1, w   # untouched
            continue
        enc = sess.encoder_output(w)
        ranks = []
        for j in range(best_of):
            gen = gens[w][j]
            assert 1 <= len(gen) <= params.max_depth and st.end_of_text not in gen[:-1], (w, j, gen)
            base = stream_ids[w] if stream_ids is not None else w * best_of
            a, b, c, total = oracle_row_check(oracle, st.is_special, enc, prompt + gen, 4, params.mask_until_len, T, seed,
                                              base + j, attempt, st.end_of_text)
            n, ex, bad = n + a, ex + b, bad + c
            assert abs(sums[w, j] - total) <= 1e-3 * len(gen), (w, j, sums[w, j], total)
            nt = n_text(gen, st.end_of_text)
            ranks.append(sums[w, j] / nt if nt > 0 else -np.inf)
        assert best[w] == int(np.argmax(ranks)), (w, ranks, best[w])
        assert rows[w] == prompt + gens[w][best[w]], w
    if record is not None:
        record.append((T, best_of, n, ex, bad))
    assert bad == 0, (n, ex, bad)
    assert ex <= max_excluded * n, (n, ex)
    return rows, sums, best


def check_sums_against_score(sess, st, params, best_of, sums):
    """out_sum_logprob of EVERY sample of the last decode_sample against Session.score of the same rows (one scoring call per
    sample index: a call scores one row per window), within 1e-3 per token."""
    prompt = [st.start_of_transcript, st.language, st.transcribe, st.no_timestamps]
    gens = sess.last_samples(best_of, params.max_depth)
    for j in range(best_of):
        rows = [prompt + gens[w][j] for w in range(sess.n_windows)]
        lp = sess.score(rows, mask_until_len=params.mask_until_len)
        for w, row in enumerate(rows):
            s = float(np.sum(lp[w, 4:len(row)].astype(np.float64)))
            assert abs(sums[w, j] - s) <= 1e-3 * (len(row) - 4), (w, j, sums[w, j], s)


def fallback_decide_ref(fp, avg, nsp, ratio):
    """Python restatement of wb_fallback_decide over a dict of thresholds (NaN: rule off) and tok_no_speech."""
    isn = lambda v: v != v
    lp_on, cr_on = not isn(fp["logprob_threshold"]), not isn(fp["compression_ratio_threshold"])
    ns_on = fp["tok_no_speech"] >= 0 and not isn(fp["no_speech_threshold"])
    silent = ns_on and nsp > fp["no_speech_threshold"]
    retry = (cr_on and not ratio <= fp["compression_ratio_threshold"]) or (lp_on and not avg >= fp["logprob_threshold"]) or \
        (ns_on and isn(nsp))
    if silent:
        retry = False
    if retry:
        return 1
    if silent and (not lp_on or not avg > fp["logprob_threshold"]):
        return 2
    return 0


def check_fallback_scenarios(eng, st, audio, params, best_of=3, temps=(0.0, 0.4, 1.0), seed=11):
    """The three fallback scenarios on one engine: rules off = waveform_to_tokens; logprob_threshold = +inf uses every
    temperature and ends with status 1; a threshold in the widest gap of the attempt-0 avg_logprobs retries exactly the
    windows below it; a sharded call returns the rows of the whole call."""
    import whisper_burn_amd as wb
    full, wins = wb.waveform_to_tokens(eng, st, audio, 16000, params=params)
    off = wb.FallbackParams(temps, best_of, None, None, None, seed, -1)
    r0 = wb.waveform_to_tokens_fallback(eng, st, audio, 16000, params=params, fallback=off)
    assert r0["tokens"] == full and r0["win_tokens"] == wins
    assert (r0["attempts"] == 1).all() and (r0["status"] == 0).all() and (r0["temperature"] == 0).all()
    assert np.isnan(r0["ratio"]).all() and np.isnan(r0["no_speech_prob"]).all() and not np.isnan(r0["avg_logprob"]).any()
    nW = len(wins)
    assert nW >= 3
    # every window fails every temperature
    inf = wb.FallbackParams(temps, best_of, float("inf"), None, None, seed, -1)
    r1 = wb.waveform_to_tokens_fallback(eng, st, audio, 16000, params=params, fallback=inf)
    assert (r1["attempts"] == len(temps)).all() and (r1["status"] == 1).all()
    assert np.allclose(r1["temperature"], np.float32(temps[-1]))
    assert all(len(r) > 4 for r in r1["win_tokens"])
    # a threshold in the widest gap between the attempt-0 averages
    a0 = np.sort(r0["avg_logprob"].astype(np.float64))
    i = int(np.argmax(np.diff(a0)))
    thr = float(0.5 * (a0[i] + a0[i + 1]))
    below = r0["avg_logprob"] < thr
    assert 0 < below.sum() < nW
    mid = wb.FallbackParams(temps, best_of, thr, None, None, seed, -1)
    r2 = wb.waveform_to_tokens_fallback(eng, st, audio, 16000, params=params, fallback=mid)
    assert ((r2["attempts"] > 1) == below).all(), (r2["attempts"], below)
    for w in range(nW):
        if not below[w]:
            assert r2["win_tokens"][w] == wins[w] and r2["attempts"][w] == 1 and r2["status"][w] == 0
            assert r2["avg_logprob"][w] == r0["avg_logprob"][w]
        else:
            assert r2["temperature"][w] > 0 and (r2["status"][w] == 0) == (r2["avg_logprob"][w] >= np.float32(thr))
    # the ratio callback sees the generated tokens; a ratio above the threshold alone asks for the retry
    seen = []
    cr = wb.FallbackParams(temps[:2], best_of, None, None, 2.4, seed, -1)
    r3 = wb.waveform_to_tokens_fallback(eng, st, audio, 16000, params=params, fallback=cr,
                                        ratio=lambda t: (seen.append(list(t)), 3.0)[1])
    assert (r3["attempts"] == 2).all() and (r3["status"] == 1).all() and np.allclose(r3["ratio"], 3.0)
    assert seen[:nW] == [[t for t in w[4:] if t != st.end_of_text] for w in wins]
    # sharded: two calls over [0, k) and [k, n) give the rows, and the per-window outputs, of the whole call
    k = nW // 2
    parts = [wb.waveform_to_tokens_fallback(eng, st, audio, 16000, params=params, win_begin=lo, win_end=hi, fallback=mid)
             for lo, hi in ((0, k), (k, nW))]
    assert parts[0]["win_tokens"] + parts[1]["win_tokens"] == r2["win_tokens"]
    for key in ("attempts", "status", "temperature", "avg_logprob"):
        assert np.array_equal(np.concatenate([parts[0][key], parts[1][key]]), r2[key]), key
    return r0, r1, r2


def oracle_sample(oracle, st, enc, T, seed, stream, attempt, max_depth, mask_until_len=5):
    """The oracle alone, sampling by the same rule: (row, positions, positions whose top-two key gap is at most delta_model).
    What the parity tests' exclusion cap is checked against before any device runs."""
    import torch
    row = [st.start_of_transcript, st.language, st.transcribe, st.no_timestamps]
    maskv = np.where(np.asarray(st.is_special).astype(bool), -np.inf, 0.0)
    enc_t = torch.as_tensor(np.asarray(enc))[None]
    n = ex = 0
    for _ in range(max_depth):
        x = oracle.forward_decoder(torch.tensor([row], dtype=torch.long), enc_t)[0, -1].double().numpy()
        l = len(row)
        mk = maskv if l <= mask_until_len else None
        M, lse = row_stats(x, mk)
        d = draw(x, mk, M, lse, T, seed, stream, attempt, l)
        n += 1
        ex += not (d["gap"] > 2e-3 / T + delta_op(d["A"], T))
        row.append(d["token"])
        if d["token"] == st.end_of_text:
            break
    return row, n, ex
