"""Whisper's timestamp rules restated in f64 NumPy (the checker side of csrc/tsrules.hip, wb_timestamp_rows and
wb_session_decode_timestamps), written from the contract in include/whisper_hip.h; the exclusion bounds of the parity tests,
the inputs of the operator test, the micro fixture of the session tests and pure-Python restatements of the segment slicing
and the seek loop."""
import numpy as np

import sample_ref as sr

I31 = sr.I31
MUTANTS = ("no_pairs", "c_plus1", "f_ge", "f_suppressed", "d_keeps_eot")


def rules(tb, n_ts, max_init=50, max_ts=-1):
    return dict(tb=int(tb), n_ts=int(n_ts), max_init=int(max_init), max_ts=int(max_ts))


def is_ts(R, v):
    return R["tb"] <= v < R["tb"] + R["n_ts"]


def history(R, gen):
    """(n_gen, prev1, prev2, last_ts) of a generated list: the per-row state the hook takes."""
    ts = [t for t in gen if is_ts(R, t)]
    return len(gen), (gen[-1] if len(gen) >= 1 else -1), (gen[-2] if len(gen) >= 2 else -1), (ts[-1] if ts else -1)


def allowed(V, R, eot, suppress, suppress_first, gen, mut=None):
    """bool [V]: the allowed set of the position behind `gen` by rules (a) - (e) and the static masks (before rule (f))."""
    tb, n_ts = R["tb"], R["n_ts"]
    ids = np.arange(V)
    T = (ids >= tb) & (ids < tb + n_ts)
    ok = np.ones(V, dtype=bool)
    if suppress is not None:
        ok &= np.asarray(suppress) == 0
    if len(gen) == 0 and suppress_first is not None:
        ok &= np.asarray(suppress_first) == 0
    last_was = len(gen) >= 1 and is_ts(R, gen[-1])
    penult_was = len(gen) < 2 or is_ts(R, gen[-2])
    case_a, case_b = last_was and penult_was, last_was and not penult_was
    if mut != "no_pairs":
        if case_a:
            ok &= ~T                                                    # (a)
        if case_b:
            ok &= ~((ids < eot) & ~T)                                   # (b)
    ts = [t for t in gen if is_ts(R, t)]
    if ts:                                                              # (c)
        t_min = ts[-1] if (case_b and mut != "c_plus1") else ts[-1] + 1
        ok &= ~(T & (ids < t_min))
    if len(gen) == 0 and n_ts > 0:                                      # (d)
        keep = (ids == eot) if mut == "d_keeps_eot" else np.zeros(V, dtype=bool)
        ok &= T | keep
        if R["max_init"] >= 0:
            ok &= ~(T & (ids > tb + R["max_init"]))
    if R["max_ts"] >= 0:                                                # (e)
        ok &= ~(T & (ids > tb + R["max_ts"]))
    return ok, T


def _lse(v):
    if len(v) == 0:
        return -np.inf
    m = v.max()
    return float(m + np.log(np.exp(v - m).sum())) if np.isfinite(m) else float(m)


def lse_err(n, A, mag):
    """Error bound of one device (max, sum) statistic m + logf(s) over n terms whose logits span at most A below the maximum:
    every term enters the sum through one expf of a rounded difference (2 ulp of expf + A 2^-24 relative from the rounding of
    the argument) and at most one rescale + one add (2 roundings), along a fixed path of at most D operations -- 4 ceil(V /
    4096) elements per thread, 6 butterfly steps, 15 folds of the waves -- of non-negative terms, so the relative error of
    s is at most D (2^-22 + (A + 2) 2^-24); logf adds 2 ulp of its result (|log s| <= log n) and the final sum one rounding
    of a number of magnitude `mag`."""
    D = 4 * ((n + 4095) // 4096) + 6 + 15 + 2
    return D * (2.0 ** -22 + (A + 2.0) * 2.0 ** -24) + 2.0 ** -22 * (1.0 + np.log(max(n, 2))) + 2.0 ** -23 * (abs(mag) + 1.0)


def delta_op(V, A, mag, T):
    """(bound on |ts_lse - mN|, bound on the top-two key gap) below which a device decision may differ from f64.
    ts_lse: lse_err above (mN is an exact maximum), doubled for the pair and again as margin.  Keys: at T = 0 the key is
    the logit itself -- exact, ties go to the lower id on both sides, bound 0; at T > 0 sample_ref.delta_op (two one-ulp
    logf, three f32 roundings, doubled twice)."""
    return 4.0 * lse_err(V, A, mag), (sr.delta_op(A, T) if T > 0 else 0.0)


def decide(x, ok, Tm, T=0.0, seed=0, stream=0, attempt=0, position=0, mut=None, sup_ok=None):
    """f64 restatement of rule (f), the pick and the recorded log-prob over an allowed set `ok`."""
    x = np.asarray(x, dtype=np.float64)
    V = len(x)
    ok = ok & (x > -np.inf)
    okT, okN = ok & Tm, ok & ~Tm
    fT, fN = (okT, okN)
    if mut == "f_suppressed":           # rule (f) over the ids the rules allow, the static masks forgotten
        fT, fN = sup_ok[0] & Tm & (x > -np.inf), sup_ok[0] & ~Tm & (x > -np.inf)
    ts_lse = _lse(x[fT])
    mN = float(x[fN].max()) if fN.any() else -np.inf
    forced = bool(ts_lse >= mN) if mut == "f_ge" else bool(ts_lse > mN)
    final = okT if forced else ok
    if not final.any():
        return dict(token=None, forced=forced, ts_lse=ts_lse, mN=mN, final=final)
    if T > 0:
        M = np.float32(np.nanmax(x.astype(np.float32)))
        key = sr.keys(x.astype(np.float32), None, M, T, seed, stream, attempt, position)
    else:
        key = x.copy()
    key = np.where(final, key, -np.inf)
    order = np.lexsort((np.arange(V), -key))
    tok = int(order[0])
    gap = float(key[order[0]] - key[order[1]]) if final.sum() > 1 else np.inf
    lse_all = _lse(x[final])
    xs = x[np.isfinite(x)]
    A = float(xs.max() - xs.min())
    fgap = abs(ts_lse - mN) if (okT.any() and okN.any()) else np.inf
    return dict(token=tok, forced=forced, ts_lse=ts_lse, mN=mN, final=final, gap=gap, fgap=fgap, A=A, lse=lse_all,
                logprob=float(x[tok] - lse_all), x_tok=float(x[tok]))


def step(x, R, eot, suppress, suppress_first, gen, T=0.0, seed=0, stream=0, attempt=0, position=0, mut=None):
    V = len(x)
    ok, Tm = allowed(V, R, eot, suppress, suppress_first, gen, mut)
    sup_ok = allowed(V, R, eot, None, None, gen, mut) if mut == "f_suppressed" else None
    return decide(x, ok, Tm, T, seed, stream, attempt, position, mut, sup_ok)


def is_excluded(d, V, T, model=False):
    """The device may decide this position differently: |ts_lse - mN| or the top-two key gap inside delta_op (delta_model =
    2e-3 + delta_op against the oracle: the 1e-3 log-prob gate of DESIGN.md section 5, once per side; a key is a logit / T)."""
    mag = max(abs(d["ts_lse"]) if np.isfinite(d["ts_lse"]) else 0.0, abs(d["mN"]) if np.isfinite(d["mN"]) else 0.0)
    df, dk = delta_op(V, d["A"], mag, T)
    if model:
        df, dk = df + 2e-3, dk + 2e-3 / (T if T > 0 else 1.0)
    return (not d["fgap"] > df) or (T > 0 or model) and (not d["gap"] > dk)


def logprob_bound(d, V):
    mag = max(abs(d["lse"]), abs(d["x_tok"]))
    return 3.0 * lse_err(V, d["A"], mag) + 2.0 ** -21 + 2.0 ** -23 * (abs(d["x_tok"]) + abs(d["logprob"]))


def stats_bound(d, V):
    return lse_err(V, d["A"], abs(d["ts_lse"]) if np.isfinite(d["ts_lse"]) else 0.0)


# ---- the operator test's inputs ------------------------------------------------------------------------------------------------
SHAPES = [(1, 263), (5, 1031), (33, 7001), (3, 51865)]
TEMPS = [0.0, 0.2, 1.0]
PAD = 5
HISTORIES = ("empty", "ts", "ts_ts", "text_ts", "ts_text", "long", "top")


def make_history(kind, R, text_id, rng):
    """A generated list of one of the history classes over the rules R (text_id: a non-timestamp id below end-of-text)."""
    tb, n = R["tb"], R["n_ts"]
    if n == 0:
        return {"empty": []}.get(kind, [text_id] * (1 + HISTORIES.index(kind) % 3))
    t = lambda i: tb + min(i, n - 1)
    a = int(rng.integers(0, max(n // 3, 1)))
    return {"empty": [], "ts": [t(a)], "ts_ts": [t(a), t(a + 2)], "text_ts": [text_id, t(a)], "ts_text": [t(a), text_id],
            "long": [t(0), text_id, t(a), t(a), text_id, t(a + 1)], "top": [t(a), text_id, t(n - 1)]}[kind]


def layout(V, where, n_ts=None):
    """(tb, n_ts, eot) of a vocabulary size: T on top of the id range (the real vocabulary at 51865) or inside it."""
    if V == 51865 and where == "top" and n_ts is None:
        return 50364, 1501, 50257
    n = min(1501, max(V // 6, 8)) if n_ts is None else n_ts
    if where == "top":
        return V - n, n, V - n - 2
    return V // 3, n, V - 2


# (name, where, n_ts, max_init, max_ts, suppress kind, temperature): every shape runs all of them
VARIANTS = [("top_T0", "top", None, 50, -1, "specials", 0.0), ("top_T02", "top", None, 50, -1, "specials", 0.2),
            ("in_T1", "inside", None, 50, -1, "specials", 1.0), ("in_T0_init0", "inside", None, 0, -1, "none", 0.0),
            ("top_T0_nolimit", "top", None, -1, -1, "random", 0.0), ("in_T02_cut", "inside", None, -1, 5, "specials", 0.2),
            ("top_T0_cut", "top", None, 50, 3, "none", 0.0), ("nts0_T1", "inside", 0, 50, -1, "specials", 1.0),
            ("nts0_T0", "top", 0, -1, -1, "none", 0.0), ("nts1_T0", "inside", 1, 50, -1, "specials", 0.0),
            ("nts1_T1", "top", 1, -1, -1, "random", 1.0), ("single_T0", "inside", None, 50, -1, "single", 0.0),
            ("single_T1", "top", None, 50, -1, "single", 1.0),
            # a suppress that leaves exactly ONE id: a text id (every history ends on case (a) or on text), a timestamp (the top
            # one; histories that leave T open), each greedy and drawn
            ("one_text_T0", "inside", None, 50, -1, "one_text", 0.0), ("one_text_T1", "top", None, 50, -1, "one_text", 1.0),
            ("one_ts_T0", "top", None, -1, -1, "one_ts", 0.0), ("one_ts_T02", "inside", None, -1, -1, "one_ts", 0.2)]
ONE_ID_HISTORIES = {"one_text": ("ts", "ts_text", "ts_ts"), "one_ts": ("empty", "text_ts", "ts_text", "long")}


def make_cases(shape, seed=0):
    R, V = shape
    out = []
    for vi, (name, where, n_ts, max_init, max_ts, sup_kind, T) in enumerate(VARIANTS):
        g = np.random.default_rng([seed, R, V, vi])
        tb, n, eot = layout(V, where, n_ts)
        Rl = rules(tb, n, max_init, max_ts)
        x = (g.standard_normal((R, V)) * 3.0).astype(np.float32)
        x[:, tb:tb + n] += g.uniform(-3.0, 5.0, (R, 1)).astype(np.float32)      # timestamps win rule (f) in some rows only
        sup = np.zeros(V, dtype=np.uint8)
        sup1 = np.zeros(V, dtype=np.uint8)
        text_id = 7
        if sup_kind == "specials":
            sup[eot + 1:eot + 1 + min(14, V - eot - 1)] = 1
            sup[tb:tb + n] = 0
            sup1[eot] = 1
            sup1[3] = 1
        elif sup_kind == "random":
            sup[g.random(V) < 0.5] = 1
            sup[[eot, text_id]] = 0
            sup[tb:tb + n:2] = 0
        elif sup_kind == "single":           # the masks leave one text id, end-of-text and one timestamp in three
            sup[:] = 1
            sup[[text_id, eot]] = 0
            sup[tb:tb + n:3] = 0
        elif sup_kind in ONE_ID_HISTORIES:   # the mask leaves ONE id
            sup[:] = 1
            sup[text_id if sup_kind == "one_text" else tb + n - 1] = 0
        pool = ONE_ID_HISTORIES.get(sup_kind, HISTORIES)
        gens = [make_history(pool[(r + vi) % len(pool)], Rl, text_id, g) for r in range(R)]
        stream = g.integers(0, I31, R).astype(np.int64)
        position = g.integers(0, 448, R).astype(np.int64)
        stream[0], position[0] = (0, I31) if vi % 2 == 0 else (I31, 0)
        if R > 1:
            stream[1], position[1] = I31, I31
        if R > 2:
            stream[2], position[2] = 0, 0
        logits = np.full((R, V + PAD), np.nan, dtype=np.float32)
        logits[:, :V] = x
        out.append(dict(name=f"R{R}_V{V}_{name}", kind=sup_kind, R=R, V=V, T=T, rules=Rl, eot=eot, logits=logits, suppress=sup, suppress_first=sup1,
                        gens=gens, seed=int(g.integers(0, 2 ** 63)) | (1 << 40), attempt=(0, I31, 3)[vi % 3],
                        stream=stream.astype(np.int32), position=position.astype(np.int32)))
    return out


def reference(case, mut=None):
    V = case["V"]
    return [step(case["logits"][r, :V], case["rules"], case["eot"], case["suppress"], case["suppress_first"], case["gens"][r],
                 case["T"], case["seed"], int(case["stream"][r]), case["attempt"], int(case["position"][r]), mut)
            for r in range(case["R"])]


def excluded(case, ref):
    return np.array([d["token"] is not None and is_excluded(d, case["V"], case["T"]) for d in ref])


def run_hook(case, rows=None, device=0, logits=None):
    import whisper_burn_amd as wb
    sel = np.arange(case["R"]) if rows is None else np.asarray(rows)
    Rl = case["rules"]
    tp = wb.TimestampParams(Rl["tb"], Rl["n_ts"], Rl["max_init"], Rl["max_ts"], temperature=case["T"], seed=case["seed"],
                            attempt=case["attempt"])
    h = np.array([history(Rl, case["gens"][r]) for r in sel], dtype=np.int32).reshape(len(sel), 4)
    x = case["logits"] if logits is None else logits
    return wb.timestamp_rows(x[sel], tp, h[:, 0], h[:, 1], h[:, 2], h[:, 3], case["stream"][sel], case["position"][sel],
                             case["eot"], V=case["V"], suppress=case["suppress"], suppress_first=case["suppress_first"], device=device)


def check_hook_case(case, ref=None, record=None):
    """The hook against the f64 restatement: token and `forced` wherever the row is not excluded (at most 1 % of the rows may
    be), the log-prob and the (ts_lse, mN) statistics within their bounds, no error word."""
    ref = ref or reference(case)
    tok, lp, forced, stats, err = run_hook(case)
    ex = excluded(case, ref)
    V = case["V"]
    margins = []
    assert err == 0, case["name"]
    assert ex.sum() <= 0.01 * case["R"], (case["name"], int(ex.sum()))
    for r, d in enumerate(ref):
        assert d["token"] is not None, (case["name"], r)
        sb = stats_bound(d, V)
        for got, want in ((stats[r, 0], d["ts_lse"]), (stats[r, 1], d["mN"])):
            if np.isfinite(want):
                assert abs(float(got) - want) <= sb, (case["name"], r, float(got), want, sb)
                margins.append(abs(float(got) - want) / sb)
            else:
                assert float(got) == want, (case["name"], r, float(got), want)
        if ex[r]:
            continue
        assert tok[r] == d["token"] and bool(forced[r]) == d["forced"], (case["name"], r, int(tok[r]), d["token"], int(forced[r]),
                                                                           d["forced"], d["fgap"], d["gap"])
        lb = logprob_bound(d, V)
        assert abs(float(lp[r]) - d["logprob"]) <= lb, (case["name"], r, float(lp[r]), d["logprob"], lb)
        margins.append(abs(float(lp[r]) - d["logprob"]) / lb)
        assert d["final"][tok[r]]
        if case["kind"] in ONE_ID_HISTORIES:      # one admissible id: one class is empty, the other holds a single term
            only = int(np.flatnonzero(case["suppress"] == 0)[0])
            x_only = float(case["logits"][r, only])
            assert d["final"].sum() == 1 and tok[r] == only and float(lp[r]) == 0.0, (case["name"], r, int(tok[r]), float(lp[r]))
            if case["kind"] == "one_text":
                assert forced[r] == 0 and stats[r, 0] == -np.inf and float(stats[r, 1]) == x_only, (case["name"], r, stats[r])
            else:
                assert forced[r] == 1 and float(stats[r, 0]) == x_only and stats[r, 1] == -np.inf, (case["name"], r, stats[r])
    if record is not None:
        record.append((case["name"], int(ex.sum()), round(max(margins), 4)))
    return tok, lp, forced, stats


# ---- the micro fixture of the session tests ----------------------------------------------------------------------------------
FIX_V, FIX_TB, FIX_NTS, FIX_DEPTH = 1031, 800, 151, 40
FIX_OFFSETS = (0, 8000, 16000, 24000)        # 1 s windows of synth_audio(48000, 3); the first three are the fixture proper
SESSION_DRAWS = [(0.0, 0, 0), (1.0, 1234, 2), (0.2, 99, 1)]


def fixture():
    """(weights, special tokens, audio, rules, suppress, prompt) of the micro fixture."""
    from whisper_burn_amd import synth
    from whisper_burn_amd.tokens import SpecialTokens
    dims = synth.micro_dims(n_state=64, n_head=1, n_layer=1, n_vocab=FIX_V)
    weights = synth.synth_weights(dims, seed=5)
    st = SpecialTokens.for_vocab(FIX_V)
    sup = (np.asarray(st.is_special) != 0).astype(np.uint8)
    sup[st.end_of_text] = 0
    return weights, st, synth.synth_audio(48000, 3), rules(FIX_TB, FIX_NTS, 50, -1), sup, [st.start_of_transcript, st.language, st.transcribe]


def fixture_encs(o32, audio, W=3, padding=10):
    import torch
    from oracle import mel as omel
    encs = []
    for off in FIX_OFFSETS[:W]:
        m = omel.prep_audio(torch.from_numpy(audio[off:off + 16000])[None])
        encs.append(o32.forward_encoder(torch.nn.functional.pad(m, (0, padding)))[0].numpy())
    return encs


def oracle_decode(oracle, enc, prompt, R, eot, suppress, suppress_first, depth, T=0.0, seed=0, stream=0, attempt=0):
    """The oracle alone under the rules: (row, per-position decide() dicts with the rule flags that fired)."""
    import torch
    row = list(prompt)
    enc_t = torch.as_tensor(np.asarray(enc))[None]
    P, out = len(prompt), []
    for _ in range(depth):
        x = oracle.forward_decoder(torch.tensor([row], dtype=torch.long), enc_t)[0, -1].double().numpy()
        gen = row[P:]
        d = step(x, R, eot, suppress, suppress_first, gen, T, seed, stream, attempt, len(row))
        last_was = len(gen) >= 1 and is_ts(R, gen[-1])
        penult = len(gen) < 2 or is_ts(R, gen[-2])
        d["fired"] = dict(a=last_was and penult, b=last_was and not penult, c=any(is_ts(R, t) for t in gen), d=len(gen) == 0,
                          f_forced=d["forced"], f_free=not d["forced"])
        out.append(d)
        row.append(d["token"])
        if d["token"] == eot:
            break
    return row, out


def oracle_row_check(oracle, enc, row, P, R, eot, suppress, suppress_first, T, seed, stream, attempt):
    """A device row against ONE teacher-forced pass of the oracle over it (sample_ref.oracle_row_check's scheme): returns
    (positions, excluded, mismatches, f64 sum of the oracle's log-probs under the filters of the row's tokens)."""
    import torch
    toks = torch.tensor([list(row)], dtype=torch.long)
    logits = oracle.forward_decoder(toks, torch.as_tensor(np.asarray(enc))[None])[0].double().numpy()
    n = ex = bad = 0
    total = 0.0
    for l in range(P, len(row)):
        x = logits[l - 1]
        d = step(x, R, eot, suppress, suppress_first, list(row[P:l]), T, seed, stream, attempt, l)
        n += 1
        if d["final"][row[l]]:
            total += float(x[row[l]] - _lse(x[d["final"]]))
        if is_excluded(d, len(x), T, model=True):
            ex += 1
            if not (allowed(len(x), R, eot, suppress, suppress_first, list(row[P:l]))[0][row[l]]):
                bad += 1                                   # excluded or not, a token outside rules (a) - (e) is a mismatch
        elif d["token"] != row[l]:
            bad += 1
    return n, ex, bad, total


def check_invariants(gen, R, eot, suppress):
    """What every row decoded under the rules satisfies outright."""
    assert len(gen) >= 1 and is_ts(R, gen[0]) and (R["max_init"] < 0 or gen[0] <= R["tb"] + R["max_init"]), gen
    ts = [t for t in gen if is_ts(R, t)]
    assert ts == sorted(ts), gen
    assert not any(suppress[t] for t in gen), gen
    body = gen[:-1] if gen[-1] == eot else gen
    flags = [is_ts(R, t) for t in body]
    for i, f in enumerate(flags):       # no lone timestamp between text: a timestamp with text on both sides has a timestamp neighbour
        if f and 0 < i < len(flags) - 1:
            assert flags[i - 1] or flags[i + 1], gen
    assert eot not in gen[:-1], gen


def check_ts_session(sess, oracle, st, params, R, suppress, T, seed, attempt, best_of, stream_ids=None, active=None,
                     max_excluded=0.05, record=None):
    """One decode_timestamps on a rewound / fresh session against the teacher-forced oracle: every sequence of every active
    window token by token outside the exclusion rule, its f64 sum within 1e-3 per token, the invariants outright, the returned
    row = the sequence of out_best = the first argmax of sum / n_text.  Returns (rows, sums, best)."""
    import whisper_burn_amd as wb
    W = sess.n_windows
    prompt = [st.start_of_transcript, st.language, st.transcribe]
    tp = wb.TimestampParams(R["tb"], R["n_ts"], R["max_init"], R["max_ts"], temperature=T, best_of=best_of, seed=seed, attempt=attempt)
    rows, sums, best = sess.decode_timestamps(params, tp, stream_ids=stream_ids, active=active)
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
            assert 1 <= len(gen) <= params.max_depth, (w, j, gen)
            check_invariants(gen, R, st.end_of_text, suppress)
            base = stream_ids[w] if stream_ids is not None else w * best_of
            a, b, c, total = oracle_row_check(oracle, enc, prompt + gen, 3, R, st.end_of_text, suppress, None, T, seed, base + j, attempt)
            n, ex, bad = n + a, ex + b, bad + c
            assert abs(sums[w, j] - total) <= 1e-3 * len(gen), (w, j, sums[w, j], total)
            nt = sr.n_text(gen, st.end_of_text)
            ranks.append(sums[w, j] / nt if nt > 0 else -np.inf)
        assert best[w] == int(np.argmax(ranks)), (w, ranks, best[w])
        assert rows[w] == prompt + gens[w][best[w]], w
    if record is not None:
        record.append((T, best_of, n, ex, bad))
    assert bad == 0, (n, ex, bad)
    assert ex <= max_excluded * n, (n, ex)
    return rows, sums, best


# ---- segments and the seek loop, restated -----------------------------------------------------------------------------------
def segments_ref(tokens, R, eot, window_index, spt=0.02):
    """Whisper transcribe()'s slicing: ([(begin, end, start_index, end_index)], advance index)."""
    toks = list(tokens)
    if eot in toks:
        toks = toks[:toks.index(eot)]
    f = [is_ts(R, t) for t in toks]
    single = len(f) >= 1 and f[-1] and (len(f) < 2 or not f[-2])
    slices = [i for i in range(1, len(f)) if f[i - 1] and f[i]]
    segs, adv = [], window_index
    if slices:
        if single:
            slices.append(len(toks))
        last = prev_end = 0
        for cur in slices:
            i0 = toks[last] - R["tb"] if f[last] else prev_end
            i1 = toks[cur - 1] - R["tb"]
            segs.append((last, cur, i0, i1))
            last, prev_end = cur, i1
        if not single:
            adv = toks[last - 1] - R["tb"]
    elif toks:
        dur = window_index
        tsl = [t for t in toks if is_ts(R, t)]
        if tsl and tsl[-1] != R["tb"]:
            dur = tsl[-1] - R["tb"]
        segs.append((0, len(toks), 0, dur))
    return segs, adv


def seek_loop_ref(n, wlen, rate, spt, decode, R, eot):
    """The seek loop over a waveform of n samples: decode(seek, len, window_index) -> generated tokens.  Returns (segments
    [(start s, end s, text tokens)], text stream, seeks)."""
    seek, segs, text, seeks = 0, [], [], []
    per = float(np.float32(spt)) * rate
    while n - seek >= 400:
        ln = min(wlen, n - seek)
        wi = int(ln / per)
        gen = decode(seek, ln, wi)
        seeks.append(seek)
        ss, adv = segments_ref(gen, R, eot, wi)
        for b, e, i0, i1 in ss:
            tt = [t for t in gen[b:e] if not is_ts(R, t)]
            segs.append((seek / rate + i0 * spt, seek / rate + i1 * spt, tt))
            text += tt
        stepn = int(round(adv * per))
        if stepn <= 0:
            stepn = ln
        seek += min(stepn, ln)
    return segs, text, seeks


# ---- procedures shared by the functional-model checks and the GPU tests ---------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def check_hook_determinism(case):
    """Bit-identical on repeat, with the rows reversed and with every row alone; a NaN row ends on end-of-text with the error
    word raised and leaves the other rows untouched."""
    a, b = run_hook(case), run_hook(case)
    R = case["R"]
    for i in range(4):
        assert np.array_equal(bits(a[i]), bits(b[i])), (case["name"], i)
    rev = run_hook(case, rows=np.arange(R)[::-1])
    for i in range(4):
        assert np.array_equal(bits(rev[i][::-1]), bits(a[i])), (case["name"], i)
    for r in range(R):
        one = run_hook(case, rows=[r])
        for i in range(4):
            assert np.array_equal(bits(one[i][0]), bits(a[i][r])), (case["name"], r, i)
    if R > 2:
        x = case["logits"].copy()
        x[2, 17] = np.nan
        tok, lp, forced, stats, err = run_hook(case, logits=x)
        assert err == 1 and tok[2] == case["eot"] and lp[2] == 0 and forced[2] == 0
        for got, ref in ((tok, a[0]), (lp, a[1]), (forced, a[2]), (stats, a[3])):
            assert np.array_equal(bits(np.delete(got, 2, axis=0)), bits(np.delete(ref, 2, axis=0))), case["name"]


def check_hook_no_admissible_id(case):
    """A row the masks and the rules leave NO id (a one-text-id suppress at the first position, where rule (d) removes the text)
    ends on end-of-text with log-prob 0, `forced` 0 and the error word raised; the other rows are untouched."""
    assert case["kind"] == "one_text" and case["rules"]["n_ts"] > 0
    a = run_hook(case)
    c = dict(case)
    c["gens"] = [[]] + list(case["gens"][1:])
    assert step(c["logits"][0, :c["V"]], c["rules"], c["eot"], c["suppress"], c["suppress_first"], [])["token"] is None
    tok, lp, forced, stats, err = run_hook(c)
    assert err == 1 and tok[0] == case["eot"] and lp[0] == 0 and forced[0] == 0, (int(tok[0]), float(lp[0]), err)
    assert stats[0, 0] == -np.inf and stats[0, 1] == -np.inf
    assert a[4] == 0
    for got, ref in zip((tok, lp, forced, stats), a[:4]):
        assert np.array_equal(bits(got[1:]), bits(ref[1:])), case["name"]


def fixture_session(eng, audio, W, max_beams):
    import whisper_burn_amd as wb
    starts = np.array(FIX_OFFSETS[:W], dtype=np.int64)
    return wb.Session.begin(eng, audio, starts, np.full(W, 16000, dtype=np.int64), max_beams=max_beams)


def check_session_shape(eng, o32, W, best_of, record=None):
    """The session checks of one launch shape on the micro fixture: parity with the teacher-forced oracle for every draw of
    SESSION_DRAWS the shape admits, identical bits after a rewind, no capture for another temperature / seed / rule
    parameter, `active` leaves the other windows untouched."""
    import whisper_burn_amd as wb
    weights, st, audio, R, sup, prompt = fixture()
    sess = fixture_session(eng, audio, W, max(best_of, 1))
    sess.set_suppress(sup)
    p = wb.decode_params(st, 1, FIX_DEPTH)
    draws = [d for d in SESSION_DRAWS if d[0] > 0 or best_of == 1]
    T1, seed1, att1 = draws[0]
    r1 = check_ts_session(sess, o32, st, p, R, sup, T1, seed1, att1, best_of, record=record)
    n_graphs, n_cap = sess.graph_count(), sess.graph_captures()
    assert n_graphs >= 1 and n_cap >= n_graphs
    sess.rewind()
    r2 = check_ts_session(sess, o32, st, p, R, sup, T1, seed1, att1, best_of)                 # again: bit-identical
    assert r1[0] == r2[0] and np.array_equal(r1[1], r2[1]) and np.array_equal(r1[2], r2[2])
    for T, seed, att in draws[1:]:
        sess.rewind()
        check_ts_session(sess, o32, st, p, R, sup, T, seed, att, best_of, record=record)      # another temperature, seed, attempt
        assert sess.graph_count() == n_graphs and sess.graph_captures() == n_cap             # ... captures nothing
    sess.rewind()
    R2 = dict(R, max_init=20, max_ts=120)                                                     # other rule parameters: no capture either
    check_ts_session(sess, o32, st, p, R2, sup, T1, seed1, att1, best_of)
    assert sess.graph_count() == n_graphs and sess.graph_captures() == n_cap
    sess.rewind()
    act = np.ones(W, dtype=np.uint8); act[1] = 0
    ids = [7 * w + 100 for w in range(W)]
    check_ts_session(sess, o32, st, p, R, sup, T1, seed1, att1, best_of, stream_ids=ids, active=act)
    sess.close()
    return r1


def check_rules_off(eng, W=3, depth=20):
    """n_timestamps = 0, no suppress masks, max_initial = -1: at T = 1 the rows are decode_sample's for the same seed / stream /
    attempt with mask_until_len = 0, at T = 0 they are Session.decode's (beam 1, mask_until_len = 0)."""
    import whisper_burn_amd as wb
    weights, st, audio, R, sup, prompt = fixture()
    prompt4 = prompt + [st.no_timestamps]
    p = wb.decode_params(st, 1, depth, mask_until_len=0)
    none = np.zeros(FIX_V, dtype=np.uint8)
    sess = fixture_session(eng, audio, W, 3)
    sess.set_special_mask(st.is_special)
    sess.set_suppress(none)
    smp = sess.decode_sample(p, wb.SampleParams(1.0, 3, 4321, 2))
    smp_all = sess.last_samples(3, depth)
    sess.rewind()
    ts = sess.decode_timestamps(p, wb.TimestampParams(0, 0, -1, -1, temperature=1.0, best_of=3, seed=4321, attempt=2), prompt=prompt4)
    assert sess.last_samples(3, depth) == smp_all                      # every sample, token for token
    assert np.array_equal(ts[2], smp[2]) and ts[0] == smp[0]
    assert np.abs(ts[1] - smp[1]).max() <= 1e-3 * depth                # (two roundings of the same log-softmax)
    sess.close()
    sess = fixture_session(eng, audio, W, 1)
    sess.set_special_mask(st.is_special)
    sess.set_suppress(none)
    greedy = sess.decode(p)
    sess.rewind()
    ts0 = sess.decode_timestamps(p, wb.TimestampParams(0, 0, -1, -1), prompt=prompt4)
    assert ts0[0] == greedy, (ts0[0], greedy)
    sess.close()


def short_context_engine():
    import whisper_burn_amd as wb
    from whisper_burn_amd import synth
    dims = synth.micro_dims(n_state=64, n_head=1, n_layer=1, n_vocab=FIX_V, n_audio_ctx=400)
    return wb.Whisper.from_tensors(synth.synth_weights(dims, seed=5))


def check_seek_loop(eng, seconds=16, depth=24):
    """waveform_to_segments on the short-context model: the segments tile the token stream in order, times are non-decreasing
    and inside the audio, the loop ends after at least 4 windows, and the whole result equals the pure-Python seek loop
    driven by per-window decode_timestamps at the same seeks."""
    import whisper_burn_amd as wb
    from whisper_burn_amd import synth
    _, st, _, R, sup, prompt = fixture()
    audio = synth.synth_audio(16000 * seconds, 3)
    p = wb.decode_params(st, 1, depth)
    tp = wb.TimestampParams(R["tb"], R["n_ts"], R["max_init"], R["max_ts"])
    segs, toks, n_win = wb.waveform_to_segments(eng, st, audio, 16000, params=p, timestamps=tp, suppress=sup, suppress_first=None,
                                                prompt=prompt)
    assert n_win >= 4 and len(segs) >= n_win
    assert [t for s in segs for t in s["tokens"]] == toks
    assert not any(is_ts(R, t) or t == st.end_of_text for t in toks)
    dur = len(audio) / 16000.0
    last = 0.0
    for s in segs:
        assert -1e-6 <= s["start"] <= s["end"] + 1e-6 and s["end"] <= dur + 0.02 + 1e-6 and s["start"] >= last - 1e-5, (s, last)
        last = s["start"]
    wlen = wb.max_waveform_samples(eng.max_mel_frames() - p.padding)

    def decode(seek, ln, wi):
        sess = wb.Session.begin(eng, audio, np.array([seek], dtype=np.int64), np.array([ln], dtype=np.int64), max_beams=1,
                                padding=p.padding)
        sess.set_suppress(sup)
        wtp = wb.TimestampParams(R["tb"], R["n_ts"], R["max_init"], wi if (R["max_ts"] < 0 or R["max_ts"] > wi) else R["max_ts"])
        rows, _, _ = sess.decode_timestamps(p, wtp, prompt=prompt)
        sess.close()
        check_invariants(rows[0][len(prompt):], R, st.end_of_text, sup)
        return rows[0][len(prompt):]

    rsegs, rtoks, seeks = seek_loop_ref(len(audio), wlen, 16000, 0.02, decode, R, st.end_of_text)
    assert len(seeks) == n_win and seeks == sorted(set(seeks)) and rtoks == toks, (seeks, n_win)
    assert len(rsegs) == len(segs)
    for a, b in zip(rsegs, segs):
        assert abs(a[0] - b["start"]) < 1e-4 and abs(a[1] - b["end"]) < 1e-4 and a[2] == b["tokens"], (a, b)
    return segs, seeks


SCRIPTED_ROWS = [[0, -5, -6, 4, 4, -7, 9, 9, -8, 12, None], [0, -5, -6, 4, 4, -7, 9, 9, -8, None], [0, -5, -6, 7, None], [0, -5, -6],
                 [-5, -6, None], [None], [], [0, 0, None], [0, -5, 49, 49, None], [0, -5, 50, 50], [3, 3, 3, 3], [-5, 2, 2, -6, 4],
                 [0, -1, 5, 5, -2, None, 7, 7]]


def check_segments_hook(n_random=200):
    """wb_segments_from_tokens against segments_ref: scripted rows (no pair, a trailing single timestamp, zero advance, a
    timestamp equal to the window end, tokens behind end-of-text) and random ones.  In the scripted rows i >= 0 is timestamp
    i, i < 0 the text id -i, None end-of-text."""
    import whisper_burn_amd as wb
    R, eot, wi = rules(100, 51), 99, 50
    tp = wb.TimestampParams(100, 51)
    g = np.random.default_rng(5)
    rows = [[eot if t is None else (100 + t if t >= 0 else -t) for t in r] for r in SCRIPTED_ROWS]
    for _ in range(n_random):
        n = int(g.integers(0, 14))
        rows.append([int(g.choice([eot, 5, 6, 100 + int(g.integers(0, 51))], p=[0.05, 0.3, 0.2, 0.45])) for _ in range(n)])
    for r in rows:
        segs, adv = wb.segments_from_tokens(r, tp, eot, wi)
        rs, radv = segments_ref(r, R, eot, wi)
        assert adv == radv and len(segs) == len(rs), (r, segs, rs)
        for a, (b, e, i0, i1) in zip(segs, rs):
            assert (a["begin"], a["end"]) == (b, e) and abs(a["start"] - 0.02 * i0) < 1e-6 and abs(a["end_time"] - 0.02 * i1) < 1e-6, (r, a)
