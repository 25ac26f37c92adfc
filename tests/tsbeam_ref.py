"""Beam search under the timestamp rules restated in f64 NumPy (the checker side of csrc/tsbeam.hip and tsbeam_chain.cpp),
written from the contract in include/whisper_hip.h on top of tsrules_ref.step: the candidates of a live beam, one step of a
window (ranking, walk, finished store), the search, Whisper's finalize, the replay rule of the parity tests, the scripted
cases of the model-free hook and the procedures the functional-model checks and the GPU tests share."""
import numpy as np

import tsrules_ref as tr

MUTANTS = ("top_b", "no_break", "store_past_c", "state_by_index")
GATE = 2e-3          # the project's 1e-3 log-prob gate, once per side


def max_candidates(B, patience):
    return int(round(B * patience))                 # (Python rounds half to even)


def candidates(x, R, eot, suppress, suppress_first, hist, k):
    """(decide() dict, [(id, lp)] of the min(k, |allowed|) best allowed ids by (logit descending, id ascending))."""
    d = tr.step(x, R, eot, suppress, suppress_first, hist)
    if d["token"] is None:
        return d, []
    xs = np.asarray(x, dtype=np.float64)
    ids = np.flatnonzero(d["final"])
    order = ids[np.lexsort((ids, -xs[ids]))][:k]
    return d, [(int(v), float(xs[v] - d["lse"])) for v in order]


def new_beam():
    return dict(gen=[], hist=[], score=0.0)


def beam_step(beams, rows, R, eot, suppress, suppress_first, B, C, n_store, mut=None, k_extra=0):
    """One step of one window.  beams: dicts (gen, hist = the tokens the rule state derives from -- gen itself, except under a
    mutant --, score); rows: their logits.  Returns dict(live = the next beams (with `parent`), newly = [(tokens, score)] walked
    this step, stored = those that enter a store holding n_store, cands = [(score, beam, rank, token)] sorted, n_walked,
    decides = the decide() dict per beam)."""
    k = (B if mut == "top_b" else B + 1) + k_extra
    cands, decides = [], []
    for j, (b, x) in enumerate(zip(beams, rows)):
        d, cl = candidates(x, R, eot, suppress, suppress_first, b["hist"], k)
        decides.append(d)
        cands += [(b["score"] + lp, j, i, v) for i, (v, lp) in enumerate(cl)]
    order = sorted(cands, key=lambda c: (-c[0], c[1], c[2]))
    live, newly, n_walked = [], [], 0
    for sc, j, i, v in order:
        if len(live) >= B:
            if mut != "no_break":
                break
            if v == eot:
                newly.append((beams[j]["gen"] + [v], sc))
            continue
        n_walked += 1
        if v == eot:
            newly.append((beams[j]["gen"] + [v], sc))
        else:
            q = len(live)
            src = beams[q] if (mut == "state_by_index" and q < len(beams)) else beams[j]
            live.append(dict(gen=beams[j]["gen"] + [v], hist=src["hist"] + [v], score=sc, parent=j))
    room = len(newly) if mut == "store_past_c" else max(0, C - n_store)
    return dict(live=live, newly=newly, stored=newly[:room], cands=order, n_walked=n_walked, decides=decides)


def rank_of(tokens, score, eot, length_penalty=-1.0):
    n_text = len(tokens) - (1 if tokens and tokens[-1] == eot else 0)
    if length_penalty < 0:
        return score / n_text if n_text > 0 else -np.inf
    return score / ((5.0 + n_text) / 6.0) ** length_penalty


def finalize(store, live, B, eot, length_penalty=-1.0):
    """Whisper's finalize: (candidates [(tokens, score)], ranks, best index)."""
    out = list(store)
    if len(out) < B:
        for b in sorted(live, key=lambda b: -b["score"]):           # (stable: ties keep the lower beam index)
            if len(out) >= B:
                break
            out.append((b["gen"], b["score"]))
    ranks = [rank_of(t, s, eot, length_penalty) for t, s in out]
    return out, ranks, (int(np.argmax(ranks)) if out else -1)


def search(rows_of, R, eot, suppress, suppress_first, B, patience, max_depth, length_penalty=-1.0, mut=None, on_step=None):
    """One window.  rows_of(beams) -> the beams' logits rows.  Returns dict(cands, ranks, best, trace = per step dict(finished,
    beams = [(token, parent, score)]), store, live, events)."""
    C = max_candidates(B, patience)
    beams, store, trace = [new_beam()], [], []
    events = set()
    for depth in range(max_depth):
        st = beam_step(beams, rows_of(beams), R, eot, suppress, suppress_first, B, C, len(store), mut)
        if on_step is not None:
            on_step(depth, beams, st)
        walked = st["cands"][:st["n_walked"]]
        if any(c[3] == eot for c in walked):
            events.add("eot_walked")
        if any(c[3] == eot for c in st["cands"][st["n_walked"]:]):
            events.add("eot_dropped")
        if len(st["stored"]) < len(st["newly"]):
            events.add("store_filled_mid_list")
        store += st["stored"]
        trace.append(dict(finished=len(st["newly"]), beams=[(b["gen"][-1], b["parent"], b["score"]) for b in st["live"]]))
        beams = st["live"]
        if len(store) >= C or not beams:
            if not beams:
                events.add("no_live_beam")
            break
    cands, ranks, best = finalize(store, beams, B, eot, length_penalty)
    return dict(cands=cands, ranks=ranks, best=best, trace=trace, store=store, live=beams, events=events)


# ---- the replay rule ---------------------------------------------------------------------------------------------------------
def replay_excluded(beams, rows, R, eot, suppress, suppress_first, B):
    """Whether the device may form another next step than the restatement from these beams and rows: a live beam whose
    rule (f) sits inside delta_op + GATE; an adjacent score gap <= GATE in the sorted top-(B + 2) lists up to and including the
    first unwalked element; a rank-(B + 2) candidate (one the device does not hold) inside the walked prefix."""
    st = beam_step(beams, rows, R, eot, suppress, suppress_first, B, 1 << 30, 0, k_extra=1)
    V = len(rows[0])
    for d in st["decides"]:
        if d["token"] is None:
            return True
        mag = max(abs(d["ts_lse"]) if np.isfinite(d["ts_lse"]) else 0.0, abs(d["mN"]) if np.isfinite(d["mN"]) else 0.0)
        if not d["fgap"] > tr.delta_op(V, d["A"], mag, 0.0)[0] + GATE:
            return True
    prefix = st["cands"][:st["n_walked"] + 1]
    if any(c[2] == B + 1 for c in prefix[:st["n_walked"]]):
        return True
    return any(a[0] - b[0] <= GATE for a, b in zip(prefix, prefix[1:]))


# ---- the oracle alone ------------------------------------------------------------------------------------------------------------
def oracle_rows(oracle, enc, prompt, beams):
    import torch
    toks = torch.tensor([list(prompt) + b["gen"] for b in beams], dtype=torch.long)
    xa = torch.as_tensor(np.asarray(enc))[None].expand(len(beams), -1, -1)
    return list(oracle.forward_decoder(toks, xa)[:, -1].double().numpy())


def oracle_search(oracle, enc, prompt, R, eot, suppress, B, patience, depth, length_penalty=-1.0):
    """The oracle's own beam search of one window with the replay rule applied to every step: (search() dict, window-steps,
    excluded window-steps)."""
    count = [0, 0]

    def rows_of(beams):
        rows = oracle_rows(oracle, enc, prompt, beams)
        count[0] += 1
        count[1] += bool(replay_excluded(beams, rows, R, eot, suppress, None, B))
        return rows

    res = search(rows_of, R, eot, suppress, None, B, patience, depth, length_penalty)
    return res, count[0], count[1]


# ---- scripted cases of the model-free hook ----------------------------------------------------------------------------------
SCRIPT_V, SCRIPT_W, SCRIPT_DEPTH = 263, 3, 12
SCRIPT_CASES = [(1, 1.0, 1), (3, 1.0, 5), (3, 2.0, 11), (5, 1.0, 5), (5, 2.0, 15)]      # (B, patience, seed): seeds whose near-ties stay outside 2 SCORE_TOL
TIE_DEPTH = 2        # window 0: the two best text ids of every row at this depth carry the same logit, and beams that differ
                     # only in which of the two they took get identical rows from then on: exact score ties
DRY_DEPTH = 5        # window 2: every row at this depth allows end-of-text alone, so the window runs out of live beams


def script_setup():
    tb, n, eot = tr.layout(SCRIPT_V, "top")
    R = tr.rules(tb, n, 8, -1)
    sup = np.zeros(SCRIPT_V, dtype=np.uint8)
    sup[eot + 1:tb] = 1
    return R, eot, sup


def script_row(seed, B, w, gen, R, eot):
    """The logits of window w's beam with generated tokens `gen`: from 10 downwards in steps of U(0.25, 0.75) for the 12 best
    ids and of 0.25 behind them, clipped at -10 (so the rows span 20 and tsrules_ref's error bounds stay small), dealt to the
    ids at random: two logits of a row are either at least 0.25 apart or exactly equal.  End-of-text and a few timestamps are
    moved near the top now and then."""
    V, tb, n = SCRIPT_V, R["tb"], R["n_ts"]
    key = list(gen)
    pair = None
    if w == 0 and len(gen) > TIE_DEPTH:
        pair = script_tie_pair(seed, B, w, gen[:TIE_DEPTH], R, eot)
        if key[TIE_DEPTH] == pair[1]:
            key[TIE_DEPTH] = pair[0]
    g = np.random.default_rng([seed, w, len(key)] + [int(t) for t in key])
    gaps = np.concatenate([[0.0], g.uniform(0.25, 0.75, 12), np.full(V - 13, 0.25)])
    x = np.empty(V, dtype=np.float32)
    x[g.permutation(V)] = np.maximum(10.0 - np.cumsum(gaps), -10.0).astype(np.float32)
    order = np.argsort(-x, kind="stable")

    def swap(v, r):
        o = order[r]
        x[v], x[o] = x[o], x[v]

    depth = len(gen)
    p_eot = (0.15, 0.9 if depth >= 6 else 0.1, 0.3)[w]
    if g.random() < p_eot:
        swap(eot, int(g.integers(0, B + 2)))
    for _ in range(3):
        if g.random() < 0.5:
            order = np.argsort(-x, kind="stable")
            swap(tb + int(g.integers(0, n)), int(g.integers(0, 6)))
    if w == 0 and depth == TIE_DEPTH:
        a, b = script_tie_pair(seed, B, w, gen, R, eot, x)
        x[b] = x[a]
    if w == 2 and depth == DRY_DEPTH:
        x[:] = -np.inf
        x[eot] = 0.0
    return x


def script_tie_pair(seed, B, w, gen, R, eot, x=None):
    """The two text ids that tie at TIE_DEPTH behind `gen`: the two best text ids below end-of-text of that row."""
    if x is None:
        x = script_row(seed, B, w, list(gen), R, eot)
        a = [int(v) for v in np.argsort(-x, kind="stable") if v < eot][:2]
        return min(a), max(a)
    a = [int(v) for v in np.argsort(-x, kind="stable") if v < eot][:2]
    return min(a), max(a)


def script_reference(B, patience, seed, length_penalty=-1.0, mut=None):
    """The restatement over the scripted rows: per window a search() dict (with min_gap = the smallest non-zero adjacent score
    gap in any walked prefix + first unwalked element, n_ties = the exact ties there)."""
    R, eot, sup = script_setup()
    out = []
    for w in range(SCRIPT_W):
        info = dict(min_gap=np.inf, n_ties=0)

        def on_step(depth, beams, st, info=info):
            prefix = st["cands"][:st["n_walked"] + 1]
            for a, b in zip(prefix, prefix[1:]):
                gap = a[0] - b[0]
                if gap == 0:
                    info["n_ties"] += 1
                else:
                    info["min_gap"] = min(info["min_gap"], gap)

        res = search(lambda beams: [script_row(seed, B, w, b["gen"], R, eot) for b in beams], R, eot, sup, None, B, patience,
                     SCRIPT_DEPTH, length_penalty, mut, on_step)
        res.update(info)
        out.append(res)
    return out


# a scripted score is a sum of <= SCRIPT_DEPTH f32 log-probs, each within tsrules_ref.logprob_bound of the restatement's (rows of
# 263 logits spanning 20, |x| <= 10, |lp| <= 25)
SCORE_TOL = SCRIPT_DEPTH * (3.0 * tr.lse_err(SCRIPT_V, 20.5, 21.0) + 2.0 ** -21 + 2.0 ** -23 * 35.0)


def check_script_case(B, patience, seed, device=0):
    """wb_timestamp_beam_search_device on the scripted rows against the restatement: candidates, best, trace (tokens, parents,
    newly finished counts) outright, scores within SCORE_TOL."""
    import whisper_burn_amd as wb
    R, eot, sup = script_setup()
    ref = script_reference(B, patience, seed)
    assert all(r["min_gap"] > 2 * SCORE_TOL for r in ref), [r["min_gap"] for r in ref]      # (the premise of the comparison)
    gens = {}

    def fill(step, win, beam, tok, par):
        nxt, rows = {}, []
        for w, q, t, p in zip(win, beam, tok, par):
            gen = [] if step == 0 else gens[(int(w), int(p))] + [int(t)]
            nxt[(int(w), int(q))] = gen
            rows.append(script_row(seed, B, int(w), gen, R, eot))
        gens.clear()
        gens.update(nxt)
        return np.stack(rows)

    tp = wb.TimestampParams(R["tb"], R["n_ts"], R["max_init"], R["max_ts"])
    beams, best, trace = wb.timestamp_beam_search_device(fill, tp, wb.BeamParams(B, patience), SCRIPT_W, SCRIPT_V, eot, SCRIPT_DEPTH,
                                                         suppress=sup, device=device)
    for w, r in enumerate(ref):
        assert [c["tokens"] for c in beams[w]] == [t for t, _ in r["cands"]], (B, patience, w, beams[w], r["cands"])
        assert np.allclose([c["score"] for c in beams[w]], [s for _, s in r["cands"]], rtol=0, atol=SCORE_TOL), (B, patience, w)
        assert best[w] == r["best"], (w, best[w], r["best"])
        assert len(trace[w]) == len(r["trace"]), (B, patience, w, len(trace[w]), len(r["trace"]))
        for t, (got, want) in enumerate(zip(trace[w], r["trace"])):
            assert got["finished"] == want["finished"], (w, t, got, want)
            assert [(a, b) for a, b, _ in got["beams"]] == [(a, b) for a, b, _ in want["beams"]], (w, t, got, want)
            assert np.allclose([c for _, _, c in got["beams"]], [c for _, _, c in want["beams"]], rtol=0, atol=SCORE_TOL), (w, t)
        for c in beams[w]:
            tr.check_invariants(c["tokens"], R, eot, sup)
    return ref


# ---- the rows hook -----------------------------------------------------------------------------------------------------------------
ROW_KS = (2, 6, 8)


def rows_reference(case):
    """The restatement's candidates of every row of an operator case at k = TOPK_MAX (a smaller k is a prefix)."""
    return [candidates(case["logits"][r, :case["V"]], case["rules"], case["eot"], case["suppress"], case["suppress_first"],
                       case["gens"][r], 8) for r in range(case["R"])]


def check_rows_case(case, k, device=0, record=None, ref=None):
    """wb_timestamp_beam_rows on one of tsrules_ref's operator cases (its logits, rules, masks and histories; temperature 0):
    ids and count outright wherever rule (f) is outside delta_op, every log-prob within logprob_bound, (ts_lse, mN) within
    stats_bound, `forced` as the restatement's."""
    import whisper_burn_amd as wb
    Rl, V, eot = case["rules"], case["V"], case["eot"]
    tp = wb.TimestampParams(Rl["tb"], Rl["n_ts"], Rl["max_init"], Rl["max_ts"])
    h = np.array([tr.history(Rl, g) for g in case["gens"]], dtype=np.int32).reshape(case["R"], 4)
    ids, lp, count, forced, stats, err = wb.timestamp_beam_rows(case["logits"], tp, h[:, 0], h[:, 1], h[:, 2], h[:, 3], eot, k, V=V,
                                                                suppress=case["suppress"], suppress_first=case["suppress_first"],
                                                                device=device)
    assert err == 0, case["name"]
    short = 0
    ref = ref if ref is not None else rows_reference(case)
    for r in range(case["R"]):
        d, cl = ref[r][0], ref[r][1][:k]
        assert d["token"] is not None
        sb = tr.stats_bound(d, V)
        for got, want in ((stats[r, 0], d["ts_lse"]), (stats[r, 1], d["mN"])):
            assert (abs(float(got) - want) <= sb) if np.isfinite(want) else (float(got) == want), (case["name"], r, float(got), want)
        mag = max(abs(d["ts_lse"]) if np.isfinite(d["ts_lse"]) else 0.0, abs(d["mN"]) if np.isfinite(d["mN"]) else 0.0)
        if not d["fgap"] > tr.delta_op(V, d["A"], mag, 0.0)[0]:
            continue
        assert count[r] == len(cl) and bool(forced[r]) == d["forced"], (case["name"], k, r, int(count[r]), len(cl))
        assert ids[r, :count[r]].tolist() == [v for v, _ in cl], (case["name"], k, r, ids[r], cl)
        assert (ids[r, count[r]:] == -1).all() and np.isnan(lp[r, count[r]:]).all()         # nothing written past the count
        short += len(cl) < k
        for i, (v, want) in enumerate(cl):
            dd = dict(d, x_tok=float(case["logits"][r, v]), logprob=want)
            assert abs(float(lp[r, i]) - want) <= tr.logprob_bound(dd, V), (case["name"], k, r, i, float(lp[r, i]), want)
    if record is not None:
        record.append((case["name"], k, short))
    return ids, lp, count, forced, stats


def check_rows_determinism(case, k=6, device=0):
    """Two runs are bit-identical; a NaN row gives the single candidate end-of-text with log-prob 0 and raises the error word."""
    import whisper_burn_amd as wb
    Rl, V, eot = case["rules"], case["V"], case["eot"]
    tp = wb.TimestampParams(Rl["tb"], Rl["n_ts"], Rl["max_init"], Rl["max_ts"])
    h = np.array([tr.history(Rl, g) for g in case["gens"]], dtype=np.int32).reshape(case["R"], 4)
    run = lambda x: wb.timestamp_beam_rows(x, tp, h[:, 0], h[:, 1], h[:, 2], h[:, 3], eot, k, V=V, suppress=case["suppress"],
                                           suppress_first=case["suppress_first"], device=device)
    a, b = run(case["logits"]), run(case["logits"])
    for u, v in zip(a[:5], b[:5]):
        assert np.array_equal(tr.bits(u), tr.bits(v)), case["name"]
    x = case["logits"].copy()
    x[0, 17] = np.nan
    ids, lp, count, forced, stats, err = run(x)
    assert err == 1 and count[0] == 1 and ids[0, 0] == eot and lp[0, 0] == 0 and forced[0] == 0, (err, count[0], ids[0], lp[0])
    for u, v in zip((ids, lp, count, forced, stats), a[:5]):
        assert np.array_equal(tr.bits(u[1:]), tr.bits(v[1:])), case["name"]


# ---- the session ------------------------------------------------------------------------------------------------------------------
def check_beam_session(sess, oracle, st, params, R, suppress, B, patience, length_penalty=-1.0, active=None, max_excluded=0.10,
                       record=None):
    """One decode_timestamps_beam on a fresh / rewound session: every window-step of the trace replayed by the restatement on
    oracle logits teacher-forced on the device's own beams and scores (non-excluded steps match in beams, parents and newly
    finished count; recorded scores within 1e-3 per generated token of the oracle's), every candidate satisfies the
    invariants, the returned row is the finalize rule over the device's candidates.  Returns (rows, score, n_cand, beams)."""
    import whisper_burn_amd as wb
    W, eot, depth = sess.n_windows, st.end_of_text, params.max_depth
    prompt = [st.start_of_transcript, st.language, st.transcribe]
    tp = wb.TimestampParams(R["tb"], R["n_ts"], R["max_init"], R["max_ts"])
    rows, score, ncand = sess.decode_timestamps_beam(params, tp, wb.BeamParams(B, patience, length_penalty), active=active)
    beams, trace = sess.last_beams(depth), sess.last_beam_trace(depth)
    C = max_candidates(B, patience)
    n = ex = 0
    for w in range(W):
        if active is not None and not active[w]:
            assert beams[w] is None and rows[w] == [] and np.isnan(score[w]) and ncand[w] == -1 and trace[w] == [], w   # untouched
            continue
        enc = sess.encoder_output(w)
        cur, n_store = [new_beam()], 0
        for t, step in enumerate(trace[w]):
            x = oracle_rows(oracle, enc, prompt, cur)
            n += 1
            stp = beam_step(cur, x, R, eot, suppress, None, B, C, n_store)
            got = [dict(gen=cur[p]["gen"] + [tok], hist=cur[p]["gen"] + [tok], score=sc, parent=p) for tok, p, sc in step["beams"]]
            if replay_excluded(cur, x, R, eot, suppress, None, B):
                ex += 1
            else:
                assert [(b["gen"][-1], b["parent"]) for b in stp["live"]] == [(b["gen"][-1], b["parent"]) for b in got], (w, t)
                assert len(stp["newly"]) == step["finished"], (w, t, len(stp["newly"]), step["finished"])
                for a, b in zip(stp["live"], got):       # one more f32 log-prob on top of the device's own score
                    assert abs(a["score"] - b["score"]) <= 1e-3, (w, t, a["score"], b["score"])
            n_store = min(C, n_store + step["finished"])
            cur = got                                      # the device's own beams and scores go on
        assert 1 <= len(beams[w]) == ncand[w] <= max(C, B), (w, ncand[w])
        for c in beams[w]:
            tr.check_invariants(c["tokens"], R, eot, suppress)
            _, _, _, total = tr.oracle_row_check(oracle, enc, prompt + c["tokens"], 3, R, eot, suppress, None, 0.0, 0, 0, 0)
            assert abs(c["score"] - total) <= 1e-3 * len(c["tokens"]), (w, c, total)
            assert np.isclose(c["rank"], rank_of(c["tokens"], c["score"], eot, float(np.float32(length_penalty))), rtol=1e-12,
                              atol=0), (w, c)                      # (wb_beam_params holds the penalty as an f32)
        best = int(np.argmax([c["rank"] for c in beams[w]]))
        assert rows[w] == prompt + beams[w][best]["tokens"] and score[w] == beams[w][best]["score"], w
        # the finalize rule: the store's entries end on end-of-text; live beams fill up to B, best score first
        n_fin = sum(1 for c in beams[w] if c["tokens"][-1] == eot)
        tail = [c["score"] for c in beams[w][n_fin:]] if n_fin < len(beams[w]) and n_fin < B else []
        assert tail == sorted(tail, reverse=True), (w, tail)
    if record is not None:
        record.append((B, patience, n, ex))
    assert ex <= max_excluded * n, (n, ex)
    return rows, score, ncand, beams


def check_session_shape(eng, o32, W, B, patience, record=None):
    """The session checks of one launch shape on tsrules_ref's micro fixture."""
    import whisper_burn_amd as wb
    weights, st, audio, R, sup, prompt = tr.fixture()
    sess = tr.fixture_session(eng, audio, W, B)
    sess.set_suppress(sup)
    p = wb.decode_params(st, 1, tr.FIX_DEPTH)
    r1 = check_beam_session(sess, o32, st, p, R, sup, B, patience, record=record)
    n_graphs, n_cap = sess.graph_count(), sess.graph_captures()
    assert n_graphs >= 1 and n_cap >= n_graphs
    sess.rewind()
    r2 = check_beam_session(sess, o32, st, p, R, sup, B, patience)                       # again: bit-identical
    assert r1[0] == r2[0] and np.array_equal(r1[1], r2[1]) and r1[3] == r2[3]
    for R2, pat2, lp2 in ((dict(R, max_init=20, max_ts=120), patience, -1.0), (R, patience + 1.0, -1.0), (R, patience, 0.6)):
        sess.rewind()
        check_beam_session(sess, o32, st, p, R2, sup, B, pat2, lp2)                      # other rules / patience / penalty ...
        # ... drop no graph and capture none of their own: the one graph a longer search may add is the single step of the
        # depth's remainder behind the last whole chunk (keyed by the launch shape, as every graph)
        grown = sess.graph_count() - n_graphs
        assert 0 <= grown <= 1 and sess.graph_captures() - n_cap == grown, (n_graphs, n_cap, sess.graph_count(), sess.graph_captures())
    sess.rewind()
    act = np.ones(W, dtype=np.uint8); act[1] = 0
    r3 = check_beam_session(sess, o32, st, p, R, sup, B, patience, active=act)
    assert r3[0][0] == r1[0][0] and r3[0][2] == r1[0][2]
    sess.close()
    return r1


def check_beam1_is_greedy(eng, W=3):
    """beam_size 1, patience 1: decode_timestamps' greedy rows token for token, the sums within the summed log-prob bound."""
    import whisper_burn_amd as wb
    weights, st, audio, R, sup, prompt = tr.fixture()
    p = wb.decode_params(st, 1, tr.FIX_DEPTH)
    tp = wb.TimestampParams(R["tb"], R["n_ts"], R["max_init"], R["max_ts"])
    sess = tr.fixture_session(eng, audio, W, 1)
    sess.set_suppress(sup)
    rows, sums, _ = sess.decode_timestamps(p, tp)
    sess.rewind()
    brows, score, ncand = sess.decode_timestamps_beam(p, tp, wb.BeamParams(1, 1.0))
    assert brows == rows, (brows, rows)
    for w in range(W):
        assert abs(score[w] - sums[w, 0]) <= 1e-4 * (len(rows[w]) - 3), (w, score[w], sums[w, 0])
    sess.close()


def check_seek_loop_beam(eng, B=3, seconds=16, depth=24):
    """waveform_to_segments(beam=...) on the short-context model: tiles the stream, ends, and equals the pure-Python seek loop
    driven by per-window decode_timestamps_beam at the same seeks."""
    import whisper_burn_amd as wb
    from whisper_burn_amd import synth
    _, st, _, R, sup, prompt = tr.fixture()
    audio = synth.synth_audio(16000 * seconds, 3)
    p = wb.decode_params(st, 1, depth)
    tp = wb.TimestampParams(R["tb"], R["n_ts"], R["max_init"], R["max_ts"])
    bp = wb.BeamParams(B)
    segs, toks, n_win = wb.waveform_to_segments(eng, st, audio, 16000, params=p, timestamps=tp, suppress=sup, suppress_first=None,
                                                prompt=prompt, beam=bp)
    assert n_win >= 4 and len(segs) >= n_win
    assert [t for s in segs for t in s["tokens"]] == toks
    assert not any(tr.is_ts(R, t) or t == st.end_of_text for t in toks)
    wlen = wb.max_waveform_samples(eng.max_mel_frames() - p.padding)

    def decode(seek, ln, wi):
        sess = wb.Session.begin(eng, audio, np.array([seek], dtype=np.int64), np.array([ln], dtype=np.int64), max_beams=B,
                                padding=p.padding)
        sess.set_suppress(sup)
        wtp = wb.TimestampParams(R["tb"], R["n_ts"], R["max_init"], wi if (R["max_ts"] < 0 or R["max_ts"] > wi) else R["max_ts"])
        rows, _, _ = sess.decode_timestamps_beam(p, wtp, bp, prompt=prompt)
        sess.close()
        return rows[0][len(prompt):]

    rsegs, rtoks, seeks = tr.seek_loop_ref(len(audio), wlen, 16000, 0.02, decode, R, st.end_of_text)
    assert len(seeks) == n_win and seeks == sorted(set(seeks)) and rtoks == toks, (seeks, n_win)
    assert len(rsegs) == len(segs)
    for a, b in zip(rsegs, segs):
        assert abs(a[0] - b["start"]) < 1e-4 and abs(a[1] - b["end"]) < 1e-4 and a[2] == b["tokens"], (a, b)
    return segs, seeks
