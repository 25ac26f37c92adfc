"""CPU: the f64 restatement of the timestamp rules (tests/tsrules_ref.py) itself.

 * it equals `transformers`' WhisperTimeStampLogitsProcessor (same -inf pattern, same argmax) on random rows under scripted
   histories, in the one layout HF can express (T on top of the vocabulary, suppress = <|notimestamps|>);
 * five mutants of the rules are each caught by those same cases;
 * the exclusion caps of the GPU tests hold on the restatement / the oracle alone, and the micro fixture's oracle rows show
   every rule firing, so that no dead rule hides behind a passing parity test;
 * the pure-Python segment slicing on scripted rows."""
import numpy as np
import pytest

import tsrules_ref as tr

V_HF, NTS_HF = 600, 101
TB_HF = V_HF - NTS_HF                 # timestamps on top; <|notimestamps|> = TB_HF - 1, end-of-text below the specials
NOTS_HF, EOT_HF = TB_HF - 1, TB_HF - 9


def _hf_histories():
    t = lambda i: TB_HF + i
    txt = 11
    top = TB_HF + NTS_HF - 1
    return [[], [t(3)], [t(3), t(5)], [txt, t(4)], [t(4), txt], [t(0), txt, t(6), t(6), txt, t(9)], [t(0), txt, top],
            [t(0), txt, top, top], [t(0), t(0)], [t(2), txt, txt]]


def _hf_rows():
    """(x, gen) pairs: random rows with the timestamp block shifted so that rule (f) goes both ways, and one constructed tie
    (ts_lse == mN exactly: one allowed timestamp whose logit equals the best text logit) one row whose suppressed id would
    decide rule (f) and a first position whose best logit is end-of-text."""
    g = np.random.default_rng(2024)
    out = []
    for gen in _hf_histories():
        for shift in (-2.0, 1.0, 4.0):
            x = (g.standard_normal(V_HF) * 3.0).astype(np.float32)
            x[TB_HF:] += np.float32(shift)
            out.append((x, gen))
    x = (g.standard_normal(V_HF) * 3.0).astype(np.float32)
    top = TB_HF + NTS_HF - 1
    gen = [TB_HF, 11, top]                        # case (b) with the last timestamp the top id: T allowed = {top}
    x[EOT_HF + 1:TB_HF] = -50.0                   # (the ids (b) leaves in N: end-of-text and the specials above it)
    x[top] = x[EOT_HF] = np.float32(2.5)
    out.append((x, gen))
    x = (g.standard_normal(V_HF) * 3.0).astype(np.float32)
    x[NOTS_HF] = np.float32(40.0)                 # the suppressed <|notimestamps|> carries the best logit by far: (f) must not see it
    x[TB_HF:] += np.float32(4.0)
    out.append((x, [11, TB_HF + 4]))
    x = (g.standard_normal(V_HF) * 3.0).astype(np.float32)
    x[EOT_HF] = np.float32(30.0)                  # the first position with end-of-text far ahead: (d) removes it all the same
    out.append((x, []))
    return out


def _suppress_hf():
    s = np.zeros(V_HF, dtype=np.uint8)
    s[NOTS_HF] = 1
    return s


def _filtered(x, gen, mut=None):
    d = tr.step(x, tr.rules(TB_HF, NTS_HF, 50, -1), EOT_HF, _suppress_hf(), None, gen, mut=mut)
    return d


def _compared_rows():
    """The rows the comparison with transformers uses: HF decides (f) in f32, so a near-tie (not the exact one) may go either
    way there and is left out -- of the comparison AND of the mutant check, which must stand on compared rows only."""
    out = []
    for x, gen in _hf_rows():
        fgap = _filtered(x, gen)["fgap"]
        if not (fgap < 1e-4 and fgap != 0.0):
            out.append((x, gen))
    return out


def test_restatement_equals_hf_timestamp_logits_processor():
    transformers = pytest.importorskip("transformers")
    import torch
    from transformers import GenerationConfig
    from transformers.generation.logits_process import WhisperTimeStampLogitsProcessor
    cfg = GenerationConfig(eos_token_id=EOT_HF, bos_token_id=EOT_HF)
    cfg.no_timestamps_token_id = NOTS_HF
    cfg.max_initial_timestamp_index = 50
    begin = 3
    proc = WhisperTimeStampLogitsProcessor(cfg, begin_index=begin)
    n = 0
    rows = _compared_rows()
    for x, gen in rows:
        d = _filtered(x, gen)
        ids = torch.tensor([[1, 2, 3] + gen], dtype=torch.long)
        hf = proc(ids, torch.from_numpy(x)[None].clone())[0].numpy()
        assert np.array_equal(np.isneginf(hf), ~d["final"]), gen
        assert int(np.argmax(hf)) == d["token"], gen
        n += 1
    assert n == len(rows) >= 28


@pytest.mark.parametrize("mut", tr.MUTANTS)
def test_each_mutant_is_caught_by_the_same_cases(mut):
    diff = 0
    for x, gen in _compared_rows():
        a, b = _filtered(x, gen), _filtered(x, gen, mut=mut)
        diff += (not np.array_equal(a["final"], b["final"])) or a["token"] != b["token"] or a["forced"] != b["forced"]
    assert diff >= 1, mut


CASES = [c for shape in tr.SHAPES for c in tr.make_cases(shape)]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_operator_cases_stay_inside_the_exclusion_cap_on_the_restatement_alone(case):
    ref = tr.reference(case)
    assert all(d["token"] is not None for d in ref)
    assert tr.excluded(case, ref).sum() <= 0.01 * case["R"]


def test_the_cases_cover_what_the_operator_test_promises():
    assert tr.SHAPES == [(1, 263), (5, 1031), (33, 7001), (3, 51865)] and tr.TEMPS == [0.0, 0.2, 1.0]
    for shape in tr.SHAPES:
        R, V = shape
        cases = tr.make_cases(shape)
        assert {c["T"] for c in cases} == set(tr.TEMPS)
        assert {c["rules"]["n_ts"] for c in cases} >= {0, 1}
        assert {c["rules"]["max_init"] for c in cases} >= {0, -1, 50}
        assert any(0 <= c["rules"]["max_ts"] < c["rules"]["n_ts"] - 1 for c in cases)
        assert {c["attempt"] for c in cases} >= {0, tr.I31}
        tops = [c for c in cases if c["rules"]["tb"] + c["rules"]["n_ts"] == V and c["rules"]["n_ts"] > 1]
        ins = [c for c in cases if c["rules"]["tb"] + c["rules"]["n_ts"] < V and c["rules"]["n_ts"] > 1]
        assert tops and ins
        if V == 51865:
            assert any((c["rules"]["tb"], c["rules"]["n_ts"]) == (50364, 1501) for c in cases)
        assert any(int((c["suppress"] == 0).sum()) == 2 + len(range(0, c["rules"]["n_ts"], 3)) for c in cases)    # `single`
        # a suppress that leaves ONE id -- a text id, a timestamp -- and exactly one admissible id in every row, at T = 0 and T > 0
        for kind in ("one_text", "one_ts"):
            ones = [c for c in cases if c["kind"] == kind]
            assert len(ones) == 2 and {c["T"] > 0 for c in ones} == {False, True}
            for c in ones:
                assert int((c["suppress"] == 0).sum()) == 1
                only = int(np.flatnonzero(c["suppress"] == 0)[0])
                assert tr.is_ts(c["rules"], only) == (kind == "one_ts")
                for d in tr.reference(c):
                    assert d["final"].sum() == 1 and d["token"] == only and d["logprob"] == 0.0 and d["gap"] == np.inf
                    assert d["forced"] == (kind == "one_ts") and (d["ts_lse"] if kind == "one_text" else d["mN"]) == -np.inf
        for c in cases:
            assert c["logits"].shape == (R, V + tr.PAD) and np.isnan(c["logits"][:, V:]).all()
            assert {0, tr.I31} & set(c["stream"].tolist()) and {0, tr.I31} & set(c["position"].tolist())
            assert not tr.is_ts(c["rules"], c["eot"])
        if R >= len(tr.HISTORIES):
            c = cases[0]
            kinds = {tr.history(c["rules"], g)[0] for g in c["gens"]}
            assert {0, 1, 2, 3, 6} <= kinds
        # over the variants every history class meets every shape, the smallest included
        seen = {tr.HISTORIES[(r + vi) % len(tr.HISTORIES)] for vi, v in enumerate(tr.VARIANTS) if v[5] not in tr.ONE_ID_HISTORIES
                for r in range(R)}
        assert seen == set(tr.HISTORIES)
    forced = [d["forced"] for c in tr.make_cases(tr.SHAPES[2]) for d in tr.reference(c)]
    assert 0.1 < np.mean(forced) < 0.9                    # rule (f) goes both ways in the operator inputs


@pytest.fixture(scope="module")
def fixture_rows():
    from oracle.model import OracleWhisper
    weights, st, audio, R, sup, prompt = tr.fixture()
    o32 = OracleWhisper(weights)
    encs = tr.fixture_encs(o32, audio, 3)
    return st, R, sup, [tr.oracle_decode(o32, enc, prompt, R, st.end_of_text, sup, None, tr.FIX_DEPTH) for enc in encs]


def test_the_fixture_s_oracle_rows_fire_every_rule_and_stay_clear_of_the_bounds(fixture_rows):
    st, R, sup, rows = fixture_rows
    fired = {k: 0 for k in ("a", "b", "c", "d", "f_forced", "f_free")}
    n = ex = 0
    fgap, gap, n_ts = np.inf, np.inf, []
    for row, ds in rows:
        gen = row[3:]
        tr.check_invariants(gen, R, st.end_of_text, sup)
        n_ts.append(sum(tr.is_ts(R, t) for t in gen))
        for d in ds:
            for k in fired:
                fired[k] += bool(d["fired"][k])
            n += 1
            ex += tr.is_excluded(d, tr.FIX_V, 0.0, model=True)
            fgap, gap = min(fgap, d["fgap"]), min(gap, d["gap"])
    print("fixture: timestamps per row", n_ts, "fired", fired, "min |ts_lse - mN| %.4f, min top-two gap %.4f" % (fgap, gap))
    assert all(v >= 1 for v in fired.values()), fired
    assert min(n_ts) >= 2 and any(tr.is_ts(R, a) and tr.is_ts(R, b) for row, _ in rows for a, b in zip(row[3:], row[4:]))
    assert ex == 0 and fgap > 2e-3 and gap > 2e-3, (n, ex, fgap, gap)


def test_the_oracle_alone_stays_inside_the_session_tests_exclusion_cap():
    """The draws of the session tests (tsrules_ref.SESSION_DRAWS), decoded by the oracle alone over the fixture's four
    windows and five streams each: at most 5 % of the positions lie inside delta_model."""
    from oracle.model import OracleWhisper
    weights, st, audio, R, sup, prompt = tr.fixture()
    o32 = OracleWhisper(weights)
    encs = tr.fixture_encs(o32, audio, 4)
    for T, seed, attempt in tr.SESSION_DRAWS:
        n = ex = 0
        for w, enc in enumerate(encs):
            for j in range(5 if T > 0 else 1):
                row, ds = tr.oracle_decode(o32, enc, prompt, R, st.end_of_text, sup, None, tr.FIX_DEPTH, T, seed, w * (5 if T > 0 else 1) + j, attempt)
                tr.check_invariants(row[3:], R, st.end_of_text, sup)
                n += len(ds)
                ex += sum(tr.is_excluded(d, tr.FIX_V, T, model=True) for d in ds)
        print("oracle alone: T", T, "positions", n, "excluded", ex)
        assert ex <= 0.05 * n, (T, n, ex)


def test_segments_restatement_on_scripted_rows():
    R = tr.rules(100, 50)
    t = lambda i: 100 + i
    eot = 99
    # two closed segments, then text to a trailing single timestamp: a third segment, the window moves wholly
    segs, adv = tr.segments_ref([t(0), 5, 6, t(4), t(4), 7, t(9), t(9), 8, t(12), eot], R, eot, 50)
    assert segs == [(0, 4, 0, 4), (4, 7, 4, 9), (7, 10, 9, 12)] and adv == 50
    # ... without the trailing timestamp's text: the window moves to the last closing timestamp
    segs, adv = tr.segments_ref([t(0), 5, 6, t(4), t(4), 7, t(9), t(9), 8, eot], R, eot, 50)
    assert segs == [(0, 4, 0, 4), (4, 7, 4, 9)] and adv == 9
    # no pair: one segment to the last timestamp, or to the window end
    assert tr.segments_ref([t(0), 5, 6, t(7), eot], R, eot, 50) == ([(0, 4, 0, 7)], 50)
    assert tr.segments_ref([t(0), 5, 6], R, eot, 50) == ([(0, 3, 0, 50)], 50)
    assert tr.segments_ref([5, 6, eot], R, eot, 50) == ([(0, 2, 0, 50)], 50)
    assert tr.segments_ref([eot], R, eot, 50) == ([], 50)
    # zero advance: a pair at <|0.00|>; a timestamp equal to the window end
    assert tr.segments_ref([t(0), t(0), eot], R, eot, 50) == ([(0, 1, 0, 0)], 0)
    assert tr.segments_ref([t(0), 5, t(49), t(49), eot], R, eot, 49) == ([(0, 3, 0, 49)], 49)
