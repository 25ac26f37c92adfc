"""CPU: the f64 restatement of beam search under the timestamp rules (tests/tsbeam_ref.py) checked against itself.

 * every mutant of tsbeam_ref.MUTANTS (top-B instead of top-(B + 1) candidates, no break behind the B-th live beam, the store
   filled past max_candidates, a child's rule state taken from its beam index instead of its parent) changes the result of a
   scripted case, so the scripted cases see those mistakes;
 * the scripted cases cover what the model-free device test relies on: end-of-text walked in front of the B-th live beam and
   dropped behind it, a store that fills in the middle of a newly-finished list, windows ending at different depths, a window
   that runs out of live beams, exact score ties, and no near-tie inside twice the score tolerance;
 * the replay rule excludes at most 10 % of the window-steps of the oracle's own beam search on the micro fixture (four 1 s
   windows, depth 40) at (B, patience) = (5, 1), (5, 2), (3, 2), the final rank gap exceeds 2e-3 on every window, and the best
   rows differ from the greedy rows on some window."""
import numpy as np
import pytest

import tsbeam_ref as tb
import tsrules_ref as tr


def _result(ref):
    return [([t for t, _ in r["cands"]], r["best"], [[(a, b) for a, b, _ in s["beams"]] for s in r["trace"]],
             [s["finished"] for s in r["trace"]]) for r in ref]


@pytest.fixture(scope="module")
def scripted():
    return {c: tb.script_reference(*c) for c in tb.SCRIPT_CASES}


@pytest.mark.parametrize("mut", tb.MUTANTS)
def test_every_mutant_changes_a_scripted_result(scripted, mut):
    changed = [c for c in tb.SCRIPT_CASES if c[0] > 1 and _result(tb.script_reference(*c, mut=mut)) != _result(scripted[c])]
    assert changed, mut


def test_scripted_cases_cover_the_walk_the_store_and_the_ties(scripted):
    events, ties = set(), 0
    for c, ref in scripted.items():
        assert min(r["min_gap"] for r in ref) > 2 * tb.SCORE_TOL, (c, [r["min_gap"] for r in ref])
        assert len({len(r["trace"]) for r in ref}) > 1, c                     # windows end at different depths
        for r in ref:
            events |= r["events"]
            ties += r["n_ties"]
            assert len(r["trace"]) <= tb.SCRIPT_DEPTH and 1 <= len(r["cands"]) <= max(tb.max_candidates(c[0], c[1]), c[0])
    assert events == {"eot_walked", "eot_dropped", "store_filled_mid_list", "no_live_beam"}, events
    assert ties >= 10, ties


def test_finalize_fills_up_with_live_beams_and_ranks_by_length():
    eot = 9
    live = [dict(gen=[1, 2], score=-3.0), dict(gen=[1, 3], score=-2.0), dict(gen=[4, 5], score=-2.0)]
    cands, ranks, best = tb.finalize([([1, eot], -4.0)], live, 3, eot)
    assert cands == [([1, eot], -4.0), ([1, 3], -2.0), ([4, 5], -2.0)] and ranks == [-4.0, -1.0, -1.0] and best == 1
    assert tb.finalize([([eot], -0.5), ([1, 2, eot], -3.0)], live, 2, eot)[1:] == ([-np.inf, -1.5], 1)
    assert tb.rank_of([1, 2, 3, eot], -4.0, eot, 1.0) == -4.0 / (8.0 / 6.0)
    assert [tb.max_candidates(5, p) for p in (1.0, 1.1, 1.5, 2.0)] == [5, 6, 8, 10] and tb.max_candidates(3, 1.5) == 4   # half-even


@pytest.fixture(scope="module")
def oracle_fixture():
    from oracle.model import OracleWhisper
    weights, st, audio, R, sup, prompt = tr.fixture()
    o32 = OracleWhisper(weights)
    encs = tr.fixture_encs(o32, audio, W=4)
    greedy = [tr.oracle_decode(o32, e, prompt, R, st.end_of_text, sup, None, tr.FIX_DEPTH)[0][len(prompt):] for e in encs]
    return o32, st, R, sup, prompt, encs, greedy


@pytest.mark.parametrize("B,patience", [(5, 1.0), (5, 2.0), (3, 2.0)])
def test_replay_rule_excludes_at_most_a_tenth_of_the_oracle_s_window_steps(oracle_fixture, B, patience):
    o32, st, R, sup, prompt, encs, greedy = oracle_fixture
    n = ex = differ = 0
    for w, enc in enumerate(encs):
        res, steps, excluded = tb.oracle_search(o32, enc, prompt, R, st.end_of_text, sup, B, patience, tr.FIX_DEPTH)
        n, ex = n + steps, ex + excluded
        ranks = sorted(res["ranks"], reverse=True)
        print(f"B {B} patience {patience} window {w}: {steps} steps, {excluded} excluded, best-rank gap {ranks[0] - ranks[1]:.4f}")
        assert ranks[0] - ranks[1] > tb.GATE, (w, ranks)
        best = res["cands"][res["best"]][0]
        tr.check_invariants(best, R, st.end_of_text, sup)
        differ += best != greedy[w]
    print(f"B {B} patience {patience}: {n} window-steps, {ex} excluded")
    assert ex <= 0.10 * n, (n, ex)
    assert differ >= 1
