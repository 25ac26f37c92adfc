"""GPU, operator level: the two kernels of beam search under the timestamp rules (csrc/tsbeam.hip) against the f64
restatement of tests/tsbeam_ref.py.

wb_timestamp_beam_rows (dec_tsbeam_rows_kernel's device function alone) on tsrules_ref's case generator at (R, V) = (1, 263),
(5, 1031), (33, 7001), (3, 51865) -- every history class, suppress masks that leave fewer than k ids, k in {2, 6, 8}: ids and
count equal the restatement outright wherever |ts_lse - mN| exceeds delta_op (the order is by logit, exact at temperature 0),
every log-prob within logprob_bound, (ts_lse, mN) within stats_bound; the guard bands are checked inside the hook; two runs are
bit-identical; a NaN row sets the error word.

wb_timestamp_beam_search_device (both kernels, no model) at V = 263, W = 3, B in {1, 3, 5}, depth <= 12 on scripted logits
whose rows hold logits either >= 0.25 apart or exactly equal: end-of-text ranked in front of and behind the B-th live beam, a
store that fills in the middle of a list, windows ending at different depths, a window that runs out of live beams, exact
score ties between sibling beams with identical rows.  Candidates, store order, best, and the trace's tokens, parents and
newly-finished counts equal the restatement outright; scores (sums of f32 log-probs against f64) within tsbeam_ref.SCORE_TOL,
and tests/test_tsbeam_ref.py asserts that no two scores that are compared lie closer than twice that."""
import pytest

import tsbeam_ref as tb
import tsrules_ref as tr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    """The inputs and their f64 candidates (k = 8; a smaller k is a prefix), computed once per shape and shared."""
    return {shape: [(c, tb.rows_reference(c)) for c in tr.make_cases(shape)] for shape in tr.SHAPES}


@pytest.mark.parametrize("shape", tr.SHAPES, ids=[f"R{r}_V{v}" for r, v in tr.SHAPES])
def test_rows_hook_matches_the_f64_restatement(cases, shape):
    rec = []
    for case, ref in cases[shape]:
        for k in tb.ROW_KS:
            tb.check_rows_case(case, k, record=rec, ref=ref)
    assert len(rec) == len(tr.VARIANTS) * len(tb.ROW_KS)
    assert sum(r[2] for r in rec) > 0                # rows whose allowed set holds fewer than k ids
    print("rows with fewer than k allowed ids:", sum(r[2] for r in rec))


@pytest.mark.parametrize("shape", tr.SHAPES[1:3], ids=[f"R{r}_V{v}" for r, v in tr.SHAPES[1:3]])
def test_rows_hook_is_bit_identical_and_flags_a_nan_row(cases, shape):
    tb.check_rows_determinism(cases[shape][0][0])


@pytest.mark.parametrize("B,patience,seed", tb.SCRIPT_CASES, ids=[f"B{b}_p{int(p)}" for b, p, _ in tb.SCRIPT_CASES])
def test_scripted_search_equals_the_restatement(B, patience, seed):
    ref = tb.check_script_case(B, patience, seed)
    print("steps per window", [len(r["trace"]) for r in ref], "candidates", [len(r["cands"]) for r in ref])
