"""GPU, operator level: wb_timestamp_rows (the device function of dec_ts_update_kernel alone) against the f64 restatement of
tests/tsrules_ref.py at (R, V) = (1, 263), (5, 1031), (33, 7001), (3, 51865): V no multiple of 4, V below the block size, V
above one prefetch batch, several rows, the real vocabulary with T = [50364, 51865).  Inputs are NaN-poisoned behind the row
and padded, the outputs sit between guard bands (checked inside the hook).

Per shape (tsrules_ref.VARIANTS): every history class, T on top of and inside the id range, n_ts in {0, 1}, a sparse suppress, a
suppress that leaves ONE id (a text id; a timestamp: log-prob exactly 0, the empty class at -inf), a row left with NO id (ends
on end-of-text with the error word), max_initial 0 / -1 / 50, max_timestamp_index cutting T, temperature 0 / 0.2 / 1.0, stream / position /
attempt at 0 and 2^31 - 1.  Token and `forced` equal the restatement outside delta_op (at most 1 % of a case's rows excluded),
log-prob and (ts_lse, mN) within their derived bounds; bit-identical on repeat, with the rows reversed and with a row alone; a
NaN row ends on end-of-text with the error word and leaves the others untouched."""
import pytest

import tsrules_ref as tr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    """The inputs and their f64 references, computed once per shape and shared."""
    out = {}
    for shape in tr.SHAPES:
        cs = tr.make_cases(shape)
        out[shape] = [(c, tr.reference(c)) for c in cs]
    return out


@pytest.mark.parametrize("shape", tr.SHAPES, ids=[f"R{r}_V{v}" for r, v in tr.SHAPES])
def test_hook_matches_the_f64_restatement(cases, shape):
    rec = []
    for case, ref in cases[shape]:
        tr.check_hook_case(case, ref=ref, record=rec)
    print("(case, excluded rows, largest error / bound):", rec)
    assert len(rec) == len(tr.VARIANTS)


@pytest.mark.parametrize("shape", tr.SHAPES, ids=[f"R{r}_V{v}" for r, v in tr.SHAPES])
def test_a_row_without_an_admissible_id_ends_on_end_of_text(cases, shape):
    tr.check_hook_no_admissible_id([c for c, _ in cases[shape] if c["kind"] == "one_text"][0])


@pytest.mark.parametrize("shape", tr.SHAPES[1:], ids=[f"R{r}_V{v}" for r, v in tr.SHAPES[1:]])
def test_hook_is_bit_identical_across_repeats_orders_and_batches(cases, shape):
    for vi in (0, 1, 2):                          # T = 0, 0.2 and 1.0
        tr.check_hook_determinism(cases[shape][vi][0])
