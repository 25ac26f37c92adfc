"""GPU, operator level: sample.hip through the test hook wb_sample_rows, against the f64 NumPy restatement in
tests/sample_ref.py.

Shapes (R, V): (1, 263), (5, 1031), (33, 7001), (3, 51865) -- V no multiple of 4 (a Philox group cut by the end of the row), V
below the block size, V above one prefetch batch (16384 ids), several rows, the real multilingual vocabulary.  Inputs sit in
NaN-poisoned rows with a padded leading dimension, outputs between guard bands (checked by the hook itself).  Each shape at
T = 0.2 and 1.0: masked and unmasked rows in one call, a mask that leaves one id, a -inf-heavy mask, stream / position /
attempt at 0 and 2^31 - 1.

The token equals the f64 argmax wherever the f64 top-two key gap exceeds delta_op = 2^-20 (A / T + 18) (sample_ref.delta_op:
two one-ulp logf and three f32 roundings per key, |g| <= 16.64, doubled for the pair and again as margin); at most 1 % of a
case's draws may be excluded (tests/test_sample_emu.py checks that on the restatement alone: none is).  The recorded
log-prob is within two f32 roundings of the f64 value."""
import numpy as np
import pytest

import sample_ref as sr

pytestmark = pytest.mark.gpu

CASES = {shape: sr.make_cases(shape) for shape in sr.SHAPES}


@pytest.mark.parametrize("shape", sr.SHAPES, ids=[f"R{r}_V{v}" for r, v in sr.SHAPES])
def test_draw_matches_the_restatement(shape):
    rec = []
    for case in CASES[shape]:
        sr.check_hook_case(case, record=rec)
    print("sample hook", rec)


def test_bit_identical_and_independent_of_the_batch():
    case = CASES[(33, 7001)][0]
    a, b = sr.run_hook(case), sr.run_hook(case)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))
    rev = sr.run_hook(case, rows=np.arange(case["R"])[::-1])
    assert np.array_equal(rev[0][::-1], a[0]) and np.array_equal(rev[1][::-1].view(np.int32), a[1].view(np.int32))
    for r in (0, 1, 2, 17, 32):
        one = sr.run_hook(case, rows=[r])
        assert one[0][0] == a[0][r] and one[1][0] == a[1][r] and one[2] == 0


def test_nan_row_ends_on_eot_and_raises_the_error_word():
    case = CASES[(5, 1031)][3]
    good = sr.run_hook(case)
    bad = dict(case)
    bad["logits"] = case["logits"].copy()
    bad["logits"][2, 1030] = np.nan                    # the last id: the tail of a cut Philox group
    tok, lp, err = sr.run_hook(bad)
    assert err == 1 and tok[2] == case["eot"] and lp[2] == 0.0
    assert np.array_equal(np.delete(tok, 2), np.delete(good[0], 2)) and good[2] == 0


def test_frequencies_follow_softmax_of_x_over_t():
    case, exp = sr.chi_square_case()
    tok, _, err = sr.run_hook(case)
    assert err == 0
    cnt = np.bincount(tok, minlength=case["V"]).astype(np.float64)
    chi2 = float(((cnt - exp) ** 2 / exp).sum())
    print(f"sample chi-square over 4096 streams: {chi2:.2f} (7 dof; 1 - 1e-6 quantile {sr.CHI2_7_1M6})")
    assert chi2 < sr.CHI2_7_1M6
