"""GPU, operator level: score.hip through the test hook wb_logprob_gather, against the f64 NumPy restatement in
tests/score_ref.py.

Every input sits inside a larger NaN-poisoned array and every output between canary bands (score_ref.run_hook); inside the
hook the device buffers the kernels write are guard-banded too and E^T carries NaN in its pad columns [V, ldv), so a kernel
that reads them into a sum fails visibly.

Shapes (R, d, V, splits): (1, 64, 263, auto) (5, 1280, 263, 1) (33, 128, 1031, 3) (130, 384, 1031, auto) -- one row, rows
that do not fill a tile, more than one row tile, V that is no multiple of the 128-column tile, one / forced / automatic
splits.  Cases per shape (score_ref.make_cases): targets at column 0, V - 1, the first and the last column of every split,
-1; duplicate probes and a probe at V - 1; masked and unmasked rows in one call; a mask that removes a whole split's
columns; a mask that leaves a single id (its log-prob is 0 up to the bound, nothing is NaN).

Bound per element: 2 (d + 4) 2^-24 max_v sum_k |h_k| |E_vk| + 4 x the error of the plain f32 NumPy evaluation against f64.
tests/test_score_emu.py shows on the CPU that this bound rejects every NumPy mutant by >= 10x on these very inputs."""
import numpy as np
import pytest

import parity_log
import score_ref as sr

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", sr.SHAPES, ids=["x".join(map(str, s[:3])) + f"/s{s[3]}" for s in sr.SHAPES])
def test_score_kernels_against_f64(shape):
    worst, at = 0.0, None
    cases = sr.make_cases(shape)
    for case in cases:
        r = sr.check_hook_case(case)
        if r >= worst:
            worst, at = r, case["name"]
    parity_log.record(f"score_kernel[{'x'.join(map(str, shape[:3]))}/s{shape[3]}]", worst, 1.0, case=at, n_cases=len(cases),
                      unit="error / bound")


def test_score_kernels_are_bit_identical_run_to_run():
    for shape in (sr.SHAPES[0], sr.SHAPES[3]):
        case = sr.make_cases(shape)[1]
        a, b = sr.run_hook(case), sr.run_hook(case)
        assert all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b)), case["name"]


def test_a_nan_row_stays_nan():
    sr.check_hook_nan_row()


def test_splits_do_not_change_the_statistics_beyond_the_bound():
    """The same call with 1, 2, 3 and every possible split: all within the bound of the f64 statement (the merge rescales to
    the common max), and the picked logits -- hence log-prob differences -- do not depend on the split at all."""
    base = sr.make_cases(sr.SHAPES[2])[1]                  # 33 x 128 x 1031, masked and unmasked rows
    ref, bound = sr.bounds(base)
    outs = []
    for req in (1, 2, 3, 9):
        c = dict(base, req=req, vs=sr.n_splits(33, 1031, req))
        got = sr.run_hook(c)
        assert sr.worst_ratio(got, ref, bound) <= 1.0, req
        outs.append(got)
    for got in outs[1:]:
        ok = np.isfinite(outs[0][0])
        assert np.allclose((got[0] + got[1])[ok], (outs[0][0] + outs[0][1])[ok], rtol=0, atol=1e-5)    # logprob + lse = the logit
