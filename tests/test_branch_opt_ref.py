"""The reference optimum the branch-length optimisation call is checked against
(tests/branch_opt_ref.py), on the oracle alone: it satisfies the call's convergence criterion,
its two methods agree, and the bounded case of the GPU tests is a real one."""
import numpy as np
import pytest

import branch_opt_ref as R
import oracle_lib as O

TOLERANCE = 1e-6      # the call's default
MIN_LENGTH = 1e-8
UPPER = 0.02          # the max_length of the GPU tests' upper-bound case (DS1 topology 0, JC69)
TOPOLOGIES = (0, 40)


def _ds1():
    st = O.load_struct("ds1_top100")
    tips, w, pids, _ = O.struct_arrays(st)
    n, P = tips.shape
    spec = O.make_spec(n, P, "JC69", "constant")
    start = np.full(2 * n - 2, 0.1)
    start[-1] = 0.0
    return spec, tips, w, pids, start, np.zeros(O.param_count(spec))


def _methods():
    # (without scipy the numpy method stands alone: nothing to compare, nothing skipped)
    return ("lbfgsb", "newton") if R.HAVE_SCIPY else ("newton",)


@pytest.mark.parametrize("tree", TOPOLOGIES)
def test_reference_meets_the_convergence_criterion_and_its_methods_agree(tree):
    spec, tips, w, pids, start, pr = _ds1()
    got = {}
    for m in _methods():
        x, ll, g, used = R.reference_optimum(spec, tips, w, pids[tree], start, pr, method=m)
        assert used == m
        crit = R.criterion(x[:-1], g, MIN_LENGTH, 10.0)
        print(tree, m, "logL", ll, "criterion", crit, "at lower bound", int(np.sum(x[:-1] <= MIN_LENGTH)))
        assert crit <= TOLERANCE
        assert np.all(x[:-1] >= MIN_LENGTH) and np.all(x[:-1] <= 10.0) and x[-1] == start[-1]
        got[m] = (x, ll)
    default = R.reference_optimum(spec, tips, w, pids[tree], start, pr)
    assert default[3] == _methods()[0]
    lls = [v[1] for v in got.values()]
    assert max(lls) - min(lls) <= 1e-8
    # every DS1 tree ends with a branch at the lower bound: the bound handling is exercised
    assert np.sum(default[0][:-1] <= MIN_LENGTH) >= 1


def test_small_max_length_puts_branches_on_the_upper_bound():
    spec, tips, w, pids, start, pr = _ds1()
    free = R.reference_optimum(spec, tips, w, pids[0], start, pr)
    assert np.sum(free[0][:-1] > UPPER) >= 1
    for m in _methods():
        x, ll, g, _ = R.reference_optimum(spec, tips, w, pids[0], start, pr, max_length=UPPER, method=m)
        at_upper = np.flatnonzero(x[:-1] >= UPPER)
        print(m, "logL", ll, "free", free[1], "at upper bound", at_upper)
        assert len(at_upper) >= 1
        assert np.array_equal(at_upper, np.flatnonzero(free[0][:-1] > UPPER))
        assert R.criterion(x[:-1], g, MIN_LENGTH, UPPER) <= TOLERANCE
        assert ll < free[1]


def test_criterion_projects_out_the_bounds():
    t = np.array([1e-8, 0.5, 10.0, 1e-8])
    g = np.array([-5.0, 1e-7, 3.0, 2.0])
    assert R.criterion(t, g, 1e-8, 10.0) == pytest.approx(2.0 * 1e-3)
    assert R.criterion(t[:3], g[:3], 1e-8, 10.0) == pytest.approx(0.5e-7)
