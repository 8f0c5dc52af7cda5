"""The reference SPR search (tests/spr_search_ref.py) on the committed cases, on the CPU: it
ends at a local optimum by the definition, the log-likelihood rises with every move, and every
decision is clear of the optimiser's tolerance -- so that tests/test_spr_search_gpu.py may ask
the engine for the SAME moves.  And one start from which the reference NNI search ends below."""
import numpy as np
import pytest

import nni_search_ref as NS
import spr_ref as SR
import spr_search_ref as S


@pytest.mark.parametrize("case", S.CASES + [S.NNI_BELOW_SPR], ids=repr)
def test_reference_search_is_well_posed(case):
    spec, tips, w, pids, start, pr = case.build()
    n = case.n
    tight, loose = case.reference(), case.reference(tol=S.LOOSE)
    for t, (a, b) in enumerate(zip(tight, loose)):
        # (a) a local optimum by the definition: no oracle delta above min_gain
        assert a.status == S.LOCAL_OPTIMUM and len(a.moves) < 100
        moves, _, lls = S.neighbourhood(spec, tips, w, a.parent_ids, a.branch_lengths, pr[t], radius=case.radius)
        assert len(moves) > 0 and np.all(lls - a.log_likelihood <= S.MIN_GAIN)
        assert a.best_delta == a.decisions[-1].best <= S.MIN_GAIN
        # (b) logL rose at every move
        lls_rounds = [d.log_likelihood for d in a.decisions]
        assert len(lls_rounds) == len(a.moves) + 1
        assert all(y > x for x, y in zip(lls_rounds, lls_rounds[1:])), lls_rounds
        # (c) every decision's margin is at least ten times what its deltas move by when the
        # optimiser stops at a criterion 100 times looser
        assert a.moves == b.moves, (t, a.moves, b.moves)
        moved = max(float(np.max(np.abs(x.delta - y.delta))) for x, y in zip(a.decisions, b.decisions))
        margin = min(d.margin for d in a.decisions)
        print(f"{case} tree {t}: moves {a.moves} gains {np.round(a.gains, 3).tolist()} logL {a.log_likelihood!r} "
              f"least margin {margin:.3e} deltas moved {moved:.3e}")
        assert margin >= 10 * moved, (t, margin, moved)
        # (d) a radius-limited case takes only moves of that distance
        if case.radius:
            assert all(m[3] <= case.radius for d in a.decisions for m in d.moves)
            assert any(m[3] > case.radius for m in SR.moves(n, pids[t]))


def test_the_cases_cover_what_they_should():
    assert {c.n for c in S.CASES} == {4, 5, 8, 12}
    assert {c.site for c in S.CASES} == {"constant", "weibull+4"}
    assert {c.subst for c in S.CASES} == {"JC69", "GTR"}
    assert all(100 <= c.P <= 300 for c in S.CASES)
    assert sorted(c.radius for c in S.CASES) == [0, 0, 0, 0, 0, 2]
    counts = [len(r.moves) for c in S.CASES for r in c.reference()]
    assert max(counts) >= 3 and min(counts) == 0, counts
    dirs = {m[1] for c in S.CASES for r in c.reference() for m in r.moves}
    assert dirs == {0, 1}, dirs


def _nni_outcome_margin(ref):
    """How far the NNI reference's deltas would have to move for it to END elsewhere: a move
    taken needs its whole margin; at the stop only the distance of the best delta from min_gain
    counts (which of the moves it does not take is the best one changes nothing)."""
    taken = [d.margin for d in ref.decisions[:-1]]
    return min(taken + [abs(ref.decisions[-1].best - NS.MIN_GAIN)])


def test_nni_hill_climbing_ends_below_the_spr_search():
    case = S.NNI_BELOW_SPR
    spec, tips, w, pids, start, pr = case.build()
    spr = case.reference()[0]
    nni = NS.reference_search(spec, tips, w, pids[0], start[0], pr[0])
    loose = NS.reference_search(spec, tips, w, pids[0], start[0], pr[0], tol=NS.LOOSE)
    assert nni.status == NS.LOCAL_OPTIMUM and spr.status == S.LOCAL_OPTIMUM
    assert nni.moves == loose.moves
    moved = max(float(np.max(np.abs(x.delta - y.delta))) for x, y in zip(nni.decisions, loose.decisions))
    margin = _nni_outcome_margin(nni)
    print(f"NNI: moves {nni.moves} logL {nni.log_likelihood!r} outcome margin {margin:.3e} deltas moved {moved:.3e}; "
          f"SPR: moves {spr.moves} logL {spr.log_likelihood!r}")
    assert margin >= 10 * moved, (margin, moved)
    assert len(nni.moves) >= 1 and len(spr.moves) >= 2
    assert nni.log_likelihood < spr.log_likelihood - S.MIN_GAIN
    # (by far: the NNI search stops at a tree with inner edges on the lower bound)
    assert spr.log_likelihood - nni.log_likelihood > 100.0
    assert np.sum(nni.branch_lengths[case.n:-1] <= 2 * NS.LO) >= 1
