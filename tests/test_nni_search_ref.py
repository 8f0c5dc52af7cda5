"""The reference NNI search (tests/nni_search_ref.py) on the committed cases, on the CPU: it
ends at a local optimum by the definition, the log-likelihood rises with every move, and every
decision is clear of the optimiser's tolerance -- so that tests/test_nni_search_gpu.py may ask
the engine for the SAME moves."""
import numpy as np
import pytest

import nni_ref as NR
import nni_search_ref as S
import oracle_lib as O


@pytest.mark.parametrize("case", S.CASES, ids=repr)
def test_reference_search_is_well_posed(case):
    spec, tips, w, pids, start, pr = case.build()
    n = case.n
    tight, loose = case.reference(), case.reference(tol=S.LOOSE)
    for t, (a, b) in enumerate(zip(tight, loose)):
        # (a) a local optimum by the definition: no oracle delta above min_gain
        assert a.status == S.LOCAL_OPTIMUM and len(a.moves) < 100
        nb = NR.all_neighbours(n, a.parent_ids, a.branch_lengths)
        lls = O.unrooted_log_likelihoods(spec, tips, w, np.stack([p for _, _, p, _ in nb]),
                                         np.stack([x for _, _, _, x in nb]), np.repeat(pr[t:t + 1], len(nb), axis=0))
        assert np.all(lls - a.log_likelihood <= S.MIN_GAIN)
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


def test_the_cases_cover_what_they_should():
    assert {c.n for c in S.CASES} == {4, 5, 8, 12}
    assert {c.site for c in S.CASES} == {"constant", "weibull+4"}
    assert {c.subst for c in S.CASES} == {"JC69", "GTR"}
    assert all(100 <= c.P <= 300 for c in S.CASES)
    counts = [len(r.moves) for c in S.CASES for r in c.reference()]
    assert max(counts) >= 3 and min(counts) == 0, counts
