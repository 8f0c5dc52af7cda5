"""tests/placement_ref.py held against itself on the CPU: the table form of the
definitions equals explicit insertion of the query into the tree, sum_a Z = L_p, an all-gap query
costs the reference tree's own log-likelihood on every edge, a copy of taxon 0 is placed on edge
0; and, on the inputs of tests/test_placement_gpu.py, the float64-against-longdouble floor of the
reference and the cap on what the rank comparisons leave out."""
import numpy as np
import pytest

import ancestral_cases as AC
import placement_cases as PC
import placement_ref as R

SMALL = [("n3", "GTR", 4, 13), ("n4", "JC69", 1, 13), ("n5", "GTR", 4, 13), ("balanced8", "JC69", 4, 13),
         ("ladder9", "GTR", 1, 13), ("random12", "GTR", 4, 13)]
TINY = 1e-16  # a thousand longdouble roundings: what two orders of the same arithmetic may differ by
ALL = [(name, subst, K, P) for name in PC.SHAPES for subst in PC.SUBSTS for K in PC.KS for P in PC.PS]


def _args(x, t, dtype=R.LD):
    return (x.pids[t], x.bls[t], *AC.model(x, t, dtype), x.vectors)


@pytest.mark.parametrize("case", SMALL, ids=lambda c: "-".join(map(str, c)))
def test_table_form_equals_explicit_insertion(case):
    x = PC.parity(*case)
    worst = 0.0
    for t in range(PC.T):
        ins, lik = R.insertion_tables(*_args(x, t), x.pendants)
        S, Z, s = R.formula_tables(*_args(x, t), x.pendants)
        worst = max(worst, float(np.max(np.abs(S - ins) / np.abs(ins))))
        # sum_a Z = L_p, in the table form and on the inserted tree (rows of P sum to 1)
        L = R.pattern_lik(*_args(x, t))
        assert np.max(np.abs(np.sum(Z, axis=2) / L - 1)) < TINY
        assert np.max(np.abs(np.sum(lik[:, :, :4], axis=2) / L - 1)) < TINY
        assert np.max(np.abs(lik[:, :, 4] / L - 1)) < TINY
        assert np.array_equal(S[:, :, 4], np.broadcast_to(s, S[:, :, 4].shape))
    print(f"{case}: table form against insertion {worst:.2e} relative")
    assert worst < TINY


def test_scoring_the_tables_is_insertion_query_by_query():
    """One query row inserted column by column, against the sum over the tables' entries."""
    x = PC.parity("n5", "GTR", 4, 13)
    S = PC.parity_tables("n5", "GTR", 4, 13)[1]
    for label, q, col, w in PC.maps(x):
        col, w = PC.resolved(x, col, w)
        ll = R.score(S, q, col, w)
        for qi, e, g in ((0, 0, 0), (3, 4, 1), (7, 6, 0), (66, 2, 1)):
            direct = R.explicit_ll(*_args(x, 1), q[qi], col, w, e, x.pendants[g])
            assert abs(ll[qi, e, g] - direct) <= TINY * abs(direct), (label, qi, e, g)


@pytest.mark.parametrize("case", SMALL, ids=lambda c: "-".join(map(str, c)))
def test_gap_query_and_copy_of_taxon_0(case):
    x = PC.parity(*case)
    S = PC.parity_tables(*case)
    for t in range(PC.T):
        for label, q, col, w in PC.maps(x):
            col, w = PC.resolved(x, col, w)
            ll = R.score(S[t], q, col, w)
            s = np.log(R.pattern_lik(*_args(x, t)))
            assert np.all(q[1] == 4)
            own = np.sum(w[w != 0] * s[col[w != 0]])
            assert np.max(np.abs(ll[1] - own)) <= TINY * abs(own)
            assert R.summarise(ll).best_edge[0] == 0, (case, t, label)


def test_float64_floor_and_rank_exclusions_on_the_gpu_inputs():
    """The reference in float64 against longdouble on every GPU parity input: the relative
    disagreement of ll stays under FLOAT64_CAP (it is the floor under the 1e-10 the GPU results
    are held to), and the rank comparisons leave out no entry under the reference itself."""
    worst = 0.0
    left_out = 0
    for case in ALL:
        x = PC.parity(*case)
        S = PC.parity_tables(*case)
        for t in range(PC.T):
            S64 = PC.tables(x, t, dtype=np.float64)
            for label, q, col, w in PC.maps(x):
                col, w = PC.resolved(x, col, w)
                ll = R.score(S[t], q, col, w)
                ll64 = R.score(S64, q, col, w)
                worst = max(worst, float(np.max(np.abs(ll64 - ll) / np.abs(ll))))
                ref = R.summarise(ll)
                delta = R.REL * float(np.max(np.abs(ref.edge_ll)))
                # (an all-gap query ties exactly on every edge and pendant length by definition:
                # placement_cases.check_result holds it to that instead)
                live = ~PC.all_gap(q)
                left_out += int(np.sum(ref.edge_gap[live] <= 2 * delta)) + \
                    int(np.sum(ref.pendant_gap[live] <= 2 * delta))
                assert np.all(np.abs(ll) > 1.0)  # (never near 0: a relative tolerance means something)
                assert ref.best_edge[0] == 0, (case, t, label)  # the copy of taxon 0
    print(f"float64 against longdouble, ll: {worst:.2e} relative; rank entries left out: {left_out}")
    assert worst < R.FLOAT64_CAP
    assert left_out == 0


def test_closed_form_star():
    """JC69, K = 1, the 3-taxon star, one pattern: the reference against the hand formula."""
    t = np.array([0.11, 0.27, 0.05, 0.0])
    Q, pi = R.gtr_q(np.ones(6), np.full(4, 0.25))
    tips = R.tip_vectors(np.array([[1], [1], [3]]))
    S, _, s = R.formula_tables([3, 3, 3], t, Q, pi, [1.0], [1.0], tips, [0.07])
    for code in range(5):
        want, s_want = R.star3_closed_form(t, 0.07, (1, 1, 3), code)
        assert abs(S[0, 0, code, 0] - want) < TINY and abs(s[0] - s_want) < TINY
