"""The references of tests/test_spr_scan_gpu.py held against themselves on the CPU (DESIGN.md
4.18), on the committed inputs of tests/spr_cases.py: the oracle's float64 build against its
longdouble build stays under spr_ref.FLOAT64_CAP relative to |logL| (the floor under the 1e-10
the GPU results are held to), and no decision the GPU test compares exactly -- the best target of
an (s, dir), the best move of a tree -- rests on a margin that the tolerance could overturn.  If
a seed ever fails the margin rule, change the seed, not the rule."""
import numpy as np
import pytest

import spr_cases as SC
import spr_ref as R

ORACLE_CASES = [c for c in SC.SMALL if c[4] != "real"]


@pytest.mark.parametrize("c", ORACLE_CASES, ids=SC.case_id)
def test_float64_floor_of_the_oracle(c):
    x = SC.case(*c)
    worst = 0.0
    for t in range(len(x.pids)):
        ll, mv, nll = SC.small_reference(c)[t]
        ll_ld, _, nll_ld = SC.small_reference(c, "ld")[t]
        if len(mv):
            worst = max(worst, float(np.max(np.abs((nll - ll) - (nll_ld - ll_ld))) / abs(ll_ld)))
        worst = max(worst, abs(ll - ll_ld) / abs(ll_ld))
    print(f"{SC.case_id(c)}: float64 against longdouble, delta relative to |logL| {worst:.2e}")
    assert worst < R.FLOAT64_CAP


@pytest.mark.parametrize("c", SC.SMALL, ids=SC.case_id)
def test_no_decision_rests_on_a_margin_under_the_tolerance(c):
    x = SC.case(*c)
    for t in range(len(x.pids)):
        ll, mv, nll = SC.small_reference(c)[t]
        clear = 2 * R.REL * abs(ll)
        for radius in (0, 1, 2, 3) if c in SC.RADIUS else (0,):
            keep = [i for i, m in enumerate(mv) if radius == 0 or m[3] <= radius]
            _, _, margin, _, move_margin = R.decisions(R.table(x.n, [mv[i] for i in keep], nll[keep] - ll))
            assert np.all(margin > clear), (SC.case_id(c), t, radius, float(np.min(margin)), clear)
            assert move_margin > clear, (SC.case_id(c), t, radius, move_margin, clear)


def test_the_radius_rule_keeps_whole_shells():
    """Distances are what the definition says on a ladder, where they can be read off: the edges
    touching the merged edge are at distance 1 and each node further along the path adds one."""
    n = 12
    x = SC.case(*SC.RADIUS[1])
    reach = R.targets(n, x.pids[0], 0, 0)  # leaf 0 of the ladder, the deepest cherry
    assert min(reach.values()) == 1 and max(reach.values()) == n - 3
    for r in (1, 2, 3):
        assert {m[3] for m in R.moves(n, x.pids[0], r)} == set(range(1, r + 1))


@pytest.mark.parametrize("name", SC.BIG)
def test_the_70_taxon_cases(name):
    """Floor and margins of what the GPU test compares on the 70-taxon trees: every (s, dir) and
    the best move at radius 3, the sampled rows at radius 0.  And the stored exponents are at work:
    between prune point and target the cumulative exponents of a rescaling pass differ."""
    import ancestral_cases as AC
    x = SC.big(name)
    for label, ref, ref_ld, whole in (
            ("radius 3", SC.big_radius3_reference(name), SC.big_radius3_reference(name, "ld"), True),
            ("sample", SC.big_sample_reference(name), SC.big_sample_reference(name, "ld"), False)):
        ll, mv, nll = ref
        ll_ld, _, nll_ld = ref_ld
        floor = float(np.max(np.abs((nll - ll) - (nll_ld - ll_ld))) / abs(ll_ld))
        print(f"{name} {label}: {len(mv)} moves, float64 against longdouble {floor:.2e}")
        assert floor < R.FLOAT64_CAP
        _, _, margin, _, move_margin = R.decisions(R.table(x.n, mv, nll - ll))
        clear = 2 * R.REL * abs(ll)
        assert np.all(margin > clear), (name, label, float(np.min(margin)), clear)
        assert not whole or move_margin > clear
    Q, _, r, _ = AC.model(x, 0, np.float64)
    cum = R.down_exponents(x.pids[0], x.bls[0], Q, r, x.vectors)
    sample = SC.big_sample(name)
    assert len(sample) >= 300
    # (a leaf against any internal node would already differ; what the ladder guarantees is
    # depth: about two powers of two per node, so some sampled move spans tens of them)
    span = max(int(np.max(np.abs(cum[s] - cum[f]))) for s, d, f, _ in sample)
    internal = max([int(np.max(np.abs(cum[s] - cum[f]))) for s, d, f, _ in sample if s >= x.n and f >= x.n] or [0])
    print(f"{name}: largest |exponent(s) - exponent(f)| over the sample {span}, both internal {internal}")
    assert span > 0
    if name == "ladder70":
        assert span >= 40 and internal >= 40
