"""tests/gp_hybrid_ref.py, the restatement of the quartet hybrid marginals by tree enumeration
(DESIGN.md 4.26), checked on the CPU: the reference's known-answer property on its two hybrid DAGs,
which requests are fully formed, the designed 11-taxon batch, and the size of every enumeration
the GPU tests ask for."""
import numpy as np
import pytest

import gp_hybrid_ref as H
import gp_ref as R

FASTA = "7-taxon-slice-of-ds1.fasta"


def _seven(nwk, seed):
    pids, _, tips, w, _ = R.load_case(nwk, FASTA)
    d = R.build_dag(pids)
    b = np.random.default_rng(seed).uniform(1e-3, 0.1, d.G)
    b[:d.R] = 0.0
    return d, b, tips, w


def _known_answer(nwk, name, seed):
    """the summands of entry `name`, sorted, are log L(T) + log(1/4) of the four trees through it"""
    d, b, tips, w = _seven(nwk, seed)
    model, q = R.Model(), R.uniform_prior(d)
    e = R.strings(d).index(name)
    got = H.hybrid(d, q, b, tips, w, model)
    req = got.requests
    assert req.formed[e] and req.summand_count[e] == 4
    first = req.first_summand[e]
    through = [t for t in R.enumerate_trees(d) if e in t]
    assert len(through) == 4
    tipv = R.tip_vectors(tips)
    want = sorted(float(np.dot(w, np.log(R.tree_likelihood(d, t, b, tipv, model)))) + np.log(0.25) for t in through)
    have = sorted(got.summands[first:first + 4])
    print(name, "max |summand - (log L + log 1/4)|", np.max(np.abs(np.array(have) - np.array(want))))
    assert np.all(np.abs(np.array(have) - np.array(want)) <= 1e-12)
    assert np.all(got.trees_per_summand[first:first + 4] == 1)
    assert abs(got.hybrid[e] - H.logsumexp_in_order(want)) <= 1e-12


def test_simplest_hybrid_marginal_known_answer():
    _known_answer("simplest-hybrid-marginal.nwk", "0010000|0001111|0000111", 1)


def test_second_simplest_hybrid_marginal_known_answer():
    _known_answer("second-simplest-hybrid-marginal.nwk", "0000001|0011110|0001110", 2)


def test_which_requests_are_fully_formed():
    for nwk in ("simplest-hybrid-marginal.nwk", "second-simplest-hybrid-marginal.nwk"):
        pids = R.load_case(nwk, FASTA)[0]
        d = R.build_dag(pids)
        req = H.requests(d)
        roots = {int(d.entries[i][2]) for i in range(d.R)}
        assert not np.any(req.formed[:d.R])   # a rootsplit entry is never central
        for e in range(d.R, d.G):
            t, _, s = (int(x) for x in d.entries[e])
            assert req.formed[e] == (t not in roots and s >= d.n), e
        assert any(int(d.entries[e][0]) in roots for e in range(d.R, d.G))
        assert np.any(req.formed)
        at = 0
        for e in np.flatnonzero(req.formed):   # summands are numbered entry by entry
            assert req.first_summand[e] == at
            at += req.summand_count[e]
        assert at == len(req.summands)


def test_the_eleven_taxon_batch():
    d = R.build_dag(H.eleven_batch())
    assert (d.node_count, d.G, d.R, d.topology_count) == (35, 56, 2, 54.0)
    assert len(R.enumerate_trees(d)) == 54
    req = H.requests(d)
    assert int(np.sum(req.formed)) == 21 and len(req.summands) == 93
    e = R.strings(d).index(H.ELEVEN_WIDE_ENTRY)
    assert [len(x) for x in req.lists[e]] == [2, 3, 3, 3] and req.summand_count[e] == 54
    rng = np.random.default_rng(3)
    import tree_utils as TU
    tips, w = TU.random_alignment(d.n, 5, rng, gap_fraction=0.1)
    b = rng.uniform(0.02, 0.4, d.G)
    got = H.hybrid(d, R.random_q(d, rng), b, tips, w, R.Model())
    assert int(np.sum(got.trees_per_summand > 1)) == 39
    assert np.all(np.isfinite(got.hybrid[req.formed])) and np.all(got.hybrid[~req.formed] == -np.inf)
    # the block of entries 10-12 is one whose entries are all formed (what the hybrid SBN estimate needs)
    t, c, _ = d.entries[10]
    assert tuple(d.block_range[t, c]) == (10, 13) and np.all(req.formed[10:13])


def test_summand_order_is_rootward_outermost_sorted_innermost():
    d = R.build_dag(H.eleven_batch())
    req = H.requests(d)
    e = R.strings(d).index(H.ELEVEN_WIDE_ENTRY)
    g, a, r, o = req.lists[e]
    first = req.first_summand[e]
    assert tuple(req.summands[first]) == (g[0], a[0], r[0], o[0])
    assert tuple(req.summands[first + 1]) == (g[0], a[0], r[0], o[1])
    assert tuple(req.summands[first + 3]) == (g[0], a[0], r[1], o[0])
    assert tuple(req.summands[first + 9]) == (g[0], a[1], r[0], o[0])
    assert tuple(req.summands[first + 27]) == (g[1], a[0], r[0], o[0])
    assert g == sorted(g) and all(x >= d.R for x in g)


def test_zero_likelihood_is_minus_infinity_not_nan():
    d = R.build_dag(H.eleven_batch())
    tips = np.zeros((d.n, 3), np.int32)
    tips[1, 1], tips[2, 1] = 1, 2   # taxa 1 and 2 differ at pattern 1
    w = np.array([1.0, 2.0, 0.0])
    cherry = next(v for v in range(d.n, d.node_count) if d.clades[v] == (frozenset([1]), frozenset([2])))
    b = np.full(d.G, 0.1)
    b[:d.R] = 0.0
    for c in range(2):
        b[d.block_range[cherry, c, 0]] = 0.0
    got = H.hybrid(d, R.uniform_prior(d), b, tips, w, H.ExactModel())
    assert not np.any(np.isnan(got.summands)) and not np.any(np.isnan(got.hybrid))
    with_cherry = np.array([any(int(d.entries[x][2]) == cherry or int(d.entries[x][0]) == cherry for x in s)
                            for s in got.requests.summands])
    assert np.any(np.isinf(got.summands)) and np.any(np.isfinite(got.summands[with_cherry == 0]))


def test_enumerations_stay_small():
    """every DAG tests/test_gp_hybrid_gpu.py restates spans at most 2000 trees (the convention of
    tests/test_gp_ref.py)"""
    counts = [R.build_dag(R.load_case(nwk, FASTA)[0]).topology_count
              for nwk in ("simplest-hybrid-marginal.nwk", "second-simplest-hybrid-marginal.nwk")]
    counts += [R.build_dag(R.random_case(i)[0]).topology_count for i in range(len(R.RANDOM_CASES))]
    counts.append(R.build_dag(H.eleven_batch()).topology_count)
    print("topologies", counts)
    assert max(counts) <= 2000


def test_the_library_counts_requests_without_a_device_and_refuses_over_the_cap():
    """mi_gp_hybrid_request_count is the host code mi_engine_gp_create runs (the DAG, then the
    request tables), with the cap on the summands given by the caller: at the cap it counts, one
    below it refuses, and a DAG over the cap gets no tables at all (nothing of size S is built)."""
    import libsbn_amd as L
    cases = [R.load_case(nwk, FASTA)[0] for nwk in ("simplest-hybrid-marginal.nwk", "second-simplest-hybrid-marginal.nwk")]
    cases += [R.random_case(i)[0] for i in range(len(R.RANDOM_CASES))] + [H.eleven_batch()]
    for pids in cases:
        req = H.requests(R.build_dag(pids))
        want = (int(np.sum(req.formed)), len(req.summands))
        assert L.gp_hybrid_request_count(pids) == want
        assert L.gp_hybrid_request_count(pids, max_summands=want[1]) == want
        assert want[1] > 1   # (max_summands 0 asks for the library's own limit)
        with pytest.raises(RuntimeError, match=f"more than {want[1] - 1} summands in all"):
            L.gp_hybrid_request_count(pids, max_summands=want[1] - 1)
    assert L.gp_hybrid_request_count(H.eleven_batch()) == (21, 93)
    with pytest.raises(RuntimeError, match=r"max_summands must be in \[0, 2\^28\]"):
        L.gp_hybrid_request_count(H.eleven_batch(), max_summands=2 ** 28 + 1)
    with pytest.raises(RuntimeError, match="not bifurcating|parent-id form"):
        bad = H.eleven_batch()
        bad[0, 0] = bad[0, 3]
        L.gp_hybrid_request_count(bad)
