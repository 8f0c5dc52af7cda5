"""Starting trees on the GPU: pairwise substitution counts and maximum-likelihood
distances, neighbour joining, and the two in one call, against tests/start_trees_ref.py.  The
shapes are the smallest that reach every edge of the kernels: one taxon short of, at and past a
four-taxon row tile; pattern counts around the four-pattern step and the 16-pattern load;
replicate counts below, at and past the four-replicate group; either side of the LDS / global
switch of the neighbour-joining kernel (128 | 129 taxa) and of the renumbering's (256 | 257)."""
import numpy as np
import pytest

import start_trees_cases as Cs
import start_trees_ref as R
import tree_utils as TU

pytestmark = pytest.mark.gpu

LD = np.longdouble


def _engine(subst, site, tips, weights, **kw):
    import libsbn_amd as L
    return L.Engine(L.PhyloModelSpecification(subst, site, "none"), tips, weights, **kw)


def _alignment(n, P, gaps, seed):
    rng = np.random.default_rng(seed)
    tips, w = TU.random_alignment(n, P, rng, gap_fraction=0.05 if gaps else 0.0)
    if gaps == "taxon":
        tips[n // 2] = 4
    return tips, w, rng


# ---- 1. counts ----

@pytest.mark.parametrize("n,P,B,gaps", [(3, 1, 1, False), (4, 3, 2, True), (5, 4, 17, True), (17, 5, 1, "taxon"),
                                         (65, 33, 2, True), (4, 129, 17, False), (17, 129, 2, True),
                                         (65, 129, 17, "taxon"), (5, 16, 4, True), (5, 17, 3, True)])
def test_counts_are_exact(n, P, B, gaps):
    tips, w, rng = _alignment(n, P, gaps, 100 * n + P)
    W = rng.integers(0, 7, size=(B, P)).astype(np.float64)
    eng = _engine("JC69", "constant", tips, w)
    out = eng.pairwise_distances(W, pair_counts=True, pair_status=True)
    want = R.pair_counts(tips, W)
    assert np.array_equal(out.pair_counts, want.astype(np.float64))
    d = out.distances
    assert d.shape == (B, n, n) and np.array_equal(d, d.transpose(0, 2, 1))
    assert np.all(d[:, np.arange(n), np.arange(n)] == 0.0)
    assert np.all((d[:, ~np.eye(n, dtype=bool)] >= 1e-8) & (d[:, ~np.eye(n, dtype=bool)] <= 10.0))
    assert eng.last_call_path() == f"pair_counts B={B} chunks=1" and eng.last_call_launches()[0] == 1
    # no replicate weights: one replicate of the engine's own pattern weights
    own = eng.pairwise_distances(pair_counts=True)
    assert np.array_equal(own.pair_counts, R.pair_counts(tips, w[None]).astype(np.float64))
    again = eng.pairwise_distances(w[None], pair_counts=True)
    assert np.array_equal(own.distances, again.distances) and np.array_equal(own.pair_counts, again.pair_counts)


def test_tip_partials_count_unit_vectors_only():
    """An engine made from tip partials: exactly e_a is state a; masks, all ones and real-valued
    vectors are missing."""
    rng = np.random.default_rng(7)
    n, P = 6, 37
    tips, w = TU.random_alignment(n, P, rng, gap_fraction=0.1)
    partials = np.zeros((n, P, 4))
    for x in range(n):
        for p in range(P):
            partials[x, p] = 1.0 if tips[x, p] > 3 else np.eye(4)[tips[x, p]]
    kind = rng.integers(0, 6, size=(n, P))
    partials[kind == 0] = [1.0, 1.0, 0.0, 0.0]           # a 0/1 mask
    partials[kind == 1] = [0.7, 0.1, 0.1, 0.1]           # real-valued
    partials[kind == 2] *= 0.5                           # a scaled unit vector is no unit vector
    codes = R.codes_from_partials(partials)
    assert 0 < (codes < 4).sum() < n * P
    eng = _engine("JC69", "constant", None, w, tip_partials=partials, use_tip_states=False)
    W = rng.integers(0, 5, size=(3, P)).astype(np.float64)
    out = eng.pairwise_distances(W, pair_counts=True)
    assert np.array_equal(out.pair_counts, R.pair_counts(codes, W).astype(np.float64))


def test_equal_rows_give_identical_bits_wherever_they_stand():
    tips, w = Cs.evolved_alignment(9, 150, 3)
    rng = np.random.default_rng(3)
    W = rng.integers(0, 5, size=(17, 150)).astype(np.float64)
    W[5] = W[16] = W[0]
    row, *_ = Cs.gtr_weibull_row(3)
    eng = _engine("GTR", "weibull+4", tips, w)
    out = eng.pairwise_distances(W, row, pair_counts=True, pair_status=True)
    one = eng.pairwise_distances(W[:1], row, pair_counts=True, pair_status=True)
    three = eng.pairwise_distances(W[[3, 0, 2]], row, pair_counts=True)
    for b in (0, 5, 16):
        assert np.array_equal(out.pair_counts[b], one.pair_counts[0])
        assert np.array_equal(out.distances[b], one.distances[0])
        assert np.array_equal(out.pair_status[b], one.pair_status[0])
    assert np.array_equal(three.distances[1], one.distances[0])
    assert not np.array_equal(out.distances[1], out.distances[0])


def test_replicates_in_chunks_within_the_arena_budget(monkeypatch):
    tips, w = Cs.evolved_alignment(7, 90, 4)
    rng = np.random.default_rng(4)
    W = rng.integers(0, 5, size=(17, 90)).astype(np.float64)
    whole = _engine("JC69", "constant", tips, w).pairwise_distances(W, pair_counts=True, pair_status=True)
    monkeypatch.setenv("MI_PHYLO_PLV_BYTES", str(3 * 21 * 16 * 8 + 100))  # three replicates' counts
    eng = _engine("JC69", "constant", tips, w)
    out = eng.pairwise_distances(W, pair_counts=True, pair_status=True)
    assert eng.last_call_launches()[0] == 6 and eng.last_call_path() == "pair_counts B=17 chunks=6"
    for f in ("distances", "pair_counts", "pair_status"):
        assert np.array_equal(getattr(out, f), getattr(whole, f)), f


# ---- 2. distances ----

def test_jc69_distances_meet_the_closed_form():
    tips, w = Cs.evolved_alignment(8, 300, 21)
    eng = _engine("JC69", "constant", tips, w)
    out = eng.pairwise_distances(pair_counts=True, pair_status=True)
    N = out.pair_counts[0]
    share = 1.0 - np.trace(N, axis1=1, axis2=2) / N.sum(axis=(1, 2))
    assert np.all(out.pair_status[0] == 0) and np.all(share < 0.7)
    for q, (i, j) in enumerate(R.pair_index(8)):
        want = float(R.jc69_distance(share[q]))
        got = out.distances[0, i, j]
        print(f"pair ({i}, {j}): {got:.17g} closed form {want:.17g} rel {abs(got - want) / want:.2e}")
        assert abs(got - want) <= 1e-9 * want


@pytest.mark.parametrize("seed", Cs.MEASURED_SEEDS)
def test_gtr_weibull_distances_are_stationary_and_maximal(seed):
    """At every returned d off the bounds the reference's long-double Newton correction
    |l'(d) / l''(d)| is <= 10 tolerance max(d, 1e-3) (the factor 10: the rounding of l' in FP64,
    orders below the tolerance at these sizes); and l(d) is not below l at any of 200
    log-spaced points of the box by more than 2^-48 |l|."""
    tips, w, row, rates, freqs, cr, cw = Cs.measured_case(seed)
    rng = np.random.default_rng(seed)
    W = np.stack([w, rng.multinomial(int(w.sum()), w / w.sum()).astype(np.float64)])
    eng = _engine("GTR", "weibull+4", tips, w)
    tol = 1e-10
    out = eng.pairwise_distances(W, row, pair_counts=True, pair_status=True, tolerance=tol)
    lik = R.PairLikelihood(rates, freqs, cr, cw)
    grid = [lik.matrices(t) for t in np.geomspace(1e-8, 10.0, 200)]
    assert np.all(out.pair_status == 0)
    worst = 0.0
    for b in range(2):
        for q, (i, j) in enumerate(R.pair_index(len(tips))):
            N, d = out.pair_counts[b, q], out.distances[b, i, j]
            l, g, h = lik.derivatives(N, d)
            corr = abs(g / h) / (tol * max(d, 1e-3))
            worst = max(worst, float(corr))
            assert h < 0 and corr <= 10.0, (b, i, j, d, float(corr))
            best = max(lik.from_matrices(N, m)[0] for m in grid)
            assert l >= best - LD(2.0) ** -48 * abs(l), (b, i, j, d)
    print(f"seed {seed}: largest Newton correction / (tolerance max(d, 1e-3)) = {worst:.3e}")


def test_status_and_bounds():
    rng = np.random.default_rng(9)
    P = 60
    base = rng.integers(0, 4, P)
    tips = np.stack([base, base, (base + 1) % 4, rng.integers(0, 4, P), rng.integers(0, 4, P)]).astype(np.int32)
    tips[3, : P // 2] = 4   # taxon 3 has data where taxon 4 has none ...
    tips[4, P // 2:] = 4    # ... and the other way round: no comparable pattern
    w = np.ones(P)
    pairs = R.pair_index(5)
    for subst, site, row in (("JC69", "constant", None), ("GTR", "weibull+4", Cs.gtr_weibull_row(1)[0])):
        eng = _engine(subst, site, tips, w)
        for lo, hi in ((1e-8, 10.0), (1e-4, 2.5)):
            out = eng.pairwise_distances(None, row, pair_status=True, min_length=lo, max_length=hi)
            st, d = out.pair_status[0], out.distances[0]
            assert st[pairs.index((0, 1))] == 1 and d[0, 1] == lo      # identical sequences
            if subst == "JC69":  # different everywhere: l rises all the way under JC69
                assert st[pairs.index((0, 2))] == 2 and d[0, 2] == hi
            assert (st[pairs.index((0, 2))] == 2) == (d[0, 2] == hi)
            assert st[pairs.index((3, 4))] == 3 and d[3, 4] == hi      # no data
            assert st[pairs.index((0, 3))] in (0, 2) and lo <= d[0, 3] <= hi


def test_iteration_limit_is_reported():
    tips, w = Cs.evolved_alignment(5, 200, 2)
    row = Cs.gtr_weibull_row(2)[0]
    eng = _engine("GTR", "weibull+4", tips, w)
    out = eng.pairwise_distances(None, row, pair_status=True, max_iterations=1, tolerance=1e-15)
    assert np.all(out.pair_status == 4)


def test_input_errors_are_reported():
    tips, w = Cs.evolved_alignment(5, 40, 2)
    eng = _engine("JC69", "constant", tips, w)
    with pytest.raises(RuntimeError, match="min_length < max_length"):
        eng.pairwise_distances(min_length=1.0, max_length=1.0)
    with pytest.raises(RuntimeError, match="min_length < max_length"):
        eng.starting_trees(min_length=2.0, max_length=1.0)
    with pytest.raises(RuntimeError, match="min_length < max_length"):
        eng.neighbour_joining(np.ones((1, 4, 4)), min_length=1.0, max_length=0.5)
    with pytest.raises(RuntimeError, match="replicate_count must be positive"):
        eng.pairwise_distances(np.zeros((0, 40)))
    with pytest.raises(RuntimeError, match="replicate_count must be positive"):
        eng.starting_trees(np.zeros((0, 40)))
    gtr = _engine("GTR", "weibull+4", tips, w)
    bad = Cs.gtr_weibull_row(2)[0].copy()
    bad[6:10] = 0.3
    with pytest.raises(RuntimeError, match="frequencies do not sum to 1"):
        gtr.pairwise_distances(None, bad)
    # (the engine goes on working)
    assert np.all(np.isfinite(gtr.pairwise_distances(None, Cs.gtr_weibull_row(2)[0]).distances))


# ---- 3. neighbour joining ----

@pytest.fixture(scope="module")
def any_engine():
    tips, w = Cs.evolved_alignment(4, 8, 1)
    return _engine("JC69", "constant", tips, w)


@pytest.mark.parametrize("n,B", [(3, 1), (4, 3), (5, 3), (64, 3), (65, 1), (128, 1), (129, 3), (257, 1), (258, 1)])
def test_neighbour_joining_against_the_reference(any_engine, n, B):
    d = np.stack([Cs.noisy_matrix(n, 1000 * n + b) for b in range(B)])
    pid, bl = any_engine.neighbour_joining(d)
    assert any_engine.last_call_path() == f"nj n={n} store={'lds' if n <= 128 else 'global'}"
    for b in range(B):
        want_pid, want_bl = R.neighbour_joining(d[b])
        assert np.array_equal(pid[b], want_pid), b
        # (the same matrix, the same rule, every operation rounded once: the same bits -- which is
        # within 1e-12, relative and absolute, a fortiori)
        assert np.array_equal(bl[b], want_bl), (b, float(np.abs(bl[b] - want_bl).max()))
        assert bl[b, -1] == 0.0 and bl[b, :-1].min() >= 1e-8
    # only i < j is read
    junk = d.copy()
    junk[:, np.tril_indices(n)[0], np.tril_indices(n)[1]] = np.nan
    pid2, bl2 = any_engine.neighbour_joining(junk)
    assert np.array_equal(pid2, pid) and np.array_equal(bl2, bl)


@pytest.mark.parametrize("kind", ["random", "ladder", "balanced"])
@pytest.mark.parametrize("n", [4, 5, 12, 33])
def test_exact_ties_of_additive_dyadic_matrices(any_engine, kind, n):
    """Every sum of the rule is exact and many Q are EQUAL (the cherries of an additive matrix):
    the lowest-(i, j) rule decides, bit for bit."""
    tree_pid, tree_bl, d = Cs.dyadic_tree_matrix(n, 40 + n, kind)
    pid, bl = any_engine.neighbour_joining(d)
    want_pid, want_bl = R.neighbour_joining(d)
    assert np.array_equal(pid[0], want_pid) and np.array_equal(bl[0], want_bl)
    assert R.splits(pid[0], bl[0]) == R.splits(tree_pid, tree_bl)


def test_every_operation_is_rounded_once(any_engine):
    """A matrix on which a fused (r-2) d - R_i joins (1, 5) where the rule joins (4, 6)
    (test_start_trees_ref.py): the kernel's arithmetic is the rule's, not a contraction of it."""
    d = Cs.contraction_sensitive_matrix()
    assert R.first_join(d) == (4, 6) and R.first_join(d, fused=True) == (1, 5)
    pid, bl = any_engine.neighbour_joining(np.stack([d, d]))
    want_pid, want_bl = R.neighbour_joining(d)
    fused_pid, _ = R.neighbour_joining(d, fused=True)
    for b in range(2):
        assert pid[b, 4] == pid[b, 6] and not np.array_equal(pid[b], fused_pid)
        assert np.array_equal(pid[b], want_pid) and np.array_equal(bl[b], want_bl)


def test_identical_sequences_join_in_slot_order(any_engine):
    """Zero distances: every Q of every round is equal."""
    n = 7
    pid, bl = any_engine.neighbour_joining(np.zeros((2, n, n)), min_length=1e-6)
    want_pid, want_bl = R.neighbour_joining(np.zeros((n, n)), min_length=1e-6)
    for b in range(2):
        assert np.array_equal(pid[b], want_pid) and np.array_equal(bl[b], want_bl)
    assert np.array_equal(want_pid, TU._polish((((((0, 1), 2), 3), 4), 5, 6), n))
    assert np.all(bl[:, :-1] == 1e-6)


def test_negative_raw_lengths_are_clamped(any_engine):
    d = np.array([[0, 1.0, 1.0, 5.0], [0, 0, 0.1, 1.0], [0, 0, 0, 1.0], [0, 0, 0, 0]])
    pid, bl = any_engine.neighbour_joining(d, min_length=1e-3, max_length=1.5)
    want_pid, want_bl = R.neighbour_joining(d, 1e-3, 1.5)
    assert np.array_equal(pid[0], want_pid) and np.array_equal(bl[0], want_bl)
    # (raw lengths: 1.725, -0.725, -0.725, 1.725, 0.775)
    assert bl[0, :-1].min() == 1e-3 and bl[0, :-1].max() == 1.5
    assert 1e-3 < bl[0, 4] < 1.5


@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_a_distance_that_is_not_finite_names_its_matrix(any_engine, value):
    d = np.stack([Cs.noisy_matrix(6, b) for b in range(3)])
    d[1, 2, 4] = value
    with pytest.raises(RuntimeError, match=r"not finite \(matrix 1\)"):
        any_engine.neighbour_joining(d)
    pid, _ = any_engine.neighbour_joining(d[[0, 2]])  # (the engine goes on working)
    assert np.array_equal(pid[1], R.neighbour_joining(d[2])[0])


# ---- 4. end to end ----

@pytest.mark.parametrize("seed", Cs.MEASURED_SEEDS)
def test_starting_trees_end_to_end(seed):
    tips, w, row, rates, freqs, cr, cw = Cs.measured_case(seed)
    n = len(tips)
    rng = np.random.default_rng(seed)
    W = np.concatenate([w[None], rng.multinomial(int(w.sum()), w / w.sum(), size=4).astype(np.float64)])
    eng = _engine("GTR", "weibull+4", tips, w)
    st = eng.starting_trees(W, row, distances=True)
    assert eng.last_call_path() == f"pair_counts B=5 chunks=1 | nj n={n} store=lds"
    pd = eng.pairwise_distances(W, row)
    pid, bl = eng.neighbour_joining(pd.distances)
    assert np.array_equal(st.distances, pd.distances)
    assert np.array_equal(st.parent_ids, pid) and np.array_equal(st.branch_lengths, bl)
    quiet = eng.starting_trees(W, row)
    assert quiet.distances is None and np.array_equal(quiet.parent_ids, pid) and np.array_equal(quiet.branch_lengths, bl)
    # the trees are what every unrooted call takes, with no renumbering
    pr = np.tile(row, (5, 1))
    ll = eng.log_likelihoods(st.parent_ids, st.branch_lengths, pr)
    assert np.all(np.isfinite(ll))
    found = eng.nni_search(st.parent_ids, st.branch_lengths, pr, max_moves=2)
    assert np.all(found.log_likelihood >= ll - 1e-9 * np.abs(ll))
    # against the reference's distances and joins.  The distances agree to the solver's tolerance
    # (1e-9 relative with its factor 10); a length is a combination of at most 2 n distances with
    # coefficients of at most 1: 1e-7 absolute covers distances below 5.  The margins of these
    # seeds (test_start_trees_ref.py) keep the joins; the trifurcation may sit elsewhere: splits.
    want_d = Cs.reference_distances(tips, w, R.PairLikelihood(rates, freqs, cr, cw))
    assert np.all(np.abs(st.distances[0] - want_d) <= 1e-9 * np.maximum(want_d, 1e-3))
    want = R.splits(*R.neighbour_joining(want_d))
    got = R.splits(st.parent_ids[0], st.branch_lengths[0])
    assert want.keys() == got.keys()
    assert max(abs(want[k] - got[k]) for k in want) <= 1e-7


def test_device_form_replays_from_a_graph():
    import torch
    tips, w, row, *_ = Cs.measured_case(Cs.MEASURED_SEEDS[0])
    n, P, B = len(tips), len(w), 6
    rng = np.random.default_rng(1)
    W = rng.multinomial(int(w.sum()), w / w.sum(), size=B).astype(np.float64)
    eng = _engine("GTR", "weibull+4", tips, w)
    ref = eng.starting_trees(W, row, distances=True)
    dev = torch.device("cuda", 0)
    d_w, d_row = torch.from_numpy(W).to(dev), torch.from_numpy(row).to(dev)
    out_pid = torch.zeros((B, 2 * n - 3), dtype=torch.int32, device=dev)
    out_bl = torch.zeros((B, 2 * n - 2), dtype=torch.float64, device=dev)
    out_d = torch.zeros((B, n, n), dtype=torch.float64, device=dev)
    gs = torch.cuda.Stream()

    def call(stream, engine, dist):
        engine.starting_trees_device(stream, B, d_w.data_ptr(), d_row.data_ptr(), out_pid.data_ptr(),
                                     out_bl.data_ptr(), out_d.data_ptr() if dist else None)

    # (the other engine runs the same call on the stream first: the kernels' code objects are
    # loaded -- into device memory -- at their first launch, which is not the engine's allocation)
    call(gs.cuda_stream, eng, True)
    torch.cuda.synchronize()
    fresh = _engine("GTR", "weibull+4", tips, w)
    fresh.reserve_start_trees(B)
    torch.cuda.synchronize()
    for dist in (True, False):
        free_before = torch.cuda.mem_get_info(0)[0]
        with torch.cuda.stream(gs):
            call(gs.cuda_stream, fresh, dist)
        torch.cuda.synchronize()
        assert torch.cuda.mem_get_info(0)[0] == free_before  # (reserved: the call allocated nothing)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=gs):
            call(torch.cuda.current_stream().cuda_stream, fresh, dist)
        for _ in range(2):
            out_pid.zero_(), out_bl.zero_(), out_d.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert np.array_equal(out_pid.cpu().numpy(), ref.parent_ids)
            assert np.array_equal(out_bl.cpu().numpy(), ref.branch_lengths)
            if dist:
                assert np.array_equal(out_d.cpu().numpy(), ref.distances)
    fresh.check_status()
    # the two halves on their own
    fresh.pairwise_distances_device(gs.cuda_stream, B, d_w.data_ptr(), d_row.data_ptr(), out_d.data_ptr())
    out_pid.zero_(), out_bl.zero_()
    fresh.neighbour_joining_device(gs.cuda_stream, B, n, out_d.data_ptr(), out_pid.data_ptr(), out_bl.data_ptr())
    torch.cuda.synchronize()
    fresh.check_status()
    assert np.array_equal(out_pid.cpu().numpy(), ref.parent_ids) and np.array_equal(out_bl.cpu().numpy(), ref.branch_lengths)


def test_sharded_handles_and_other_alphabets():
    import libsbn_amd as L
    tips, w, row, *_ = Cs.measured_case(Cs.MEASURED_SEEDS[1])
    rng = np.random.default_rng(2)
    W = rng.multinomial(int(w.sum()), w / w.sum(), size=3).astype(np.float64)
    single = _engine("GTR", "weibull+4", tips, w)
    want = single.starting_trees(W, row, distances=True)
    by_trees = _engine("GTR", "weibull+4", tips, w, shard_devices=[0, 0], shard_mode="trees")
    got = by_trees.starting_trees(W, row, distances=True)
    for f in ("parent_ids", "branch_lengths", "distances"):
        assert np.array_equal(getattr(got, f), getattr(want, f)), f
    assert np.array_equal(by_trees.pairwise_distances(W, row).distances, want.distances)
    pid, bl = by_trees.neighbour_joining(want.distances)
    assert np.array_equal(pid, want.parent_ids) and np.array_equal(bl, want.branch_lengths)
    by_patterns = _engine("GTR", "weibull+4", tips, w, shard_devices=[0, 0], shard_mode="patterns")
    for call in (lambda: by_patterns.pairwise_distances(W, row), lambda: by_patterns.starting_trees(W, row),
                 lambda: by_patterns.reserve_start_trees(3)):
        with pytest.raises(RuntimeError, match="pattern-sharded engines do not compute pairwise distances"):
            call()
    pid, bl = by_patterns.neighbour_joining(want.distances)  # (needs no alignment: the first shard's)
    assert np.array_equal(pid, want.parent_ids) and np.array_equal(bl, want.branch_lengths)
    import aa_utils as A
    aa_tips, aa_w = A.random_aa_alignment(5, 16, rng)
    aa = L.Engine(L.PhyloModelSpecification("WAG", "constant", "none"), aa_tips, aa_w)
    for call in (lambda: aa.pairwise_distances(), lambda: aa.starting_trees(), lambda: aa.reserve_start_trees(1)):
        with pytest.raises(RuntimeError, match="4-state only"):
            call()
    pid, bl = aa.neighbour_joining(want.distances)
    assert np.array_equal(pid, want.parent_ids)
