"""Split tables of tree batches on the GPU against tests/splits_ref.py: the
table (indices, bits, first occurrences, tree counts), its statistics, Robinson-Foulds distances
and squared branch scores, the hand-over of the index array to the reduced gradient call, and
the errors.  The taxon counts are the smallest at which each boundary of the lane map exists:
31 | 32 | 33 (the tail mask at a full word and one bit into the next), 64 | 65 (two words, then
four lanes per tree for three), 257 (working bitsets in memory instead of LDS), 2049 (65 words:
the second word pass).  Every row of every table is compared."""
import os
import subprocess

import numpy as np
import pytest

import splits_ref as R
import tree_utils as TU

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _engine(**kw):
    """Any engine serves: the split calls take their taxon count as an argument."""
    import libsbn_amd as L
    tips = np.random.default_rng(5).integers(0, 4, size=(4, 7)).astype(np.int32)
    return L.Engine(L.PhyloModelSpecification("JC69", "constant", "strict"), tips, np.ones(7), **kw)


@pytest.fixture(scope="module")
def eng():
    return _engine()


_BATCHES = {}


def _batch(n, T, dyadic=False):
    """(parent ids, lengths, the reference's table): computed once, shared, never changed."""
    key = (n, T, dyadic)
    if key not in _BATCHES:
        pids, bls = R.random_batch(n, T, np.random.default_rng(1000 * n + T), dyadic)
        pids.setflags(write=False), bls.setflags(write=False)
        _BATCHES[key] = (pids, bls, R.table(pids))
    return _BATCHES[key]


def _check_table(table, want, n):
    index, splits, first, trees = want
    assert table.split_count == len(splits)
    assert np.array_equal(table.split_index, index)
    assert np.array_equal(table.bits, R.words(splits, n))
    assert np.array_equal(table.first, first) and np.array_equal(table.trees, trees)


SHAPES = [(n, T) for n in (3, 4, 5, 31, 32, 33, 64, 65) for T in (1, 7, 65)] + [(257, 2), (2049, 2)]


@pytest.mark.parametrize("n,T", SHAPES)
def test_table_is_the_references(eng, n, T):
    import libsbn_amd as L
    pids, bls, want = _batch(n, T)
    table = eng.split_index(pids)
    _check_table(table, want, n)
    W = (n + 31) // 32
    assert eng.last_call_path() == f"splits n={n} W={W} store={'lds' if n <= 128 else 'global'}"
    # the trivial split of leaf v has index v; a split never holds taxon 0, no bit at or above n
    assert np.array_equal(table.split_index[0, :n], np.arange(n))
    strings = L.split_strings(table.bits, n)
    assert strings == R.strings(want[1], n) and all(s[0] == "0" for s in strings)
    if n & 31:
        assert not np.any(table.bits[:, -1] >> np.uint32(n & 31))
    # the duplicate of tree 0 and its other rooting share its indices, edge for edge as sets
    if T >= 3:
        assert np.array_equal(table.split_index[T - 1], table.split_index[0])
    if T >= 2 and n >= 4:
        assert set(table.split_index[1][:-2]) == set(table.split_index[0][:-2])
    # no statistics asked for by lengths or weights: counts in column 0, zeros beside them
    assert np.array_equal(table.stats[:, 0], want[3].astype(float)) and not np.any(table.stats[:, 1:])


@pytest.mark.parametrize("n,T,keep", [(5, 7, 3), (33, 65, 40), (65, 7, 1), (257, 2, 1)])
def test_appending_trees_changes_nothing_earlier(eng, n, T, keep):
    pids, bls, want = _batch(n, T)
    whole, head = eng.split_index(pids, bls), eng.split_index(pids[:keep], bls[:keep])
    S = head.split_count
    assert np.array_equal(whole.split_index[:keep], head.split_index)
    assert np.array_equal(whole.bits[:S], head.bits) and np.array_equal(whole.first[:S], head.first)


def test_rows_at_and_above_the_count_stay_untouched(eng):
    from libsbn_amd.engine import _ptr
    pids, bls, want = _batch(12, 8)
    T, E, S = 8, 21, len(want[1])
    cap = T * E
    index, count = np.empty((T, E + 2), np.int32), np.zeros(1, np.int32)
    bits, first, trees = np.full((cap, 1), 0xABCD, np.uint32), np.full(cap, -7, np.int32), np.full(cap, -7, np.int32)
    stats = np.full((cap, 3), -7.0)
    assert eng._lib.mi_engine_split_index(eng._h, T, 12, _ptr(np.ascontiguousarray(pids)), None, None, cap, _ptr(index),
                                          _ptr(count), _ptr(bits), _ptr(first), _ptr(trees), _ptr(stats)) == 0
    assert count[0] == S < cap
    assert np.all(bits[S:] == 0xABCD) and np.all(first[S:] == -7) and np.all(trees[S:] == -7) and np.all(stats[S:] == -7.0)
    assert np.array_equal(first[:S], want[2])


def test_collision_path_gives_the_same_bytes(monkeypatch):
    """Hash bits 0: every split starts at slot 0 and probes linearly; 4: sixteen home slots."""
    pids, bls, want = _batch(12, 8)
    w = np.arange(1.0, 9.0)
    ref = _engine().split_index(pids, bls, w)
    _check_table(ref, want, 12)
    for bits in ("0", "4"):
        monkeypatch.setenv("MI_PHYLO_SPLIT_HASH_BITS", bits)
        got = _engine().split_index(pids, bls, w)
        for name in ("split_index", "bits", "first", "trees", "stats"):
            assert getattr(got, name).tobytes() == getattr(ref, name).tobytes(), (bits, name)


@pytest.mark.parametrize("n,T", [(5, 7), (33, 65), (65, 7), (257, 2)])
def test_statistics_are_exact_with_dyadic_inputs(eng, n, T):
    """Integer weights and lengths that are multiples of 2^-10: every product and sum is exact."""
    pids, bls, want = _batch(n, T, dyadic=True)
    w = np.random.default_rng(n).integers(1, 5, size=T).astype(float)
    table = eng.split_index(pids, bls, w)
    _check_table(table, want, n)
    ref = R.stats(want[0], len(want[1]), bls, w)
    assert table.stats.tobytes() == ref.tobytes()
    assert table.stats.tobytes() == R.stats(want[0], len(want[1]), bls, w, ordered=True).tobytes()
    unweighted = eng.split_index(pids, bls)
    assert unweighted.stats.tobytes() == R.stats(want[0], len(want[1]), bls, None).tobytes()


@pytest.mark.parametrize("n,T", [(5, 7), (33, 65), (100, 7)])
def test_statistics_with_random_doubles(eng, n, T):
    import torch
    pids, bls, want = _batch(n, T)
    rng = np.random.default_rng(7 * n)
    w = rng.uniform(0.1, 2.0, T)
    S = len(want[1])
    table = eng.split_index(pids, bls, w)
    ref = R.stats(want[0], S, bls, w)
    assert np.all(np.abs(table.stats - ref) <= 1e-14 * np.abs(ref))
    # the stated order: one accumulator in ascending tree order, bit for bit
    assert table.stats.tobytes() == R.stats(want[0], S, bls, w, ordered=True).tobytes()
    assert eng.split_index(pids, bls, w).stats.tobytes() == table.stats.tobytes()
    # the same trees followed by extra trees: the rows of the shared splits
    extra = TU.random_trees(n, 3, rng)
    longer = eng.split_index(np.concatenate([pids, extra[0]]), np.concatenate([bls, extra[1]]),
                             np.concatenate([w, np.zeros(3)]))
    assert longer.stats[:S].tobytes() == table.stats.tobytes()
    # ... and with weights of their own: the rows of the splits they do not hold
    heavier = eng.split_index(np.concatenate([pids, extra[0]]), np.concatenate([bls, extra[1]]),
                              np.concatenate([w, np.ones(3)]))
    untouched = np.setdiff1d(np.arange(S), heavier.split_index[T:, :-2])
    assert len(untouched) > 0 and heavier.stats[untouched].tobytes() == table.stats[untouched].tobytes()
    # the device form
    dev = torch.device("cuda", 0)
    E, cap = 2 * n - 3, T * (2 * n - 3)
    d = {k: torch.from_numpy(np.array(v)).to(dev) for k, v in (("pid", pids), ("bl", bls), ("w", w))}
    o_index = torch.zeros((T, E + 2), dtype=torch.int32, device=dev)
    o_count = torch.zeros(1, dtype=torch.int32, device=dev)
    o_bits = torch.zeros((cap, (n + 31) // 32), dtype=torch.int32, device=dev)
    o_first, o_trees = (torch.zeros(cap, dtype=torch.int32, device=dev) for _ in range(2))
    o_stats = torch.zeros((cap, 3), dtype=torch.float64, device=dev)
    eng.split_index_device(None, T, n, d["pid"].data_ptr(), cap, o_index.data_ptr(), o_count.data_ptr(),
                           o_bits.data_ptr(), o_first.data_ptr(), o_trees.data_ptr(), o_stats.data_ptr(),
                           d["bl"].data_ptr(), d["w"].data_ptr())
    eng.check_status()
    assert int(o_count.cpu()[0]) == S
    assert o_stats.cpu().numpy()[:S].tobytes() == table.stats.tobytes()
    assert np.array_equal(o_index.cpu().numpy(), want[0])


RF_SHAPES = [(n, T) for n in (3, 4, 5, 33, 100) for T in (1, 2, 64, 65)]


@pytest.mark.parametrize("n,T", RF_SHAPES)
def test_rf_and_branch_score_are_the_references(eng, n, T):
    pids, bls, want = _batch(n, T, dyadic=True)
    index = want[0]
    rf, bs = eng.rf_distances(index, bls)
    assert np.array_equal(rf, R.rf(index, n))
    assert np.array_equal(rf, rf.T) and not np.any(np.diag(rf)) and np.array_equal(eng.rf_distances(index), rf)
    # dyadic lengths: every term and sum is exact
    assert bs.tobytes() == R.branch_score(index, bls).tobytes()
    assert np.array_equal(bs, bs.T) and not np.any(np.diag(bs))
    if T >= 2 and n >= 4:
        assert rf[0, 1] == 0  # two rootings of one tree
    if T >= 3:
        assert rf[0, T - 1] == 0  # the duplicate of tree 0
    # random doubles: 1e-13 relative to the exactly rounded sum, and the stated order bit for bit
    pids2, bls2, want2 = _batch(n, T)
    rf2, bs2 = eng.rf_distances(want2[0], bls2)
    exact = R.branch_score(want2[0], bls2)
    assert np.array_equal(rf2, R.rf(want2[0], n))
    assert np.all(np.abs(bs2 - exact) <= 1e-13 * np.abs(exact))
    assert bs2.tobytes() == R.branch_score(want2[0], bls2, ordered=True).tobytes()
    assert np.array_equal(bs2, bs2.T) and not np.any(np.diag(bs2))
    # a pair's result depends neither on T nor on its place in the launch
    if T >= 64:
        pick = [T - 1, 5, 0]
        sub_index = eng.split_index(pids2[pick]).split_index
        assert np.array_equal(eng.rf_distances(sub_index), rf2[np.ix_(pick, pick)])


@pytest.mark.parametrize("n", [4, 5, 33, 100])
def test_rf_of_an_nni_neighbour_is_two(eng, n):
    import libsbn_amd as L
    rng = np.random.default_rng(n)
    pids, bls = TU.random_trees(n, 1, rng)
    trees, lengths = [pids[0]], [bls[0]]
    for v in sorted({n, (3 * n - 3) // 2, 2 * n - 4}):
        for which in (0, 1):
            p, b = L.nni_neighbour(n, pids[0], bls[0], v, which)
            trees.append(p), lengths.append(b)
    for v in range(n, min(2 * n - 3, n + 3)):
        p, b = R.reroot(pids[0], bls[0], v)
        trees.append(p), lengths.append(b)
    table = eng.split_index(np.stack(trees), np.stack(lengths))
    rf, bs = eng.rf_distances(table.split_index, np.stack(lengths))
    moved = len(trees) - min(2 * n - 3, n + 3) + n
    assert np.all(rf[0, 1:moved] == 2) and np.all(rf[0, moved:] == 0) and np.all(bs[0, moved:] == 0.0)


def test_index_array_is_the_reduced_gradient_calls_branch_index():
    """16 DS1-shaped trees, several sharing splits: out_split_index handed over as branch_index
    with index_count = S gives the host scatter-add of the per-tree branch gradients by the
    reference's split sets (the tolerance of the reduced call's own test)."""
    import libsbn_amd as L
    import oracle_lib as O
    tips, w, pids, bls = O.struct_arrays(O.load_struct("ds1_sub10"))
    n, T = 27, 16
    rng = np.random.default_rng(3)
    extra, extra_bl = TU.random_trees(n, 3, rng)
    rerooted = [R.reroot(pids[k], bls[k], int(rng.integers(n, 2 * n - 3))) for k in (1, 2, 3)]
    pids = np.concatenate([pids, extra, np.stack([r[0] for r in rerooted])])
    bls = np.concatenate([bls, extra_bl, np.stack([r[1] for r in rerooted])])
    assert pids.shape == (T, 2 * n - 3)
    eng = L.Engine(L.PhyloModelSpecification("JC69", "weibull+4", "strict"), tips, w)
    pr = np.ones((T, 2))
    pr[:, 0] = rng.uniform(0.3, 1.5, T)
    tw = rng.uniform(0.1, 2.0, T)
    table = eng.split_index(pids, bls, tw)
    index, splits, first, trees = R.table(pids)
    S = len(splits)
    assert np.array_equal(table.split_index, index) and table.split_count == S and S < T * (2 * n - 3)
    per_tree = np.stack([g.gradient["branch_lengths"] for g in eng.gradients(pids, bls, pr)])
    for weights in (None, tw):
        wt = np.ones(T) if weights is None else weights
        want = np.zeros(S)
        for t in range(T):
            for v, s in enumerate(R.edge_splits(pids[t])):
                want[splits.index(s)] += wt[t] * per_tree[t][v]
        _, _, ig, _ = eng.gradients_reduced(pids, bls, pr, table.split_index, S, weights)
        assert np.max(np.abs(ig - want)) <= 1e-10 * np.max(np.abs(want))


def test_refused_trees_are_named(eng):
    pids, bls, want = _batch(12, 8)
    bad = np.array(pids)
    bad[5, 3] = 2  # a leaf as a parent
    with pytest.raises(RuntimeError, match=r"not in the reference's post-order id form \(tree 5\)"):
        eng.split_index(bad)
    # a root of degree 2: one of the root's three children moved under another
    n = 6
    two = np.array([[6, 6, 7, 7, 8, 8, 9, 9, 9]], np.int32)
    assert eng.split_index(two).split_count == 9
    two[0, 8 - 1] = 8  # node 7 now hangs under node 8: three children there, two at the root
    with pytest.raises(RuntimeError, match=r"\(tree 0\)"):
        eng.split_index(two)
    batch = np.concatenate([np.array(_batch(n, 7)[0][:3]), two])
    with pytest.raises(RuntimeError, match=r"\(tree 3\)"):
        eng.split_index(batch)
    # the engine goes on
    _check_table(eng.split_index(pids), want, 12)


def test_capacity_one_short_is_refused_with_the_count(eng):
    import torch
    pids, bls, want = _batch(12, 8)
    S = len(want[1])
    assert eng.split_index(pids, split_capacity=S).split_count == S
    with pytest.raises(RuntimeError, match=rf"split_capacity \(S = {S}\)"):
        eng.split_index(pids, split_capacity=S - 1)
    # the device form reports it through the status word and writes no row past the capacity
    dev = torch.device("cuda", 0)
    cap = S - 1
    d_pid = torch.from_numpy(np.array(pids)).to(dev)
    o_index = torch.zeros((8, 23), dtype=torch.int32, device=dev)
    o_count = torch.zeros(1, dtype=torch.int32, device=dev)
    o_rows = torch.full((3, cap + 4), -7, dtype=torch.int32, device=dev)
    eng.split_index_device(None, 8, 12, d_pid.data_ptr(), cap, o_index.data_ptr(), o_count.data_ptr(),
                           o_rows[0].data_ptr(), o_rows[1].data_ptr(), o_rows[2].data_ptr())
    with pytest.raises(RuntimeError, match=rf"split_capacity \(S = {S}\)"):
        eng.check_status()
    rows = o_rows.cpu().numpy()
    assert int(o_count.cpu()[0]) == S and np.all(rows[:, cap:] == -7)
    assert np.array_equal(rows[1, :cap], want[2][:cap])
    eng.check_status()


def test_device_form_replays_from_a_graph():
    import torch
    n, T = 33, 7
    pids, bls, want = _batch(n, T)
    w = np.arange(1.0, T + 1)
    first = _engine()
    ref = first.split_index(pids, bls, w)
    ref_rf, ref_bs = first.rf_distances(ref.split_index, bls)
    S, E, cap = ref.split_count, 2 * n - 3, T * (2 * n - 3)
    dev = torch.device("cuda", 0)
    d_pid, d_bl, d_w = (torch.from_numpy(np.array(x)).to(dev) for x in (pids, bls, w))
    o_index = torch.zeros((T, E + 2), dtype=torch.int32, device=dev)
    o_count = torch.zeros(1, dtype=torch.int32, device=dev)
    o_bits = torch.zeros((cap, 2), dtype=torch.int32, device=dev)
    o_first, o_trees = (torch.zeros(cap, dtype=torch.int32, device=dev) for _ in range(2))
    o_stats = torch.zeros((cap, 3), dtype=torch.float64, device=dev)
    o_rf = torch.zeros((T, T), dtype=torch.int32, device=dev)
    o_bs = torch.zeros((T, T), dtype=torch.float64, device=dev)
    gs = torch.cuda.Stream()

    def call(stream, engine):
        engine.split_index_device(stream, T, n, d_pid.data_ptr(), cap, o_index.data_ptr(), o_count.data_ptr(),
                                  o_bits.data_ptr(), o_first.data_ptr(), o_trees.data_ptr(), o_stats.data_ptr(),
                                  d_bl.data_ptr(), d_w.data_ptr())
        engine.rf_distances_device(stream, T, n, o_index.data_ptr(), o_rf.data_ptr(), o_bs.data_ptr(),
                                   d_bl.data_ptr())

    # (the other engine runs the same calls on the stream first: the kernels' code objects are
    # loaded -- into device memory -- at their first launch, which is not the engine's allocation)
    call(gs.cuda_stream, first)
    torch.cuda.synchronize()
    fresh = _engine()
    fresh.reserve_splits(T, n)
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info(0)[0]
    with torch.cuda.stream(gs):
        call(gs.cuda_stream, fresh)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info(0)[0] == free_before  # (reserved: the calls allocated nothing)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=gs):
        call(torch.cuda.current_stream().cuda_stream, fresh)
    for _ in range(2):
        for o in (o_index, o_count, o_bits, o_first, o_trees, o_stats, o_rf, o_bs):
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert int(o_count.cpu()[0]) == S
        assert o_index.cpu().numpy().tobytes() == ref.split_index.tobytes()
        assert o_bits.cpu().numpy()[:S].tobytes() == ref.bits.tobytes()
        assert o_first.cpu().numpy()[:S].tobytes() == ref.first.tobytes()
        assert o_trees.cpu().numpy()[:S].tobytes() == ref.trees.tobytes()
        assert o_stats.cpu().numpy()[:S].tobytes() == ref.stats.tobytes()
        assert o_rf.cpu().numpy().tobytes() == ref_rf.tobytes() and o_bs.cpu().numpy().tobytes() == ref_bs.tobytes()
    fresh.check_status()


@pytest.mark.parametrize("n", [5, 33, 257])
def test_support_of_a_tree_among_its_own_copies_is_one(eng, n):
    rng = np.random.default_rng(n)
    pids, bls = TU.random_trees(n, 2, rng)
    copies = np.stack([pids[0]] * 3 + [R.reroot(pids[0], bls[0], 2 * n - 4)[0]])
    assert np.all(eng.split_support(pids[0], copies) == 1.0)
    assert np.all(eng.split_support(pids[0], copies, tree_weights=[0.5, 1.0, 2.0, 0.25]) == 1.0)
    # among copies and one other tree: 1 on the shared edges, 4/5 elsewhere
    mixed = eng.split_support(pids[0], np.concatenate([copies, pids[1:]]))
    shared = np.array([s in set(R.edge_splits(pids[1])) for s in R.edge_splits(pids[0])])
    assert np.all(mixed[shared] == 1.0) and np.all(mixed[~shared] == 0.8)


def test_sharded_handle_lets_its_first_shard_do_the_work():
    pids, bls, want = _batch(12, 8)
    many = _engine(shard_devices=[0, 0])
    table = many.split_index(pids, bls)
    _check_table(table, want, 12)
    assert np.array_equal(many.rf_distances(table.split_index), R.rf(want[0], 12))


def test_cpp_adapter(tmp_path):
    exe = tmp_path / "splits_example"
    lib = os.path.join(REPO, "libsbn_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(REPO, "tests/cpp/splits_example.cpp"),
                    "-L" + lib, "-lmi_phylo", "-lmi_phylo_host", "-Wl,-rpath," + lib, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe), os.path.join(REPO, "tests/golden/data")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all checks passed" in out.stdout
