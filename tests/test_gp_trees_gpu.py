"""Trees of the subsplit DAG on the device against tests/gp_trees_ref.py: the
index, log q, the GP lengths, the rooted TrainSimpleAverage, the sampler, the enumerator and
de-rooting; the identity M_p = sum_tau q(tau) L_p(tau | b) through the library's own calls; the
DAG-only object; what is refused."""
import csv
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

import gp_ref as R
import gp_trees_ref as TR
import tree_utils as TU

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10   # relative to max(1, |ref|): the project's bound against its oracle

GTR_RATES = np.array([0.10, 0.27, 0.08, 0.12, 0.31, 0.12])
GTR_FREQS = np.array([0.34, 0.16, 0.21, 0.29])
MODELS = {"JC69": lambda: R.Model(), "GTR": lambda: R.Model(GTR_RATES, GTR_FREQS)}
_engines = {}


def _lib():
    import libsbn_amd as L
    return L


def _plain_engine(n, subst="JC69", site="constant", P=4):
    """an engine of n taxa that only has to exist (the tree calls read no pattern)"""
    key = (n, subst, site, P)
    if key not in _engines:
        L = _lib()
        rng = np.random.default_rng(n)
        if subst == "WAG":
            import aa_utils as A
            tips, w = A.random_aa_alignment(n, P, rng)
        else:
            tips, w = TU.random_alignment(n, P, rng)
        _engines[key] = L.Engine(L.PhyloModelSpecification(subst, site, "strict"), np.asarray(tips, np.int32), np.asarray(w, float),
                                 device=0)
    return _engines[key]


def _model_engine(tips, w, subst):
    L = _lib()
    eng = L.Engine(L.PhyloModelSpecification(subst, "constant", "strict"), np.asarray(tips, np.int32), np.asarray(w, float), device=0)
    row = np.ones(eng.param_count)
    for start, length in eng.block_specification().values():
        if length == 6:
            row[start:start + 6] = GTR_RATES
        elif length == 4:
            row[start:start + 4] = GTR_FREQS
    return eng, row


def _close(x, ref, tol=TOL):
    x, ref = np.asarray(x, float), np.asarray(ref, float)
    return np.all(np.abs(x - ref) <= tol * np.maximum(1.0, np.abs(ref)))


def _lengths(d, seed):
    b = np.random.default_rng(seed).uniform(0.02, 0.4, d.G)
    b[:d.R] = 0.0
    return b


def _ds1_rooted(count):
    st = json.load(open(os.path.join(REPO, "tests", "golden", "ds1_top100.struct.json")))
    return np.stack([R.root_above_leaf0(t["parent_ids"]) for t in st["trees"][:count]])


def _batch(n, T, seed):
    """T rooted trees of n taxa: a caterpillar, a balanced tree, then NNI batches (DS1's topologies at 27)"""
    if n == 27:
        return _ds1_rooted(T)
    rng = np.random.default_rng(seed)
    trees = [TU.ladder_topology(n, rooted=True), TU.balanced_topology(n, rooted=True)][:T]
    if T > 2:
        trees += list(R.nni_batch(n, T - 2, 2 if n > 3 else 1, rng))
    return np.stack(trees).astype(np.int32)


def _load_trees(nwk):
    L = _lib()
    tc = L._hostapi.TreeCollection.of_newick_file(os.path.join(R.GOLDEN, nwk))
    return np.stack(tc.parent_ids).astype(np.int32)


def _check_built(d, gp, got, pids_ref, entries_ref, q, b):
    """sampled or enumerated trees against the restatement's, and against the index and log q calls"""
    assert got.parent_ids.tobytes() == np.ascontiguousarray(pids_ref).tobytes()
    assert got.entries.tobytes() == np.ascontiguousarray(entries_ref).tobytes()
    assert _close(got.log_q, [TR.log_q(d, q, e) for e in entries_ref])
    assert _close(got.branch_lengths, [TR.branch_lengths(d, b, e, 0.0) for e in entries_ref])
    again = gp.tree_index(got.parent_ids)
    assert again.entries.tobytes() == got.entries.tobytes() and (again.nodes >= 0).all()
    assert gp.tree_log_prob(got.entries).tobytes() == got.log_q.tobytes()
    assert gp.tree_branch_lengths(got.entries, 7.0).tobytes() == got.branch_lengths.tobytes()


# ---- 1. exactness against the restatement, at every clade-word boundary ----
@pytest.mark.parametrize("n,T", [(3, 1), (4, 7), (5, 65), (27, 7), (32, 7), (33, 65), (64, 7), (65, 65)])
def test_index_sample_enumerate_match_the_restatement(n, T):
    pids = _batch(n, T, 100 + n)
    dag_trees = pids[::2]   # (the other trees may leave the DAG: sentinels)
    d = R.build_dag(dag_trees)
    eng = _plain_engine(n)
    gp = eng.gp_create_dag(dag_trees)
    rng = np.random.default_rng(n)
    q, b = R.random_q(d, rng), _lengths(d, n)
    gp.set_sbn_parameters(q)
    gp.set_branch_lengths(b)
    got = gp.tree_index(pids)
    assert eng.last_call_path() == f"gp_trees n={n} T={T} store=lds"
    ent_ref, nodes_ref = TR.index_batch(d, pids)
    assert got.nodes.tobytes() == nodes_ref.tobytes()
    assert got.entries.tobytes() == ent_ref.tobytes()
    assert (ent_ref[::2] < d.G).all()
    lq = gp.tree_log_prob(got.entries)
    ref = np.array([TR.log_q(d, q, e) for e in ent_ref])
    assert not np.isnan(lq).any() and np.array_equal(np.isinf(lq), np.isinf(ref))
    assert _close(lq[np.isfinite(ref)], ref[np.isfinite(ref)])
    assert _close(gp.tree_branch_lengths(got.entries, 3.5), [TR.branch_lengths(d, b, e, 3.5) for e in ent_ref])
    # the sampler
    K = T
    s = gp.sample_trees(K, seed=77, first_sample=5, cdf=True)
    cdf = TR.cdf(d, q)
    assert s.cdf.tobytes() == cdf.tobytes()
    built = [TR.sample_tree(d, cdf, 77, 5 + k) for k in range(K)]
    _check_built(d, gp, s, np.stack([p for p, _ in built]), np.stack([e for _, e in built]), q, b)
    # the enumerator: the first trees and the last ones
    total = gp.topology_count()
    assert total == int(round(d.topology_count)) or d.topology_count > 2 ** 53
    ranks = sorted(set(range(min(total, 4))) | set(range(max(total - 3, 0), total)))
    for first, count in ((ranks[0], min(total, 4)), (max(total - 3, 0), total - max(total - 3, 0))):
        e = gp.enumerate_trees(first, count)
        built = [TR.number_tree(d.n, *TR.unrank(d, r)) for r in range(first, first + count)]
        _check_built(d, gp, e, np.stack([p for p, _ in built]), np.stack([x for _, x in built]), q, b)
    gp.close()


def test_the_global_store_serves_257_taxa():
    n = 257
    pids = np.stack([TU.ladder_topology(n, rooted=True), TU.balanced_topology(n, rooted=True)]).astype(np.int32)
    d = R.build_dag(pids[:1])
    eng = _plain_engine(n)
    gp = eng.gp_create_dag(pids[:1])
    got = gp.tree_index(pids)
    assert eng.last_call_path() == f"gp_trees n={n} T=2 store=global"
    ent_ref, nodes_ref = TR.index_batch(d, pids)
    assert got.nodes.tobytes() == nodes_ref.tobytes() and got.entries.tobytes() == ent_ref.tobytes()
    assert (ent_ref[0] < d.G).all() and (ent_ref[1] == d.G).any()
    q, b = gp.get_sbn_parameters(), gp.get_branch_lengths()
    s = gp.sample_trees(2, seed=3)
    assert eng.last_call_path() == f"gp_trees n={n} T=2 store=global"
    built = [TR.sample_tree(d, TR.cdf(d, q), 3, k) for k in range(2)]
    _check_built(d, gp, s, np.stack([p for p, _ in built]), np.stack([e for _, e in built]), q, b)
    e = gp.enumerate_trees()
    assert len(e.log_q) == 1 and e.parent_ids.tobytes() == s.parent_ids[:1].tobytes() and e.log_q[0] == 0.0
    gp.close()


# ---- 2. DAG shapes ----
def _wide_rootsplit_batch():
    """70 trees of 9 taxa with distinct rootsplits: the rootsplits are a block of 70 entries"""
    n, rng, seen, trees = 9, np.random.default_rng(9), set(), []
    while len(trees) < 70:
        side = frozenset(int(x) for x in np.flatnonzero(rng.integers(0, 2, n - 1)) + 1)
        if not side or side in seen:
            continue
        seen.add(side)

        def caterpillar(taxa):
            t = taxa[0]
            for x in taxa[1:]:
                t = (t, x)
            return t
        trees.append(TU._polish((caterpillar(sorted(side)), caterpillar(sorted(set(range(n)) - side))), n))
    return np.stack(trees).astype(np.int32)


@pytest.mark.parametrize("shape", ["wide", "one_tree"])
def test_dag_shapes(shape):
    pids = _wide_rootsplit_batch() if shape == "wide" else _batch(6, 1, 1)
    n = pids.shape[1] // 2 + 1
    d = R.build_dag(pids)
    assert d.R == (70 if shape == "wide" else 1)
    gp = _plain_engine(n).gp_create_dag(pids)
    q, b = R.random_q(d, np.random.default_rng(2)), _lengths(d, 2)
    gp.set_sbn_parameters(q)
    gp.set_branch_lengths(b)
    ent_ref, nodes_ref = TR.index_batch(d, pids)
    got = gp.tree_index(pids)
    assert got.entries.tobytes() == ent_ref.tobytes() and got.nodes.tobytes() == nodes_ref.tobytes()
    s = gp.sample_trees(65, seed=11, cdf=True)
    cdf = TR.cdf(d, q)
    assert s.cdf.tobytes() == cdf.tobytes()
    built = [TR.sample_tree(d, cdf, 11, k) for k in range(65)]
    _check_built(d, gp, s, np.stack([p for p, _ in built]), np.stack([e for _, e in built]), q, b)
    e = gp.enumerate_trees()
    pid_ref, ent_all = TR.enumerate_numbered(d)
    _check_built(d, gp, e, pid_ref, ent_all, q, b)
    assert abs(np.sum(np.exp(e.log_q)) - 1.0) < 1e-12
    gp.close()


# ---- 3. sentinels ----
@pytest.mark.parametrize("case", [0, 2])
def test_nni_neighbours_that_leave_the_dag(case):
    pids, _, _ = R.random_case(case)
    d = R.build_dag(pids)
    gp = _plain_engine(d.n).gp_create_dag(pids)
    near = np.concatenate([TR.nni_neighbours(p) for p in pids[:2]])
    ent_ref, nodes_ref = TR.index_batch(d, near)
    assert (ent_ref == d.G).any() and (ent_ref[(ent_ref == d.G).any(axis=1)] < d.G).any()
    got = gp.tree_index(near)
    assert got.entries.tobytes() == ent_ref.tobytes() and got.nodes.tobytes() == nodes_ref.tobytes()
    lq = gp.tree_log_prob(got.entries)
    outside = (ent_ref == d.G).any(axis=1)
    assert not np.isnan(lq).any() and (lq[outside] == -np.inf).all() and np.isfinite(lq[~outside]).all()
    q_before = gp.get_sbn_parameters()
    with pytest.raises(RuntimeError, match=r"outside the DAG \(tree \d+\)") as err:
        gp.train_simple_average(got.entries)
    assert outside[int(re.search(r"tree (\d+)", str(err.value)).group(1))]   # (whichever such tree reported first)
    assert gp.get_sbn_parameters().tobytes() == q_before.tobytes()
    gp.close()


# ---- 4. values ----
@pytest.mark.parametrize("weighted", [False, True])
def test_simple_average_against_the_restatement(weighted):
    pids, _, _ = R.random_case(3)
    d = R.build_dag(pids)
    gp = _plain_engine(d.n).gp_create_dag(pids)
    trees = gp.enumerate_trees()   # (every tree of the DAG, some weight each: blocks of several entries)
    rng = np.random.default_rng(8)
    pick = rng.integers(0, len(trees.log_q), 65)
    w = rng.uniform(0.0, 2.0, 65) if weighted else None
    q = gp.train_simple_average(trees.entries[pick], w)
    assert _close(q, TR.simple_average(d, trees.entries[pick], w))
    assert gp.get_sbn_parameters().tobytes() == q.tobytes()
    gp.close()


def _named(gp, d, values):
    return {s: float(values[i]) for i, s in enumerate(gp.strings()) if i < d.R or set(s.split("|")[2]) != {"0"}}


def test_the_reference_known_answers_through_the_device_call():
    from test_gp_trees_ref import FIVE_TAXON_SA
    pids = _load_trees("five_taxon_rooted.nwk")
    d = R.build_dag(pids)
    gp = _plain_engine(5).gp_create_dag(pids)
    q = gp.train_simple_average(gp.tree_index(pids).entries)
    got = _named(gp, d, q)
    assert set(got) == set(FIVE_TAXON_SA)
    for name, value in FIVE_TAXON_SA.items():
        assert abs(got[name] - value) <= 1e-12
    # the rooted indexer representation of ((0,1),(2,(3,4)))
    names = gp.strings()
    ent = gp.tree_index(np.array([5, 5, 7, 6, 6, 8, 7, 8], np.int32)).entries[0]
    assert {names[e] for e in ent if e < d.R or set(names[e].split("|")[2]) != {"0"}} == \
        {"00111", "11000|00111|00011", "00100|00011|00001", "00111|11000|01000"}
    trees = gp.enumerate_trees()
    assert len(trees.log_q) == 4 and len({p.tobytes() for p in trees.parent_ids}) == 4
    assert abs(np.sum(np.exp(trees.log_q)) - 1.0) < 1e-12
    gp.close()
    # the 20-taxon sample against the reference's CSV, at its 1e-6
    pids = _load_trees("rooted_simple_average.nwk")
    d = R.build_dag(pids)
    gp = _plain_engine(20).gp_create_dag(pids)
    q = gp.train_simple_average(gp.tree_index(pids).entries)
    with open(os.path.join(R.GOLDEN, "rooted_simple_average_results.csv")) as f:
        correct = {row[0].replace("|", ""): float(row[1]) for row in csv.reader(f) if row}
    got = _named(gp, d, q)
    assert {name.replace("|", "") for name in got} == set(correct)
    for name, value in got.items():
        assert abs(value - correct[name.replace("|", "")]) < 1e-6
    gp.close()


# ---- 5. the identity M_p = sum_tau q(tau) L_p(tau | b), through the library's own calls ----
IDENTITY = {"five": ("five_taxon_rooted.nwk", "five_taxon.fasta"), "hello2": ("hello_rooted_two_trees.nwk", "hello.fasta")}


@pytest.mark.parametrize("subst", ["JC69", "GTR"])
@pytest.mark.parametrize("case", list(IDENTITY) + [f"random{i}" for i in range(len(R.RANDOM_CASES))])
def test_the_marginal_is_the_mixture_of_its_trees(case, subst):
    if case in IDENTITY:
        pids, _, tips, w, _ = R.load_case(*IDENTITY[case])
    else:
        pids, tips, w = R.random_case(int(case[len("random"):]))
    d = R.build_dag(pids)
    eng, row = _model_engine(tips, w, subst)
    gp = eng.gp_create(pids, params=row)
    q, b = R.random_q(d, np.random.default_rng(5)), _lengths(d, 3)
    gp.set_sbn_parameters(q)
    gp.set_branch_lengths(b)
    trees = gp.enumerate_trees()
    assert len(trees.log_q) == int(d.topology_count)
    un = eng.deroot_trees(trees.parent_ids, trees.branch_lengths)
    _, s = eng.pattern_log_likelihoods(un.parent_ids, un.branch_lengths, np.tile(row, (len(trees.log_q), 1)))
    mix, _ = eng.pattern_mixture(s, w, tree_log_weights=trees.log_q)
    got = gp.likelihoods(per_pattern=True, matrix=True)
    assert _close(mix, got.pattern_log_marginal)
    # restricted to the trees through an entry e: exp(matrix[e]) q_e
    for e in sorted({0, d.R, d.G // 2, d.G - 1}):
        through = (trees.entries == e).any(axis=1)
        assert through.any()
        part, _ = eng.pattern_mixture(s[through], w, tree_log_weights=trees.log_q[through])
        assert _close(part, got.matrix[e] + math.log(q[e]))
    gp.close()


def test_deroot_follows_the_restatement():
    rng = np.random.default_rng(4)
    for n, T in ((3, 3), (5, 7), (33, 65)):
        pids = _batch(n, T, n)
        bl = rng.uniform(0.1, 1.0, (T, 2 * n - 1))
        bl[:, -1] = 0.0
        got = _plain_engine(n).deroot_trees(pids, bl)
        for t in range(T):
            pid, lengths, edge = TR.deroot(pids[t], bl[t])
            assert got.parent_ids[t].tobytes() == pid.tobytes() and got.root_edge[t] == edge
            assert got.branch_lengths[t].tobytes() == lengths.tobytes()
    plain = _plain_engine(5).deroot_trees(_batch(5, 7, 5))
    assert plain.branch_lengths is None and plain.parent_ids.tobytes() == _plain_engine(5).deroot_trees(_batch(5, 7, 5), np.ones((7, 9))).parent_ids.tobytes()


# ---- 6. bits ----
def test_a_sample_depends_on_seed_and_number_alone():
    pids = _ds1_rooted(20)
    gp = _plain_engine(27).gp_create_dag(pids)
    whole = gp.sample_trees(65, seed=9, first_sample=100)
    parts = [gp.sample_trees(k, seed=9, first_sample=f) for f, k in ((100, 10), (110, 30), (140, 25))]
    for name in ("parent_ids", "entries", "log_q", "branch_lengths"):
        assert np.concatenate([getattr(p, name) for p in parts]).tobytes() == getattr(whole, name).tobytes()
    for k in (0, 31, 64):
        alone = gp.sample_trees(1, seed=9, first_sample=100 + k)
        assert alone.parent_ids.tobytes() == whole.parent_ids[k].tobytes() and alone.log_q[0] == whole.log_q[k]
    assert gp.sample_trees(65, seed=10, first_sample=100).parent_ids.tobytes() != whole.parent_ids.tobytes()
    gp.close()


def test_graph_replay_gives_the_same_bits():
    import torch
    n, K = 27, 65
    pids = _ds1_rooted(20)
    eng = _plain_engine(n)
    gp = eng.gp_create_dag(pids)
    G = gp.entry_count
    host_s, host_e = gp.sample_trees(K, seed=4, first_sample=2, cdf=True), gp.enumerate_trees(1, K)   # (this DAG has 66 topologies)
    host_i = gp.tree_index(host_s.parent_ids)
    host_d = eng.deroot_trees(host_e.parent_ids, host_e.branch_lengths)
    gp.reserve_trees(K)
    eng.reserve_deroot(K, n)
    dev = "cuda:0"
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)   # noqa: E731
    f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)  # noqa: E731
    sp, se, sq, sb, sc = i32(K, 2 * n - 2), i32(K, 2 * n - 1), f64(K), f64(K, 2 * n - 1), f64(G)
    ep, ee, eq, eb = i32(K, 2 * n - 2), i32(K, 2 * n - 1), f64(K), f64(K, 2 * n - 1)
    ie, inodes, iq, ib = i32(K, 2 * n - 1), i32(K, 2 * n - 1), f64(K), f64(K, 2 * n - 1)
    dp, db, de = i32(K, 2 * n - 3), f64(K, 2 * n - 2), i32(K)
    outputs = [sp, se, sq, sb, sc, ep, ee, eq, eb, ie, inodes, iq, ib, dp, db, de]
    gs = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=gs):
        s = torch.cuda.current_stream().cuda_stream
        gp.sample_trees_device(s, K, 4, 2, sp.data_ptr(), se.data_ptr(), sq.data_ptr(), sb.data_ptr(), sc.data_ptr())
        gp.enumerate_trees_device(s, 1, K, ep.data_ptr(), ee.data_ptr(), eq.data_ptr(), eb.data_ptr())
        gp.tree_index_device(s, K, sp.data_ptr(), ie.data_ptr(), inodes.data_ptr())
        gp.tree_log_prob_device(s, K, ie.data_ptr(), iq.data_ptr())
        gp.tree_branch_lengths_device(s, K, ie.data_ptr(), 0.0, ib.data_ptr())
        eng.deroot_trees_device(s, K, n, ep.data_ptr(), eb.data_ptr(), dp.data_ptr(), db.data_ptr(), de.data_ptr())
    torch.cuda.synchronize()
    expected = [host_s.parent_ids, host_s.entries, host_s.log_q, host_s.branch_lengths, host_s.cdf, host_e.parent_ids,
                host_e.entries, host_e.log_q, host_e.branch_lengths, host_i.entries, host_i.nodes, host_s.log_q,
                host_s.branch_lengths, host_d.parent_ids, host_d.branch_lengths, host_d.root_edge]
    for _ in range(2):
        for o in outputs:
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for o, ref in zip(outputs, expected):
            assert o.cpu().numpy().tobytes() == np.ascontiguousarray(ref).tobytes()
    eng.check_status()
    del graph
    gp.close()


# ---- 7. the DAG-only object ----
@pytest.mark.parametrize("kind", ["four_categories", "twenty_states"])
def test_dag_only_object(kind):
    L = _lib()
    pids, tips, w = R.random_case(1)
    d = R.build_dag(pids)
    full_eng, row = _model_engine(tips, w, "JC69")
    full_eng.gp_create(pids, params=row).close()   # (whatever an engine reserves at a first creation is the engine's)
    other = _plain_engine(d.n, "JC69", "weibull+4") if kind == "four_categories" else _plain_engine(d.n, "WAG")
    near = np.concatenate([pids, TR.nni_neighbours(pids[0])])
    for eng in (full_eng, other):   # (... and so are the staging blocks of its host calls: the calls below, on a throw-away object)
        prime = eng.gp_create_dag(pids)
        prime.tree_index(near)
        prime.train_simple_average(prime.sample_trees(65, seed=1, cdf=True).entries)
        prime.close()
    held = L._capi.load().mi_device_bytes_held()
    full = full_eng.gp_create(pids, params=row)
    with_full = L._capi.load().mi_device_bytes_held()
    gp = other.gp_create_dag(pids)
    assert with_full < L._capi.load().mi_device_bytes_held() < with_full + (with_full - held)   # (no vectors)
    s, f = gp.structure(), full.structure()
    assert s.entries.tobytes() == f.entries.tobytes() and s.clades.tobytes() == f.clades.tobytes()
    assert gp.strings() == full.strings()
    assert gp.get_sbn_parameters().tobytes() == full.get_sbn_parameters().tobytes()
    assert gp.get_branch_lengths().tobytes() == full.get_branch_lengths().tobytes()
    a, b = gp.tree_index(near), full.tree_index(near)
    assert a.entries.tobytes() == b.entries.tobytes() and a.nodes.tobytes() == b.nodes.tobytes()
    x, y = gp.sample_trees(65, seed=1, cdf=True), full.sample_trees(65, seed=1, cdf=True)
    for name in ("parent_ids", "entries", "log_q", "branch_lengths", "cdf"):
        assert getattr(x, name).tobytes() == getattr(y, name).tobytes()
    assert gp.train_simple_average(x.entries).tobytes() == full.train_simple_average(y.entries).tobytes()
    for call in (gp.populate, gp.likelihoods, gp.branch_derivatives, gp.estimate_sbn_parameters, gp.hybrid_marginals,
                 gp.optimize_branch_lengths, gp.reserve_hybrid):
        with pytest.raises(RuntimeError, match="this object is DAG-only"):
            call()
    gp.close()
    full.close()
    assert L._capi.load().mi_device_bytes_held() == held


# ---- 8. what is refused ----
def test_what_is_refused():
    import torch
    pids, _, _ = R.random_case(0)
    d = R.build_dag(pids)
    eng = _plain_engine(d.n)
    gp = eng.gp_create_dag(pids)
    q = R.random_q(d, np.random.default_rng(1))
    # (the setter refuses such a q; the device holds whatever a kernel or a caller wrote there)
    with pytest.raises(RuntimeError, match="finite and not negative"):
        gp.set_sbn_parameters(np.where(np.arange(d.G) == 1, np.nan, q))
    # a visited block whose parameters are all 0: the rootsplits, then a block below
    gp.set_sbn_parameters(np.where(np.arange(d.G) < d.R, 0.0, q))
    with pytest.raises(RuntimeError, match=r"all 0 \(sample [012], the rootsplits\)"):
        gp.sample_trees(3, seed=1)
    root = int(d.entries[0][2])
    lo, hi = d.block_range[root, 1]
    zero = q.copy()
    zero[:d.R] = 0.0
    zero[0] = 1.0
    zero[lo:hi] = 0.0
    gp.set_sbn_parameters(zero)
    with pytest.raises(RuntimeError, match=rf"all 0 \(sample [012], block of node {root}, clade 1\)"):
        gp.sample_trees(3, seed=1)
    gp.set_sbn_parameters(q)
    total = gp.topology_count()
    with pytest.raises(RuntimeError, match=f"the DAG has {total} topologies"):
        gp.enumerate_trees(total - 1, 2)
    gp.close()
    # a device form beyond the reservation
    gp = eng.gp_create_dag(pids)
    out = torch.zeros(4 * (2 * d.n - 1), dtype=torch.int32, device="cuda:0")
    with pytest.raises(RuntimeError, match="reserved 0"):
        gp.tree_index_device(None, 2, out.data_ptr(), out.data_ptr())
    gp.reserve_trees(2)
    with pytest.raises(RuntimeError, match="of 3 trees, mi_gp_reserve_trees reserved 2"):
        gp.tree_log_prob_device(None, 3, out.data_ptr(), out.data_ptr())
    bad = pids[:1].copy()
    bad[0, 0] = bad[0, 2] if bad[0, 0] != bad[0, 2] else bad[0, 3]
    with pytest.raises(RuntimeError, match=r"\(tree 0\)"):
        gp.tree_index(bad)
    gp.close()


def test_a_refused_reservation_leaves_the_earlier_one_working(monkeypatch):
    """Over MI_PHYLO_PLV_BYTES a batch is refused with the sizes in the message; the caller's smaller batches
    (what the message advises) are served by the reservation that was there, with the right bytes."""
    L = _lib()
    monkeypatch.setenv("MI_PHYLO_PLV_BYTES", "1000000")
    pids, _, _ = R.random_case(1)
    d = R.build_dag(pids)
    tips, w = TU.random_alignment(d.n, 4, np.random.default_rng(0))
    eng = L.Engine(L.PhyloModelSpecification("JC69", "constant", "strict"), np.asarray(tips, np.int32), np.asarray(w, float), device=0)
    gp = eng.gp_create_dag(pids)
    ent_ref, nodes_ref = TR.index_batch(d, pids)
    assert gp.tree_index(pids).entries.tobytes() == ent_ref.tobytes()
    held = L._capi.load().mi_device_bytes_held()
    many = np.tile(pids, (100000 // len(pids), 1))
    with pytest.raises(RuntimeError, match=rf"workspace of {len(many)} trees of {d.n} taxa takes \d+ bytes, over the budget of 1000000 bytes \(MI_PHYLO_PLV_BYTES\)"):
        gp.tree_index(many)
    with pytest.raises(RuntimeError, match="MI_PHYLO_PLV_BYTES"):
        gp.sample_trees(len(many), seed=1)
    with pytest.raises(RuntimeError, match="MI_PHYLO_PLV_BYTES"):
        gp.reserve_trees(len(many))
    # out of range is refused for its range, before anything is reserved
    with pytest.raises(RuntimeError, match=f"the DAG has {gp.topology_count()} topologies"):
        gp.enumerate_trees(0, 10 ** 6)
    assert L._capi.load().mi_device_bytes_held() == held
    got = gp.tree_index(pids)
    assert got.entries.tobytes() == ent_ref.tobytes() and got.nodes.tobytes() == nodes_ref.tobytes()
    q = gp.get_sbn_parameters()
    s = gp.sample_trees(len(pids), seed=6)
    built = [TR.sample_tree(d, TR.cdf(d, q), 6, k) for k in range(len(pids))]
    _check_built(d, gp, s, np.stack([p for p, _ in built]), np.stack([e for _, e in built]), q, gp.get_branch_lengths())
    assert _close(gp.train_simple_average(got.entries), TR.simple_average(d, ent_ref))
    gp.close()
    eng.close()


@pytest.mark.parametrize("n,T", [(5, 7), (27, 65)])
def test_the_forced_global_store_gives_the_same_bits(monkeypatch, n, T):
    L = _lib()
    pids = _batch(n, T, 100 + n)
    results = []
    for store in ("lds", "global"):
        monkeypatch.setenv("MI_PHYLO_GP_TREES_STORE", store)
        tips, w = TU.random_alignment(n, 4, np.random.default_rng(0))
        eng = L.Engine(L.PhyloModelSpecification("JC69", "constant", "strict"), np.asarray(tips, np.int32), np.asarray(w, float),
                       device=0)
        gp = eng.gp_create_dag(pids[::2])
        index = gp.tree_index(pids)
        assert eng.last_call_path() == f"gp_trees n={n} T={T} store={store}"
        s = gp.sample_trees(T, seed=12, first_sample=3)
        assert eng.last_call_path() == f"gp_trees n={n} T={T} store={store}"
        e = gp.enumerate_trees(0, min(T, gp.topology_count()))
        results.append([index.entries, index.nodes, s.parent_ids, s.entries, s.log_q, s.branch_lengths, e.parent_ids, e.entries,
                        e.log_q])
        gp.close()
        eng.close()
    for a, b in zip(*results):
        assert a.tobytes() == b.tobytes()
    ent_ref, nodes_ref = TR.index_batch(R.build_dag(pids[::2]), pids)
    assert results[1][0].tobytes() == ent_ref.tobytes() and results[1][1].tobytes() == nodes_ref.tobytes()


def test_cpp_adapter(tmp_path):
    """tests/cpp/gp_trees_example.cpp: the five-taxon DAG through Engine::GpCreateDag, TreeIndex,
    TrainSimpleAverage, SampleTrees, EnumerateTrees and DerootTrees; its printed numbers are the Python calls'."""
    exe = tmp_path / "gp_trees_example"
    lib = os.path.join(REPO, "libsbn_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(REPO, "tests/cpp/gp_trees_example.cpp"), "-L" + lib, "-lmi_phylo",
                    "-lmi_phylo_host", "-Wl,-rpath," + lib, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe), os.path.join(REPO, "tests/golden/data")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = dict(line.split(" ", 1) for line in out.stdout.strip().splitlines())

    def hexes(name):
        return np.array([float.fromhex(x) for x in lines[name].split()])

    def ints(name):
        return np.array([int(x) for x in lines[name].split()], np.int32)
    pids, _, tips, w, _ = R.load_case("five_taxon_rooted.nwk", "five_taxon.fasta")
    eng, _ = _model_engine(tips, w, "JC69")
    gp = eng.gp_create_dag(pids)
    index = gp.tree_index(pids)
    assert ints("entries").tobytes() == index.entries.tobytes()
    assert hexes("trained_q").tobytes() == gp.train_simple_average(index.entries).tobytes()
    s = gp.sample_trees(8, seed=42, first_sample=3)
    assert ints("sampled_parent_ids").tobytes() == s.parent_ids.tobytes() and hexes("sampled_log_q").tobytes() == s.log_q.tobytes()
    e = gp.enumerate_trees()
    assert ints("enumerated_parent_ids").tobytes() == e.parent_ids.tobytes() and hexes("enumerated_log_q").tobytes() == e.log_q.tobytes()
    un = eng.deroot_trees(e.parent_ids, e.branch_lengths)
    assert ints("derooted_parent_ids").tobytes() == un.parent_ids.tobytes() and ints("root_edge").tobytes() == un.root_edge.tobytes()
    assert hexes("derooted_lengths").tobytes() == un.branch_lengths.tobytes()
    gp.close()
