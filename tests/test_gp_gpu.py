"""Generalized pruning on the device (Engine.gp_create) against tests/gp_ref.py:
brute force over the enumerated trees of small DAGs, invariants of the DS1 DAG, rescaling,
derivatives, the SBN estimate, the optimiser and the plumbing."""
import json
import os
import subprocess

import numpy as np
import pytest

import gp_ref as R

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10   # relative: the project's bound against its oracle

GTR_RATES = np.array([0.10, 0.27, 0.08, 0.12, 0.31, 0.12])
GTR_FREQS = np.array([0.34, 0.16, 0.21, 0.29])
MODELS = {"JC69": lambda: R.Model(), "GTR": lambda: R.Model(GTR_RATES, GTR_FREQS)}

FILES = {"hello1": ("hello_rooted.nwk", "hello.fasta"), "hello2": ("hello_rooted_two_trees.nwk", "hello.fasta"),
         "five": ("five_taxon_rooted.nwk", "five_taxon.fasta"), "ds1r5": ("ds1-reduced-5.nwk", "ds1-reduced-5.fasta"),
         "seven": ("simplest-hybrid-marginal-all-trees.nwk", "7-taxon-slice-of-ds1.fasta")}
CASES = list(FILES) + [f"random{i}" for i in range(len(R.RANDOM_CASES))]
_loaded = {}


def _load(case):
    """(parent_ids, tips, weights) of a case, read once"""
    if case not in _loaded:
        if case in FILES:
            pids, _, tips, w, _ = R.load_case(*FILES[case])
        else:
            pids, tips, w = R.random_case(int(case[len("random"):]))
        _loaded[case] = (pids, tips, w)
    return _loaded[case]


def _engine(tips, w, subst="JC69"):
    """an engine with one rate category and its one parameter row"""
    import libsbn_amd as L
    eng = L.Engine(L.PhyloModelSpecification(subst, "constant", "strict"), np.asarray(tips, np.int32), np.asarray(w, float),
                   device=0)
    row = np.ones(eng.param_count)
    for start, length in eng.block_specification().values():
        if length == 6:
            row[start:start + 6] = GTR_RATES
        elif length == 4:
            row[start:start + 4] = GTR_FREQS
    return eng, row


def _lengths(d, seed):
    b = np.random.default_rng(seed).uniform(0.02, 0.4, d.G)
    b[:d.R] = 0.0
    return b


def _close(x, ref, tol=TOL):
    x, ref = np.asarray(x, float), np.asarray(ref, float)
    return np.all(np.abs(x - ref) <= tol * np.abs(ref))


def _close_log(x, ref, tol=TOL):
    """per-PATTERN log values: an all-gap pattern has M = sum q = 1 up to the rounding of that sum, a
    log of a few 1e-16 either side of 0 in the library and in gp_ref alike: measured against at least 1"""
    x, ref = np.asarray(x, float), np.asarray(ref, float)
    return np.all(np.abs(x - ref) <= tol * np.maximum(np.abs(ref), 1.0))


# ---- 1. the DAG ----
@pytest.mark.parametrize("case", ["five", "ds1r5", "random2"])
def test_structure_follows_the_numbering_rule(case):
    pids, tips, w = _load(case)
    eng, row = _engine(tips, w)
    gp = eng.gp_create(pids, params=row)
    d, s = R.build_dag(pids), gp.structure()
    assert (s.taxon_count, s.node_count, s.rootsplit_count, s.entry_count, s.pattern_count) == \
        (d.n, d.node_count, d.R, d.G, len(w))
    assert np.array_equal(s.entries, d.entries) and np.array_equal(s.block_range, d.block_range)
    assert np.array_equal(s.levels, d.levels) and s.topology_count == d.topology_count
    for v, (a, b) in enumerate(d.clades):
        assert s.clades[v, 0, 0] == sum(1 << x for x in a) and s.clades[v, 1, 0] == sum(1 << x for x in b)
    assert gp.strings() == R.strings(d)
    q = gp.get_sbn_parameters()
    assert np.array_equal(q, R.uniform_prior(d))
    b = gp.get_branch_lengths()
    assert np.all(b[:d.R] == 0.0) and np.all(b[d.R:] == 0.1)
    assert np.allclose(gp.node_probabilities(q), R.node_probabilities(d, q), rtol=0, atol=1e-15)
    assert np.allclose(gp.inverted_probabilities(q), R.inverted_probabilities(d, q), rtol=0, atol=1e-15)
    gp.close()


def test_hot_start_is_the_mean_over_the_trees_that_hold_the_entry():
    pids, bl, tips, w, _ = R.load_case("hello_rooted_two_trees.nwk", "hello.fasta")
    eng, row = _engine(tips, w)
    gp = eng.gp_create(pids, branch_lengths=bl, params=row)
    assert np.allclose(gp.get_branch_lengths(), R.hot_start(R.build_dag(pids), bl), rtol=1e-15, atol=0)
    gp.close()


# ---- 2. brute force ----
@pytest.mark.parametrize("q_kind", ["uniform", "random"])
@pytest.mark.parametrize("subst", ["JC69", "GTR"])
@pytest.mark.parametrize("case", CASES)
def test_every_entry_and_the_marginal_against_brute_force(case, subst, q_kind):
    pids, tips, w = _load(case)
    d = R.build_dag(pids)
    eng, row = _engine(tips, w, subst)
    gp = eng.gp_create(pids, params=row)
    q = R.uniform_prior(d) if q_kind == "uniform" else R.random_q(d, np.random.default_rng(5))
    b = _lengths(d, 3)
    gp.set_sbn_parameters(q)
    gp.set_branch_lengths(b)
    gp.populate()
    assert eng.last_call_path().startswith(f"gp_populate n={d.n} nodes={d.node_count} G={d.G} ")
    got = gp.likelihoods(per_pattern=True)
    ref = R.values(d, q, b, tips, w, MODELS[subst]())
    full = got.per_gpcsp_log_likelihood + np.sum(w) * np.log(q)
    full[:d.R] = got.per_gpcsp_log_likelihood[:d.R]   # (conditional on the rootsplit)
    print(case, subst, q_kind, "max relative error", np.max(np.abs(full - ref["full"]) / np.abs(ref["full"])),
          abs(got.log_marginal - ref["log_marginal"]) / abs(ref["log_marginal"]))
    assert _close(full, ref["full"])
    assert _close(got.log_marginal, ref["log_marginal"])
    assert _close_log(got.pattern_log_marginal, ref["pattern_log_marginal"])
    assert np.array_equal(gp.components_of_full_log_marginal()[d.R:], full[d.R:])
    gp.close()


def _random_tips(n, P, seed):
    rng = np.random.default_rng(seed)
    tips = rng.integers(0, 4, (n, P)).astype(np.int32)
    tips[rng.random((n, P)) < 0.1] = 4
    w = rng.integers(1, 5, P).astype(float)
    w[0] = 1e6
    if P > 2:
        w[1] = 0.0
    return tips, w


@pytest.mark.parametrize("patterns", [1, 63, 64, 65, 129])   # around the kernels' tile width 64
def test_pattern_counts_around_the_tile_width(patterns):
    pids = R.random_case(2)[0]
    d = R.build_dag(pids)
    sizes, through0, through1 = R.shape_summary(d)
    assert {1, 2} <= sizes and max(sizes) >= 3 and through0 >= 2 and through1 >= 2
    assert np.max(np.bincount(d.levels[d.n:])) > 1   # a level of several nodes: several workgroups per tile
    tips, w = _random_tips(d.n, patterns, patterns)
    eng, row = _engine(tips, w, "GTR")
    gp = eng.gp_create(pids, params=row)
    assert gp.tile_width == 64
    q, b = R.random_q(d, np.random.default_rng(6)), _lengths(d, 4)
    gp.set_sbn_parameters(q)
    gp.set_branch_lengths(b)
    got = gp.likelihoods()
    ref = R.values(d, q, b, tips, w, MODELS["GTR"]())
    full = got.per_gpcsp_log_likelihood + np.sum(w) * np.log(q)
    full[:d.R] = got.per_gpcsp_log_likelihood[:d.R]
    assert _close(full, ref["full"]) and _close(got.log_marginal, ref["log_marginal"])
    gp.close()


# ---- 3. invariants at a size brute force cannot reach ----
def _logsumexp(x):
    top = np.max(x, axis=0)
    return top + np.log(np.sum(np.exp(x - top), axis=0))


def test_ds1_dag_invariants():
    st = json.load(open(os.path.join(REPO, "tests", "golden", "ds1_top100.struct.json")))
    tips, w = np.array(st["patterns"], np.int32), np.array(st["weights"], float)
    pids = np.stack([R.root_above_leaf0(t["parent_ids"]) for t in st["trees"]])
    eng, row = _engine(tips, w)
    gp = eng.gp_create(pids, params=row)
    s, q = gp.structure(), gp.get_sbn_parameters()
    assert s.topology_count >= 100
    got = gp.likelihoods(matrix=True, per_pattern=True)
    rows = np.log(q)[:, None] + got.matrix
    log_m = got.pattern_log_marginal
    assert _close(np.dot(w, log_m), got.log_marginal)
    for x in range(s.taxon_count):   # every tree enters each leaf exactly once
        into = np.flatnonzero(s.entries[:, 2] == x)
        assert _close_log(_logsumexp(rows[into]), log_m), x
    for t in range(s.taxon_count, s.node_count):   # the trees through t, counted by either clade
        (a0, a1), (b0, b1) = s.block_range[t]
        assert _close_log(_logsumexp(rows[a0:a1]), _logsumexp(rows[b0:b1])), t
    gp.close()


def test_single_tree_dag_is_plain_pruning():
    pids, _, tips, w, _ = R.load_case("fluA.tree", "fluA.fa")
    d = R.build_dag(pids)
    assert d.topology_count == 1.0
    eng, row = _engine(tips, w)
    gp = eng.gp_create(pids, params=row)
    b = np.full(d.G, 0.01)
    gp.set_branch_lengths(b)
    got = gp.likelihoods()
    tree = R.enumerate_trees(d)[0]
    plain = float(np.dot(w, R.tree_likelihood(d, tree, b, R.tip_vectors(tips), R.Model(), log_domain=True)))
    assert _close(got.log_marginal, plain)
    assert _close(got.per_gpcsp_log_likelihood, np.full(d.G, plain))
    gp.close()


# ---- 4. rescaling ----
def test_results_do_not_depend_on_the_threshold():
    pids, tips, w = _load("five")
    eng, row = _engine(tips, w)
    out = []
    for threshold in (None, 2.0 ** -8):
        gp = eng.gp_create(pids, params=row, rescaling_threshold=threshold)
        got, der = gp.likelihoods(), gp.branch_derivatives()
        out.append(np.concatenate([got.per_gpcsp_log_likelihood, [got.log_marginal], der.gradient, der.hessian]))
        gp.close()
    assert _close(out[1], out[0], 1e-12)


def test_deep_caterpillar_does_not_underflow():
    import tree_utils as TU
    n, P = 600, 17
    base = TU.ladder_topology(n, rooted=True)
    other = base.copy()
    other[300], other[301] = base[301], base[300]   # one NNI move
    pids = np.stack([base, other])
    d = R.build_dag(pids)
    assert d.topology_count == 2.0
    tips, w = _random_tips(n, P, 7)
    eng, row = _engine(tips, w)
    gp = eng.gp_create(pids, params=row)
    b = np.ones(d.G)
    b[:d.R] = 0.0
    gp.set_branch_lengths(b)
    got = gp.likelihoods()
    assert np.isfinite(got.log_marginal) and np.all(np.isfinite(got.per_gpcsp_log_likelihood))
    ref = R.log_marginal_deep(d, R.uniform_prior(d), b, tips, w, R.Model())
    assert ref < -600 * np.log(4.0)   # (4^-600 is about 1e-361: a plain double holds no such likelihood)
    assert _close(got.log_marginal, ref)
    gp.close()


# ---- 5. derivatives ----
@pytest.mark.parametrize("subst", ["JC69", "GTR"])
def test_gradient_against_central_differences(subst):
    """g against central differences of gp_ref's long-double log_marginal, step 1e-6.  Bound: 1e-6
    relative per entry, entries below a thousandth of the largest measured against that floor (the
    difference's own error is h^2 f'''/6 + 2^-64 |log M| / h, about 1e-11 absolute here)."""
    pids, tips, w = _load("five")
    d = R.build_dag(pids)
    eng, row = _engine(tips, w, subst)
    gp = eng.gp_create(pids, params=row)
    q, b = R.random_q(d, np.random.default_rng(8)), _lengths(d, 9)
    gp.set_sbn_parameters(q)
    gp.set_branch_lengths(b)
    g = gp.branch_derivatives().gradient
    model, h = MODELS[subst](), np.longdouble(1e-6)
    fd = np.zeros(d.G)
    for e in range(d.R, d.G):
        hi, lo = b.astype(np.longdouble), b.astype(np.longdouble)
        hi[e] += h
        lo[e] -= h
        fd[e] = float((R.log_marginal(d, q, hi, tips, w, model, np.longdouble) -
                       R.log_marginal(d, q, lo, tips, w, model, np.longdouble)) / (2 * h))
    print(subst, "max |g - fd| / |fd|", np.max(np.abs(g - fd)[d.R:] / np.abs(fd[d.R:])))
    assert np.all(np.abs(g - fd) <= 1e-6 * np.maximum(np.abs(fd), 1e-3 * np.max(np.abs(fd))))
    assert np.all(g[:d.R] == 0.0)
    gp.close()


@pytest.mark.parametrize("subst", ["JC69", "GTR"])
@pytest.mark.parametrize("case", ["five", "ds1r5", "random1"])
def test_derivatives_against_the_analytic_reference(case, subst):
    """1e-9 relative per entry; H is a difference of two sums and is measured against the larger of
    |H| and S, a gradient entry against at least a thousandth of the largest."""
    pids, tips, w = _load(case)
    d = R.build_dag(pids)
    eng, row = _engine(tips, w, subst)
    gp = eng.gp_create(pids, params=row)
    q, b = R.random_q(d, np.random.default_rng(10)), _lengths(d, 11)
    gp.set_sbn_parameters(q)
    gp.set_branch_lengths(b)
    got = gp.branch_derivatives()
    ref = R.values(d, q, b, tips, w, MODELS[subst]())
    e = slice(d.R, d.G)
    floor = 1e-3 * np.max(np.abs(ref["g"]))
    assert np.all(np.abs(got.gradient - ref["g"])[e] <= 1e-9 * np.maximum(np.abs(ref["g"][e]), floor))
    assert np.all(np.abs(got.derivative - ref["derivative"])[e] <= 1e-9 * np.maximum(np.abs(ref["derivative"][e]), floor))
    assert np.all(np.abs(got.gsq - ref["S"])[e] <= 1e-9 * ref["S"][e])
    assert np.all(np.abs(got.hessian - ref["H"])[e] <= 1e-9 * np.maximum(np.abs(ref["H"][e]), ref["S"][e]))
    full = got.log_likelihood + np.sum(w) * np.log(q)
    assert _close(full[e], ref["full"][e])
    gp.close()


# ---- 6. the SBN estimate ----
def test_sbn_estimate_on_five_taxa():
    pids, tips, w = _load("five")
    d = R.build_dag(pids)
    eng, row = _engine(tips, w)
    gp = eng.gp_create(pids, params=row)
    q0, b = R.uniform_prior(d), gp.get_branch_lengths()
    ref = R.values(d, q0, b, tips, w, R.Model())
    new = gp.estimate_sbn_parameters()
    assert np.array_equal(new, gp.get_sbn_parameters())
    # the rootsplits as the reference's test computes them: softmax(log-likelihood given the rootsplit + log prior)
    x = ref["full"][:d.R] + np.log(q0[:d.R])
    want = np.exp(x - _logsumexp(x))
    assert np.allclose(new[:d.R], want, rtol=1e-9, atol=0)
    assert abs(np.sum(new[:d.R]) - 1) < 1e-12
    for v in range(d.n, d.node_count):
        for lo, hi in d.block_range[v]:
            assert abs(np.sum(new[lo:hi]) - 1) < 1e-12
            if hi - lo == 1:
                assert new[lo] == 1.0
            else:
                # within a block: softmax(per_gpcsp + log q)
                y = ref["full"][lo:hi] - (np.sum(w) - 1) * np.log(q0[lo:hi])
                assert np.allclose(new[lo:hi], np.exp(y - _logsumexp(y)), rtol=1e-8, atol=0)
    gp.close()


# ---- 7. the optimiser ----
@pytest.mark.parametrize("case", ["hello2", "five", "ds1r5"])
def test_optimiser(case):
    """tolerance 1e-4 is what the reference's own tests give its EstimateBranchLengths; the iteration
    limit is the library's largest: on ds1-reduced-5, where 49 of 60 branches end on the lower bound,
    the restated rule needs 624 evaluations (hello: 42, five taxa: 11)."""
    pids, tips, w = _load(case)
    d = R.build_dag(pids)
    eng, row = _engine(tips, w)
    gp = eng.gp_create(pids, params=row)
    q, b0, tol = R.uniform_prior(d), gp.get_branch_lengths(), 1e-4
    res = gp.optimize_branch_lengths(tolerance=tol, max_iterations=1000)
    print(case, "evaluations", res.evaluations, "status", res.status, "marginal", res.trace[-1])
    assert res.status == 0 and res.evaluations == len(res.trace)
    assert "gp_populate" in eng.last_call_path() and f"opt evals={res.evaluations}" in eng.last_call_path()
    assert np.all(np.diff(res.trace) >= -2.0 ** -48 * np.abs(res.trace[:-1]))
    assert np.all(res.branch_lengths[:d.R] == 0.0)
    tmin, tmax = np.exp(-13.9), np.exp(1.1)
    assert np.all((res.branch_lengths[d.R:] >= tmin) & (res.branch_lengths[d.R:] <= tmax))
    model = R.Model()
    at = R.values(d, q, res.branch_lengths, tips, w, model)
    print(case, "criterion by the reference", R.criterion(res.branch_lengths, at["g"], d.R, tmin, tmax))
    assert R.criterion(res.branch_lengths, at["g"], d.R, tmin, tmax) <= tol
    assert _close(res.trace[-1], at["log_marginal"])

    def evaluate(x):
        v = R.values(d, q, x, tips, w, model)
        return v["log_marginal"], v["g"], v["H"], v["S"]
    _, ref_trace, _, ref_status = R.optimize(evaluate, b0, d.R, tol, 1000, tmin, tmax)
    assert ref_status == 0
    assert at["log_marginal"] >= ref_trace[-1] - d.G * tol
    again = gp.optimize_branch_lengths(tolerance=tol, max_iterations=1000)
    assert again.status == 0 and again.evaluations == 1
    assert again.branch_lengths.tobytes() == res.branch_lengths.tobytes()
    gp.close()


# ---- 8. plumbing ----
def test_graph_replay_gives_the_same_bits():
    import torch
    pids, tips, w = _load("ds1r5")
    d = R.build_dag(pids)
    eng, row = _engine(tips, w, "GTR")
    gp = eng.gp_create(pids, params=row)
    gp.set_branch_lengths(_lengths(d, 12))
    host = gp.likelihoods()
    per = torch.zeros(d.G, dtype=torch.float64, device="cuda:0")
    marg = torch.zeros(1, dtype=torch.float64, device="cuda:0")
    gs = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=gs):
        s = torch.cuda.current_stream().cuda_stream
        gp.populate_device(s)
        gp.likelihoods_device(s, per.data_ptr(), marg.data_ptr())
    torch.cuda.synchronize()
    for _ in range(2):
        per.zero_()
        marg.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert per.cpu().numpy().tobytes() == host.per_gpcsp_log_likelihood.tobytes()
        assert float(marg.cpu()[0]) == host.log_marginal
    gp.close()


def test_close_releases_what_the_object_holds():
    import libsbn_amd as L
    pids, tips, w = _load("five")
    eng, row = _engine(tips, w)
    gp = eng.gp_create(pids, params=row)
    gp.close()   # (whatever the engine itself reserves at a first creation is the engine's)
    held = L._capi.load().mi_device_bytes_held()
    gp = eng.gp_create(pids, params=row)
    assert L._capi.load().mi_device_bytes_held() > held
    gp.likelihoods(matrix=True)
    gp.optimize_branch_lengths(max_iterations=3)
    gp.close()
    assert L._capi.load().mi_device_bytes_held() == held


def test_what_is_refused():
    import libsbn_amd as L
    import aa_utils as A
    pids, tips, w = _load("five")
    eng, row = _engine(tips, w)
    with pytest.raises(RuntimeError, match="trees of 4 taxa, the engine has 5"):
        eng.gp_create(pids[:, :6], params=row)
    bad = pids.copy()
    bad[0, 0] = bad[0, 2]   # three children under one node
    with pytest.raises(RuntimeError, match="not bifurcating"):
        eng.gp_create(bad, params=row)
    gp = eng.gp_create(pids, params=row)
    with pytest.raises(RuntimeError, match=f"sbn_parameters has 3 entries, the DAG {gp.entry_count}"):
        gp.set_sbn_parameters(np.ones(3))
    with pytest.raises(RuntimeError, match="branch_lengths has"):
        gp.set_branch_lengths(np.ones(gp.entry_count + 1))
    with pytest.raises(RuntimeError, match="rescaling_threshold"):
        eng.gp_create(pids, params=row, rescaling_threshold=2.0)
    gp.close()
    many = L.Engine(L.PhyloModelSpecification("JC69", "weibull+4", "strict"), tips, w, device=0)
    with pytest.raises(RuntimeError, match="one rate category"):
        many.gp_create(pids, params=np.ones(many.param_count))
    sharded = L.Engine(L.PhyloModelSpecification("JC69", "constant", "strict"), tips, w, shard_devices=[0, 0])
    with pytest.raises(RuntimeError, match="sharded handle"):
        sharded.gp_create(pids, params=row)
    sharded.close()
    aa_tips, aa_w = A.random_aa_alignment(5, 8, np.random.default_rng(0))
    aa = L.Engine(L.PhyloModelSpecification("WAG", "constant", "strict"), aa_tips, aa_w, device=0)
    with pytest.raises(RuntimeError, match="4-state only"):
        aa.gp_create(pids, params=np.ones(aa.param_count))


def test_cpp_adapter(tmp_path):
    """tests/cpp/gp_example.cpp: the five-taxon case through Engine::GpCreate; its printed numbers
    are the Python call's, bit for bit."""
    exe = tmp_path / "gp_example"
    lib = os.path.join(REPO, "libsbn_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(REPO, "tests/cpp/gp_example.cpp"), "-L" + lib, "-lmi_phylo",
                    "-lmi_phylo_host", "-Wl,-rpath," + lib, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe), os.path.join(REPO, "tests/golden/data")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = dict(line.split(" ", 1) for line in out.stdout.strip().splitlines())

    def hexes(name):
        return np.array([float.fromhex(x) for x in lines[name].split()])
    pids, tips, w = _load("five")
    eng, row = _engine(tips, w)
    gp = eng.gp_create(pids, params=row)
    got, der = gp.likelihoods(), gp.branch_derivatives()
    assert hexes("per_gpcsp").tobytes() == got.per_gpcsp_log_likelihood.tobytes()
    assert hexes("log_marginal")[0] == got.log_marginal
    assert hexes("gradient").tobytes() == der.gradient.tobytes()
    assert hexes("hessian").tobytes() == der.hessian.tobytes()
    assert hexes("estimated_q").tobytes() == gp.estimate_sbn_parameters().tobytes()
    res = gp.optimize_branch_lengths()
    assert hexes("optimised_lengths").tobytes() == res.branch_lengths.tobytes()
    assert int(lines["status"]) == res.status
    gp.close()
