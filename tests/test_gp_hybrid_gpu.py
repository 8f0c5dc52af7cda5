"""Quartet hybrid marginals on the device (GeneralizedPruning.hybrid_marginals)
against tests/gp_hybrid_ref.py, the restatement by tree enumeration: every summand and every
entry, the request tables, the tile edges, rescaling, a likelihood of zero, the hybrid SBN
estimate, graph replay and the plumbing."""
import os
import subprocess

import numpy as np
import pytest

import gp_hybrid_ref as H
import gp_ref as R

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10   # relative to max(1, |ref|): the bound the gp outputs are held to

GTR_RATES = np.array([0.10, 0.27, 0.08, 0.12, 0.31, 0.12])
GTR_FREQS = np.array([0.34, 0.16, 0.21, 0.29])
MODELS = {"JC69": lambda: H.ExactModel(), "GTR": lambda: H.ExactModel(GTR_RATES, GTR_FREQS)}
FILES = {"simplest": "simplest-hybrid-marginal.nwk", "second": "second-simplest-hybrid-marginal.nwk"}
CASES = list(FILES) + [f"random{i}" for i in range(len(R.RANDOM_CASES))] + ["eleven"]
_loaded, _restated = {}, {}


def _load(case):
    """(parent_ids, tips with gaps, weights with a 0 and a 1e6) of a case, made once"""
    if case not in _loaded:
        import tree_utils as TU
        if case in FILES:
            pids = R.load_case(FILES[case], "7-taxon-slice-of-ds1.fasta")[0]
        elif case == "eleven":
            pids = H.eleven_batch()
        else:
            pids = R.random_case(int(case[len("random"):]))[0]
        tips, w = TU.random_alignment(pids.shape[1] // 2 + 1, 9, np.random.default_rng(len(case)), gap_fraction=0.1)
        w[0], w[-1] = 0.0, 1e6
        _loaded[case] = (pids, np.asarray(tips, np.int32), np.asarray(w, float))
    return _loaded[case]


def _engine(tips, w, subst="JC69"):
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


def _inputs(case, q_kind):
    pids, tips, w = _load(case)
    d = R.build_dag(pids)
    q = R.uniform_prior(d) if q_kind == "uniform" else R.random_q(d, np.random.default_rng(5))
    return pids, tips, w, d, q, _lengths(d, 3)


def _restate(case, subst, q_kind):
    """the restatement of a case, computed once and shared"""
    key = (case, subst, q_kind)
    if key not in _restated:
        _, tips, w, d, q, b = _inputs(case, q_kind)
        _restated[key] = H.hybrid(d, q, b, tips, w, MODELS[subst]())
    return _restated[key]


def _error(x, ref):
    """max |x - ref| / max(1, |ref|) over the finite entries; -inf must sit exactly where ref has it"""
    x, ref = np.asarray(x, float), np.asarray(ref, float)
    assert not np.any(np.isnan(x))
    assert np.array_equal(np.isneginf(x), np.isneginf(ref))
    on = np.isfinite(ref)
    return float(np.max(np.abs(x[on] - ref[on]) / np.maximum(1.0, np.abs(ref[on])), initial=0.0))


# ---- 1. against the restatement ----
@pytest.mark.parametrize("q_kind", ["uniform", "random"])
@pytest.mark.parametrize("subst", ["JC69", "GTR"])
@pytest.mark.parametrize("case", CASES)
def test_every_summand_and_entry_against_enumeration(case, subst, q_kind):
    pids, tips, w, d, q, b = _inputs(case, q_kind)
    ref = _restate(case, subst, q_kind)
    eng, row = _engine(tips, w, subst)
    gp = eng.gp_create(pids, params=row)
    gp.set_sbn_parameters(q)
    gp.set_branch_lengths(b)
    got = gp.hybrid_marginals(summands=True)
    formed = int(np.sum(ref.requests.formed))
    assert eng.last_call_path().startswith(f"gp_hybrid formed={formed} summands={len(ref.summands)} tiles=1 z=")
    errors = _error(got.summands, ref.summands), _error(got.hybrid, ref.hybrid)
    print(case, subst, q_kind, "max relative error: summands %.3g hybrid %.3g" % errors)
    assert max(errors) <= TOL
    assert np.all(got.hybrid[~ref.requests.formed] == -np.inf) and np.all(np.isfinite(got.hybrid[ref.requests.formed]))
    assert np.array_equal(gp.hybrid_marginals(), got.hybrid)
    gp.close()


@pytest.mark.parametrize("case", CASES)
def test_requests_equal_the_restatement(case):
    pids, tips, w = _load(case)
    want = H.requests(R.build_dag(pids))
    eng, row = _engine(tips, w)
    gp = eng.gp_create(pids, params=row)
    got = gp.hybrid_requests()
    assert np.array_equal(got.formed, want.formed)
    assert np.array_equal(got.first_summand[want.formed], want.first_summand[want.formed])
    assert np.array_equal(got.summand_count, want.summand_count)
    assert np.array_equal(got.summands, want.summands)   # (the order is part of the contract)
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


@pytest.mark.parametrize("patterns", [1, 63, 64, 65, 129])   # the tile edges: padding lanes are never summed
def test_pattern_counts_around_the_tile_width(patterns):
    pids = R.random_case(2)[0]
    d = R.build_dag(pids)
    tips, w = _random_tips(d.n, patterns, patterns)
    q, b = R.random_q(d, np.random.default_rng(6)), _lengths(d, 4)
    ref = H.hybrid(d, q, b, tips, w, MODELS["GTR"]())
    assert len(ref.summands) > int(np.sum(ref.requests.formed)) > 0
    eng, row = _engine(tips, w, "GTR")
    gp = eng.gp_create(pids, params=row)
    gp.set_sbn_parameters(q)
    gp.set_branch_lengths(b)
    got = gp.hybrid_marginals(summands=True)
    errors = _error(got.summands, ref.summands), _error(got.hybrid, ref.hybrid)
    print(patterns, "patterns: max relative error %.3g %.3g" % errors)
    assert max(errors) <= TOL
    gp.close()


@pytest.mark.parametrize("patterns", [9, 129])
def test_results_do_not_depend_on_the_z_split(monkeypatch, patterns):
    """the (rootward, sister) pairs of a request dealt over 1, 3, 6 (the widest request's pairs) or
    more workgroups than any request has pairs: the same bits"""
    pids = H.eleven_batch()
    tips, w = _random_tips(11, patterns, 21)
    out = []
    for z in ("", "1", "3", "6", "50"):
        monkeypatch.setenv("MI_PHYLO_GP_HYBRID_Z", z) if z else monkeypatch.delenv("MI_PHYLO_GP_HYBRID_Z", raising=False)
        eng, row = _engine(tips, w, "GTR")
        gp = eng.gp_create(pids, params=row)
        got = gp.hybrid_marginals(summands=True)
        assert eng.last_call_path().endswith(" z=" + (z or "6"))
        out.append(got.summands.tobytes() + got.hybrid.tobytes())
        gp.close()
    assert all(x == out[0] for x in out[1:])


# ---- 2. rescaling ----
def test_results_do_not_depend_on_the_threshold():
    pids, tips, w = _load("eleven")
    eng, row = _engine(tips, w)
    out = []
    for threshold in (None, 2.0 ** -8):
        gp = eng.gp_create(pids, params=row, rescaling_threshold=threshold)
        got = gp.hybrid_marginals(summands=True)
        out.append(np.concatenate([got.summands, got.hybrid[np.isfinite(got.hybrid)]]))
        gp.close()
    assert len(out[0]) == 93 + 21 and np.all(np.isfinite(out[0]))
    print("threshold 2^-8 against the default:", np.max(np.abs(out[1] - out[0]) / np.abs(out[0])))
    assert np.all(np.abs(out[1] - out[0]) <= 1e-12 * np.abs(out[0]))


def test_deep_caterpillar_does_not_underflow():
    """every vector of this DAG is rescaled many times over: the reference refuses it by assertion"""
    import tree_utils as TU
    n, P = 600, 9
    base = TU.ladder_topology(n, rooted=True)
    other = base.copy()
    other[300], other[301] = base[301], base[300]   # one NNI move
    pids = np.stack([base, other])
    d = R.build_dag(pids)
    assert d.topology_count == 2.0
    tips, w = _random_tips(n, P, 7)
    b = np.ones(d.G)
    b[:d.R] = 0.0
    q = R.uniform_prior(d)
    ref = H.hybrid(d, q, b, tips, w, R.Model(), log_domain=True)
    assert np.min(ref.summands) < -600 * np.log(4.0) and np.any(ref.trees_per_summand > 1)
    eng, row = _engine(tips, w)
    gp = eng.gp_create(pids, params=row)
    gp.set_branch_lengths(b)
    got = gp.hybrid_marginals(summands=True)
    errors = _error(got.summands, ref.summands), _error(got.hybrid, ref.hybrid)
    print("deep caterpillar: max relative error %.3g %.3g" % errors)
    assert max(errors) <= TOL
    gp.close()


# ---- 3. a likelihood of zero ----
def test_zero_likelihood_is_minus_infinity_and_drops_out():
    """The cherry (1,2) with both its branches 0 and taxa 1, 2 different at a pattern of positive
    weight: every summand through the cherry is -inf.  The central entry into the cherry has only
    such summands (-inf); an entry with the cherry's parent in one of its lists has some, and its
    logsumexp is over the rest."""
    pids = H.eleven_batch()
    d = R.build_dag(pids)
    tips = np.random.default_rng(4).integers(0, 4, (d.n, 5)).astype(np.int32)
    tips[1, 1], tips[2, 1] = 1, 2
    w = np.array([1.0, 2.0, 0.0, 3.0, 1.0])
    cherry = next(v for v in range(d.n, d.node_count) if d.clades[v] == (frozenset([1]), frozenset([2])))
    b = _lengths(d, 8)
    for c in range(2):
        b[d.block_range[cherry, c, 0]] = 0.0
    q = R.uniform_prior(d)
    ref = H.hybrid(d, q, b, tips, w, H.ExactModel())
    central = next(e for e in range(d.R, d.G) if int(d.entries[e][2]) == cherry)
    req = ref.requests
    mixed = [e for e in np.flatnonzero(req.formed)
             if 0 < np.sum(np.isneginf(ref.summands[req.first_summand[e]:req.first_summand[e] + req.summand_count[e]]))
             < req.summand_count[e]]
    assert req.formed[central] and ref.hybrid[central] == -np.inf and mixed
    eng, row = _engine(tips, w)
    gp = eng.gp_create(pids, params=row)
    gp.set_branch_lengths(b)
    got = gp.hybrid_marginals(summands=True)
    assert not np.any(np.isnan(got.summands)) and not np.any(np.isnan(got.hybrid))
    assert got.hybrid[central] == -np.inf
    assert max(_error(got.summands, ref.summands), _error(got.hybrid, ref.hybrid)) <= TOL
    for e in mixed:
        s = got.summands[req.first_summand[e]:req.first_summand[e] + req.summand_count[e]]
        assert np.isfinite(got.hybrid[e]) and abs(got.hybrid[e] - H.logsumexp_in_order(s[np.isfinite(s)])) <= 1e-12 * abs(got.hybrid[e])
    gp.close()


# ---- 4. the SBN estimate ----
@pytest.mark.parametrize("case", ["eleven", "random1"])
def test_hybrid_sbn_estimate_follows_the_rule(case):
    """eleven: every block of several entries is fully formed, entries 10-12 among them; random1 has
    blocks that take the hybrid values next to one of two unformed entries, which takes the
    per-entry ones"""
    pids, tips, _ = _load(case)
    w = np.arange(1.0, tips.shape[1] + 1)   # (moderate weights: a softmax that saturates would show nothing)
    d = R.build_dag(pids)
    q, b = R.random_q(d, np.random.default_rng(9)), _lengths(d, 10)
    eng, row = _engine(tips, w)

    def fresh():
        gp = eng.gp_create(pids, params=row)
        gp.set_sbn_parameters(q)
        gp.set_branch_lengths(b)
        return gp
    gp = fresh()
    hybrid, per = gp.hybrid_marginals(), gp.likelihoods().per_gpcsp_log_likelihood
    want, took = H.sbn_estimate_rule(d, q, per, hybrid)
    plain, none = H.sbn_estimate_rule(d, q, per, np.full(d.G, -np.inf))
    mixed = [(int(lo), int(hi)) for v in range(d.n, d.node_count) for lo, hi in d.block_range[v]
             if hi - lo > 1 and not np.all(np.isfinite(hybrid[lo:hi]))]
    assert took and not none and not set(mixed) & set(took)
    if case == "eleven":
        assert (10, 13) in took
    else:
        assert mixed   # a block with an unformed entry takes the per-entry values
    assert any(not np.allclose(want[lo:hi], plain[lo:hi], rtol=1e-3, atol=0) for lo, hi in took)
    for lo, hi in mixed:
        assert np.array_equal(want[lo:hi], plain[lo:hi])
    new = gp.estimate_sbn_parameters(hybrid=True)
    assert np.array_equal(new, gp.get_sbn_parameters())
    assert np.allclose(new, want, rtol=1e-12, atol=0)
    gp.close()
    # hybrid=False is the estimate as it was: the same bits with or without the hybrid machinery in use
    a, c = fresh(), fresh()
    c.reserve_hybrid()
    c.hybrid_marginals()
    first, second = a.estimate_sbn_parameters(), c.estimate_sbn_parameters(hybrid=False)
    assert first.tobytes() == second.tobytes()
    assert np.allclose(first, plain, rtol=1e-12, atol=0)
    a.close()
    c.close()


def test_hybrid_marginals_after_the_optimiser_are_those_of_the_accepted_lengths():
    """optimize_branch_lengths populates at trial points: the host form must not read those vectors"""
    pids, tips, w = _load("second")
    eng, row = _engine(tips, w)
    gp = eng.gp_create(pids, params=row)
    gp.hybrid_marginals()
    res = gp.optimize_branch_lengths(max_iterations=5)
    after = gp.hybrid_marginals()
    other = eng.gp_create(pids, params=row)
    other.set_branch_lengths(res.branch_lengths)
    assert after.tobytes() == other.hybrid_marginals().tobytes()
    gp.close()
    other.close()


# ---- 5. plumbing ----
def test_graph_replay_and_bytes_held():
    import torch
    import libsbn_amd as L
    pids, tips, w, d, q, b = _inputs("eleven", "random")
    eng, row = _engine(tips, w, "GTR")
    gp = eng.gp_create(pids, params=row)
    gp.close()   # (whatever the engine itself reserves at a first creation is the engine's)
    held = L._capi.load().mi_device_bytes_held()
    gp = eng.gp_create(pids, params=row)
    gp.set_sbn_parameters(q)
    gp.set_branch_lengths(b)
    before = L._capi.load().mi_device_bytes_held()
    gp.reserve_hybrid()
    assert L._capi.load().mi_device_bytes_held() > before
    host = gp.hybrid_marginals(summands=True)
    S = len(host.summands)
    hyb = torch.zeros(d.G, dtype=torch.float64, device="cuda:0")
    each = torch.zeros(S, dtype=torch.float64, device="cuda:0")
    gs = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=gs):
        s = torch.cuda.current_stream().cuda_stream
        gp.populate_device(s)
        gp.hybrid_marginals_device(s, hyb.data_ptr(), each.data_ptr())
    torch.cuda.synchronize()
    for _ in range(2):
        hyb.zero_()
        each.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert hyb.cpu().numpy().tobytes() == host.hybrid.tobytes()
        assert each.cpu().numpy().tobytes() == host.summands.tobytes()
    del graph
    gp.close()
    assert L._capi.load().mi_device_bytes_held() == held


def test_what_is_refused(monkeypatch):
    import torch
    pids, tips, w = _load("eleven")
    eng, row = _engine(tips, w)
    gp = eng.gp_create(pids, params=row)
    out = torch.zeros(gp.entry_count, dtype=torch.float64, device="cuda:0")
    with pytest.raises(RuntimeError, match="before mi_gp_reserve_hybrid"):
        gp.hybrid_marginals_device(None, out.data_ptr())
    gp.close()
    monkeypatch.setenv("MI_PHYLO_PLV_BYTES", "1000")
    small, row = _engine(tips, w)
    gp = small.gp_create(pids, params=row)
    with pytest.raises(RuntimeError, match=r"need \d+ bytes of evolved vectors and \d+ bytes of partial sums.*budget of 1000 bytes"):
        gp.reserve_hybrid()
    with pytest.raises(RuntimeError, match="MI_PHYLO_PLV_BYTES"):
        gp.hybrid_marginals()
    gp.close()


def test_cpp_adapter(tmp_path):
    """tests/cpp/gp_hybrid_example.cpp: the second-simplest hybrid DAG through the C++ adapter; its
    printed numbers are the Python call's, bit for bit."""
    exe = tmp_path / "gp_hybrid_example"
    lib = os.path.join(REPO, "libsbn_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(REPO, "tests/cpp/gp_hybrid_example.cpp"), "-L" + lib,
                    "-lmi_phylo", "-lmi_phylo_host", "-Wl,-rpath," + lib, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe), os.path.join(REPO, "tests/golden/data")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = dict(line.split(" ", 1) for line in out.stdout.strip().splitlines())

    def hexes(name):
        return np.array([float.fromhex(x) for x in lines[name].split()])
    pids, _, tips, w, _ = R.load_case("second-simplest-hybrid-marginal.nwk", "7-taxon-slice-of-ds1.fasta")
    eng, row = _engine(tips, w)
    gp = eng.gp_create(pids, params=row)
    got, req = gp.hybrid_marginals(summands=True), gp.hybrid_requests()
    assert hexes("hybrid").tobytes() == got.hybrid.tobytes()
    assert hexes("summands").tobytes() == got.summands.tobytes()
    assert [int(x) for x in lines["summand_entries"].split()] == req.summands.reshape(-1).tolist()
    assert hexes("estimated_q").tobytes() == gp.estimate_sbn_parameters(hybrid=True).tobytes()
    gp.close()
