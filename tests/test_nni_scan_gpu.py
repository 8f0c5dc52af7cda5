"""The NNI neighbourhood scan (mi_engine_nni_scan_unrooted, Engine.nni_scan): delta[t][v][i] =
logL(neighbour i of inner edge v) - logL(tree t) from one walk per tree.  The reference is the
oracle's log-likelihood of every neighbour rebuilt and renumbered by tests/nni_ref.py (which
does not use the library): |logL + delta - oracle logL(neighbour)| <= 1e-10 |oracle logL|, the
project's standing tolerance, and logL itself to the same bound."""
import numpy as np
import pytest

import nni_ref as R
import oracle_lib as O
import tree_utils as TU

pytestmark = pytest.mark.gpu

KERNEL = "nni_scan_hbm_kernel"
TOL = 1e-10


def _engine(subst, site, tips, w, **kw):
    import libsbn_amd as L
    return L.Engine(L.PhyloModelSpecification(subst, site, "strict"), tips, w, device=0, **kw)


def _model_params(spec, subst, site, T, rng):
    import test_gpu_parity as TG
    blocks = {}
    if subst == "GTR":
        gr, gf = TU.random_gtr_params(T, rng)
        blocks.update({"GTR rates": gr, "frequencies": gf})
    if site != "constant":
        blocks["Weibull shape"] = rng.uniform(0.4, 1.6, size=(T, 1))
    return TG._params(spec, T, **blocks)


def _site(K):
    return "constant" if K == 1 else f"weibull+{K}"


def _path(eng, rescaled=False):
    p = eng.last_call_path()
    assert p.startswith(KERNEL + " ") and " nni" in p and " store=hbm " in p, p
    assert ("rescaled" in p) == rescaled, p
    assert eng.last_call_info()[0] == KERNEL
    return p


def _oracle_neighbours(spec, tips, w, pid, bl, pr_row, rescaling):
    """Oracle log-likelihood of every neighbour of one tree, [2n-1][2] by (v, i)."""
    n = tips.shape[0]
    nb = R.all_neighbours(n, pid, bl)
    out = np.zeros((2 * n - 1, 2))
    if nb:
        pids = np.stack([x[2] for x in nb])
        bls = np.stack([x[3] for x in nb])
        ll = O.unrooted_log_likelihoods(spec, tips, w, pids, bls, np.repeat(pr_row[None], len(nb), axis=0),
                                        rescaling, 4)
        for (v, i, _, _), x in zip(nb, ll):
            out[v, i] = x
    return out


def _check(result, spec, tips, w, pids, bls, pr, rescaling=False, label=""):
    """logL and logL + delta against the oracle; zeros off the inner edges; the best move."""
    ll, delta, best = result
    n = tips.shape[0]
    T = len(pids)
    assert delta.shape == (T, 2 * n - 1, 2) and best.shape == (T,)
    oll = O.unrooted_log_likelihoods(spec, tips, w, pids, bls, pr, rescaling, 4)
    worst_ll = np.max(np.abs(ll - oll) / np.abs(oll))
    worst = 0.0
    edges = np.zeros(2 * n - 1, bool)
    edges[n:2 * n - 3] = True
    for t in range(T):
        want = _oracle_neighbours(spec, tips, w, pids[t], bls[t], pr[t], rescaling)
        got = ll[t] + delta[t]
        if edges.any():
            worst = max(worst, np.max(np.abs(got[edges] - want[edges]) / np.abs(want[edges])))
        assert np.all(delta[t][~edges] == 0), (label, t)
        assert best[t] == R.best_move(n, delta[t]), (label, t, best[t])
    print(f"{label}: logL {worst_ll:.2e}, logL + delta {worst:.2e}")
    assert worst_ll <= TOL, (label, worst_ll)
    assert worst <= TOL, (label, worst)


def _shape(name, rng):
    """(tips-free) topologies of the smallest shapes, T = 3 trees each."""
    if name == "n4":
        return 4, np.stack([TU.random_topology(4, rng) for _ in range(3)])
    if name == "n5":
        return 5, np.stack([TU.random_topology(5, rng) for _ in range(3)])
    if name == "balanced8":
        return 8, np.stack([TU.balanced_topology(8)] * 3)
    if name == "ladder9":
        return 9, np.stack([TU.ladder_topology(9)] * 3)
    return 12, np.stack([TU.random_topology(12, rng) for _ in range(3)])


SHAPES = ("n4", "n5", "balanced8", "ladder9", "random12")


def _case(name, P, subst, K, seed):
    rng = np.random.default_rng(seed)
    n, pids = _shape(name, rng)
    T = len(pids)
    tips, w = TU.random_alignment(n, P, rng)
    bls = rng.uniform(0.01, 0.5, size=(T, 2 * n - 2))
    bls[:, -1] = 0.0
    spec = O.make_spec(n, P, subst, _site(K))
    pr = _model_params(spec, subst, _site(K), T, rng)
    return tips, w, pids, bls, spec, pr


def test_balanced_eight_has_three_internal_root_children():
    """The tree in which the scan's three root-adjacent cases (c0 below the set-up root, c1 and
    c2 below the fixed node) all occur."""
    pid = TU.balanced_topology(8)
    root = 2 * 8 - 3
    kids = [v for v in range(root) if pid[v] == root]
    assert len(kids) == 3 and all(v >= 8 for v in kids), kids


# ---- 1. smallest shapes against the oracle ----

@pytest.mark.parametrize("P", [13, 70])
@pytest.mark.parametrize("K", [1, 2, 4, 6])
@pytest.mark.parametrize("subst", ["JC69", "GTR"])
def test_small_shapes_match_oracle(subst, K, P):
    for k, name in enumerate(SHAPES):
        tips, w, pids, bls, spec, pr = _case(name, P, subst, K, 1000 + 10 * K + k)
        eng = _engine(subst, _site(K), tips, w)
        res = eng.nni_scan(pids, bls, pr)
        assert f"K={K}" in _path(eng)
        assert eng.last_call_info()[1:] == (3, 3)
        _check(res, spec, tips, w, pids, bls, pr, label=f"{name} {subst} K={K} P={P}")


# ---- 2. real-valued tip partials (the other instantiation) ----

def _one_hot(tips):
    parts = np.zeros(tips.shape + (4,))
    for s in range(4):
        parts[..., s] = (tips == s) | (tips > 3)
    return parts


@pytest.mark.parametrize("subst,K", [("JC69", 4), ("GTR", 1), ("GTR", 6)])
def test_tip_partials_match_oracle(subst, K):
    for k, name in enumerate(("balanced8", "random12")):
        tips, w, pids, bls, spec, pr = _case(name, 70, subst, K, 2000 + 10 * K + k)
        eng = _engine(subst, _site(K), None, w, use_tip_states=False, tip_partials=_one_hot(tips))
        res = eng.nni_scan(pids, bls, pr)
        _path(eng)
        _check(res, spec, tips, w, pids, bls, pr, label=f"partials {name} {subst} K={K}")


# ---- 3. rescaling ----

@pytest.mark.parametrize("subst,K", [("JC69", 4), ("GTR", 2)])
def test_rescaling_on_and_off_agree(subst, K):
    for k, name in enumerate(("balanced8", "random12")):
        tips, w, pids, bls, spec, pr = _case(name, 70, subst, K, 3000 + 10 * K + k)
        eng = _engine(subst, _site(K), tips, w)
        ll, d, best = eng.nni_scan(pids, bls, pr)
        _path(eng)
        rll, rd, rbest = eng.nni_scan(pids, bls, pr, rescaling=True)
        _path(eng, rescaled=True)
        assert np.all(np.abs(rll - ll) <= 1e-12 * np.abs(ll))
        assert np.all(np.abs((rll[:, None, None] + rd) - (ll[:, None, None] + d)) <= 1e-12 * np.abs(ll)[:, None, None])
        assert np.array_equal(best, rbest)
        _check((rll, rd, rbest), spec, tips, w, pids, bls, pr, rescaling=True, label=f"rescaled {name} {subst} K={K}")


def _big_case(n, P, pid, seed):
    rng = np.random.default_rng(seed)
    tips, w = TU.random_alignment(n, P, rng)
    pids = np.stack([pid(rng)])
    bls = rng.uniform(0.01, 0.5, size=(1, 2 * n - 2))
    bls[:, -1] = 0.0
    spec = O.make_spec(n, P, "JC69", "weibull+4")
    pr = _model_params(spec, "JC69", "weibull+4", 1, rng)
    return tips, w, pids, bls, spec, pr


def test_ladder_200_taxa_rescaled_matches_oracle():
    tips, w, pids, bls, spec, pr = _big_case(200, 40, lambda rng: TU.ladder_topology(200), 31)
    eng = _engine("JC69", "weibull+4", tips, w)
    res = eng.nni_scan(pids, bls, pr, rescaling=True)
    _path(eng, rescaled=True)
    _check(res, spec, tips, w, pids, bls, pr, rescaling=True, label="ladder 200")


# ---- 4. beyond 257 taxa: the other tree set-up kernels ----

def test_random_300_taxa_matches_oracle():
    tips, w, pids, bls, spec, pr = _big_case(300, 20, lambda rng: TU.random_topology(300, rng), 41)
    eng = _engine("JC69", "weibull+4", tips, w)
    res = eng.nni_scan(pids, bls, pr)
    _path(eng)
    _check(res, spec, tips, w, pids, bls, pr, label="random 300")


# ---- 5. a second reference: the engine's own log-likelihood call on mi_nni_neighbour's trees ----

def _ds1(T, subst="JC69", seed=51):
    st = O.load_struct("ds1_top100")
    tips, w, pids, bls = O.struct_arrays(st)
    n, P = tips.shape
    spec = O.make_spec(n, P, subst, "weibull+4")
    pr = _model_params(spec, subst, "weibull+4", T, np.random.default_rng(seed))
    return tips, w, pids[:T], bls[:T], spec, pr


def test_ds1_matches_log_likelihoods_of_mi_nni_neighbour_trees():
    from libsbn_amd import nni_neighbour
    tips, w, pids, bls, spec, pr = _ds1(2)
    n, P = tips.shape
    assert (n, P) == (27, 934)
    eng = _engine("JC69", "weibull+4", tips, w)
    ll, d, best = eng.nni_scan(pids, bls, pr)
    _path(eng)
    own = eng.log_likelihoods(pids, bls, pr)
    for t in range(2):
        moves = [(v, i) for v in R.inner_edges(n) for i in (0, 1)]
        assert len(moves) == 48
        nb = [nni_neighbour(n, pids[t], bls[t], v, i) for v, i in moves]
        nll = eng.log_likelihoods(np.stack([x[0] for x in nb]), np.stack([x[1] for x in nb]),
                                  np.repeat(pr[t:t + 1], len(nb), axis=0))
        got = np.array([d[t, v, i] for v, i in moves])
        err = np.max(np.abs(got - (nll - own[t]))) / abs(own[t])
        print(f"DS1 tree {t}: delta against the log-likelihood call {err:.2e}")
        assert err <= TOL
        assert best[t] == R.best_move(n, d[t])


# ---- 6. logL is the HBM gradient call's, bit for bit ----

@pytest.mark.parametrize("rescaling", [False, True])
def test_log_likelihood_is_the_hbm_gradient_calls(monkeypatch, rescaling):
    tips, w, pids, bls, spec, pr = _ds1(5, "GTR", 61)
    eng = _engine("GTR", "weibull+4", tips, w)
    ll, _, _ = eng.nni_scan(pids, bls, pr, rescaling=rescaling)
    monkeypatch.setenv("MI_PHYLO_GRADIENT_PATH", "hbm")
    hbm = _engine("GTR", "weibull+4", tips, w)
    ref = hbm.gradients(pids, bls, pr, rescaling=rescaling, gradient_blocks=())
    assert hbm.last_call_info()[0] == "gradient_hbm_kernel"
    assert np.array_equal(ll, np.array([x.log_likelihood for x in ref]))


# ---- 8. three taxa: nothing to exchange ----

def test_three_taxa():
    rng = np.random.default_rng(81)
    tips, w = TU.random_alignment(3, 13, rng)
    pids = np.array([[3, 3, 3]] * 2, np.int32)
    bls = rng.uniform(0.01, 0.5, size=(2, 4))
    spec = O.make_spec(3, 13, "JC69", "weibull+4")
    pr = _model_params(spec, "JC69", "weibull+4", 2, rng)
    eng = _engine("JC69", "weibull+4", tips, w)
    ll, d, best = eng.nni_scan(pids, bls, pr)
    _path(eng)
    assert np.all(best == -1) and np.all(d == 0) and d.shape == (2, 5, 2)
    oll = O.unrooted_log_likelihoods(spec, tips, w, pids, bls, pr, False, 4)
    assert np.all(np.abs(ll - oll) <= TOL * np.abs(oll))


# ---- 9. the walk in parts of the vector arena ----

def test_chunked_call_is_bit_identical(monkeypatch):
    tips, w, pids, bls, spec, pr = _case("random12", 70, "GTR", 4, 91)
    rng = np.random.default_rng(92)
    T, n = 5, 12
    pids = np.stack([TU.random_topology(n, rng) for _ in range(T)])
    bls = rng.uniform(0.01, 0.5, size=(T, 2 * n - 2))
    pr = _model_params(spec, "GTR", "weibull+4", T, rng)
    whole = _engine("GTR", "weibull+4", tips, w)
    ref = whole.nni_scan(pids, bls, pr)
    assert whole.last_call_launches()[0] == 1
    per_eval = (n - 1) * 4 * 2 * 64 * 4 * 8  # [node][category][two tiles of 64 patterns][state] doubles
    monkeypatch.setenv("MI_PHYLO_PLV_BYTES", str(2 * per_eval + per_eval // 2))
    parts = _engine("GTR", "weibull+4", tips, w)
    got = parts.nni_scan(pids, bls, pr)
    assert parts.last_call_launches()[0] == 3
    for x, y in zip(ref, got):
        assert np.array_equal(x, y)
    _check(got, spec, tips, w, pids, bls, pr, label="chunked")


# ---- 10. sharded handles ----

def test_sharded_handles():
    tips, w, pids, bls, spec, pr = _ds1(7, "JC69", 101)
    n = tips.shape[0]
    one = _engine("JC69", "weibull+4", tips, w)
    ref = one.nni_scan(pids, bls, pr)
    trees = _engine("JC69", "weibull+4", tips, w, shard_devices=[0, 0])
    got = trees.nni_scan(pids, bls, pr)
    _path(trees)
    for x, y in zip(ref, got):
        assert np.array_equal(x, y)
    pats = _engine("JC69", "weibull+4", tips, w, shard_devices=[0, 0], shard_mode="patterns")
    ll, d, best = pats.nni_scan(pids, bls, pr)
    scale = np.abs(ref[0])
    assert np.all(np.abs(ll - ref[0]) <= 1e-12 * scale)
    assert np.all(np.abs((ll[:, None, None] + d) - (ref[0][:, None, None] + ref[1])) <= 1e-12 * scale[:, None, None])
    assert np.all(d[:, :n] == 0) and np.all(d[:, -2:] == 0)
    assert [int(b) for b in best] == [R.best_move(n, d[t]) for t in range(len(pids))]


# ---- 11. the device-pointer call, reserved, from a graph ----

def test_device_call_replayed_from_a_graph():
    torch = pytest.importorskip("torch")
    T = 16
    tips, w, pids, bls, spec, pr = _ds1(T, "JC69", 111)
    N = 2 * tips.shape[0] - 1
    eng = _engine("JC69", "weibull+4", tips, w)
    ref = eng.nni_scan(pids, bls, pr)
    dev = torch.device("cuda", 0)
    d_pid = torch.from_numpy(np.ascontiguousarray(pids, np.int32)).to(dev)
    d_bl = torch.from_numpy(np.ascontiguousarray(bls)).to(dev)
    d_pr = torch.from_numpy(np.ascontiguousarray(pr)).to(dev)
    outs = [torch.zeros(T, dtype=torch.float64, device=dev),
            torch.zeros((T, N, 2), dtype=torch.float64, device=dev),
            torch.zeros(T, dtype=torch.int32, device=dev)]
    gs = torch.cuda.Stream()

    def call(stream, engine=None):
        (engine or fresh).nni_scan_device(stream, T, d_pid.data_ptr(), d_bl.data_ptr(), d_pr.data_ptr(),
                                          outs[1].data_ptr(), out_ll=outs[0].data_ptr(),
                                          out_best=outs[2].data_ptr())

    # (the other engine runs the same call on the stream first: the kernels' code objects are
    # loaded -- into device memory -- at their first launch, which is not the engine's allocation)
    call(gs.cuda_stream, eng)
    torch.cuda.synchronize()
    fresh = _engine("JC69", "weibull+4", tips, w)
    fresh.reserve_nni_scan(T)
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info(0)[0]
    with torch.cuda.stream(gs):
        call(gs.cuda_stream)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info(0)[0] == free_before  # (reserved: the call allocated nothing)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=gs):
        call(torch.cuda.current_stream().cuda_stream)
    _path(fresh)
    for _ in range(3):
        for o in outs:
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for o, r in zip(outs, ref):
            assert np.array_equal(o.cpu().numpy(), r)
    fresh.check_status()


# ---- 12. refusals ----

def test_twenty_state_engine_refuses():
    import aa_utils as A
    rng = np.random.default_rng(121)
    tips, w = A.random_aa_alignment(6, 20, rng)
    pids, bls = TU.random_trees(6, 2, rng)
    eng = _engine("WAG", "constant", tips, w)
    with pytest.raises(RuntimeError, match="4-state only"):
        eng.nni_scan(pids, bls, None)
    with pytest.raises(RuntimeError, match="4-state only"):
        eng.reserve_nni_scan(2)


def test_bad_tree_is_reported():
    tips, w, pids, bls, spec, pr = _case("n5", 13, "JC69", 1, 131)
    bad = pids.copy()
    bad[1, 0] = 0
    eng = _engine("JC69", "constant", tips, w)
    with pytest.raises(RuntimeError, match="post-order id form"):
        eng.nni_scan(bad, bls, pr)
