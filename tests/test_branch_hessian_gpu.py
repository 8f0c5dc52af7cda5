"""The branch-length Hessian call (mi_engine_branch_hessian_unrooted, Engine.branch_hessian):
the diagonal d^2 logL / d t_j^2 per tree and branch, the squared-derivative sum S_j, and the
first-order outputs of the same pass.  Checked against four-point central differences of the
oracle's analytic gradient, the closed form of a three-taxon tree, and the engine's own
gradient call."""
import numpy as np
import pytest

import hessian_fd as H
import oracle_lib as O
import tree_utils as TU

pytestmark = pytest.mark.gpu

WALK = "gradient_walk_hess_kernel"  # K <= 4 with tip masks
HBM = "gradient_hbm_hess_kernel"    # everything else, and MI_PHYLO_GRADIENT_PATH=hbm


def _params(spec, T, **blocks):
    import test_gpu_parity as TG
    return TG._params(spec, T, **blocks)


def _engine(subst, site, tips, w, **kw):
    import libsbn_amd as L
    return L.Engine(L.PhyloModelSpecification(subst, site, "strict"), tips, w, device=0, **kw)


def _model_params(spec, subst, site, T, rng):
    blocks = {}
    if subst == "GTR":
        gr, gf = TU.random_gtr_params(T, rng)
        blocks.update({"GTR rates": gr, "frequencies": gf})
    if site != "constant":
        blocks["Weibull shape"] = rng.uniform(0.4, 1.6, size=(T, 1))
    return _params(spec, T, **blocks)


def _check_fd(h, fd, bls, skip_short=True):
    """|H - FD| <= 1e-6 max |H| per tree (branches shorter than 1e-3 left out of the comparison)."""
    for t in range(h.shape[0]):
        keep = np.ones(h.shape[1], bool)
        if skip_short:
            keep[:bls.shape[1] - 1] = bls[t, :-1] >= 1e-3
        scale = np.max(np.abs(h[t]))
        assert scale > 0
        err = np.max(np.abs(h[t, keep] - fd[t, keep]))
        assert err <= 1e-6 * scale, (t, err, scale)
    assert np.all(h[:, -2:] == 0)


def _path(eng, kernel, store=None, rescaled=False):
    p = eng.last_call_path()
    assert p.startswith(kernel + " ") and " hess" in p and ("rescaled" in p) == rescaled, p
    if store:
        assert f" store={store} " in p, p
    assert eng.last_call_info()[0] == kernel
    return p


# ---- 1. finite differences of the oracle's analytic gradient ----

@pytest.mark.parametrize("subst,site", [("JC69", "constant"), ("JC69", "weibull+2"),
                                        ("JC69", "weibull+3"), ("GTR", "weibull+4")])
def test_ds1_matches_oracle_finite_differences(subst, site):
    st = O.load_struct("ds1_top100")
    tips, w, pids, bls = O.struct_arrays(st)
    n, P = tips.shape
    T = 3
    pids, bls = pids[:T], bls[:T]
    spec = O.make_spec(n, P, subst, site)
    pr = _model_params(spec, subst, site, T, np.random.default_rng(11))
    eng = _engine(subst, site, tips, w)
    ll, g, h = eng.branch_hessian(pids, bls, pr)
    assert f"K={spec.category_count}" in _path(eng, WALK, "lds")
    _check_fd(h, H.fd_hessian_diagonal(spec, tips, w, pids, bls, pr), bls)
    og = O.unrooted_gradients(spec, tips, w, pids, bls, pr, False, 4)
    assert np.allclose(ll, og["log_likelihood"], rtol=1e-11, atol=0)
    assert np.max(np.abs(g - og["branch_lengths"])) <= 1e-10 * np.max(np.abs(g))


def _random_case(n, P, T, site, seed):
    rng = np.random.default_rng(seed)
    tips, w = TU.random_alignment(n, P, rng)
    pids, _ = TU.random_trees(n, T, rng)
    bls = rng.uniform(0.01, 0.5, size=(T, 2 * n - 2))
    bls[:, -1] = 0.0
    spec = O.make_spec(n, P, "JC69", site)
    pr = _model_params(spec, "JC69", site, T, rng)
    return tips, w, pids, bls, spec, pr


def test_arena_random_trees_match_oracle_finite_differences(monkeypatch):
    """40 x 600 x 64 random trees with the walk's stored vectors in the arena: the first four
    against the oracle, all 64 against the HBM Hessian kernel."""
    tips, w, pids, bls, spec, pr = _random_case(40, 600, 64, "weibull+4", 5)
    monkeypatch.setenv("MI_PHYLO_GRADIENT_STORE", "arena")
    eng = _engine("JC69", "weibull+4", tips, w)
    ll, g, h, s = eng.branch_hessian(pids, bls, pr, squared_gradient=True)
    _path(eng, WALK, "arena")
    _check_fd(h[:4], H.fd_hessian_diagonal(spec, tips, w, pids[:4], bls[:4], pr[:4]), bls[:4],
              skip_short=False)
    monkeypatch.setenv("MI_PHYLO_GRADIENT_PATH", "hbm")
    hbm = _engine("JC69", "weibull+4", tips, w)
    ref = hbm.branch_hessian(pids, bls, pr, squared_gradient=True)
    _path(hbm, HBM, "hbm")
    for x, y in zip((ll, g, h, s), ref):
        assert np.max(np.abs(x - y)) <= 1e-12 * np.max(np.abs(y))


def test_six_categories_match_oracle_finite_differences():
    tips, w, pids, bls, spec, pr = _random_case(12, 200, 3, "weibull+6", 6)
    eng = _engine("JC69", "weibull+6", tips, w)
    _, _, h = eng.branch_hessian(pids, bls, pr)
    assert "K=6" in _path(eng, HBM, "hbm")
    _check_fd(h, H.fd_hessian_diagonal(spec, tips, w, pids, bls, pr), bls, skip_short=False)


def test_real_valued_tip_partials_match_finite_differences_of_the_gradient():
    """Ambiguous real-valued tip partials (no mask form: the HBM Hessian kernel).  The oracle
    takes tip states only, so the reference is four-point differences of the same engine's
    gradient call (gradient_hbm_kernel).  That call shares the tree set-up, model instances and
    transition matrices with the Hessian call, so an error there would cancel; those steps are
    checked against the oracle by every other case here and by tests/test_gpu_parity.py."""
    tips, w, pids, bls, spec, pr = _random_case(10, 120, 2, "weibull+4", 7)
    rng = np.random.default_rng(8)
    n, P = tips.shape
    parts = np.zeros((n, P, 4))
    for i in range(n):
        for p in range(P):
            s = tips[i, p]
            parts[i, p] = 1.0 if s > 3 else 0.0
            if s <= 3:
                parts[i, p, s] = 1.0
    parts[:3] = np.where(parts[:3] > 0, 1.0, rng.uniform(0.05, 0.4, size=parts[:3].shape))
    eng = _engine("JC69", "weibull+4", None, w, use_tip_states=False, tip_partials=parts)
    _, g, h = eng.branch_hessian(pids, bls, pr)
    _path(eng, HBM, "hbm")
    T, nbr = len(pids), 2 * n - 3
    fd = np.zeros_like(h)
    for t in range(T):
        for j in range(nbr):
            hh = 1e-4 * bls[t, j]
            rows = np.repeat(bls[t:t + 1], 4, axis=0)
            for k, s in enumerate((1.0, -1.0, 2.0, -2.0)):
                rows[k, j] += s * hh
            gr = eng.gradients(np.repeat(pids[t:t + 1], 4, axis=0), rows, np.repeat(pr[t:t + 1], 4, axis=0),
                               gradient_blocks=())
            gj = [x.gradient["branch_lengths"][j] for x in gr]
            fd[t, j] = (8.0 * (gj[0] - gj[1]) - (gj[2] - gj[3])) / (12.0 * hh)
    _check_fd(h, fd, bls, skip_short=False)


def test_ladder_200_taxa_rescaled_matches_oracle_finite_differences():
    rng = np.random.default_rng(9)
    n, P = 200, 24
    tips, w = TU.random_alignment(n, P, rng)
    pids = np.stack([TU.ladder_topology(n)])
    bls = rng.uniform(0.01, 0.5, size=(1, 2 * n - 2))
    bls[:, -1] = 0.0
    spec = O.make_spec(n, P, "JC69", "weibull+4")
    pr = _model_params(spec, "JC69", "weibull+4", 1, rng)
    eng = _engine("JC69", "weibull+4", tips, w)
    _, _, h = eng.branch_hessian(pids, bls, pr, rescaling=True)
    _path(eng, WALK, rescaled=True)
    _check_fd(h, H.fd_hessian_diagonal(spec, tips, w, pids, bls, pr, rescaling=True), bls,
              skip_short=False)


# ---- 2. S exactly: one pattern of weight 1 at a time, the oracle's gradient is d log L_p / dt ----

@pytest.mark.parametrize("name,T,site", [("hello", 1, "weibull+4"), ("ds1_top100", 2, "weibull+4"),
                                         ("ds1_top100", 2, "constant"), ("ds1_top100", 2, "weibull+2"),
                                         ("ds1_top100", 2, "weibull+3")])
def test_squared_gradient_sum_matches_per_pattern_oracle(name, T, site):
    """The walk's per-pattern reduction of D1 depends on K (the 4x4 blocks of a register are
    categories for K > 2, further patterns below): every K."""
    st = O.load_struct(name)
    tips, w, pids, bls = O.struct_arrays(st)
    n, P = tips.shape
    pids, bls = pids[:T], bls[:T]
    spec = O.make_spec(n, P, "JC69", site)
    pr = _model_params(spec, "JC69", site, T, np.random.default_rng(12))
    eng = _engine("JC69", site, tips, w)
    _, _, _, s = eng.branch_hessian(pids, bls, pr, squared_gradient=True)
    _path(eng, WALK)
    one = O.make_spec(n, 1, "JC69", site)
    want = np.zeros_like(s)
    for p in range(P):
        gp = O.unrooted_gradients(one, tips[:, p:p + 1], np.ones(1), pids, bls, pr, False, 4)
        want += w[p] * gp["branch_lengths"] ** 2
    assert np.max(np.abs(s - want) / np.maximum(np.abs(want), 1e-300)) <= 1e-10
    assert np.all(s[:, -2:] == 0)


# ---- 3. closed form: three-taxon JC69 star tree ----

def test_star_tree_closed_form():
    rng = np.random.default_rng(13)
    P = 50
    tips = rng.integers(0, 5, size=(3, P)).astype(np.int32)
    w = rng.integers(1, 4, size=P).astype(float)
    pids = np.array([[3, 3, 3]], np.int32)
    bls = np.array([[0.05, 0.17, 0.42, 0.0]])
    ll0, g0, h0, s0 = H.jc69_star_tree(tips, w, bls[0, :3])
    eng = _engine("JC69", "constant", tips, w)
    ll, g, h, s = eng.branch_hessian(pids, bls, None, squared_gradient=True)
    _path(eng, WALK)
    assert abs(ll[0] - ll0) <= 1e-12 * abs(ll0)
    for got, want in ((g, g0), (h, h0), (s, s0)):
        assert np.max(np.abs(got[0, :3] - want)) <= 1e-12 * np.max(np.abs(want))
        assert np.all(got[0, 3:] == 0)


# ---- 4. the first-order outputs are the gradient call's ----

@pytest.mark.parametrize("subst,site", [("JC69", "weibull+4"), ("GTR", "weibull+4"), ("JC69", "constant")])
def test_first_order_outputs_match_the_gradient_call(monkeypatch, subst, site):
    """log L and g of the Hessian call: bit for bit those of the gradient call on the same
    kernel family (the walk's branch sums and the HBM kernel's, reduced in the same tile
    order), within 1e-12 of the default (look-up walk) gradient call."""
    st = O.load_struct("ds1_top100")
    tips, w, pids, bls = O.struct_arrays(st)
    n, P = tips.shape
    T = 40
    pids, bls = pids[:T], bls[:T]
    spec = O.make_spec(n, P, subst, site)
    pr = _model_params(spec, subst, site, T, np.random.default_rng(14))

    def grad(eng):
        ref = eng.gradients(pids, bls, pr, gradient_blocks=())
        return np.array([x.log_likelihood for x in ref]), np.stack([x.gradient["branch_lengths"] for x in ref])

    eng = _engine(subst, site, tips, w)
    ll, g, _ = eng.branch_hessian(pids, bls, pr)
    _path(eng, WALK)
    rll, rg = grad(eng)
    assert np.all(np.abs(ll - rll) <= 1e-12 * np.abs(rll))
    assert np.max(np.abs(g - rg)) <= 1e-12 * np.max(np.abs(rg))
    monkeypatch.setenv("MI_PHYLO_GRADIENT_WALK", "v2")
    v2 = _engine(subst, site, tips, w)
    vll, vg = grad(v2)
    assert v2.last_call_info()[0] == "gradient_walk_kernel"
    assert np.array_equal(ll, vll) and np.array_equal(g, vg)
    monkeypatch.delenv("MI_PHYLO_GRADIENT_WALK")
    monkeypatch.setenv("MI_PHYLO_GRADIENT_PATH", "hbm")
    hbm = _engine(subst, site, tips, w)
    hll, hg = grad(hbm)
    assert hbm.last_call_info()[0] == "gradient_hbm_kernel"
    ll2, g2, _ = hbm.branch_hessian(pids, bls, pr)
    _path(hbm, HBM, "hbm")
    assert np.array_equal(ll2, hll) and np.array_equal(g2, hg)


# ---- 5. the two implementations agree; rescaling on and off agree ----

@pytest.mark.parametrize("subst,site", [("JC69", "constant"), ("JC69", "weibull+2"), ("JC69", "weibull+3"),
                                        ("GTR", "weibull+4")])
def test_walk_and_hbm_kernel_agree(monkeypatch, subst, site):
    st = O.load_struct("ds1_top100")
    tips, w, pids, bls = O.struct_arrays(st)
    n, P = tips.shape
    T = 30
    spec = O.make_spec(n, P, subst, site)
    pr = _model_params(spec, subst, site, T, np.random.default_rng(19))
    eng = _engine(subst, site, tips, w)
    monkeypatch.setenv("MI_PHYLO_GRADIENT_PATH", "hbm")
    hbm = _engine(subst, site, tips, w)
    for rescaling in (False, True):
        a = eng.branch_hessian(pids[:T], bls[:T], pr, rescaling=rescaling, squared_gradient=True)
        _path(eng, WALK, "lds", rescaled=rescaling)
        b = hbm.branch_hessian(pids[:T], bls[:T], pr, rescaling=rescaling, squared_gradient=True)
        _path(hbm, HBM, "hbm", rescaled=rescaling)
        for x, y in zip(a, b):
            assert np.max(np.abs(x - y)) <= 1e-12 * np.max(np.abs(y))


def test_rescaling_on_and_off_agree():
    st = O.load_struct("ds1_top100")
    tips, w, pids, bls = O.struct_arrays(st)
    n, P = tips.shape
    T = 20
    spec = O.make_spec(n, P, "GTR", "weibull+4")
    pr = _model_params(spec, "GTR", "weibull+4", T, np.random.default_rng(15))
    eng = _engine("GTR", "weibull+4", tips, w)
    a = eng.branch_hessian(pids[:T], bls[:T], pr, squared_gradient=True)
    _path(eng, WALK)
    b = eng.branch_hessian(pids[:T], bls[:T], pr, rescaling=True, squared_gradient=True)
    _path(eng, WALK, rescaled=True)
    for x, y in zip(a, b):
        assert np.max(np.abs(x - y)) <= 1e-10 * np.max(np.abs(x))


# ---- 6. sharded handles, graphs, refusal ----

def test_sharded_handles():
    st = O.load_struct("ds1_top100")
    tips, w, pids, bls = O.struct_arrays(st)
    n, P = tips.shape
    T = 37
    spec = O.make_spec(n, P, "JC69", "weibull+4")
    pr = _model_params(spec, "JC69", "weibull+4", T, np.random.default_rng(16))
    one = _engine("JC69", "weibull+4", tips, w)
    ref = one.branch_hessian(pids[:T], bls[:T], pr, squared_gradient=True)
    trees = _engine("JC69", "weibull+4", tips, w, shard_devices=[0, 0])
    got = trees.branch_hessian(pids[:T], bls[:T], pr, squared_gradient=True)
    _path(trees, WALK)
    for x, y in zip(ref, got):
        assert np.array_equal(x, y)
    pats = _engine("JC69", "weibull+4", tips, w, shard_devices=[0, 0], shard_mode="patterns")
    got = pats.branch_hessian(pids[:T], bls[:T], pr, squared_gradient=True)
    for x, y in zip(ref, got):
        assert np.max(np.abs(x - y)) <= 1e-12 * np.max(np.abs(x))


def test_device_call_replayed_from_a_graph():
    torch = pytest.importorskip("torch")
    st = O.load_struct("ds1_top100")
    tips, w, pids, bls = O.struct_arrays(st)
    n, P = tips.shape
    N, T = 2 * n - 1, 64
    spec = O.make_spec(n, P, "JC69", "weibull+4")
    pr = _model_params(spec, "JC69", "weibull+4", T, np.random.default_rng(17))
    eng = _engine("JC69", "weibull+4", tips, w)
    ref = eng.branch_hessian(pids[:T], bls[:T], pr, squared_gradient=True)
    dev = torch.device("cuda", 0)
    d_pid = torch.from_numpy(np.ascontiguousarray(pids[:T], np.int32)).to(dev)
    d_bl = torch.from_numpy(np.ascontiguousarray(bls[:T])).to(dev)
    d_pr = torch.from_numpy(np.ascontiguousarray(pr)).to(dev)
    outs = [torch.zeros(T, dtype=torch.float64, device=dev)] + \
           [torch.zeros((T, N), dtype=torch.float64, device=dev) for _ in range(3)]
    eng.reserve_hessian(T)
    gs = torch.cuda.Stream()

    def call(stream):
        eng.branch_hessian_device(stream, T, d_pid.data_ptr(), d_bl.data_ptr(), d_pr.data_ptr(),
                                  outs[2].data_ptr(), out_ll=outs[0].data_ptr(),
                                  out_branch=outs[1].data_ptr(), out_gsq=outs[3].data_ptr())

    with torch.cuda.stream(gs):
        call(gs.cuda_stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=gs):
        call(torch.cuda.current_stream().cuda_stream)
    _path(eng, WALK)
    for _ in range(3):
        for o in outs:
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for o, r in zip(outs, ref):
            assert np.array_equal(o.cpu().numpy(), r)
    eng.check_status()


def test_twenty_state_engine_refuses():
    import aa_utils as A
    rng = np.random.default_rng(18)
    tips, w = A.random_aa_alignment(6, 20, rng)
    pids, bls = TU.random_trees(6, 2, rng)
    eng = _engine("WAG", "constant", tips, w)
    with pytest.raises(RuntimeError, match="4-state only"):
        eng.branch_hessian(pids, bls, None)
    with pytest.raises(RuntimeError, match="4-state only"):
        eng.reserve_hessian(2)
