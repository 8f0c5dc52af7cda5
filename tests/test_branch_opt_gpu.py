"""The branch-length optimisation call (mi_engine_optimize_branch_lengths_unrooted,
Engine.optimize_branch_lengths): maximum-likelihood branch lengths of a batch of unrooted trees
under box bounds, iterated on the device.  Optimality is judged with the ORACLE evaluated at
the returned lengths (never with the engine's own outputs) and against the independent
reference optimum of tests/branch_opt_ref.py."""
import numpy as np
import pytest

import branch_opt_ref as R
import oracle_lib as O
import tree_utils as TU

pytestmark = pytest.mark.gpu

WALK = "gradient_walk_hess_kernel"  # K <= 4 with tip masks
HBM = "gradient_hbm_hess_kernel"    # everything else
TOL, LO, HI = 1e-6, 1e-8, 10.0      # the call's defaults
UPPER = 0.02                        # tests/test_branch_opt_ref.py shows the case is real


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


def _ds1(subst="JC69", site="constant", T=4, seed=21, first=0):
    st = O.load_struct("ds1_top100")
    tips, w, pids, _ = O.struct_arrays(st)
    n, P = tips.shape
    spec = O.make_spec(n, P, subst, site)
    pr = _model_params(spec, subst, site, T, np.random.default_rng(seed))
    start = np.full((T, 2 * n - 2), 0.1)
    start[:, -1] = 0.0
    return spec, tips, w, pids[first:first + T], start, pr


def _path(eng, kernel, store=None, rescaled=False):
    p = eng.last_call_path()
    assert p.startswith(kernel + " ") and " hess" in p and " opt iters=" in p and " evals=" in p, p
    assert ("rescaled" in p) == rescaled, p
    if store:
        assert f" store={store} " in p, p
    assert eng.last_call_info()[0] == kernel
    return p


def _evaluators(spec, tips, w, pids, start, pr, rescaling=False):
    return [R.OracleTree(spec, tips, w, pids[t], pr[t], rescaling, fixed_entry=start[t, -1])
            for t in range(len(pids))]


def _check(eng, res, fs, pids, start, pr, rescaling=False, lo=LO, hi=HI, tol=TOL, reference=True,
           all_converged=True):
    """Checks 1 to 4 of a result against the oracle evaluators fs (one per tree)."""
    T, nb = len(pids), pids.shape[1]
    assert res.branch_lengths.shape == (T, nb + 1) and res.status.shape == (T,)
    assert np.array_equal(res.branch_lengths[:, -1], start[:, -1])  # the fixed node's entry
    assert np.all(res.branch_lengths[:, :nb] >= lo) and np.all(res.branch_lengths[:, :nb] <= hi)
    assert np.all((res.status >= 0) & (res.status <= 2)) and np.all(res.iterations >= 1)
    if all_converged:
        assert np.all(res.status == 0), (res.status, res.iterations)
    # 1. self-consistency: logL is the oracle's at the returned lengths; g, H are a Hessian
    # call's of the same engine there
    ll2, g2, h2 = eng.branch_hessian(pids, res.branch_lengths, pr, rescaling=rescaling)
    for got, want in ((res.gradient, g2), (res.hessian, h2)):
        assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))
    refs = []
    for t in range(T):
        x = res.branch_lengths[t, :nb]
        oll, og = fs[t](x)
        oll, og = oll[0], og[0]
        rel = abs(res.log_likelihood[t] - oll) / abs(oll)
        crit = R.criterion(x, og, lo, hi)
        oll0, _ = fs[t](np.clip(start[t, :nb], lo, hi))
        print(f"tree {t}: status {res.status[t]} evals {res.iterations[t]} logL {oll!r} "
              f"engine-oracle {rel:.2e} criterion {crit:.3e} gain {oll - oll0[0]:.6f}")
        assert rel <= 1e-10
        # 2. optimality with the oracle's gradient
        if res.status[t] == 0:
            assert crit <= 2 * tol, (t, crit)
        # 4. monotone: no worse than the clamped start, whatever the status
        assert oll >= oll0[0], (t, oll, oll0[0])
        # 3. the same optimum as the reference method
        if reference and res.status[t] == 0:
            rx, rll, _, method = R.reference_optimum(None, None, None, pids[t], start[t], pr[t], rescaling,
                                                     lo, hi, f=fs[t])
            err = R.relative_length_error(x, rx[:nb])
            print(f"        reference ({method}) logL {rll!r} diff {oll - rll:.2e} lengths {err:.2e}")
            assert abs(oll - rll) <= 1e-7
            assert err <= 1e-5
            refs.append(rx)
    return refs


# ---- 5. coverage: every configuration through checks 1 to 4 ----

@pytest.mark.parametrize("subst,site", [("JC69", "constant"), ("JC69", "weibull+4"), ("GTR", "weibull+4")])
def test_ds1_optimum_matches_oracle_and_reference(subst, site):
    spec, tips, w, pids, start, pr = _ds1(subst, site, T=4)
    eng = _engine(subst, site, tips, w)
    res = eng.optimize_branch_lengths(pids, start, pr)
    assert f"K={spec.category_count}" in _path(eng, WALK, "lds")
    _check(eng, res, _evaluators(spec, tips, w, pids, start, pr), pids, start, pr)
    # 6. every DS1 tree ends with a branch on the lower bound
    assert np.all(np.sum(res.branch_lengths[:, :-1] == LO, axis=1) >= 1)


def _evolved_alignment(pids, n, P, rng, change=0.08):
    """Tip states evolved down the tree (a state changes with probability `change` per
    branch), so that the data carry a signal about every branch."""
    root = 2 * n - 3  # (the trifurcating root of the parent-id vector)
    states = np.zeros((root + 1, P), np.int32)
    states[root] = rng.integers(0, 4, size=P)
    for v in range(root - 1, -1, -1):
        flip = rng.random(P) < change
        states[v] = np.where(flip, rng.integers(0, 4, size=P), states[pids[v]])
    return states[:n].copy(), rng.integers(1, 6, size=P).astype(np.float64)


def _evolved_case(n, P, T, site, seed, start=0.1, change=0.08):
    """T random topologies and an alignment evolved down the first of them; every branch
    starts at `start`."""
    rng = np.random.default_rng(seed)
    pids, _ = TU.random_trees(n, T, rng)
    tips, w = _evolved_alignment(pids[0], n, P, rng, change)
    bls = np.full((T, 2 * n - 2), start)
    bls[:, -1] = 0.0
    spec = O.make_spec(n, P, "JC69", site)
    pr = _model_params(spec, "JC69", site, T, rng)
    return tips, w, pids, bls, spec, pr


def test_six_categories_run_the_hbm_kernel():
    tips, w, pids, start, spec, pr = _evolved_case(12, 200, 3, "weibull+6", 31)
    eng = _engine("JC69", "weibull+6", tips, w)
    res = eng.optimize_branch_lengths(pids, start, pr)
    assert "K=6" in _path(eng, HBM, "hbm")
    _check(eng, res, _evaluators(spec, tips, w, pids, start, pr), pids, start, pr)


def test_real_valued_tip_partials():
    """Tip 0 carries real-valued partial vectors (no mask form: the HBM Hessian kernel).  The
    oracle takes tip states only; the likelihood is linear in a tip's vector, which
    RealTipOracleTree uses to build logL and the gradient from the oracle's per-pattern values."""
    tips, w, pids, start, spec, pr = _evolved_case(8, 40, 2, "weibull+4", 32)
    rng = np.random.default_rng(33)
    n, P = tips.shape
    tips[rng.random((n, P)) < 0.05] = 4  # some gaps
    parts = np.zeros((n, P, 4))
    for i in range(n):
        for p in range(P):
            parts[i, p] = 1.0 if tips[i, p] > 3 else 0.0
            if tips[i, p] <= 3:
                parts[i, p, tips[i, p]] = 1.0
    parts[0] = np.where(parts[0] > 0, 1.0, rng.uniform(0.05, 0.4, size=parts[0].shape))
    eng = _engine("JC69", "weibull+4", None, w, use_tip_states=False, tip_partials=parts)
    res = eng.optimize_branch_lengths(pids, start, pr)
    _path(eng, HBM, "hbm")
    one = O.make_spec(n, 1, "JC69", "weibull+4")
    fs = [R.RealTipOracleTree(one, tips, w, parts[0], pids[t], pr[t]) for t in range(len(pids))]
    # (the evaluator itself: with one-hot vectors it is the oracle on the states)
    hot = R.RealTipOracleTree(one, tips, w, np.where(parts[0] == 1.0, 1.0, 0.0), pids[0], pr[0])
    plain = R.OracleTree(spec, tips, w, pids[0], pr[0])
    for a, b in zip(hot(start[0, :-1]), plain(start[0, :-1])):
        assert np.max(np.abs(a - b)) <= 1e-11 * np.max(np.abs(b))
    _check(eng, res, fs, pids, start, pr)


def test_ladder_200_taxa_rescaled():
    """(160 patterns evolved down the ladder: with 24 or 96 the likelihood has several local
    optima in the branch lengths -- the two reference methods end 12 logL units apart -- and
    "the same optimum" is not defined.)"""
    rng = np.random.default_rng(35)
    n, P = 200, 160
    pids = np.stack([TU.ladder_topology(n)])
    tips, w = _evolved_alignment(pids[0], n, P, rng, change=0.1)
    start = np.full((1, 2 * n - 2), 0.1)
    start[:, -1] = 0.0
    spec = O.make_spec(n, P, "JC69", "weibull+4")
    pr = _model_params(spec, "JC69", "weibull+4", 1, rng)
    eng = _engine("JC69", "weibull+4", tips, w)
    res = eng.optimize_branch_lengths(pids, start, pr, rescaling=True)
    _path(eng, WALK, rescaled=True)
    _check(eng, res, _evaluators(spec, tips, w, pids, start, pr, True), pids, start, pr, rescaling=True)


def test_arena_store_36_taxa_1812_patterns(monkeypatch):
    """36 taxa x 1812 patterns with the walk's stored vectors in the arena.  The alignment is
    random, evolved down the first of two random topologies.  (Tip states drawn independently
    carry no signal: 57 of the 69 optimal branches sit on max_length, the rest are flat
    directions, and neither reference method reaches the convergence criterion in 100 s --
    4e-5 and 1e-4 -- or agrees with the other on the lengths to better than 6e-5: there is no
    optimum to compare with.)"""
    tips, w, pids, start, spec, pr = _evolved_case(36, 1812, 2, "weibull+4", 35)
    monkeypatch.setenv("MI_PHYLO_GRADIENT_STORE", "arena")
    eng = _engine("JC69", "weibull+4", tips, w)
    res = eng.optimize_branch_lengths(pids, start, pr)
    _path(eng, WALK, "arena")
    _check(eng, res, _evaluators(spec, tips, w, pids, start, pr), pids, start, pr)


def test_gradient_and_hessian_at_the_optimum_match_the_analytic_reference():
    """res.gradient and res.hessian per branch at the lengths where the optimiser stops, branches
    ON the lower bound among them, against tests/dense_ref.py (long double, no pre-order pass)
    under the bounds of tests/test_branch_hessian_edges_gpu.py.  (_check compares them with the
    same engine's Hessian call only.)"""
    import dense_ref as D
    tips, w, pids, start, spec, pr = _evolved_case(8, 49, 2, "weibull+4", 41)
    eng = _engine("JC69", "weibull+4", tips, w)
    res = eng.optimize_branch_lengths(pids, start, pr)
    _path(eng, WALK, "lds")
    _check(eng, res, _evaluators(spec, tips, w, pids, start, pr), pids, start, pr)
    Q, pi = D.gtr_q(np.ones(6), np.full(4, 0.25))
    for t in range(len(pids)):
        x = res.branch_lengths[t]
        assert np.sum((x[:-1] == LO) | (x[:-1] == HI)) >= 1, x
        m = O.model_set(spec, pr[t])
        ref = D.branch_derivatives(pids[t], x, Q, pi, m.cat_rates[:4], m.cat_weights[:4],
                                   D.tip_vectors(tips), w)
        tol = D.tolerances(ref, 1e-10)
        for got in (res.log_likelihood[t], res.gradient[t], res.hessian[t]):
            assert np.all(np.isfinite(np.asarray(got))), got
        rll = abs(res.log_likelihood[t] - ref.log_likelihood) / (1e-10 * abs(ref.log_likelihood))
        rg = np.max(np.abs(res.gradient[t, :-2] - ref.g[:-2]) / tol.g[:-2])
        rh = np.max(np.abs(res.hessian[t, :-2] - ref.H[:-2]) / tol.H[:-2])
        print(f"ratio optimum tree {t}: logL={float(rll):.3e} g={float(rg):.3e} H={float(rh):.3e} "
              f"on a bound: {np.flatnonzero((x[:-1] == LO) | (x[:-1] == HI))}")
        assert np.all(np.array([rll, rg, rh], dtype=D.LD) <= 1.0)  # (a NaN is not)
        assert np.all(res.gradient[t, -2:] == 0) and np.all(res.hessian[t, -2:] == 0)


# ---- 6. the upper bound ----

def test_small_max_length_ends_on_the_upper_bound():
    spec, tips, w, pids, start, pr = _ds1(T=1)
    eng = _engine("JC69", "constant", tips, w)
    res = eng.optimize_branch_lengths(pids, start, pr, max_length=UPPER)
    _path(eng, WALK)
    refs = _check(eng, res, _evaluators(spec, tips, w, pids, start, pr), pids, start, pr, hi=UPPER)
    at_upper = np.flatnonzero(res.branch_lengths[0, :-1] == UPPER)
    assert len(at_upper) >= 1
    assert np.array_equal(at_upper, np.flatnonzero(refs[0][:-1] >= UPPER))
    assert np.sum(res.branch_lengths[0, :-1] == LO) >= 1


# ---- 7. idempotence ----

def test_restart_from_the_optimum_changes_nothing():
    spec, tips, w, pids, start, pr = _ds1("JC69", "weibull+4", T=12)
    eng = _engine("JC69", "weibull+4", tips, w)
    first = eng.optimize_branch_lengths(pids, start, pr)
    assert np.all(first.status == 0)
    again = eng.optimize_branch_lengths(pids, first.branch_lengths, pr)
    print("evaluations of the restart:", again.iterations)
    assert np.all(again.status == 0)
    assert np.array_equal(again.branch_lengths, first.branch_lengths)
    assert np.all(again.iterations <= 2)  # the first evaluation and at most one more


# ---- 8. the iteration limit ----

def test_iteration_limit():
    spec, tips, w, pids, start, pr = _ds1(T=5)
    eng = _engine("JC69", "constant", tips, w)
    res = eng.optimize_branch_lengths(pids, start, pr, max_iterations=3)
    assert "opt iters=3 evals=15 " in _path(eng, WALK)
    assert np.all(res.status == 1) and np.all(res.iterations == 3)
    _check(eng, res, _evaluators(spec, tips, w, pids, start, pr), pids, start, pr, reference=False,
           all_converged=False)


# ---- 9. packing of the active trees ----

def test_packing_changes_the_cost_not_the_results():
    spec, tips, w, pids, start, pr = _ds1("JC69", "weibull+4", T=64)
    eng = _engine("JC69", "weibull+4", tips, w)
    opt = eng.optimize_branch_lengths(pids, start, pr)
    assert np.all(opt.status == 0)
    fresh = np.arange(2, 64, 4)  # 16 trees started away from their optimum, spread over the batch
    mixed = opt.branch_lengths.copy()
    mixed[fresh] = start[fresh]
    packed = eng.optimize_branch_lengths(pids, mixed, pr, check_interval=1)
    path = _path(eng, WALK)
    evals = eng.last_call_info()[1]
    assert "batches=64x1,16x" in path, path
    plain = eng.optimize_branch_lengths(pids, mixed, pr, check_interval=1, pack_active=False)
    plain_path = _path(eng, WALK)
    plain_evals = eng.last_call_info()[1]
    alone = eng.optimize_branch_lengths(pids[fresh], start[fresh], pr[fresh], check_interval=1)
    print(path, "|", plain_path, "| evaluations", evals, plain_evals, "max", packed.iterations.max())
    assert np.all(packed.status == 0) and np.all(plain.status == 0) and np.all(alone.status == 0)
    assert np.all(packed.iterations[np.setdiff1d(np.arange(64), fresh)] == 1)

    def same(a_ll, a_bl, b_ll, b_bl):
        assert np.all(np.abs(a_ll - b_ll) <= 1e-9 * np.abs(b_ll))
        for x, y in zip(a_bl, b_bl):
            assert R.relative_length_error(x[:-1], y[:-1]) <= 1e-5

    same(packed.log_likelihood, packed.branch_lengths, plain.log_likelihood, plain.branch_lengths)
    same(packed.log_likelihood[fresh], packed.branch_lengths[fresh], alone.log_likelihood, alone.branch_lengths)
    assert np.array_equal(packed.iterations, plain.iterations)
    assert evals < 64 * packed.iterations.max()
    assert evals < plain_evals == 64 * packed.iterations.max()


# ---- 10. handles and refusals ----

def test_tree_sharded_handle_gives_the_single_engines_results():
    spec, tips, w, pids, start, pr = _ds1("JC69", "weibull+4", T=9)
    one = _engine("JC69", "weibull+4", tips, w)
    ref = one.optimize_branch_lengths(pids, start, pr)
    trees = _engine("JC69", "weibull+4", tips, w, shard_devices=[0, 0])
    got = trees.optimize_branch_lengths(pids, start, pr)
    _path(trees, WALK)
    assert np.all(ref.status == 0)
    for name in ("branch_lengths", "log_likelihood", "gradient", "hessian", "iterations", "status"):
        assert np.array_equal(getattr(ref, name), getattr(got, name)), name


def test_refusals():
    import aa_utils as A
    spec, tips, w, pids, start, pr = _ds1(T=3)
    pats = _engine("JC69", "constant", tips, w, shard_devices=[0, 0], shard_mode="patterns")
    with pytest.raises(RuntimeError, match="pattern-sharded"):
        pats.optimize_branch_lengths(pids, start, pr)
    eng = _engine("JC69", "constant", tips, w)
    with pytest.raises(RuntimeError, match="max_iterations"):
        eng.optimize_branch_lengths(pids, start, pr, max_iterations=1001)
    with pytest.raises(RuntimeError, match="max_iterations"):
        eng.optimize_branch_lengths(pids, start, pr, max_iterations=0)
    with pytest.raises(RuntimeError, match="min_length"):
        eng.optimize_branch_lengths(pids, start, pr, min_length=1.0, max_length=0.5)
    bad = pids.copy()
    bad[1, 5] = 2  # a tip as a parent: not the reference's id form
    with pytest.raises(RuntimeError, match=r"\(tree 1\)"):
        eng.optimize_branch_lengths(bad, start, pr)
    # (the engine is still usable, and the error does not stick)
    assert np.all(eng.optimize_branch_lengths(pids, start, pr).status == 0)
    rng = np.random.default_rng(36)
    atips, aw = A.random_aa_alignment(6, 20, rng)
    apids, abls = TU.random_trees(6, 2, rng)
    aa = _engine("WAG", "constant", atips, aw)
    with pytest.raises(RuntimeError, match="4-state only"):
        aa.optimize_branch_lengths(apids, abls, None)
    with pytest.raises(RuntimeError, match="4-state only"):
        aa.reserve_branch_opt(2)


# ---- 11. the reserved device-pointer call ----

def test_reserved_device_call_allocates_nothing_and_matches_the_host_call():
    import torch
    spec, tips, w, pids, start, pr = _ds1("JC69", "weibull+4", T=64)
    n = tips.shape[0]
    N, T = 2 * n - 1, 64
    # 40 of the trees start at their optimum, so that the call also packs (24 are left)
    other = _engine("JC69", "weibull+4", tips, w)
    opt = other.optimize_branch_lengths(pids, start, pr)
    done = np.arange(T) % 8 < 5
    start[done] = opt.branch_lengths[done]
    ref = other.optimize_branch_lengths(pids, start, pr, check_interval=1)
    assert "batches=64x1,24x" in _path(other, WALK)
    dev = torch.device("cuda", 0)
    d_pid = torch.from_numpy(np.ascontiguousarray(pids, np.int32)).to(dev)
    d_bl = torch.from_numpy(np.ascontiguousarray(start)).to(dev)
    d_pr = torch.from_numpy(np.ascontiguousarray(pr)).to(dev)
    o_bl = torch.zeros((T, N - 1), dtype=torch.float64, device=dev)
    o_ll = torch.zeros(T, dtype=torch.float64, device=dev)
    o_g = torch.zeros((T, N), dtype=torch.float64, device=dev)
    o_h = torch.zeros((T, N), dtype=torch.float64, device=dev)
    o_it = torch.zeros(T, dtype=torch.int32, device=dev)
    o_st = torch.full((T,), 7, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream()

    def call(engine):
        engine.optimize_branch_lengths_device(stream.cuda_stream, T, d_pid.data_ptr(), d_bl.data_ptr(),
                                              d_pr.data_ptr(), o_bl.data_ptr(), o_ll.data_ptr(),
                                              o_st.data_ptr(), out_branch=o_g.data_ptr(),
                                              out_hess=o_h.data_ptr(), out_iterations=o_it.data_ptr(),
                                              check_interval=1)
        torch.cuda.synchronize()

    # The same call of ANOTHER engine first, on the same stream: what the HIP runtime sets up
    # on the first use of a stream (its queue, signals, staging for the 4-byte reads) is not the
    # engine's, and what is measured below is the engine under test alone.
    call(other)
    for o in (o_bl, o_ll, o_g, o_h, o_it):
        o.zero_()
    o_st.fill_(7)
    eng = _engine("JC69", "weibull+4", tips, w)
    eng.reserve_branch_opt(T)
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info(0)[0]
    call(eng)
    free_after = torch.cuda.mem_get_info(0)[0]
    assert "batches=64x1,24x" in _path(eng, WALK)
    eng.check_status()
    assert free_after == free_before, (free_before, free_after)
    for got, want in ((o_bl, ref.branch_lengths), (o_ll, ref.log_likelihood), (o_g, ref.gradient),
                      (o_h, ref.hessian), (o_it, ref.iterations), (o_st, ref.status)):
        assert np.array_equal(got.cpu().numpy(), want)
    host = eng.optimize_branch_lengths(pids, start, pr, check_interval=1)
    for name in ("branch_lengths", "log_likelihood", "gradient", "hessian", "iterations", "status"):
        assert np.array_equal(getattr(host, name), getattr(ref, name)), name
