"""The variational fit over the rooted trees of the subsplit DAG on the GPU against
tests/gp_vi_ref.py: the by-value calls against the numpy rules, the state-driven particles bit for
bit against the by-value calls, every step teacher-forced against the composition of the host-form
calls and the numpy update, a fit against its steps, a graph's replays and a checkpoint bit for bit,
long blocks, a one-tree DAG and -inf entries, the score identity over all trees, DAG-only objects on
other engines, what is refused, and that a fit raises its bound.
Shapes: hello (3 taxa), five_taxon_rooted (4 trees span its DAG), random rooted trees of 9 taxa."""
import os
import subprocess

import numpy as np
import pytest

import gp_ref as GR
import gp_trees_ref as TR
import gp_vi_ref as GV
import tree_utils as TU
import vi_fit_ref as F

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}
FILES = {"hello": ("hello_rooted.nwk", "hello.fasta"), "five": ("five_taxon_rooted.nwk", "five_taxon.fasta")}


def _case(name):
    """(engine, GeneralizedPruning, numpy DAG, model parameter row) of a fixture: made once"""
    import libsbn_amd as L
    if name not in _CACHE:
        pids, bls, tips, w, _ = GR.load_case(*FILES[name])
        eng = L.Engine(L.PhyloModelSpecification("JC69", "constant", "strict"), tips, w, device=0)
        params = np.ones(eng.param_count)
        gp = eng.gp_create(pids, bls, params)
        _CACHE[name] = (eng, gp, GR.build_dag(pids), params)
    return _CACHE[name]


def _start(gp, rng=None):
    """initial tables: the defaults of vi_create, log_params perturbed with rng"""
    phi = np.log(gp.get_sbn_parameters())
    if rng is not None:
        phi = phi + rng.normal(0.0, 1.0, phi.shape)
    return phi, gp.default_q_params()


def _fit(name, K, estimator="vimco", anneal_steps=0, seed=11, first_sample=0, rng=None, max_steps=16, step_size=(0.01, 0.005),
         start=None, case=None, **kw):
    eng, gp, d, params = _case(name) if case is None else case
    phi, q = _start(gp, rng) if start is None else start
    fit = gp.vi_create(phi, q, model_params=params, particle_count=K, estimator=estimator, anneal_steps=anneal_steps,
                       max_steps=max_steps, step_size=step_size, seed=seed, first_sample=first_sample, **kw)
    o = F.Options(K, 1, estimator, anneal_steps, kw.get("prior_rate", 10.0), kw.get("step_decay", 0.99),
                  kw.get("adam_beta0", 0.9), kw.get("adam_beta1", 0.999), kw.get("adam_epsilon", 1e-8), seed)
    return fit, GV.Composer(gp, o, params)


def _same_state(a, b):
    for name in ("log_params", "q_params", "sbn_moments", "q_moments", "step_size"):
        if np.asarray(getattr(a, name)).tobytes() != np.asarray(getattr(b, name)).tobytes():
            return False
    return (a.b0, a.b1, a.sbn_step_size, a.steps, a.successes, a.first_sample) == \
        (b.b0, b.b1, b.sbn_step_size, b.steps, b.successes, b.first_sample)


_WORST = {"element": 0.0, "trace": 0.0}


def _close(got, want, tol, what="element"):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    with np.errstate(invalid="ignore"):
        err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    err = np.where(same, 0.0, err)
    _WORST[what] = max(_WORST[what], float(np.max(err, initial=0.0)))
    assert np.all(err <= tol), (what, float(np.max(err)))


def _check_step(before, after, row, comp):
    """the fit's state and trace row after a step against the reference's step from `before`"""
    want, want_row = comp.step(F.state_of(before))
    for name in ("log_params", "q_params", "sbn_moments", "q_moments", "step_size"):
        _close(getattr(after, name), getattr(want, name), 1e-12)
    _close([after.b0, after.b1, after.sbn_step_size], [want.b0, want.b1, want.sbn_step_size], 1e-12)
    assert (after.steps, after.successes, after.first_sample) == (want.steps, want.successes, want.first_sample)
    assert row[0] == want_row[0] and row[5] == want_row[5]
    _close(row[1:3], want_row[1:3], 1e-10, "trace")
    _close(row[3:5], want_row[3:5], 1e-12)
    print("largest relative differences so far:", _WORST)


# ---- 0. the by-value calls are the numpy rules ----
@pytest.mark.parametrize("name,T", [("hello", 3), ("five", 70)])
def test_by_value_calls_against_the_numpy_rules(name, T):
    eng, gp, d, params = _case(name)
    rng = np.random.default_rng(4)
    phi = rng.normal(0.0, 1.0, d.G)
    lo = next((lo for lo, hi in TR.blocks(d) if hi - lo > 1), None)
    if lo is not None:
        phi[lo] = -np.inf
    lq, q = gp.log_normalize(phi)
    want_lq, want_q = GV.log_normalize(d, phi)
    _close(lq, want_lq, 1e-12)
    _close(q, want_q, 1e-12)
    kept = gp.get_sbn_parameters()
    gp.set_sbn_parameters(q)
    trees = gp.sample_trees(T, 3, first_sample=9)
    gp.set_sbn_parameters(kept)
    N = 2 * d.n - 1
    qp = np.stack([rng.normal(-2.5, 0.3, d.G), rng.uniform(0.1, 0.4, d.G)], axis=1)
    draw = gp.branch_sample(trees.entries, qp, 3, first_sample=9, prior_rate=7.0)
    bl, eps, lqb, lp = GV.branch_sample(trees.entries, qp, 3, 9, 7.0)
    for got, want in ((draw.branch_lengths, bl), (draw.epsilon, eps), (draw.log_q, lqb), (draw.log_prior, lp)):
        _close(got, want, 1e-12)
    assert np.all(draw.branch_lengths[:, -1] == 0.0)
    given = gp.branch_sample(trees.entries, qp, 0, prior_rate=7.0, epsilon=draw.epsilon)   # (the draws handed back)
    assert given.branch_lengths.tobytes() == draw.branch_lengths.tobytes() and given.log_q.tobytes() == draw.log_q.tobytes()
    un = eng.deroot_trees_mapped(trees.parent_ids, draw.branch_lengths)
    plain = eng.deroot_trees(trees.parent_ids, draw.branch_lengths)
    assert un.parent_ids.tobytes() == plain.parent_ids.tobytes() and un.branch_lengths.tobytes() == plain.branch_lengths.tobytes()
    for t in range(T):
        _, want_bl, edge, new_id = GV.deroot_mapped(trees.parent_ids[t], draw.branch_lengths[t])
        assert un.new_id[t].tobytes() == new_id.tobytes() and un.root_edge[t] == edge
        assert np.array_equal(un.branch_lengths[t], want_bl)
    g, ll, w = rng.normal(0.0, 30.0, (T, N)), rng.normal(-80.0, 5.0, T), rng.uniform(0.5, 1.5, T)
    got, lf = gp.branch_gradient(trees.entries, qp, draw, un.new_id, g, ll, log_q_topology=trees.log_q, tree_weights=w,
                                 beta=0.25, prior_rate=7.0)
    c0, c1 = GV.branch_terms(trees.entries, qp, draw.branch_lengths, draw.epsilon, un.new_id, g, 7.0, w)
    want = GV.ordered_sums(trees.entries, d.G, c0, c1)
    scale = GV.ordered_sums(trees.entries, d.G, np.abs(c0), np.abs(c1))
    assert np.all(np.abs(got - want) <= 1e-12 * np.maximum(1.0, scale)) and np.all(got[:d.R] == 0.0)
    _close(lf, GV.log_f(ll, draw.log_prior, trees.log_q, draw.log_q, 0.25), 1e-12)
    for estimator in ("plain", "vimco", "given"):
        tg, a = gp.topology_gradient(trees.entries, phi, lf, estimator=estimator)
        want_a = GV.factors(lf, estimator)
        _close(a, want_a, 1e-10 if estimator != "given" else 0.0)
        want_tg, scale = GV.topology_gradient(d, q, trees.entries, a)   # (from the library's factors: the sums alone)
        assert np.all(np.abs(tg - want_tg) <= 1e-12 * np.maximum(1.0, scale))


# ---- 1. the state-driven particles are the by-value particles ----
@pytest.mark.parametrize("first_sample", [5, 2 ** 32 - 1])
@pytest.mark.parametrize("name,K", [("hello", 2), ("five", 2), ("five", 3), ("five", 5), ("five", 63), ("five", 64),
                                    ("five", 65), ("five", 130)])
def test_state_driven_particles_are_the_by_value_particles(name, K, first_sample):
    fit, comp = _fit(name, K, first_sample=first_sample, rng=np.random.default_rng(3))
    eng, gp = comp.e, comp.gp
    for t in range(2):
        before = fit.state()
        assert before.steps == t and before.first_sample == first_sample
        fit.fit(1)
        assert eng.last_call_path().startswith(f"gp_vi_fit n={fit.taxon_count} K={K} G={gp.entry_count} steps=1 | ")
        pid, ent, bl, ll, lqt, lqb, lprior = fit.particles()
        trees, draw, un = comp.particles(F.state_of(before))
        assert pid.tobytes() == trees.parent_ids.tobytes() and ent.tobytes() == trees.entries.tobytes()
        assert lqt.tobytes() == trees.log_q.tobytes()
        assert bl.tobytes() == draw.branch_lengths.tobytes()
        assert lqb.tobytes() == draw.log_q.tobytes() and lprior.tobytes() == draw.log_prior.tobytes()
        _close(ll, eng.log_likelihoods(un.parent_ids, un.branch_lengths, np.tile(comp.model_params, (K, 1))), 1e-12)
    assert first_sample < 2 ** 32 <= first_sample + 2 * K or first_sample == 5
    fit.close()


# ---- 2. one step, teacher-forced ----
@pytest.mark.parametrize("anneal_steps", [0, 4])
@pytest.mark.parametrize("estimator", ["plain", "vimco"])
def test_six_steps_teacher_forced(estimator, anneal_steps):
    fit, comp = _fit("five", 5, estimator, anneal_steps, rng=np.random.default_rng(7))
    betas = []
    for t in range(6):
        before = fit.state()
        row = fit.fit(1)[0]
        _check_step(before, fit.state(), row, comp)
        betas.append(row[0])
    assert betas == ([1.0] * 6 if anneal_steps == 0 else [0.25, 0.5, 0.75, 1.0, 1.0, 1.0])
    after = fit.state()
    assert after.steps == 6 and after.successes == 6 and np.any(after.q_moments != 0.0) and np.any(after.sbn_moments != 0.0)
    R = comp.gp.rootsplit_count
    assert np.all(after.q_moments[:, :R] == 0.0) and np.all(after.q_params[:R] == [0.0, 1.0])   # (carried, never drawn from)
    fit.close()


@pytest.mark.parametrize("name,K", [("hello", 2), ("five", 65)])
def test_steps_teacher_forced_at_the_other_shapes(name, K):
    fit, comp = _fit(name, K, "vimco", 4, rng=np.random.default_rng(8))
    for t in range(2):
        before = fit.state()
        row = fit.fit(1)[0]
        _check_step(before, fit.state(), row, comp)
    fit.close()


# ---- 3. a fit is its steps ----
def test_a_fit_is_its_steps():
    import torch
    name, K = "five", 3
    kw = dict(anneal_steps=5)
    start = _start(_case(name)[1], np.random.default_rng(21))
    whole, _ = _fit(name, K, start=start, **kw)
    trace = whole.fit(7, check_interval=7)
    assert trace.shape == (7, 6) and np.all(trace[:, 5] == 1.0) and np.all(np.isfinite(trace))
    want = whole.state()
    assert want.steps == 7 and want.successes == 7

    single, _ = _fit(name, K, start=start, **kw)
    rows = np.concatenate([single.fit(1) for _ in range(7)])
    assert rows.tobytes() == trace.tobytes() and _same_state(single.state(), want)

    checked, _ = _fit(name, K, start=start, **kw)
    assert checked.fit(7, check_interval=1).tobytes() == trace.tobytes() and _same_state(checked.state(), want)

    split, _ = _fit(name, K, start=start, **kw)
    assert np.concatenate([split.fit(3), split.fit(4, check_interval=2)]).tobytes() == trace.tobytes()
    assert _same_state(split.state(), want)

    replayed, _ = _fit(name, K, start=start, **kw)
    gs = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=gs):
        replayed.step_device(torch.cuda.current_stream().cuda_stream)   # (one stream: the graph is a chain)
    torch.cuda.synchronize()
    assert replayed.state().steps == 0   # (a capture runs nothing)
    graph.replay()   # (the runtime uploads the executable graph at its first launch)
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info(0)[0]
    for _ in range(6):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info(0)[0] == free_before
    replayed.engine.check_status()
    assert _same_state(replayed.state(), want)
    assert replayed.trace().tobytes() == trace.tobytes()
    for a, b in zip(replayed.particles(), whole.particles()):
        assert a.tobytes() == b.tobytes()
    for f in (whole, single, checked, split, replayed):
        f.close()


# ---- 4. checkpoint ----
def test_a_checkpoint_resumes_bit_for_bit():
    start = _start(_case("five")[1], np.random.default_rng(22))
    whole, _ = _fit("five", 4, start=start, anneal_steps=6)
    trace = whole.fit(7)
    first, _ = _fit("five", 4, start=start, anneal_steps=6)
    head = first.fit(3)
    saved = first.state()
    fresh, _ = _fit("five", 4, start=(np.zeros_like(start[0]), np.ones_like(start[1])), anneal_steps=6)
    fresh.set_state(saved)
    assert _same_state(fresh.state(), saved)
    tail = fresh.fit(4)
    assert np.concatenate([head, tail]).tobytes() == trace.tobytes()
    assert _same_state(fresh.state(), whole.state())
    for f in (whole, first, fresh):
        f.close()


# ---- 5. long blocks, a DAG of one tree, a -inf entry ----
def _dag_case(pids, subst="JC69", site="constant", P=9, seed=0):
    import libsbn_amd as L
    n = pids.shape[1] // 2 + 1
    rng = np.random.default_rng(seed)
    if subst == "WAG":
        import aa_utils as A
        tips, w = A.random_aa_alignment(n, P, rng)
    else:
        tips, w = TU.random_alignment(n, P, rng)
    eng = L.Engine(L.PhyloModelSpecification(subst, site, "strict"), np.asarray(tips, np.int32), np.asarray(w, float), device=0)
    params = np.ones(eng.param_count)   # (a Weibull shape of 1 among them)
    return eng, eng.gp_create_dag(pids), GR.build_dag(pids), params


def _two_steps(case, K, rng, **kw):
    fit, comp = _fit(None, K, "vimco", 4, rng=rng, case=case, **kw)
    for t in range(2):
        before = fit.state()
        row = fit.fit(1)[0]
        assert row[5] == 1.0
        _check_step(before, fit.state(), row, comp)
    return fit


def test_a_rootsplit_block_of_more_than_64_entries():
    rng = np.random.default_rng(31)
    pids = np.stack([np.asarray(TU.random_topology(9, rng, rooted=True), np.int32) for _ in range(150)])
    case = _dag_case(pids)
    assert case[2].R > 64 and case[1].rootsplit_count == case[2].R
    fit = _two_steps(case, 8, np.random.default_rng(32))
    assert len({tuple(p) for p in fit.particles()[0]}) > 1
    fit.close()


def test_a_dag_of_one_tree():
    case = _dag_case(np.asarray(TU.balanced_topology(6, rooted=True), np.int32)[None, :])
    fit = _two_steps(case, 3, np.random.default_rng(33))
    pid, _, _, _, lqt, _, _ = fit.particles()
    assert np.all(pid == pid[0]) and np.all(lqt == 0.0)
    assert np.all(fit.state().log_params == _start(case[1], np.random.default_rng(33))[0])   # (its gradient is zero)
    fit.close()


def test_a_block_with_a_minus_inf_entry():
    case = _case("five")
    d = case[2]
    phi, q = _start(case[1], np.random.default_rng(34))
    lo = next(lo for lo, hi in TR.blocks(d) if hi - lo > 1)
    phi[lo] = -np.inf
    fit = _two_steps(case, 6, None, start=(phi, q))
    assert not np.any(fit.particles()[1] == lo)
    st = fit.state()
    assert st.log_params[lo] == -np.inf and np.all(np.isfinite(np.delete(st.log_params, lo)))
    fit.close()


# ---- 6. the score identity over all trees ----
@pytest.mark.parametrize("name", ["five", "nine"])
def test_the_score_has_mean_zero_over_all_trees(name):
    if name == "five":
        _, gp, d, _ = _case("five")
    else:
        _, gp, d, _ = _dag_case(GR.nni_batch(9, 6, 3, np.random.default_rng(41)))
    phi = np.random.default_rng(42).normal(0.0, 1.0, d.G)
    _, q = gp.log_normalize(phi)
    kept = gp.get_sbn_parameters()
    gp.set_sbn_parameters(q)
    trees = gp.enumerate_trees()
    gp.set_sbn_parameters(kept)
    prob = np.exp(trees.log_q)
    assert len(prob) == gp.topology_count() and abs(prob.sum() - 1.0) <= 1e-12
    got, factors = gp.topology_gradient(trees.entries, phi, prob, estimator="given")
    assert factors.tobytes() == prob.tobytes()
    _, scale = GV.topology_gradient(d, q, trees.entries, prob)
    assert np.all(np.abs(got) <= 1e-12 * scale)


# ---- 7. DAG-only objects on other engines ----
@pytest.mark.parametrize("subst,site", [("WAG", "constant"), ("JC69", "weibull+4")])
def test_a_dag_only_object_on_another_engine(subst, site):
    pids = GR.load_case(*FILES["five"])[0]
    case = _dag_case(pids, subst, site, P=17, seed=5)
    _two_steps(case, 2, np.random.default_rng(51)).close()


# ---- 8. what is refused ----
def test_what_is_refused_on_the_host():
    import libsbn_amd as L
    from libsbn_amd import _capi
    lib = _capi.load()
    eng, gp, d, params = _case("five")
    phi, q = _start(gp)
    gp.vi_create(phi, q, model_params=params, particle_count=4, max_steps=2).close()   # (the reservations are made)
    held = lib.mi_device_bytes_held()

    def refused(match, **kw):
        args = dict(log_params=phi, q_params=q, model_params=params, particle_count=4, max_steps=2)
        args.update(kw)
        with pytest.raises(RuntimeError, match=match):
            gp.vi_create(**args)
        assert lib.mi_device_bytes_held() == held

    refused("rows must be 1", rows=3)
    refused("rows must be 1", rows=2)
    refused("VIMCO estimator needs at least 2", particle_count=1)
    for rate in (0.0, -1.0, np.inf, np.nan):
        refused("prior_rate must be finite and positive", prior_rate=rate)
    refused("the tables given", log_params=phi[:-1])
    refused("the tables given", q_params=q[:-1])
    for bad in (np.nan, np.inf):
        broken = phi.copy()
        broken[3] = bad
        refused(r"log_params must be finite or -inf \(entry 3\)", log_params=broken)
    fit = gp.vi_create(phi, q, model_params=params, particle_count=4, max_steps=2)
    assert lib.mi_device_bytes_held() > held
    assert (fit.rows, fit.rootsplit_count, fit.pcsp_count, fit.variable_count, fit.parameter_count) == (1, d.R, 0, d.G, d.G)
    fit.fit(2)
    with pytest.raises(RuntimeError, match="beyond the trace capacity"):
        fit.fit(1)
    with pytest.raises(RuntimeError, match="mi_gp_vi_particles"):
        L.VariationalFit.particles(fit)
    fit.close()
    assert lib.mi_device_bytes_held() == held
    unrooted = eng.vi_create(None, np.zeros(3), np.ones((2, 2)))
    with pytest.raises(RuntimeError, match="not a fit over a subsplit DAG"):
        L.RootedVariationalFit.particles(unrooted)
    unrooted.close()


def test_two_shards_are_refused():
    import torch
    import libsbn_amd as L
    if torch.cuda.device_count() < 1:
        pytest.skip("no device")
    pids, _, tips, w, _ = GR.load_case(*FILES["five"])
    eng = L.Engine(L.PhyloModelSpecification("JC69", "constant", "strict"), tips, w, shard_devices=[0, 0])
    gp = eng.gp_create_dag(pids)
    with pytest.raises(RuntimeError, match="single-device engine"):
        gp.vi_create(particle_count=2)
    gp.close()
    eng.close()


def test_errors_of_the_state_are_reported_at_the_first_check():
    eng, gp, d, params = _case("five")
    phi, q = _start(gp)
    broken = q.copy()
    broken[d.R:, 1] = 0.0
    fit = gp.vi_create(phi, broken, model_params=params, particle_count=3, max_steps=2)
    with pytest.raises(RuntimeError, match=r"sigma must be finite and positive.*\(tree \d+, edge \d+\)"):
        fit.fit(1)
    fit.close()
    empty = phi.copy()
    empty[:d.R] = -np.inf
    fit = gp.vi_create(empty, q, model_params=params, particle_count=3, max_steps=2)
    with pytest.raises(RuntimeError, match=r"all 0 \(sample \d+, the rootsplits\)"):
        fit.fit(1)
    fit.close()
    good = gp.vi_create(phi, q, model_params=params, particle_count=3, max_steps=2)   # (the engine serves on)
    assert np.all(good.fit(2)[:, 5] == 1.0)
    good.close()


def test_a_sentinel_entry_names_its_tree_and_node():
    eng, gp, d, params = _case("five")
    trees = gp.sample_trees(3, 1)
    q = gp.default_q_params()
    for sentinel in (-1, d.G):
        ent = trees.entries.copy()
        ent[1, 2] = sentinel
        with pytest.raises(RuntimeError, match=r"names no entry of the DAG.*\(tree 1, node 2\)"):
            gp.branch_sample(ent, q, 1)
    ent = trees.entries.copy()
    ent[:, -1] = d.G   # (the root's slot has no length: its entry is not read)
    assert gp.branch_sample(ent, q, 1).branch_lengths.tobytes() == gp.branch_sample(trees.entries, q, 1).branch_lengths.tobytes()


# ---- 9. a fit helps ----
def test_a_fit_raises_its_bound():
    eng, gp, d, params = _case("five")
    fit = gp.vi_create(model_params=params, particle_count=16, estimator="vimco", anneal_steps=100, max_steps=300,
                       step_size=(0.01, 0.01), sbn_step_size=0.01, seed=2024)
    trace = fit.fit(300)
    first, last = trace[:30, 2], trace[-30:, 2]
    print("mean bound of the first 30 steps:", first.mean(), "+-", first.std(), "of the last 30:", last.mean(), "+-", last.std())
    assert np.all(trace[:, 5] == 1.0)
    assert last.mean() > first.mean()
    q, b = fit.export()
    lq, want_q = gp.log_normalize(fit.state().log_params)
    _close(q, want_q, 1e-12)
    assert np.all(b > 0.0) and np.all(np.isfinite(b))
    elbo, bound = fit.estimate(64, seed=5)
    assert np.isfinite(elbo) and elbo <= bound
    fit.close()


# ---- 10. the C++ adapter ----
def test_cpp_adapter(tmp_path):
    """tests/cpp/gp_vi_example.cpp: the five-taxon DAG through GeneralizedPruning::ViCreate, Engine::ViFit and
    ViParticles; its printed numbers are the Python calls'."""
    import libsbn_amd as L
    exe = tmp_path / "gp_vi_example"
    lib = os.path.join(REPO, "libsbn_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(REPO, "tests/cpp/gp_vi_example.cpp"), "-L" + lib, "-lmi_phylo",
                    "-lmi_phylo_host", "-Wl,-rpath," + lib, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe), os.path.join(REPO, "tests/golden/data")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = dict(line.split(" ", 1) for line in out.stdout.strip().splitlines())

    def hexes(name):
        return np.array([float.fromhex(x) for x in lines[name].split()])
    pids, _, tips, w, _ = GR.load_case(*FILES["five"])
    eng = L.Engine(L.PhyloModelSpecification("JC69", "constant", "strict"), tips, w, device=0)
    params = np.ones(eng.param_count)
    gp = eng.gp_create(pids, None, params)
    phi, q = hexes("log_params"), hexes("q_params").reshape(-1, 2)
    assert phi.tobytes() == np.log(gp.get_sbn_parameters()).tobytes()
    fit = gp.vi_create(phi, q, model_params=params, particle_count=8, anneal_steps=4, max_steps=8, step_size=(0.01, 0.005),
                       seed=20261021)
    assert fit.fit(5, check_interval=2).tobytes() == hexes("trace").reshape(5, 6).tobytes()
    st = fit.state()
    assert st.log_params.tobytes() == hexes("fitted_log_params").tobytes()
    assert st.q_params.tobytes() == hexes("fitted_q_params").tobytes()
    pid, _, bl, ll, _, _, _ = fit.particles()
    assert pid.tobytes() == np.array(lines["particle_parent_ids"].split(), np.int32).tobytes()
    assert bl.tobytes() == hexes("particle_lengths").tobytes() and ll.tobytes() == hexes("particle_log_likelihoods").tobytes()
    fit.close()
    gp.close()
