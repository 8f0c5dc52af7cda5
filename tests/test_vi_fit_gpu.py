"""The device-resident variational fit on the GPU against tests/vi_fit_ref.py:
the state-driven draws bit for bit against the by-value calls, every step teacher-forced against
the composition of the host-form calls and the numpy update, a fit against its steps, a graph's
replays and a checkpoint bit for bit, the optimiser call alone, the errors, and the C++ adapter.
Shapes: hello (3 taxa: one topology, every PCSP a PSP), five_taxon, DS1 with its first 20 topologies as
the support."""
import json
import os
import subprocess

import numpy as np
import pytest

import vi_fit_ref as F

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}


def _case(name):
    """(engine, support parent ids, their branch lengths, the model parameter row) of a fixture:
    made once, never changed."""
    import libsbn_amd as L
    if name not in _CACHE:
        with open(os.path.join(REPO, "tests", "golden", {"ds1": "ds1_top100"}.get(name, name) + ".struct.json")) as f:
            st = json.load(f)
        count = 20 if name == "ds1" else len(st["trees"])
        pids = np.array([t["parent_ids"] for t in st["trees"][:count]], np.int32)
        bls = np.array([t["branch_lengths"] for t in st["trees"][:count]], np.float64)
        eng = L.Engine(L.PhyloModelSpecification("JC69", "constant", "strict"), np.array(st["patterns"], np.int32),
                       np.array(st["weights"], np.float64))
        pids.setflags(write=False)
        _CACHE[name] = (eng, pids, bls, np.ones(eng.param_count))
    return _CACHE[name]


def _start(name, rows, rng=None):
    """Initial tables of a fixture: q by mode matching from the support's mean branch lengths,
    log_params zero or, with rng, standard normal."""
    import libsbn_amd as L
    eng, pids, bls, _ = _case(name)
    sup = eng.sbn_index(pids)
    table = eng.psp_table(sup)
    split = eng.split_index(pids, branch_lengths=bls)
    q = L.lognormal_mode_match(split.stats[:, 1] / split.stats[:, 0], table)
    if rows == 1:
        q = q[:table.rootsplit_count].copy()
    phi = np.zeros(sup.parameter_count) if rng is None else rng.normal(0.0, 1.0, sup.parameter_count)
    return phi, q


def _fit(name, K, rows=3, estimator="vimco", anneal_steps=0, seed=11, first_sample=0, rng=None, max_steps=16,
         step_size=(0.01, 0.005), start=None, **kw):
    eng, pids, _, params = _case(name)
    phi, q = _start(name, rows, rng) if start is None else start
    fit = eng.vi_create(pids, phi, q, particle_count=K, rows=rows, estimator=estimator, anneal_steps=anneal_steps,
                        max_steps=max_steps, step_size=step_size, seed=seed, first_sample=first_sample,
                        model_params=params, **kw)
    o = F.Options(K, rows, estimator, anneal_steps, kw.get("prior_rate", 10.0), kw.get("step_decay", 0.99),
                  kw.get("adam_beta0", 0.9), kw.get("adam_beta1", 0.999), kw.get("adam_epsilon", 1e-8), seed)
    return fit, F.Composer(eng, pids, o, params)


def _same_state(a, b):
    for name in ("log_params", "q_params", "sbn_moments", "q_moments", "step_size"):
        if np.asarray(getattr(a, name)).tobytes() != np.asarray(getattr(b, name)).tobytes():
            return False
    return (a.b0, a.b1, a.sbn_step_size, a.steps, a.successes, a.first_sample) == \
        (b.b0, b.b1, b.sbn_step_size, b.steps, b.successes, b.first_sample)


_WORST = {"element": 0.0, "trace": 0.0}


def _close(got, want, tol, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    with np.errstate(invalid="ignore"):   # (inf against inf: equal below)
        err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    err = np.where(same, 0.0, err)
    _WORST[what] = max(_WORST[what], float(np.max(err, initial=0.0)))
    assert np.all(err <= tol), (what, float(np.max(err)))


def _check_step(before, after, row, comp):
    """The fit's state and trace row after a step against the reference's step from `before`."""
    want, want_row = comp.step(F.state_of(before))
    for name in ("log_params", "q_params", "sbn_moments", "q_moments", "step_size"):
        _close(getattr(after, name), getattr(want, name), 1e-12, "element")
    _close([after.b0, after.b1, after.sbn_step_size], [want.b0, want.b1, want.sbn_step_size], 1e-12, "element")
    assert (after.steps, after.successes, after.first_sample) == (want.steps, want.successes, want.first_sample)
    assert row[0] == want_row[0] and row[5] == want_row[5]
    _close(row[1:3], want_row[1:3], 1e-10, "trace")
    _close(row[3:5], want_row[3:5], 1e-12, "element")
    print("largest relative differences so far:", _WORST)


# ---- 1. state-driven draws are the by-value draws ----
@pytest.mark.parametrize("first_sample", [5, 2 ** 32 - 1])
@pytest.mark.parametrize("name,K", [("hello", 2), ("five_taxon", 2), ("five_taxon", 3), ("ds1", 63), ("ds1", 64),
                                    ("ds1", 65), ("ds1", 130)])
def test_state_driven_draws_are_the_by_value_draws(name, K, first_sample):
    fit, comp = _fit(name, K, first_sample=first_sample, rng=np.random.default_rng(3))
    eng = comp.e
    for t in range(2):
        before = fit.state()
        assert before.steps == t and before.first_sample == first_sample
        fit.fit(1)
        assert eng.last_call_path().startswith(f"vi_fit n={fit.taxon_count} K={K} rows=3 steps=1 | ")
        pid, bl, ll, lqt, lqb, lprior = fit.particles()
        base = first_sample + t * K
        want_pid, _, _, _ = eng.sbn_sample(comp.support, comp.descent, before.log_params, K, comp.o.seed, first_sample=base)
        assert pid.tobytes() == want_pid.tobytes()
        _, both, index, draw = comp.particles(F.state_of(before))
        assert bl.tobytes() == draw.branch_lengths.tobytes()
        assert lqb.tobytes() == draw.log_q.tobytes() and lprior.tobytes() == draw.log_prior.tobytes()
        assert lqt.tobytes() == eng.sbn_log_prob(both, before.log_params, trees=slice(len(comp.ids), None))[1].tobytes()
        assert np.all(np.isfinite(ll))
    if name == "hello":
        assert np.all(pid == pid[0])   # (one topology)
    else:
        assert first_sample < 2 ** 32 <= first_sample + 2 * K or first_sample == 5
    fit.close()


# ---- 2. one step, teacher-forced ----
@pytest.mark.parametrize("anneal_steps", [0, 4])
@pytest.mark.parametrize("estimator", ["plain", "vimco"])
@pytest.mark.parametrize("rows", [1, 3])
def test_six_steps_teacher_forced(rows, estimator, anneal_steps):
    fit, comp = _fit("five_taxon", 5, rows, estimator, anneal_steps, rng=np.random.default_rng(7))
    betas = []
    for t in range(6):
        before = fit.state()
        row = fit.fit(1)[0]
        _check_step(before, fit.state(), row, comp)
        betas.append(row[0])
    want = [1.0] * 6 if anneal_steps == 0 else [0.25, 0.5, 0.75, 1.0, 1.0, 1.0]
    assert betas == want
    after = fit.state()
    assert after.steps == 6 and after.successes == 6 and np.any(after.q_moments != 0.0) and np.any(after.sbn_moments != 0.0)
    fit.close()


@pytest.mark.parametrize("name,K", [("hello", 2), ("ds1", 65)])
def test_steps_teacher_forced_at_the_other_shapes(name, K):
    fit, comp = _fit(name, K, 3, "vimco", 4, rng=np.random.default_rng(8))
    for t in range(2):
        before = fit.state()
        row = fit.fit(1)[0]
        _check_step(before, fit.state(), row, comp)
    fit.close()


# ---- 3. a fit is its steps ----
@pytest.mark.parametrize("name,K", [("five_taxon", 3), ("ds1", 64)])
def test_a_fit_is_its_steps(name, K):
    import torch
    kw = dict(anneal_steps=5, rng=None)
    start = _start(name, 3, np.random.default_rng(21))
    whole, _ = _fit(name, K, start=start, **kw)
    trace = whole.fit(7, check_interval=7)
    assert trace.shape == (7, 6) and np.all(trace[:, 5] == 1.0) and np.all(np.isfinite(trace))
    assert whole.engine.last_call_path().startswith(f"vi_fit n={whole.taxon_count} K={K} rows=3 steps=7 | ")
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
    assert replayed.particles()[0].tobytes() == whole.particles()[0].tobytes()
    assert replayed.particles()[1].tobytes() == whole.particles()[1].tobytes()
    for f in (whole, single, checked, split, replayed):
        f.close()


# ---- 4. checkpoint ----
def test_a_checkpoint_resumes_bit_for_bit():
    start = _start("five_taxon", 3, np.random.default_rng(22))
    whole, _ = _fit("five_taxon", 4, start=start, anneal_steps=6)
    trace = whole.fit(7)
    first, _ = _fit("five_taxon", 4, start=start, anneal_steps=6)
    head = first.fit(3)
    saved = first.state()
    fresh, _ = _fit("five_taxon", 4, start=(np.zeros_like(start[0]), np.ones_like(start[1])), anneal_steps=6)
    fresh.set_state(saved)
    assert _same_state(fresh.state(), saved)
    tail = fresh.fit(4)
    assert np.concatenate([head, tail]).tobytes() == trace.tobytes()
    assert _same_state(fresh.state(), whole.state())
    for f in (whole, first, fresh):
        f.close()


# ---- 5. the optimiser call alone ----
def _tables(N):
    """P SBN parameters and V variables with P + 2 V = N."""
    V = N // 3
    return N - 2 * V, V


def _update_case(N, K=5, seed=0):
    P, V = _tables(N)
    rng = np.random.default_rng(100 + N + seed)
    phi = rng.normal(size=P)
    q = np.stack([rng.normal(size=V), rng.uniform(0.05, 1.0, V)], axis=1).reshape(V, 2)
    g_sbn, g_q = rng.normal(size=P) * 10.0, rng.normal(size=(V, 2)) * 10.0
    terms = [rng.normal(-100.0, 5.0, K), rng.normal(0.0, 1.0, K), rng.normal(-5.0, 1.0, K), rng.normal(3.0, 1.0, K)]
    return phi, q, g_sbn, g_q, terms


@pytest.mark.parametrize("N", [1, 255, 256, 257, 100000])
def test_update_alone_is_the_numpy_rule(N):
    eng = _case("five_taxon")[0]
    phi, q, g_sbn, g_q, terms = _update_case(N)
    fit = eng.vi_create(None, phi, q, particle_count=5, step_size=(0.01, 0.003), sbn_step_size=0.002, max_steps=4)
    assert (fit.parameter_count, fit.variable_count) == _tables(N)
    ref = F.State(phi, q, step_size=[0.01, 0.003], sbn_step_size=0.002)
    o = F.Options(5)
    for t in range(3):   # (the third with a gradient of zeros: Adam's moments alone move the tables)
        gs, gq = (g_sbn * (1 - t), g_q * (1 - t))
        row = fit.update(gs, gq, *terms)
        ref, want_row = F.update(ref, o, gs, gq, *terms)
        got = fit.state()
        for name in ("log_params", "q_params", "sbn_moments", "q_moments", "step_size"):
            _close(getattr(got, name), getattr(ref, name), 1e-12, "element")
        _close([got.b0, got.b1], [ref.b0, ref.b1], 1e-12, "element")
        assert (got.steps, got.successes) == (ref.steps, ref.successes) == (t + 1, t + 1)
        assert row[0] == 1.0 and row[5] == 1.0
        _close(row[1:3], want_row[1:3], 1e-10, "trace")
        _close(row[3:5], want_row[3:5], 1e-12, "element")
    with pytest.raises(RuntimeError, match="holds the tables only"):
        fit.fit(1)
    fit.close()


@pytest.mark.parametrize("bad", ["nan_sbn", "nan_q", "inf_sbn", "-inf_q", "sigma_zero", "sigma_negative"])
@pytest.mark.parametrize("N", [1, 255, 256, 257, 100000])
def test_update_alone_failed_steps(N, bad):
    P, V = _tables(N)
    if V == 0 and not bad.endswith("sbn"):
        bad = "nan_sbn" if bad == "nan_q" else "inf_sbn"   # (one element: the SBN table's)
    eng = _case("five_taxon")[0]
    phi, q, g_sbn, g_q, terms = _update_case(N, seed=1)
    o = F.Options(5)
    if bad == "nan_sbn":
        g_sbn[-1] = np.nan
    elif bad == "nan_q":
        g_q[-1, 1] = np.nan
    elif bad == "inf_sbn":
        g_sbn[-1] = np.inf
    elif bad == "-inf_q":
        g_q[-1, 0] = -np.inf
    else:   # the last sigma is what the first step takes to exactly 0, resp. below it
        g_q[-1, 1] = -4.0
        moved, _, _ = F.adam(0.0, 0.0, 0.0, -4.0, 0.003, o.adam_beta0, o.adam_beta1, o)
        q[-1, 1] = -moved if bad == "sigma_zero" else -0.5 * moved
        assert q[-1, 1] > 0.0 and (q[-1, 1] + moved == 0.0 or bad == "sigma_negative")
    fit = eng.vi_create(None, phi, q, particle_count=5, step_size=(0.01, 0.003), sbn_step_size=0.002, max_steps=4)
    before = fit.state()
    row = fit.update(g_sbn, g_q, *terms)
    after = fit.state()
    assert row[5] == 0.0 and row[3:5].tolist() == [0.005, 0.0015]
    for name in ("log_params", "q_params", "sbn_moments", "q_moments"):
        assert getattr(after, name).tobytes() == getattr(before, name).tobytes()
    assert after.step_size.tolist() == [0.005, 0.0015] and after.sbn_step_size == 0.002
    assert (after.steps, after.successes, after.b0, after.b1) == (1, 0, 1.0, 1.0)
    _close(row[1:3], F.trace_sums(*terms), 1e-10, "trace")
    # ... and the fit goes on: the same update with the offending entry mended succeeds
    g_sbn[~np.isfinite(g_sbn)] = 0.0
    g_q[~np.isfinite(g_q)] = 0.0
    if bad.startswith("sigma"):
        g_q[-1, 1] = 4.0
    row = fit.update(g_sbn, g_q, *terms)
    assert row[5] == 1.0 and fit.state().successes == 1
    fit.close()


def test_update_keeps_a_variable_without_gradient_in_place():
    eng = _case("five_taxon")[0]
    phi, q, g_sbn, g_q, terms = _update_case(300)
    g_sbn[7] = 0.0
    g_q[11] = 0.0
    fit = eng.vi_create(None, phi, q, particle_count=5)
    fit.update(g_sbn, g_q, *terms)
    after = fit.state()
    assert after.log_params[7] == phi[7] and after.q_params[11].tobytes() == q[11].tobytes()
    assert np.all(np.delete(after.log_params, 7) != np.delete(phi, 7))
    fit.close()


def test_update_with_gradients_whose_square_overflows():
    """Entries of +-1e300, 1.7e308, around 2^500 (where the root's scaled form takes over) and
    1e-300 among ordinary ones: the device's step is the reference's, the size of a huge entry's
    first step is the step size, its stored second moment +inf, and its later steps are zero."""
    eng = _case("five_taxon")[0]
    phi, q, g_sbn, g_q, terms = _update_case(300)
    q[:, 1] += 1.0   # (room for a sigma to fall by a whole step)
    special = np.array([1e300, -1e300, 1.7e308, -1.7e308, 2.0 ** 500, np.nextafter(2.0 ** 500, np.inf), -2.0 ** 501,
                        2.0 ** 511, 1e-300, -1e-300])
    g_sbn[:10], g_q[:10, 0], g_q[10:20, 1] = special, special, special
    fit = eng.vi_create(None, phi, q, particle_count=5, step_size=(0.01, 0.003), sbn_step_size=0.002, max_steps=4)
    ref = F.State(phi, q, step_size=[0.01, 0.003], sbn_step_size=0.002)
    o = F.Options(5)
    for t in range(2):
        row = fit.update(g_sbn, g_q, *terms)
        ref, _ = F.update(ref, o, g_sbn, g_q, *terms)
        got = fit.state()
        assert row[5] == 1.0
        for name in ("log_params", "q_params", "sbn_moments", "q_moments"):
            _close(getattr(got, name), getattr(ref, name), 1e-12, "element")
        if t == 0:
            moved = got.log_params[:4] - phi[:4]
            assert np.all(np.abs(np.abs(moved) - 0.002) <= 1e-15) and np.all(np.sign(moved) == [1, -1, 1, -1])
            assert np.all(np.isinf(got.sbn_moments[1, :4])) and np.all(np.isfinite(got.sbn_moments[1, 4:]))
            first = got
    assert got.log_params[:4].tobytes() == first.log_params[:4].tobytes()   # (an infinite second moment: no step)
    assert np.all(np.isfinite(got.log_params)) and np.all(np.isfinite(got.q_params))
    fit.close()


def test_update_device_form():
    import torch
    eng = _case("five_taxon")[0]
    phi, q, g_sbn, g_q, terms = _update_case(257)
    a = eng.vi_create(None, phi, q, particle_count=5)
    b = eng.vi_create(None, phi, q, particle_count=5)
    want = a.update(g_sbn, g_q, *terms)
    dev = [torch.tensor(x, device="cuda:0") for x in (g_sbn, g_q, *terms)]
    out = torch.zeros(6, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    b.update_device(None, *[x.data_ptr() for x in dev], out.data_ptr())
    eng.check_status()
    assert out.cpu().numpy().tobytes() == want.tobytes() and _same_state(a.state(), b.state())
    a.close()
    b.close()


# ---- 6. a fit helps ----
def test_a_fit_raises_the_bound():
    """five_taxon, its trees the support, K = 16, q from mode matching, log_params zero, 300 steps,
    VIMCO, annealed over the 300 steps, step sizes 0.01.  The sign alone is asserted.  Seed 1 is the
    first seed tried (on the device).  Seen: mean bound of the first 30 steps -109.173, of the last 30
    -73.522, difference 35.651 against a standard deviation of 8.432 over the last 30."""
    start = _start("five_taxon", 3)
    fit, _ = _fit("five_taxon", 16, estimator="vimco", anneal_steps=300, seed=1, start=start, max_steps=300,
                  step_size=(0.01, 0.01), sbn_step_size=0.01)
    trace = fit.fit(300, check_interval=100)
    first, last = trace[:30, 2], trace[-30:, 2]
    print("mean bound of the first 30 steps", np.mean(first), "of the last 30", np.mean(last), "difference",
          np.mean(last) - np.mean(first), "standard deviation over the last 30", np.std(last), "successes",
          int(np.sum(trace[:, 5])))
    assert np.all(np.isfinite(trace[:, 2]))
    assert np.mean(last) > np.mean(first)
    elbo, estimate = fit.estimate(64, seed=5)
    assert np.isfinite(elbo) and np.isfinite(estimate) and elbo <= estimate
    fit.close()


# ---- 7. twenty states ----
def test_twenty_states_teacher_forced():
    import aa_utils as A
    import libsbn_amd as L
    import splits_ref as SR
    rng = np.random.default_rng(31)
    tips, w = A.random_aa_alignment(5, 17, rng)
    eng = L.Engine(L.PhyloModelSpecification("WAG", "constant", "strict"), tips, w)
    pids, _ = SR.random_batch(5, 4, rng)
    sup = eng.sbn_index(pids)
    table = eng.psp_table(sup)
    V = table.variable_count
    q = np.stack([rng.normal(-2.0, 0.3, V), rng.uniform(0.1, 0.4, V)], axis=1)
    phi = rng.normal(size=sup.parameter_count)
    params = np.ones(eng.param_count)
    fit = eng.vi_create(pids, phi, q, particle_count=2, anneal_steps=3, seed=9, max_steps=4, model_params=params)
    comp = F.Composer(eng, pids, F.Options(2, 3, "vimco", 3, seed=9), params)
    for t in range(2):
        before = fit.state()
        row = fit.fit(1)[0]
        assert eng.last_call_path().startswith("vi_fit n=5 K=2 rows=3 steps=1 | ")
        _check_step(before, fit.state(), row, comp)
    assert fit.state().successes == 2
    fit.close()


# ---- 8. errors ----
def test_what_is_refused_on_the_host():
    import libsbn_amd as L
    eng, pids, _, params = _case("five_taxon")
    phi, q = _start("five_taxon", 3)
    held = L._capi.load().mi_device_bytes_held()
    with pytest.raises(RuntimeError, match="VIMCO estimator needs at least 2"):
        eng.vi_create(pids, phi, q, particle_count=1, estimator="vimco", model_params=params)
    with pytest.raises(RuntimeError, match="rows must be 1"):
        eng.vi_create(pids, phi, q, particle_count=2, rows=2, model_params=params)
    for rate in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(RuntimeError, match="prior_rate must be finite and positive"):
            eng.vi_create(pids, phi, q, particle_count=2, prior_rate=rate, model_params=params)
    with pytest.raises(RuntimeError, match="the tables given"):
        eng.vi_create(pids, phi[:-1], q, particle_count=2, model_params=params)
    st = json.load(open(os.path.join(REPO, "tests", "golden", "five_taxon.struct.json")))
    handle = L.Engine(L.PhyloModelSpecification("JC69", "constant", "strict"), np.array(st["patterns"], np.int32),
                      np.array(st["weights"], np.float64), shard_devices=[0, 0])
    with pytest.raises(RuntimeError, match="single-device engine"):
        handle.vi_create(pids, phi, q, particle_count=2, model_params=params)
    handle.close()
    assert L._capi.load().mi_device_bytes_held() == held
    fit = eng.vi_create(pids, phi, q, particle_count=2, max_steps=3, model_params=params)
    assert L._capi.load().mi_device_bytes_held() > held
    fit.fit(2)
    with pytest.raises(RuntimeError, match="beyond the trace capacity of 3"):
        fit.fit(2)
    assert fit.fit(1).shape == (1, 6) and fit.state().steps == 3
    fit.close()
    assert L._capi.load().mi_device_bytes_held() == held


def test_a_bad_initial_sigma_is_reported_at_the_first_check():
    eng, pids, _, params = _case("five_taxon")
    phi, q = _start("five_taxon", 3)
    bad = q.copy()
    bad[:, 1] = np.where(np.arange(len(q)) < 12, -0.5, 0.0)   # (every rootsplit: whichever tree is drawn has one)
    fit = eng.vi_create(pids, phi, bad, particle_count=2, model_params=params)
    with pytest.raises(RuntimeError, match=r"branch model: an edge's summed sigma .*tree \d+.*"):
        fit.fit(3, check_interval=1)
    assert fit.state().steps == 1   # (the first check point)
    fit.close()
    # the engine stays usable
    good = eng.vi_create(pids, phi, q, particle_count=2, model_params=params)
    assert good.fit(1)[0, 5] == 1.0
    good.close()


# ---- 9. the C++ adapter ----
def test_cpp_adapter(tmp_path):
    """tests/cpp/vi_fit_example.cpp: a fit of five steps on five_taxon through Engine::ViCreate,
    ViFit and ViUpdate; its printed numbers are the Python call's."""
    exe = tmp_path / "vi_fit_example"
    lib = os.path.join(REPO, "libsbn_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(REPO, "tests/cpp/vi_fit_example.cpp"),
                    "-L" + lib, "-lmi_phylo", "-lmi_phylo_host", "-Wl,-rpath," + lib, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe), os.path.join(REPO, "tests/golden/data")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = dict(line.split(" ", 1) for line in out.stdout.strip().splitlines())
    assert lines["status"] == "all checks passed"

    def hexes(name):
        return np.array([float.fromhex(x) for x in lines[name].split()])
    eng = _case("five_taxon")[0]
    pids = np.array([int(x) for x in lines["support"].split()], np.int32).reshape(-1, 7)
    phi, q = hexes("log_params"), hexes("q_params").reshape(-1, 2)
    fit = eng.vi_create(pids, phi, q, particle_count=8, anneal_steps=4, seed=20261021, max_steps=8,
                        step_size=(0.01, 0.005), model_params=np.ones(eng.param_count))
    trace = fit.fit(5)
    assert hexes("trace").tobytes() == trace.tobytes()
    state = fit.state()
    assert hexes("fitted_log_params").tobytes() == state.log_params.tobytes()
    assert hexes("fitted_q_params").tobytes() == state.q_params.tobytes()
    row = fit.update(np.ones(fit.parameter_count), np.ones((fit.variable_count, 2)), *[np.arange(8.0) * s for s in (-1, 0.5, 0.25, 0.125)])
    assert hexes("update_row").tobytes() == row.tobytes()
    fit.close()
