"""PSP indexing and the log-normal branch-length models on the GPU against
tests/branch_model_ref.py: the PSP table and the index rows integer for integer, the draws and the
branch lengths per element, log q and the prior against fsum over the device's own epsilon and
theta, the gradient against the reference over the device's own theta, epsilon and branch gradient,
the errors, one whole variational step from a captured graph, and the C++ adapter.  Taxon counts 3
(no internal edge below the root's children: every down entry is the sentinel), 4, 5, DS1's 27, 65
(127 edges: two rounds of a wave) and 257."""
import json
import os
import subprocess

import numpy as np
import pytest

import branch_model_ref as B
import sbn_ref as R
import splits_ref as SR

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATE = 10.0


def _engine(n=4, patterns=7, **kw):
    """Any engine serves the index and model calls; the gradient tests take one of the trees' n."""
    import libsbn_amd as L
    tips = np.random.default_rng(5).integers(0, 4, size=(n, patterns)).astype(np.int32)
    return L.Engine(L.PhyloModelSpecification("JC69", "constant", "strict"), tips, np.ones(patterns), **kw)


@pytest.fixture(scope="module")
def eng():
    return _engine()


def _golden(name):
    with open(os.path.join(REPO, "tests", "golden", name)) as f:
        return json.load(f)


_CACHE = {}


def _ds1_engine():
    import libsbn_amd as L
    if "ds1_engine" not in _CACHE:
        st = _golden("ds1_top100.struct.json")
        _CACHE["ds1_engine"] = L.Engine(L.PhyloModelSpecification("JC69", "constant", "strict"),
                                        np.array(st["patterns"], np.int32), np.array(st["weights"], np.float64))
    return _CACHE["ds1_engine"]


def _ds1_pids():
    return np.array([t["parent_ids"] for t in _golden("ds1_top100.struct.json")["trees"]], np.int32)


def _case(n):
    """(parent ids [65 or 1000][2n-3], support tree count, the reference support of those first
    trees, its PSP table, the reference's index rows of every tree): computed once, never changed.
    The support is that of the first 7 trees (2 at 257 taxa, where the brute force enumerates 511
    rootings of 511 nodes per tree): the later trees leave it and get the sentinel."""
    if n not in _CACHE:
        T = 1000 if n == 27 else 65
        pids, _ = SR.random_batch(n, T, np.random.default_rng(9000 + n))
        pids.setflags(write=False)
        T0 = 2 if n == 257 else 7
        ref = R.Support(pids[:T0])
        table = B.psp_table(ref)
        _CACHE[n] = (pids, T0, ref, table, [B.psp_index(ref, pid, table, 3) for pid in pids])
    return _CACHE[n]


def _check_table(got, table):
    assert got.psp_of_pcsp.dtype == np.int32 and got.psp_of_pcsp.tolist() == table[0]
    assert (got.rootsplit_count, got.variable_count) == table[1:]


# ---- PSP indexing ----
@pytest.mark.parametrize("n,T", [(n, T) for n in (3, 4, 5, 27, 65, 257) for T in (1, 7, 65)] + [(27, 1000)])
def test_psp_table_and_index_are_the_references(eng, n, T):
    import libsbn_amd as L
    pids, T0, ref, table, want = _case(n)
    T0 = min(T0, T)
    if T0 < len(ref.pids):   # (T = 1: the support of the first tree alone)
        ref = R.Support(pids[:T0])
        table = B.psp_table(ref)
        want = [B.psp_index(ref, pid, table, 3) for pid in pids[:T]]
    sup = eng.sbn_index(pids[:T], support_tree_count=T0)
    got = eng.psp_table(sup)
    _check_table(got, table)
    assert L.psp_strings(sup, got) == B.psp_strings(ref, table)
    for rows in (1, 3):
        index = eng.psp_index(sup, got, rows=rows)
        assert eng.last_call_path() == f"branch_model n={n} rows={rows}"
        assert index.dtype == np.int32 and index.shape == (T, rows, 2 * n - 3)
        assert index.tolist() == [w[:rows] for w in want[:T]]
        assert eng.psp_index(sup, got, rows=rows).tobytes() == index.tobytes()
    V = got.variable_count
    if n == 3:
        assert np.all(index[:, 1] == V)
    if T > T0 and n > 4:
        assert np.any(index[T0:] == V) and np.all(index[:T0, 0] < V) and np.all(index[:T0, 2] < V)
    # a part of the batch, by trees=
    part = eng.psp_index(sup, got, rows=3, trees=slice(T // 2, T))
    assert part.tobytes() == index[T // 2:].tobytes()


def test_ds1_trees_behind_the_support(eng):
    pids = _ds1_pids()
    ref = R.Support(pids[:50])
    table = B.psp_table(ref)
    sup = eng.sbn_index(pids, support_tree_count=50)
    got = eng.psp_table(sup)
    _check_table(got, table)
    index = eng.psp_index(sup, got, rows=3)
    assert index.tolist() == [B.psp_index(ref, pid, table, 3) for pid in pids]
    V = got.variable_count
    assert np.all(index[:50, 0] < V) and np.all(index[:50, 2] < V)
    assert np.any(index[50:, 0] == V) and np.any(index[50:, 2] == V) and np.any(index[50:, 1, 27:] == V)


# ---- the draw, log q and the prior ----
def _q_params(V, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.normal(-2.5, 0.3, V), rng.uniform(0.1, 0.4, V)], axis=1)


def _index(eng, n, T, rows):
    """(parent ids, index [T][rows][2n-3], V) of T trees that are their own support, so that every
    edge has a variable: the device's own rows, which the tests above hold to the reference."""
    pids = _ds1_pids()[:T] if n == "ds1" else _case(n)[0][:T]
    sup = eng.sbn_index(pids)
    table = eng.psp_table(sup)
    return pids, eng.psp_index(sup, table, rows=rows), table.variable_count if rows == 3 else table.rootsplit_count


def _close(got, want, tol):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    worst = float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))
    print("largest difference over max(1, |ref|)", worst, "bound", tol)
    return worst <= tol


def _check_sample(index, q, got, seed, first, epsilon=None):
    want_bl, want_eps, _, _ = B.sample(index.tolist(), q, seed, first, RATE, epsilon=epsilon)
    assert _close(got.epsilon, want_eps, 1e-12)
    assert _close(got.branch_lengths, want_bl, 1e-12)
    assert np.all(got.branch_lengths[:, -1] == 0.0)
    # log q and the prior over the device's own epsilon and theta: x is mu + sigma eps, rounded as the device rounds it
    lq, lp = [], []
    for t, rows in enumerate(index.tolist()):
        params = [B.edge_params(rows, q, v) for v in range(index.shape[2])]
        eps = got.epsilon[t].tolist()
        lq.append(B.log_q([m + s * e for (m, s), e in zip(params, eps)], [s for _, s in params], eps))
        lp.append(B.log_exp_prior(got.branch_lengths[t, :-1].tolist(), RATE))
    assert _close(got.log_q, lq, 1e-10)
    assert _close(got.log_prior, lp, 1e-10)


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("n,T", [(3, 1), (5, 7), (65, 7), (257, 2), (27, 65)])
def test_sample_is_the_references(eng, n, T, rows):
    _, index, V = _index(eng, n, T, rows)
    q = _q_params(V, 100 * n + rows)
    seed, first = 2 ** 63 + 4242 + n, 2 ** 32 - 3   # (a seed with its top bit set, sample numbers across 2^32)
    got = eng.branch_model_sample(index, q, seed, first_sample=first, prior_rate=RATE)
    assert eng.last_call_path() == f"branch_model n={n} rows={rows}"
    _check_sample(index, q, got, seed, first)
    # the same draw handed back
    again = eng.branch_model_sample(index, q, 0, prior_rate=RATE, epsilon=got.epsilon)
    for name in ("branch_lengths", "epsilon", "log_q", "log_prior"):
        assert getattr(again, name).tobytes() == getattr(got, name).tobytes()
    # antithetic draws: the same call with the negated epsilon
    anti = eng.branch_model_sample(index, q, 0, prior_rate=RATE, epsilon=-got.epsilon)
    assert anti.epsilon.tobytes() == (-got.epsilon).tobytes()
    _check_sample(index, q, anti, None, None, epsilon=-got.epsilon)


def test_a_thousand_samples_in_parts(eng):
    pids, index, V = _index(eng, "ds1", 100, 3)
    index = np.ascontiguousarray(np.tile(index, (10, 1, 1)))
    q = _q_params(V, 3)
    seed, first = 99, 10 ** 12
    whole = eng.branch_model_sample(index, q, seed, first_sample=first, prior_rate=RATE)
    _check_sample(index[:130], q, eng.branch_model_sample(index[:130], q, seed, first_sample=first, prior_rate=RATE),
                  seed, first)
    a = eng.branch_model_sample(index[:300], q, seed, first_sample=first, prior_rate=RATE)
    b = eng.branch_model_sample(index[300:], q, seed, first_sample=first + 300, prior_rate=RATE)
    again = eng.branch_model_sample(index, q, seed, first_sample=first, prior_rate=RATE)
    for name in ("branch_lengths", "epsilon", "log_q", "log_prior"):
        assert np.concatenate([getattr(a, name), getattr(b, name)]).tobytes() == getattr(whole, name).tobytes() \
            == getattr(again, name).tobytes()
    # the same trees ten times: ten different draws
    assert not np.array_equal(whole.epsilon[:100], whole.epsilon[100:200])


def test_sampler_moments_on_the_device(eng):
    from test_branch_model_ref import moment_bounds
    case = _golden("psp_kats.json")["sampler_moments"]
    T, E = case["tree_count"], 2 * case["taxon_count"] - 3
    index = np.zeros((T, 1, E), np.int32)
    got = eng.branch_model_sample(index, [[0.0, 1.0]], case["seed"], prior_rate=RATE)
    assert _close(got.branch_lengths[:, :-1], np.exp(got.epsilon), 1e-12)   # (mu 0, sigma 1: x is epsilon itself)
    mean, var, ks = B.moments_and_ks(got.epsilon.ravel())
    b_mean, b_var, b_ks = moment_bounds(T * E)
    print("mean", mean, "variance", var, "KS", ks, "bounds", b_mean, b_var, b_ks)
    assert abs(mean) <= b_mean and abs(var - 1.0) <= b_var and ks <= b_ks
    want = [B.normal(case["seed"], t, v) for t in (0, 640, T - 1) for v in range(E)]
    assert _close(got.epsilon[[0, 640, T - 1]].ravel(), want, 1e-12)


def test_tiny_lengths_stay_finite(eng):
    index = np.zeros((65, 1, 51), np.int32)
    got = eng.branch_model_sample(index, [[-40.0, 3.0]], 7, prior_rate=RATE)
    assert np.all(np.isfinite(got.branch_lengths)) and np.all(got.branch_lengths[:, :-1] > 0.0)
    assert not np.any(np.isnan(got.log_q)) and np.all(np.isfinite(got.log_q)) and np.all(np.isfinite(got.log_prior))
    _check_sample(index[:7], [[-40.0, 3.0]], eng.branch_model_sample(index[:7], [[-40.0, 3.0]], 7, prior_rate=RATE), 7, 0)


# ---- the gradient and log_f ----
def _likelihood(n, pids, bl):
    if n != "ds1" and ("engine", n) not in _CACHE:
        _CACHE[("engine", n)] = _engine(n, 40)
    e = _ds1_engine() if n == "ds1" else _CACHE[("engine", n)]
    out = e.gradients(pids, bl)
    return np.array([g.log_likelihood for g in out]), np.array([g.gradient["branch_lengths"] for g in out])


def _check_gradient(eng, index, q, sample, g, ll, weights, lqt, beta):
    grad, log_f = eng.branch_model_gradient(index, q, sample, g, ll, log_q_topology=lqt, tree_weights=weights,
                                            beta=beta, prior_rate=RATE)
    assert grad.shape == (len(q), 2)
    want, size = B.gradient(index.tolist(), q, sample.branch_lengths, sample.epsilon, g, weights, RATE)
    bound = 1e-10 * np.maximum(1.0, np.array(size))
    print("largest difference over its bound", float(np.max(np.abs(grad - np.array(want)) / bound)))
    assert np.all(np.abs(grad - np.array(want)) <= bound)
    named = np.zeros(len(q), bool)
    named[index[(index >= 0) & (index < len(q))]] = True
    assert np.all(grad[~named] == 0.0) and not np.any(np.signbit(grad[~named]))   # exactly 0 where no entry names the variable
    want_f = B.log_f(ll.tolist(), sample.log_prior.tolist(), None if lqt is None else list(lqt), sample.log_q.tolist(), beta)
    assert _close(log_f, want_f, 1e-12)
    again = eng.branch_model_gradient(index, q, sample, g, ll, log_q_topology=lqt, tree_weights=weights, beta=beta,
                                      prior_rate=RATE)
    assert again[0].tobytes() == grad.tobytes() and again[1].tobytes() == log_f.tobytes()
    return grad


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("n,T", [(5, 7), (65, 7), ("ds1", 100)])
def test_gradient_is_the_references(eng, n, T, rows, weighted):
    pids, index, V = _index(eng, n, T, rows)
    rng = np.random.default_rng(17 + rows)
    q = _q_params(V, 5)
    sample = eng.branch_model_sample(index, q, 31, prior_rate=RATE)
    ll, g = _likelihood(n, pids, sample.branch_lengths)
    weights = rng.uniform(0.2, 3.0, T) if weighted else None
    lqt = rng.normal(-30.0, 2.0, T) if weighted else None
    _check_gradient(eng, index, q, sample, g, ll, weights, lqt, 0.37 if weighted else 1.0)
    assert eng.last_call_path() == f"branch_model n={27 if n == 'ds1' else n} rows={rows}"


def test_gradient_of_one_long_run_and_of_many_empty_variables(eng):
    """Every entry names ONE variable (2667 entries: the wave's path), and V far above the entries."""
    n, T = 65, 7
    pids, index, _ = _index(eng, n, T, 3)
    V, j = 100000, 77777
    index = np.full_like(index, j)
    q = np.zeros((V, 2))
    q[j] = (-1.0, 0.05)   # (three rows: mu -3, sigma 0.15)
    sample = eng.branch_model_sample(index, q, 8, prior_rate=RATE)
    ll, g = _likelihood(n, pids, sample.branch_lengths)
    grad = _check_gradient(eng, index, q, sample, g, ll, None, None, 1.0)
    assert np.count_nonzero(grad) == 2
    # runs of 17 (the shortest the wave takes), 16 (the longest a lane takes) and 18 entries
    runs = np.full((1, 1, 51), 11, np.int32)
    runs[0, 0, :17], runs[0, 0, 17:33] = 5, 9
    q2 = np.tile([[-2.0, 0.3]], (12, 1))
    s2 = eng.branch_model_sample(runs, q2, 8, prior_rate=RATE, epsilon=np.linspace(-2, 2, 51)[None])
    _check_gradient(eng, runs, q2, s2, np.linspace(-50, 50, 53)[None], np.array([-7000.0]), None, None, 1.0)


# ---- errors ----
def test_bad_parameters_name_their_tree_and_edge(eng):
    _, index, V = _index(eng, 5, 7, 3)
    good = _q_params(V, 1)
    sample = eng.branch_model_sample(index, good, 1, prior_rate=RATE)
    g, ll = np.zeros((7, 9)), np.zeros(7)
    j = int(index[4, 2, 3])   # the up PSP of edge 3 of tree 4
    users = [(t, v) for t in range(7) for v in range(7) if j in index[t, :, v]]
    for column, bad in ((1, -1.0), (1, -np.inf), (1, np.inf), (1, np.nan), (0, np.nan)):
        q = good.copy()
        q[j, column] = bad
        for call in (lambda: eng.branch_model_sample(index, q, 1, prior_rate=RATE),
                     lambda: eng.branch_model_gradient(index, q, sample, g, ll, prior_rate=RATE)):
            with pytest.raises(RuntimeError, match=r"sigma must be finite and positive.*\(tree (\d+), edge (\d+)\)") as err:
                call()
            t, v = (int(x) for x in str(err.value).rsplit("(tree ", 1)[1].rstrip(")").split(", edge "))
            assert (t, v) in users
    # sigma = 0: a variable's own, and an edge all of whose rows are the sentinel
    q = good.copy()
    q[:, 1] = 0.0
    with pytest.raises(RuntimeError, match=r"sigma must be finite and positive.*\(tree \d+, edge \d+\)"):
        eng.branch_model_sample(index, q, 1, prior_rate=RATE)
    lone = np.full((1, 1, 7), V, np.int32)
    lone[0, 0, :6] = 0
    with pytest.raises(RuntimeError, match=r"\(tree 0, edge 6\)"):
        eng.branch_model_sample(lone, good, 1, prior_rate=RATE)
    # an index far outside [0, V) names nothing and is never read through
    wild = index.copy()
    wild[0, 1, :] = [-1, -2 ** 31, 2 ** 31 - 1, V, V + 1, 10 ** 9, -7]
    got = eng.branch_model_sample(wild, good, 1, prior_rate=RATE)   # (the status word is clear again)
    assert np.all(np.isfinite(got.branch_lengths))
    # refused on the host
    with pytest.raises(RuntimeError, match="rows must be 1"):
        eng.branch_model_sample(index[:, :2], good, 1, prior_rate=RATE)
    with pytest.raises(RuntimeError, match="rows must be 1"):
        eng.branch_model_gradient(index[:, :2], good, sample, g, ll, prior_rate=RATE)
    with pytest.raises(RuntimeError, match="rows must be 1"):   # (the device forms check before they touch a pointer)
        eng.psp_index_device(None, 7, 5, None, None, 4, 4, None, 6, 2, None)
    with pytest.raises(RuntimeError, match="rows must be 1"):
        eng.reserve_branch_model(7, 5, 2)
    for rate in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(RuntimeError, match="prior_rate must be finite and positive"):
            eng.branch_model_sample(index, good, 1, prior_rate=rate)
    with pytest.raises(RuntimeError, match="tree_count must be positive"):
        eng.branch_model_sample(index[:0], good, 1, prior_rate=RATE)


def test_a_sharded_handle_lets_its_first_shard_work(eng):
    handle = _engine(shard_devices=[0, 0])
    pids, _, _, _, _ = _case(5)
    for e in (handle, _engine(20, 9)):   # (and an engine of another taxon count: the alignment plays no part)
        sup = e.sbn_index(pids[:7])
        table = e.psp_table(sup)
        index = e.psp_index(sup, table)
        assert index.tobytes() == eng.psp_index(eng.sbn_index(pids[:7]), table).tobytes()
        q = _q_params(table.variable_count, 2)
        a, b = e.branch_model_sample(index, q, 5, prior_rate=RATE), eng.branch_model_sample(index, q, 5, prior_rate=RATE)
        assert a.branch_lengths.tobytes() == b.branch_lengths.tobytes() and a.log_q.tobytes() == b.log_q.tobytes()
        g, ll = np.ones((7, 9)), np.full(7, -50.0)
        for x, y in zip(e.branch_model_gradient(index, q, a, g, ll), eng.branch_model_gradient(index, q, b, g, ll)):
            assert x.tobytes() == y.tobytes()
        e.reserve_branch_model(7, 5, 3)
    with pytest.raises(RuntimeError, match="single-device engine"):
        handle.reserve_branch_model(7, 5, 3) or handle.psp_index_device(None, 7, 5, None, None, 4, 4, None, 6, 3, None)


# ---- one whole step from a captured graph ----
def test_a_whole_step_replays_from_one_graph():
    import torch
    import libsbn_amd as L
    n, T0, K = 27, 20, 64
    pids = _ds1_pids()[:T0]
    st = _golden("ds1_top100.struct.json")

    def engine():
        return L.Engine(L.PhyloModelSpecification("JC69", "constant", "strict"), np.array(st["patterns"], np.int32),
                        np.array(st["weights"], np.float64))

    first = engine()
    sup = first.sbn_index(pids)
    S, C, parents, P, E = sup.rootsplit_count, sup.pcsp_count, sup.parent_count, sup.parameter_count, 2 * n - 3
    desc = first.sbn_descent(sup)
    table = first.psp_table(sup)
    V = table.variable_count
    phi = np.random.default_rng(4).normal(0.0, 1.0, P)
    split = first.split_index(pids, branch_lengths=np.array([t["branch_lengths"] for t in st["trees"][:T0]]))
    q = L.lognormal_mode_match(split.stats[:, 1] / split.stats[:, 0], table)
    assert split.split_count == S and q.shape == (V, 2)
    seed, first_sample, beta = 777, 10 ** 6, 0.8
    dev = torch.device("cuda:0")
    i32, f64 = torch.int32, torch.float64
    d_range, d_desc, d_psp = (torch.tensor(np.ascontiguousarray(x), device=dev) for x in (sup.parent_range, desc, table.psp_of_pcsp))
    d_phi, d_q, d_none = torch.tensor(phi, device=dev), torch.tensor(q, device=dev), torch.zeros(1, dtype=f64, device=dev)
    all_pid = torch.zeros((T0 + K, E), dtype=i32, device=dev)
    all_pid[:T0] = torch.tensor(pids, device=dev)

    def zeros(shape, dtype=f64):
        return torch.zeros(shape, dtype=dtype, device=dev)

    o_edge, o_params, o_lp = zeros(K, i32), zeros((K, n - 1), i32), zeros(K)
    o_root, o_slot, o_counts = zeros((T0 + K, E), i32), zeros((T0 + K, 2 * E, 3), i32), zeros(3, i32)
    o_bits, o_clades, o_prange, o_parent = zeros((S, 1), i32), zeros((C, 3), i32), zeros((C, 2), i32), zeros(C, i32)
    o_index, o_bl, o_eps, o_lqb, o_lprior = zeros((K, 3, E), i32), zeros((K, E + 1)), zeros((K, E)), zeros(K), zeros(K)
    o_ll, o_g, o_rooting, o_lqt = zeros(K), zeros((K, E + 2)), zeros((K, E)), zeros(K)
    o_qgrad, o_f, o_grad, o_factors, o_glq = zeros((V, 2)), zeros(K), zeros(P), zeros(K), zeros(K)
    outputs = (all_pid[T0:], o_edge, o_index, o_bl, o_eps, o_lqb, o_lprior, o_ll, o_g, o_lqt, o_qgrad, o_f, o_grad,
               o_factors, o_glq)

    def step(stream, e):
        samples, root, slot = all_pid[T0:].data_ptr(), o_root[T0:].data_ptr(), o_slot[T0:].data_ptr()
        e.sbn_sample_device(stream, K, n, S, C, parents, d_range.data_ptr(), d_desc.data_ptr(), d_phi.data_ptr(),
                            seed, first_sample, samples, o_edge.data_ptr(), o_params.data_ptr(), o_lp.data_ptr())
        e.sbn_index_device(stream, T0 + K, n, all_pid.data_ptr(), T0, S, C, o_root.data_ptr(), o_slot.data_ptr(),
                           o_counts.data_ptr(), o_bits.data_ptr(), o_clades.data_ptr(), o_prange.data_ptr(),
                           o_parent.data_ptr())
        e.psp_index_device(stream, K, n, root, slot, S, C, d_psp.data_ptr(), V, 3, o_index.data_ptr())
        e.branch_model_sample_device(stream, K, n, 3, o_index.data_ptr(), V, d_q.data_ptr(), seed, first_sample, RATE,
                                     o_bl.data_ptr(), o_eps.data_ptr(), o_lqb.data_ptr(), o_lprior.data_ptr())
        e.gradients_device(stream, K, samples, o_bl.data_ptr(), d_none.data_ptr(), o_ll.data_ptr(), o_g.data_ptr())
        e.sbn_log_prob_device(stream, K, n, samples, root, slot, S, C, parents, d_range.data_ptr(), d_phi.data_ptr(),
                              False, o_rooting.data_ptr(), o_lqt.data_ptr())
        e.branch_model_gradient_device(stream, K, n, 3, o_index.data_ptr(), V, d_q.data_ptr(), o_bl.data_ptr(),
                                       o_eps.data_ptr(), o_lqb.data_ptr(), o_lprior.data_ptr(), o_g.data_ptr(),
                                       o_ll.data_ptr(), beta, RATE, o_qgrad.data_ptr(), o_f.data_ptr(),
                                       log_q_topology=o_lqt.data_ptr())
        e.sbn_topology_gradient_device(stream, K, n, samples, root, slot, S, C, parents, d_range.data_ptr(),
                                       d_phi.data_ptr(), False, o_f.data_ptr(), "vimco", o_grad.data_ptr(),
                                       o_factors.data_ptr(), o_glq.data_ptr())

    def snapshot():
        torch.cuda.synchronize()
        return [o.cpu().numpy().tobytes() for o in outputs]

    gs = torch.cuda.Stream()
    step(gs.cuda_stream, first)   # the uncaptured calls (and the kernels' code objects are loaded at their first launch)
    first.check_status(gs.cuda_stream)
    want = snapshot()
    # ... are the host forms'
    s_pid = all_pid[T0:].cpu().numpy()
    both = first.sbn_index(np.concatenate([pids, s_pid]), support_tree_count=T0)
    h_index = first.psp_index(both, table, rows=3, trees=slice(T0, None))
    h_sample = first.branch_model_sample(h_index, q, seed, first_sample=first_sample, prior_rate=RATE)
    assert h_index.tobytes() == o_index.cpu().numpy().tobytes() and np.all(h_index[:, 0] < S) and np.all(h_index[:, 2] < V)
    assert h_sample.branch_lengths.tobytes() == o_bl.cpu().numpy().tobytes()
    assert h_sample.log_q.tobytes() == o_lqb.cpu().numpy().tobytes()
    h_grad, h_f = first.branch_model_gradient(h_index, q, h_sample, o_g.cpu().numpy(), o_ll.cpu().numpy(),
                                              log_q_topology=o_lqt.cpu().numpy(), beta=beta, prior_rate=RATE)
    assert h_grad.tobytes() == o_qgrad.cpu().numpy().tobytes() and h_f.tobytes() == o_f.cpu().numpy().tobytes()
    assert np.all(np.isfinite(h_grad)) and np.all(np.isfinite(o_grad.cpu().numpy())) and np.count_nonzero(h_grad) > 0

    fresh = engine()
    fresh.reserve_sbn(T0 + K, n)
    fresh.reserve(K, True)
    fresh.reserve_branch_model(K, n, 3)
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info(0)[0]
    with torch.cuda.stream(gs):
        step(gs.cuda_stream, fresh)
    assert snapshot() == want
    assert torch.cuda.mem_get_info(0)[0] == free_before   # (reserved: the calls allocated nothing)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=gs):
        step(torch.cuda.current_stream().cuda_stream, fresh)   # (one stream: the graph is a chain)
    for _ in range(2):
        for o in outputs:
            o.zero_()
        graph.replay()
        assert snapshot() == want
    fresh.check_status()


def test_cpp_adapter(tmp_path, eng):
    """tests/cpp/branch_model_example.cpp: 64 sampled trees indexed by PSP, one draw and the gradient
    through Engine::PspTable, PspIndex, BranchModelSample and BranchModelGradient; its printed numbers
    are the Python call's."""
    exe = tmp_path / "branch_model_example"
    lib = os.path.join(REPO, "libsbn_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(REPO, "tests/cpp/branch_model_example.cpp"),
                    "-L" + lib, "-lmi_phylo", "-lmi_phylo_host", "-Wl,-rpath," + lib, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe), os.path.join(REPO, "tests/golden/data")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = dict(line.split(" ", 1) for line in out.stdout.strip().splitlines())
    assert lines["status"] == "all checks passed"
    pids = np.array([int(x) for x in lines["support"].split()], np.int32).reshape(-1, 7)
    theta = np.array([float.fromhex(x) for x in lines["log_params"].split()])
    sup = eng.sbn_index(pids)
    pid, _, _, lp = eng.sbn_sample(sup, eng.sbn_descent(sup), theta, 64, 20261021)
    both = eng.sbn_index(np.concatenate([pids, pid]), support_tree_count=len(pids))
    table = eng.psp_table(both)
    S, V = table.rootsplit_count, table.variable_count
    index = eng.psp_index(both, table, rows=3, trees=slice(len(pids), None))
    assert [int(x) for x in lines["first_index"].split()] == index[0].ravel().tolist()
    j = np.arange(V)
    q = np.stack([np.where(j < S, -2.0 - 0.05 * j, 0.01 * (j % 7)), np.where(j < S, 0.5, 0.02)], axis=1)
    draw = eng.branch_model_sample(index, q, 20261021, first_sample=5)
    k, v = np.arange(64.0)[:, None], np.arange(9.0)[None]
    g = np.where(v < 7, 3.0 - 0.5 * v + 0.01 * k, 0.0)
    grad, log_f = eng.branch_model_gradient(index, q, draw, g, -70.0 - 0.25 * np.arange(64), log_q_topology=lp, beta=0.5)

    def hexes(name):
        return np.array([float.fromhex(x) for x in lines[name].split()])
    assert hexes("log_q").tobytes() == draw.log_q.tobytes()
    assert hexes("first_lengths").tobytes() == draw.branch_lengths[0].tobytes()
    assert hexes("gradient").tobytes() == grad.tobytes()
    assert hexes("log_f").tobytes() == log_f.tobytes()
