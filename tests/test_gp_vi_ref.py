"""The reference of the rooted variational fit (tests/gp_vi_ref.py) against itself,
without a device: the bindings exist; the gradient of log q(tau) against central differences of log
q; sum_tau q(tau) grad log q(tau) = 0 over every tree of a DAG; the reparametrisation terms against
central differences of logL + log prior - log q_branch at fixed epsilon, the likelihood through the
CPU oracle and the numpy de-rooting; new_id against its defining property."""
import numpy as np
import pytest

import gp_ref as GR
import gp_trees_ref as TR
import gp_vi_ref as GV
import oracle_lib as O

# Finite-difference bounds: ten times the worst error / max(1, |value|) measured for this reference
# on the CPU: 1.632e-11 for the gradient of log q, 3.255e-9 for the reparametrisation
# terms (hello 2.351e-9, five_taxon 3.255e-9), each rounded up at the third digit before the factor
# ten; both with a step of 1e-5, the second on sums of logL of about -100, whose differences lose
# the digits.
TOL_LOG_Q = 1.64e-10
TOL_TERMS = 3.26e-8
_WORST = {"log_q": 0.0, "terms": 0.0}


def _err(got, want):
    got, want = np.asarray(got, float), np.asarray(want, float)
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))


def _five():
    pids, bls, tips, w, _ = GR.load_case("five_taxon_rooted.nwk", "five_taxon.fasta")
    return pids, bls, tips, w


def test_the_bindings_exist():
    import libsbn_amd as L
    from libsbn_amd import _capi
    for name in ("mi_gp_vi_create", "mi_gp_vi_particles", "mi_gp_reserve_vi", "mi_gp_log_normalize", "mi_gp_branch_sample",
                 "mi_gp_branch_gradient", "mi_gp_topology_gradient", "mi_engine_deroot_trees_mapped"):
        assert name in _capi.SYMBOLS
        assert hasattr(_capi.load(), name)
    for name in ("mi_gp_log_normalize", "mi_gp_branch_sample", "mi_gp_branch_gradient", "mi_gp_topology_gradient",
                 "mi_engine_deroot_trees_mapped"):
        assert name + "_device" in _capi.SYMBOLS
    for method in ("vi_create", "reserve_vi", "log_normalize", "branch_sample", "branch_gradient", "topology_gradient"):
        assert callable(getattr(L.GeneralizedPruning, method))
    assert issubclass(L.RootedVariationalFit, L.VariationalFit)
    assert callable(L.Engine.deroot_trees_mapped)


def test_gradient_of_log_q_against_central_differences():
    pids = _five()[0]
    d = GR.build_dag(pids)
    _, entries = TR.enumerate_numbered(d)
    rng = np.random.default_rng(5)
    phi = rng.normal(0.0, 1.0, d.G)
    _, q = GV.log_normalize(d, phi)
    h = 1e-5
    for ent in entries[:: max(1, len(entries) // 7)]:
        got = GV.grad_log_q(d, q, ent)
        want = np.zeros(d.G)
        for j in range(d.G):
            up, down = phi.copy(), phi.copy()
            up[j] += h
            down[j] -= h
            want[j] = (GV.log_q_topology(GV.log_normalize(d, up)[1], ent) -
                       GV.log_q_topology(GV.log_normalize(d, down)[1], ent)) / (2 * h)
        _WORST["log_q"] = max(_WORST["log_q"], _err(got, want))
    print("worst error of grad log q against central differences:", _WORST["log_q"])
    assert _WORST["log_q"] <= TOL_LOG_Q


def test_the_score_has_mean_zero_over_all_trees():
    pids = _five()[0]
    d = GR.build_dag(pids)
    _, entries = TR.enumerate_numbered(d)
    assert len(entries) == int(round(d.topology_count)) >= 4
    phi = np.random.default_rng(6).normal(0.0, 1.0, d.G)
    phi[next(lo for lo, hi in TR.blocks(d) if hi - lo > 1)] = -np.inf   # (an entry no tree can take)
    _, q = GV.log_normalize(d, phi)
    prob = np.exp([GV.log_q_topology(q, e) for e in entries])
    assert abs(prob.sum() - 1.0) <= 1e-12
    got, scale = GV.topology_gradient(d, q, entries, prob)   # GIVEN factors q(tau)
    assert np.all(np.abs(got) <= 1e-12 * np.maximum(scale, 1e-300))


@pytest.mark.parametrize("case", ["hello", "five_taxon"])
def test_reparametrisation_terms_against_central_differences(case):
    nwk, fasta = {"hello": ("hello_rooted.nwk", "hello.fasta"), "five_taxon": ("five_taxon_rooted.nwk", "five_taxon.fasta")}[case]
    pids, _, tips, w, _ = GR.load_case(nwk, fasta)
    d = GR.build_dag(pids)
    n, N = d.n, 2 * d.n - 1
    entries, _ = TR.index_batch(d, pids)
    T = len(pids)
    rng = np.random.default_rng(9)
    qp = np.stack([rng.normal(-2.5, 0.3, d.G), rng.uniform(0.1, 0.4, d.G)], axis=1)
    eps = rng.normal(0.0, 1.0, (T, N - 1))
    rate = 10.0
    spec = O.make_spec(n, tips.shape[1], "JC69", "constant")
    params = np.ones((T, max(O.param_count(spec), 1)))

    def objective(table):
        """sum_t logL + log prior - log q_branch at the fixed epsilon, and what the terms need"""
        bl, _, lq, lp = GV.branch_sample(entries, table, 0, 0, rate, epsilon=eps)
        un = [GV.deroot_mapped(pids[t], bl[t]) for t in range(T)]
        upid, ubl = np.stack([u[0] for u in un]), np.stack([u[1] for u in un])
        ll = O.unrooted_log_likelihoods(spec, tips, w, upid, ubl, params)
        return float(np.sum(ll + lp - lq)), bl, upid, ubl, np.stack([u[3] for u in un])

    _, bl, upid, ubl, new_id = objective(qp)
    g = O.unrooted_gradients(spec, tips, w, upid, ubl, params)["branch_lengths"]
    c0, c1 = GV.branch_terms(entries, qp, bl, eps, new_id, g, rate)
    got = GV.ordered_sums(entries, d.G, c0, c1)
    assert np.all(got[:d.R] == 0.0)   # (no edge draws from a rootsplit row)
    h = 1e-5
    want = np.zeros((d.G, 2))
    for j in range(d.R, d.G):
        for c in range(2):
            up, down = qp.copy(), qp.copy()
            up[j, c] += h
            down[j, c] -= h
            want[j, c] = (objective(up)[0] - objective(down)[0]) / (2 * h)
    _WORST["terms"] = max(_WORST["terms"], _err(got, want))
    print("worst error of the reparametrisation terms against central differences:", _WORST["terms"])
    assert _err(got, want) <= TOL_TERMS


def test_new_id_satisfies_its_defining_property():
    rng = np.random.default_rng(12)
    pids = list(_five()[0]) + list(GR.nni_batch(9, 6, 3, rng)) + list(GR.load_case("hello_rooted.nwk", "hello.fasta")[0])
    for pid in pids:
        n = len(pid) // 2 + 1
        bl = rng.uniform(0.01, 1.0, 2 * n - 1)
        bl[-1] = 0.0
        out, lengths, edge, new_id = GV.deroot_mapped(pid, bl)
        want_out, want_lengths, want_edge = TR.deroot(pid, bl)
        assert out.tobytes() == want_out.tobytes() and edge == want_edge
        assert new_id[2 * n - 2] == -1 and sorted(new_id[:-1]) == sorted(list(range(2 * n - 3)) + [edge])
        a, b = [v for v in range(2 * n - 2) if pid[v] == 2 * n - 2]
        assert new_id[a] == new_id[b] == edge
        sums = np.zeros(2 * n - 2)
        for v in range(2 * n - 2):
            sums[new_id[v]] += bl[v]
        assert np.array_equal(sums, want_lengths) and np.array_equal(lengths, want_lengths)
