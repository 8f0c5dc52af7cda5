"""The plain-Python restatement of PSP indexing and the log-normal branch-length models
(tests/branch_model_ref.py) pinned to the reference: the doctest's PSP strings, the
PSP counts, the closed-form log density, the gradient against central differences, the moments of
the normal draw, and the C ABI's new symbols.  No device."""
import json
import math
import os

import numpy as np

import branch_model_ref as B
import sbn_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _golden(name):
    with open(os.path.join(GOLDEN, name)) as fh:
        return json.load(fh)


def _pids(name):
    return np.array([t["parent_ids"] for t in _golden(name + ".struct.json")["trees"]], np.int32)


def as_sbn_support(ref):
    """A libsbn_amd.SbnSupport with the reference support's tables (no slots: the strings need
    none): a clade is 2 split + side, side 1 the side with taxon 0."""
    import libsbn_amd as L
    n = ref.n
    number = {s: i for i, s in enumerate(ref.rootsplits)}

    def clade(c):
        return 2 * number[R._minorise(c, n)] + (1 if 0 in c else 0)

    bits = np.array([[sum(1 << (i & 31) for i in s if i >> 5 == w) for w in range((n + 31) // 32)]
                     for s in ref.rootsplits], np.uint32)
    clades = np.array([[clade(c) for c in f] for f in ref.pcsps], np.int32).reshape(-1, 3)
    E = 2 * n - 3
    return L.SbnSupport(n, np.array(ref.pids, np.int32), len(ref.pids), np.zeros((0, E), np.int32),
                        np.zeros((0, 2 * E, 3), np.int32), bits, clades, np.array(ref.parent_range, np.int32),
                        np.array(ref.pcsp_parent, np.int32))


def test_the_doctests_psp_strings():
    import libsbn_amd as L
    ref = R.Support(_pids("five_taxon"))
    table = B.psp_table(ref)
    strings = L.psp_strings(as_sbn_support(ref), L.PspTable(np.array(table[0], np.int32), table[1], table[2]))
    assert strings == B.psp_strings(ref, table)
    assert len(strings) == table[2] + 1 and strings[-1] == "" and "" not in strings[:-1]
    for case in _golden("psp_kats.json")["representations"]:
        rows = B.psp_index(ref, case["parent_ids"], table, 3)
        assert [[strings[j] for j in row] for row in rows] == case["strings"]
        assert B.psp_index(ref, case["parent_ids"], table, 1) == rows[:1]


def test_psp_counts():
    for pids in (_pids("five_taxon"), _pids("ds1_top100")[:20]):
        ref = R.Support(pids)
        _, S, V = B.psp_table(ref)
        pairs = set()
        for pid in pids:
            for _, down, up in B.tree_psps(pid):
                pairs.update(p for p in (down, up) if p is not None)
        assert S == ref.S and V - S == len(pairs)
        # every tree of the support finds all its variables
        table = B.psp_table(ref)
        for pid in pids[:3]:
            rows = B.psp_index(ref, pid, table, 3)
            n = ref.n
            assert all(j < S for j in rows[0]) and all(S <= j < V for j in rows[2])
            assert [j == V for j in rows[1]] == [v < n for v in range(2 * n - 3)]


def test_closed_form_log_prob():
    case = _golden("psp_kats.json")["closed_form_log_prob"]
    mus, sigmas = [p[0] for p in case["params"]], [p[1] for p in case["params"]]
    want = math.fsum(-math.log(x * s * math.sqrt(2.0 * math.pi)) - (math.log(x) - m) ** 2 / (2.0 * s * s)
                     for x, m, s in zip(case["sample"], mus, sigmas))
    got = B.general_log_prob(case["sample"], mus, sigmas)
    assert abs(got - want) <= 1e-12 * abs(want)
    # log_q is the same density written in x = log(value) and eps = (x - mu) / sigma
    xs = [math.log(v) for v in case["sample"]]
    eps = [(x - m) / s for x, m, s in zip(xs, mus, sigmas)]
    assert abs(B.log_q(xs, sigmas, eps) - want) <= 1e-12 * abs(want)


def _objective(index, q, eps, weights, rate, a, b):
    """sum_t w_t (log p_t - log q_t) with eps held fixed and the smooth synthetic log likelihood
    sum_v a_v sin(theta_v) - b_v theta_v^2; returns the value and the likelihood's branch gradient."""
    bl, _, lq, lp = B.sample(index, q, 0, 0, rate, epsilon=eps)
    total, grads = [], []
    for t, theta in enumerate(bl):
        like = math.fsum(a[v] * math.sin(x) - b[v] * x * x for v, x in enumerate(theta[:-1]))
        total.append(weights[t] * (like + lp[t] - lq[t]))
        grads.append([a[v] * math.cos(x) - 2.0 * b[v] * x for v, x in enumerate(theta[:-1])] + [0.0, 0.0])
    return math.fsum(total), bl, grads


def test_gradient_against_central_differences():
    pids = _pids("five_taxon")
    ref = R.Support(pids)
    table = B.psp_table(ref)
    rng = np.random.default_rng(11)
    for rows in (1, 3):
        index = [B.psp_index(ref, pid, table, rows) for pid in pids]
        Vn = table[2] if rows == 3 else table[1]
        if rows == 1:
            assert max(max(r) for t in index for r in t) < Vn
        q = np.stack([rng.normal(-1.0, 0.3, Vn), rng.uniform(0.2, 0.5, Vn)], axis=1)
        T, E = len(index), len(index[0][0])
        eps = rng.normal(0.0, 1.0, (T, E))
        weights = rng.uniform(0.5, 2.0, T)
        a, b = rng.normal(0.0, 2.0, E), rng.uniform(0.0, 1.0, E)
        rate = 10.0
        _, bl, g = _objective(index, q, eps, weights, rate, a, b)
        got, _ = B.gradient(index, q, bl, eps, g, weights, rate)
        h, worst = 1e-6, 0.0
        for j in range(Vn):
            for k in (0, 1):
                up, down = q.copy(), q.copy()
                up[j][k] += h
                down[j][k] -= h
                fd = (_objective(index, up, eps, weights, rate, a, b)[0] -
                      _objective(index, down, eps, weights, rate, a, b)[0]) / (2.0 * h)
                worst = max(worst, abs(fd - got[j][k]) / max(1.0, abs(got[j][k])))
                assert abs(fd - got[j][k]) <= 1e-6 * max(1.0, abs(got[j][k])), (rows, j, k, fd, got[j][k])
        print("rows", rows, "largest relative difference", worst)


def moment_bounds(N):
    return 5.0 / math.sqrt(N), 5.0 * math.sqrt(2.0 / N), 1.95 / math.sqrt(N)


def test_sampler_moments():
    case = _golden("psp_kats.json")["sampler_moments"]
    T, E = case["tree_count"], 2 * case["taxon_count"] - 3
    N = T * E
    assert N == 65535
    draws = [B.normal(case["seed"], t, v) for t in range(T) for v in range(E)]
    mean, var, ks = B.moments_and_ks(draws)
    b_mean, b_var, b_ks = moment_bounds(N)
    print("mean", mean, "variance", var, "KS", ks, "bounds", b_mean, b_var, b_ks)
    assert abs(mean) <= b_mean and abs(var - 1.0) <= b_var and ks <= b_ks
    # the stream is disjoint from the topology sampler's: its counter has a 1 where that one has 0
    import sbn_vi_ref as V
    assert V.philox4x32_10([3, 1, 5, 0], [7, 0]) != V.philox4x32_10([3, 0, 5, 0], [7, 0])


def test_capi_binds_the_new_symbols():
    from libsbn_amd import _capi
    lib = _capi.load()
    for name in ("mi_engine_psp_table", "mi_engine_psp_index", "mi_engine_branch_model_sample",
                 "mi_engine_branch_model_gradient", "mi_engine_reserve_branch_model"):
        assert name in _capi.SYMBOLS and hasattr(lib, name)
        if not name.startswith("mi_engine_reserve"):
            assert name + "_device" in _capi.SYMBOLS and hasattr(lib, name + "_device")


def test_mode_match_is_the_references_heuristic():
    import libsbn_amd as L
    table = L.PspTable(np.array([4, -1, 5], np.int32), 4, 6)
    modes = np.array([0.05, 2.0, 1e-9, 0.3])
    q = L.lognormal_mode_match(modes, table)
    assert q.shape == (6, 2) and np.all(q[4:] == 0.0)
    for j, m in enumerate(modes):
        sigma = -0.1 * math.log(min(max(m, 1e-6), 1 - 1e-6))
        assert abs(q[j][1] - sigma) <= 1e-15 and abs(q[j][0] - (sigma * sigma + math.log(max(m, 1e-6)))) <= 1e-14
