"""Bootstrap weights drawn on the device (Engine.bootstrap_weights), the KH / SH / AU tests on
matrices (Engine.topology_tests_matrix), the fused call (Engine.topology_tests), their device
forms and the C++ adapter.

The sampler is integer-exact, so it is compared with tests/topology_tests_ref.py bit for bit.  The
statistics are compared on the GPU's own C_0, L and counts: means bit for bit with a sequential
loop, KH / SH counts as integers, bp / elw with Engine.rell, and the AU fit with 50-digit mpmath to
1e-10 absolute."""
import math
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import rell_ref as RR
import topology_tests_ref as R

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
F0 = 2 ** 32 + 5  # first replicate: the high counter word is not zero


def _engine(monkeypatch=None, hist=None):
    import libsbn_amd as L
    if hist:
        monkeypatch.setenv("MI_PHYLO_BOOT_HIST", hist)
    tips, w, *_ = RR.case("n5", 13, "JC69", 1, 1)
    return L.Engine(L.PhyloModelSpecification("JC69", "constant", "strict"), tips, w, device=0)


@pytest.fixture(scope="module")
def eng():
    """Any engine serves the matrix calls: the alignment plays no part."""
    return _engine()


def _weights(P, seed):
    """Integer weights with zeros; from three patterns on, one of weight 10^6 next to weights of 1."""
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 6, size=P).astype(np.float64)
    w[rng.random(P) < 0.3] = 0.0
    w[0] = 2.0
    if P >= 3:
        w[P // 2 - 1: P // 2 + 2] = [1.0, 1.0e6, 1.0]
    return w


# ---- 1. the sampler, bit for bit ----

@pytest.mark.parametrize("P", [1, 2, 63, 64, 65, 257])
def test_sampler_equals_the_restatement(eng, P):
    w = _weights(P, P)
    for n in (1, 2, 255, 513, 1026):
        ref = R.bootstrap_weights(w, 65, n, seed=77 + P, first_replicate=F0)
        for B in (1, 3, 65):
            got = eng.bootstrap_weights(B, sites=n, seed=77 + P, first_replicate=F0, weights=w)
            assert got.dtype == np.float64 and got.shape == (B, P)
            assert np.array_equal(got, ref[:B]), (P, n, B)
        assert np.all(ref.sum(axis=1) == n) and np.all(ref[:, w == 0] == 0)


def test_sampler_at_the_largest_total_and_default_sites(eng):
    w = np.array([2147483640.0, 7.0])  # N = 2^31 - 1
    for n in (2, 513):
        got = eng.bootstrap_weights(3, sites=n, seed=1, first_replicate=F0, weights=w)
        assert np.array_equal(got, R.bootstrap_weights(w, 3, n, 1, F0))
    # sites defaults to N, weights to the engine's own
    own = eng.bootstrap_weights(5, seed=9)
    N = int(eng._weights.sum())
    assert np.array_equal(own, R.bootstrap_weights(eng._weights, 5, N, 9)) and np.all(own.sum(axis=1) == N)


def test_rows_depend_on_the_replicate_number_only(eng):
    w = _weights(65, 3)
    a = eng.bootstrap_weights(12, sites=300, seed=4, first_replicate=F0, weights=w)
    b = eng.bootstrap_weights(5, sites=300, seed=4, first_replicate=F0 + 7, weights=w)
    assert np.array_equal(b, a[7:])
    assert not np.array_equal(eng.bootstrap_weights(12, sites=300, seed=5, first_replicate=F0, weights=w), a)


def test_both_histogram_forms_give_the_same_bits(monkeypatch):
    """MI_PHYLO_BOOT_HIST=global against lds, an engine under each; and the loops over replicates of
    either form (more replicates than workgroups)."""
    engines = {h: _engine(monkeypatch, h) for h in ("lds", "global")}
    for P, B, n in ((1, 3, 5), (65, 33, 513), (257, 9, 1026)):
        w = _weights(P, 10 + P)
        ref = R.bootstrap_weights(w, B, n, 21, F0)
        for h, e in engines.items():
            assert np.array_equal(e.bootstrap_weights(B, sites=n, seed=21, first_replicate=F0, weights=w), ref), (h, P)
    w = np.array([1.0, 0.0, 3.0, 1.0, 2.0])
    ref = R.bootstrap_weights(w, 2051, 3, 2, 0)
    for h, e in engines.items():
        assert np.array_equal(e.bootstrap_weights(2051, sites=3, seed=2, weights=w), ref), h


@pytest.mark.parametrize("P", [6144, 6145])
def test_sampler_at_and_past_the_lds_row_limit(eng, P):
    """kBootLdsPatterns = 6144: the last row that is kept in LDS, the first that is not."""
    w = _weights(P, 5)
    got = eng.bootstrap_weights(3, sites=513, seed=8, first_replicate=F0, weights=w)
    assert np.array_equal(got, R.bootstrap_weights(w, 3, 513, 8, F0))


# ---- 2. hand-over ----

def test_the_matrix_is_what_rell_and_starting_trees_take(eng):
    rng = np.random.default_rng(2)
    P = eng.pattern_count
    s = rng.uniform(-9.0, -2.0, size=(7, P))
    N = int(eng._weights.sum())
    W = eng.bootstrap_weights(33, seed=6, first_replicate=F0)
    ref = R.bootstrap_weights(eng._weights, 33, N, 6, F0)
    for a, b in zip(eng.rell(s, W), eng.rell(s, ref)):
        assert np.array_equal(a, b)
    row = np.ones(eng.param_count)  # (the strict clock's rate)
    st = eng.starting_trees(replicate_weights=W, params=row)
    assert st.parent_ids.shape == (33, 2 * eng.taxon_count - 3)
    assert np.array_equal(st.parent_ids, eng.starting_trees(replicate_weights=ref, params=row).parent_ids)


# ---- 3. the statistics on the GPU's own matrices ----

def _trees(T, P, seed):
    """Competitive trees: a common row plus noise; the last tree (T >= 3) is worse than tree 0 on every
    pattern by a constant and never wins."""
    rng = np.random.default_rng(seed)
    s = rng.uniform(-9.0, -2.0, size=P)[None, :] + 0.3 * rng.standard_normal((T, P))
    if T >= 3:
        s[T - 1] = s[0] - 0.3
    w = rng.integers(1, 5, size=P).astype(np.float64)
    return s, w


def _check_table(eng, s, w, sites, reps, seed, first, res):
    T, N = s.shape[0], int(w.sum())
    K = len(sites)
    # the blocks' weights by the restatement, the products and their reductions by Engine.rell
    counts, first_k = np.zeros((K, T), np.int64), first
    for k in range(K):
        Wk = R.bootstrap_weights(w, reps[k], sites[k], seed, first_k)
        first_k += reps[k]
        c, best, bp, elw = eng.rell(s, Wk)
        counts[k] = np.bincount(best, minlength=T)
        if k == 0:
            assert np.array_equal(res.replicate_log_likelihood, c) and np.array_equal(res.best_tree, best)
            assert np.array_equal(res.bootstrap_proportion, bp) and np.array_equal(res.expected_likelihood_weight, elw)
    assert res.counts.dtype == np.int32 and np.array_equal(res.counts, counts)
    L = eng.rell(s, w[None, :])[0][0]
    assert np.array_equal(res.log_likelihood, L)
    table, mean, kh, sh = R.table_from(res.replicate_log_likelihood, L, res.counts, sites, reps, N,
                                       elw=res.expected_likelihood_weight)
    assert np.array_equal(res.column_mean, mean)
    B = float(reps[0])
    assert np.array_equal(np.rint(res.p_kh * B), kh) and np.array_equal(np.rint(res.p_sh * B), sh)
    assert np.array_equal(res.p_kh, kh / B) and np.array_equal(res.p_sh, sh / B)
    assert np.array_equal(res.delta, table[:, 1]) and np.array_equal(res.usable_scales, table[:, 10])
    worst = 0.0
    for t in range(T):
        p, d, c, rss, usable = R.au_fit_mp(res.counts[:, t], sites, reps, N)
        assert usable == res.usable_scales[t]
        if usable < 2:
            assert res.p_au[t] == res.bootstrap_proportion[t]
            assert math.isnan(res.au_d[t]) and math.isnan(res.au_c[t]) and math.isnan(res.au_rss[t])
            continue
        err = max(abs(float(p - res.p_au[t])), abs(float(d - res.au_d[t])), abs(float(c - res.au_c[t])),
                  abs(float(rss - res.au_rss[t])))
        worst = max(worst, err)
    return worst, int(np.sum(res.usable_scales >= 2))


@pytest.mark.parametrize("P", [13, 131])
@pytest.mark.parametrize("T", [1, 2, 17, 65])
def test_statistics_on_the_gpus_own_matrices(eng, T, P):
    s, w = _trees(T, P, 100 * T + P)
    N = int(w.sum())
    for K in (1, 3):
        for B in (16, 100):
            sites = [N, N // 2, N + N // 2][:K]
            reps = [B] * K
            res = eng.topology_tests_matrix(s, w, sites, reps, seed=T + P, first_replicate=F0,
                                            replicate_log_likelihoods=True)
            worst, fitted = _check_table(eng, s, w, sites, reps, T + P, F0, res)
            print(f"T={T} P={P} K={K} B={B}: AU against 50 digits {worst:.2e} over {fitted} fitted trees")
            assert worst <= 1e-10
            if T >= 3:  # the tree that never wins: the fewer-than-two-scales rule
                assert np.all(res.counts[:, T - 1] == 0) and res.usable_scales[T - 1] == 0
                assert res.p_au[T - 1] == 0.0 and math.isnan(res.au_d[T - 1])
            if T == 1:
                assert res.p_kh[0] == 1.0 and res.p_sh[0] == 1.0 and res.bootstrap_proportion[0] == 1.0
            if K == 3 and B == 100 and T == 17:
                assert fitted >= 2  # (the fit itself is exercised)


def test_unequal_blocks_continue_the_replicate_numbers(eng):
    s, w = _trees(5, 21, 9)
    N = int(w.sum())
    sites, reps = [N, N - 7, 2 * N + 1], [40, 7, 65]
    res = eng.topology_tests_matrix(s, w, sites, reps, seed=3, first_replicate=F0, replicate_log_likelihoods=True)
    worst, _ = _check_table(eng, s, w, sites, reps, 3, F0, res)
    assert worst <= 1e-10


# ---- 4. ties and position independence ----

def test_equal_rows_and_permutations(eng):
    T, P = 9, 31
    s, w = _trees(T, P, 5)
    s[0] = s.max(axis=0) + 0.01  # the best tree, on every pattern ...
    s[7] = s[0]            # ... and its copies
    s[T - 1] = s[0]
    N = int(w.sum())
    sites, reps = [N, N // 2, 2 * N], [64, 64, 64]
    res = eng.topology_tests_matrix(s, w, sites, reps, seed=2, first_replicate=1)
    for t in (0, 7, T - 1):
        assert res.p_kh[t] == 1.0 and res.p_sh[t] == 1.0 and res.delta[t] == 0.0
        assert res.log_likelihood[t] == res.log_likelihood[0] and res.column_mean[t] == res.column_mean[0]
    assert np.all(res.counts[:, 7] == 0) and np.all(res.counts[:, T - 1] == 0)
    assert res.bootstrap_proportion[7] == 0.0 and res.usable_scales[7] == 0
    # the other trees permuted: their rows move with them, bit for bit (elw: its denominator is a sum over the trees)
    perm = np.array([0, 3, 5, 1, 6, 2, 4, 7, 8])
    res2 = eng.topology_tests_matrix(s[perm], w, sites, reps, seed=2, first_replicate=1)
    assert np.array_equal(res2.counts, res.counts[:, perm])
    assert np.array_equal(res2.column_mean, res.column_mean[perm])
    for j, name in enumerate(R.COLUMNS):
        if name == "elw":
            assert np.all(np.abs(res2.table[:, j] - res.table[perm, j]) <= 1e-12)
        else:
            assert np.array_equal(res2.table[:, j], res.table[perm, j], equal_nan=True), name


# ---- 5. the fused call ----

def test_fused_call_equals_its_two_halves():
    import libsbn_amd as L
    tips, w, pids, bls, _, spec, pr = RR.bootstrap_case(5, 13, 1, 4, 2)
    T, P, N = len(pids), tips.shape[1], int(w.sum())
    eng = L.Engine(L.PhyloModelSpecification("JC69", "constant", "strict"), tips, w, device=0)
    scales = (1.0, 0.5, 1.5)
    r = eng.topology_tests(pids, bls, pr, scales=scales, replicates=64, seed=12, first_replicate=F0,
                           replicate_log_likelihoods=True)
    assert np.array_equal(r.sites, [math.floor(x * N + 0.5) for x in scales]) and np.array_equal(r.replicates, [64] * 3)
    ll, s = eng.pattern_log_likelihoods(pids, bls, pr)
    assert np.array_equal(r.tree_log_likelihood, ll) and np.array_equal(r.pattern_log_likelihood, s)
    m = eng.topology_tests_matrix(s, w, r.sites, r.replicates, seed=12, first_replicate=F0,
                                  replicate_log_likelihoods=True)
    assert np.array_equal(r.table, m.table, equal_nan=True) and np.array_equal(r.counts, m.counts)
    assert np.array_equal(r.column_mean, m.column_mean) and np.array_equal(r.best_tree, m.best_tree)
    assert np.array_equal(r.replicate_log_likelihood, m.replicate_log_likelihood)
    # L is the weighted row sum of s, within the bound of a P-term fused-multiply-add chain
    ref = s.astype(LD) @ w.astype(LD)
    bound = P * 2.0 ** -53 * (np.abs(s) @ np.abs(w))
    assert np.all(np.abs(r.log_likelihood.astype(LD) - ref) <= bound)
    assert np.all(np.abs(r.log_likelihood - ll) <= 1e-10 * np.abs(ll))
    # the default call: ten scales (replicates cut down to keep the test short)
    d = eng.topology_tests(pids, bls, pr, replicates=50, seed=1)
    assert d.counts.shape == (10, T) and d.sites[0] == N and np.all(d.counts.sum(axis=1) == 50)


# ---- 6. the device forms, captured ----

def test_device_forms_replay_from_a_graph_with_the_same_bits():
    import torch
    import libsbn_amd as L
    T, P = 17, 131
    s, w = _trees(T, P, 8)
    N = int(w.sum())
    sites, reps, seed = [N, N // 2, N + N // 2], [100, 64, 100], 31
    eng = _engine()
    ref = eng.topology_tests_matrix(s, w, sites, reps, seed=seed, first_replicate=F0, replicate_log_likelihoods=True)
    ref_w = eng.bootstrap_weights(64, sites=N // 2, seed=seed, first_replicate=F0 + 100, weights=w)
    dev = torch.device("cuda", 0)
    d_s, d_w = torch.from_numpy(s).to(dev), torch.from_numpy(w).to(dev)
    o_table = torch.zeros((T, 11), dtype=torch.float64, device=dev)
    o_counts = torch.zeros((3, T), dtype=torch.int32, device=dev)
    o_mean = torch.zeros(T, dtype=torch.float64, device=dev)
    o_c = torch.zeros((100, T), dtype=torch.float64, device=dev)
    o_best = torch.zeros(100, dtype=torch.int32, device=dev)
    o_w = torch.zeros((64, P), dtype=torch.float64, device=dev)
    outs = [o_table, o_counts, o_mean, o_c, o_best, o_w]
    gs = torch.cuda.Stream()

    def call(stream, engine):
        engine.topology_tests_device(stream, T, P, d_s.data_ptr(), d_w.data_ptr(), sites, reps, seed, F0,
                                     o_table.data_ptr(), o_counts.data_ptr(), out_mean=o_mean.data_ptr(),
                                     out_replicate_ll=o_c.data_ptr(), out_best=o_best.data_ptr())
        engine.bootstrap_weights_device(stream, P, d_w.data_ptr(), 64, N // 2, seed, F0 + 100, o_w.data_ptr())

    def check():
        assert np.array_equal(o_counts.cpu().numpy(), ref.counts), (o_counts.cpu().numpy(), ref.counts)
        assert np.array_equal(o_table.cpu().numpy(), ref.table, equal_nan=True)
        assert np.array_equal(o_counts.cpu().numpy(), ref.counts) and np.array_equal(o_mean.cpu().numpy(), ref.column_mean)
        assert np.array_equal(o_c.cpu().numpy(), ref.replicate_log_likelihood)
        assert np.array_equal(o_best.cpu().numpy(), ref.best_tree) and np.array_equal(o_w.cpu().numpy(), ref_w)

    fresh = _engine()
    fresh.reserve_topology_tests(T, P, 100)
    fresh.reserve_bootstrap_weights(64, P)
    torch.cuda.synchronize()
    lib = L._capi.load()
    held = lib.mi_device_bytes_held()
    with torch.cuda.stream(gs):
        call(gs.cuda_stream, fresh)
    torch.cuda.synchronize()
    check()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=gs):
        call(torch.cuda.current_stream().cuda_stream, fresh)
    for _ in range(2):
        for o in outs:
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        check()
    assert lib.mi_device_bytes_held() == held  # (reserved: neither the calls nor the replays allocated)
    fresh.check_status()
    # what the host form refuses about the weights reaches a device form's caller through the status word
    bad = torch.from_numpy(np.where(np.arange(P) == 4, 1.5, w)).to(dev)
    fresh.bootstrap_weights_device(gs.cuda_stream, P, bad.data_ptr(), 64, N, seed, 0, o_w.data_ptr())
    with pytest.raises(RuntimeError, match=r"integer site counts \(pattern 4\)"):
        fresh.check_status(gs.cuda_stream)
    assert not o_w.cpu().numpy().any()  # (zeros, nothing drawn)
    fresh.topology_tests_device(gs.cuda_stream, T, P, d_s.data_ptr(), d_w.data_ptr(), [N + 1, N], [16, 16], seed, 0,
                                o_table.data_ptr(), o_counts.data_ptr())
    with pytest.raises(RuntimeError, match=r"sites\[0\] must equal"):
        fresh.check_status(gs.cuda_stream)


# ---- 7. refusals ----

def test_sampler_refusals(eng):
    for w, msg in (([1.0, 2.5], "integer site counts"), ([1.0, -2.0], "integer site counts"),
                   ([1.0, float("nan")], "integer site counts"), ([0.0, 0.0], "1 <= N < 2\\^31"),
                   ([2.0 ** 30, 2.0 ** 30], "1 <= N < 2\\^31"), ([3.0e9, 1.0], "1 <= N < 2\\^31"),
                   ([float("inf"), 1.0], "integer site counts")):
        with pytest.raises(RuntimeError, match=msg):
            eng.bootstrap_weights(2, sites=4, weights=np.array(w))
    for n in (0, -3, 2 ** 33 + 1):
        with pytest.raises(RuntimeError, match=r"sites must be in \[1, 2\^33\]"):
            eng.bootstrap_weights(2, sites=n, weights=np.array([1.0, 2.0]))
    with pytest.raises(RuntimeError, match="must be positive"):
        eng.bootstrap_weights(0, sites=4, weights=np.array([1.0, 2.0]))


def test_matrix_call_refusals(eng):
    s, w = _trees(3, 13, 1)
    N = int(w.sum())
    with pytest.raises(RuntimeError, match=r"sites\[0\] must equal"):
        eng.topology_tests_matrix(s, w, [N - 1, N], [8, 8])
    with pytest.raises(RuntimeError, match="pairwise distinct"):
        eng.topology_tests_matrix(s, w, [N, N + 2, N + 2], [8, 8, 8])
    with pytest.raises(RuntimeError, match="at least one replicate"):
        eng.topology_tests_matrix(s, w, [N, N + 2], [8, 0])
    with pytest.raises(RuntimeError, match=r"sites must be in \[1, 2\^33\]"):
        eng.topology_tests_matrix(s, w, [N, 0], [8, 8])
    with pytest.raises(RuntimeError, match="one entry per block"):
        eng.topology_tests_matrix(s, w, [N, N + 1], [8])
    with pytest.raises(RuntimeError, match=r"block_count must be in \[1, 64\]"):
        eng.topology_tests_matrix(s, w, [N + k for k in range(65)], [2] * 65)
    bad = w.copy()
    bad[2] = 0.5
    with pytest.raises(RuntimeError, match="integer site counts"):
        eng.topology_tests_matrix(s, bad, [N], [8])
    with pytest.raises(RuntimeError, match="must share P"):
        eng.topology_tests_matrix(s, w[:-1], [N], [8])


def test_fused_call_refusals():
    import aa_utils as A
    import libsbn_amd as L
    import tree_utils as TU
    tips, w, pids, bls, _, spec, pr = RR.bootstrap_case(5, 13, 1, 4, 2)
    model = L.PhyloModelSpecification("JC69", "constant", "strict")
    kw = dict(scales=(1.0, 0.5), replicates=8)
    sharded = L.Engine(model, tips, w, device=0, shard_devices=[0, 0], shard_mode="trees")
    with pytest.raises(RuntimeError, match="single-device"):
        sharded.topology_tests(pids, bls, pr, **kw)
    by_pattern = L.Engine(model, tips, w, device=0, shard_devices=[0, 0], shard_mode="patterns")
    with pytest.raises(RuntimeError, match="pattern-sharded"):
        by_pattern.topology_tests(pids, bls, pr, **kw)
    # ... while a handle of one shard passes the call through, and the matrix call takes any handle
    one = L.Engine(model, tips, w, device=0, shard_devices=[0], shard_mode="trees")
    plain = L.Engine(model, tips, w, device=0)
    assert np.array_equal(one.topology_tests(pids, bls, pr, **kw).table, plain.topology_tests(pids, bls, pr, **kw).table,
                          equal_nan=True)
    s, wm = _trees(3, 13, 1)
    assert sharded.topology_tests_matrix(s, wm, [int(wm.sum())], [8]).table.shape == (3, 11)
    # scales[0] must be 1 (sites[0] = N)
    with pytest.raises(RuntimeError, match=r"sites\[0\] must equal"):
        plain.topology_tests(pids, bls, pr, scales=(0.5, 1.0), replicates=8)
    # engine weights that are no integer site counts
    frac = w.copy()
    frac[3] += 0.5
    frac[4] += 0.5
    with pytest.raises(RuntimeError, match="integer site counts"):
        L.Engine(model, tips, frac, device=0).topology_tests(pids, bls, pr, **kw)
    rng = np.random.default_rng(1)
    atips, aw = A.random_aa_alignment(6, 20, rng)
    apids, abls = TU.random_trees(6, 2, rng)
    aa = L.Engine(L.PhyloModelSpecification("WAG", "constant", "strict"), atips, aw, device=0)
    with pytest.raises(RuntimeError, match="4-state only"):
        aa.topology_tests(apids, abls, None, **kw)


# ---- 8. the C++ adapter ----

def test_cpp_adapter_gives_the_python_call_bit_for_bit(tmp_path):
    import libsbn_amd as L
    exe = tmp_path / "topology_tests_example"
    lib = os.path.join(REPO, "libsbn_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(REPO, "tests/cpp/topology_tests_example.cpp"),
                    "-L" + lib, "-lmi_phylo", "-lmi_phylo_host", "-Wl,-rpath," + lib, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe), os.path.join(REPO, "tests/golden/data")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    got, shape = {}, None
    for line in out.stdout.splitlines():
        name, *rest = line.split()
        if name == "shape":
            shape = tuple(int(x) for x in rest)
        else:
            got.setdefault(name, []).append(int(rest[1]) if name in ("topo.counts", "topo.sites")
                                            else float.fromhex(rest[1]))
    tips, w, pids, bls = O.struct_arrays(O.load_struct("hello"))
    T, P, B = len(pids), tips.shape[1], 64
    assert shape == (T, P, B)
    eng = L.Engine(L.PhyloModelSpecification("JC69", "weibull+4", "strict"), tips, w, device=0)
    pr = np.zeros((T, eng.param_count))
    pr[:, eng.block_specification()["Weibull shape"][0]] = 0.8
    r = eng.topology_tests(pids, bls, pr, scales=(1.0, 0.5, 1.5), replicates=B, seed=5, first_replicate=3)
    assert np.array_equal(got["boot.w"], eng.bootstrap_weights(4, seed=5, first_replicate=3).reshape(-1))
    assert np.array_equal(got["topo.ll"], r.tree_log_likelihood)
    assert np.array_equal(got["topo.s"], r.pattern_log_likelihood.reshape(-1))
    assert np.array_equal(got["topo.table"], r.table.reshape(-1), equal_nan=True)
    assert np.array_equal(got["topo.mean"], r.column_mean)
    assert np.array_equal(got["topo.counts"], r.counts.reshape(-1)) and np.array_equal(got["topo.sites"], r.sites)
