"""RELL re-summation (mi_engine_rell, Engine.rell), its reductions, the fused bootstrap call
(Engine.rell_bootstrap), the tree-mixture marginal (Engine.pattern_mixture) and the C++ adapter.

The product C[b][t] = sum_p W[b][p] s[t][p] is checked against numpy long double with the forward
bound of a P-term fused-multiply-add chain, |C - ref| <= P 2^-53 sum_p |W[b][p] s[t][p]|; its
order of summation is part of the interface (equal rows give equal bits, wherever they sit)."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import rell_ref as RR

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


@pytest.fixture(scope="module")
def eng():
    """Any engine serves the matrix calls: the alignment plays no part."""
    import libsbn_amd as L
    tips, w, *_ = RR.case("n5", 13, "JC69", 1, 1)
    return L.Engine(L.PhyloModelSpecification("JC69", "constant", "strict"), tips, w, device=0)


def _matrices(B, T, P, seed):
    """s uniform in [-60, -4]; W integer counts with zeros and one all-zero row."""
    rng = np.random.default_rng(seed)
    s = rng.uniform(-60.0, -4.0, size=(T, P))
    w = rng.integers(0, 6, size=(B, P)).astype(np.float64)
    w[rng.random((B, P)) < 0.3] = 0.0
    w[B // 2] = 0.0
    return s, w


# ---- 1. the product alone ----

@pytest.mark.parametrize("P", [1, 3, 4, 5, 13, 131])
def test_product_within_the_fma_chain_bound(eng, P):
    for B in (1, 15, 16, 17, 33):
        for T in (1, 3, 16, 17, 19):
            s, w = _matrices(B, T, P, 100 * P + 10 * B + T)
            c, best, bp, elw = eng.rell(s, w)
            ref = w.astype(LD) @ s.astype(LD).T
            bound = P * 2.0 ** -53 * (np.abs(w) @ np.abs(s).T)
            err = np.abs(c.astype(LD) - ref)
            assert c.shape == (B, T) and np.all(err <= bound), (B, T, P, float((err - bound).max()))
            assert np.all(c[B // 2] == 0.0)  # the all-zero replicate: zeros, no NaN from any padding


# ---- 2. position independence and ties ----

def test_equal_rows_give_equal_bits_wherever_they_sit(eng):
    B, T = 33, 19
    for P in (5, 13, 131):
        s, w = _matrices(B, T, P, 7 + P)
        w[B // 2] = w[1]  # (no all-zero row here: every replicate has a strict order but the copies)
        s[7] = s[0]
        s[T - 1] = s[0]
        w[B - 1] = w[0]
        c, best, bp, elw = eng.rell(s, w)
        assert np.array_equal(c[:, 7], c[:, 0]) and np.array_equal(c[:, T - 1], c[:, 0])
        assert np.array_equal(c[B - 1], c[0])
        # the same pair of rows alone in a call, and in other places of a larger one
        c11, *_ = eng.rell(s[:1], w[:1])
        assert c11[0, 0] == c[0, 0] == c[B - 1, T - 1] == c[0, 7]
        c12, *_ = eng.rell(s[3:4], w[20:21])
        assert c12[0, 0] == c[20, 3]
        # the tie rule: never a later copy
        assert np.array_equal(best, np.argmax(c, axis=1))
        assert not np.any((best == 7) | (best == T - 1))
        assert bp[7] == 0.0 and bp[T - 1] == 0.0


# ---- 3. the reductions against numpy on the GPU's own C ----

@pytest.mark.parametrize("B,T,P", [(1, 1, 4), (17, 3, 13), (33, 19, 131), (128, 32, 65), (100, 1, 5)])
def test_reductions_match_numpy_on_the_same_matrix(eng, B, T, P):
    s, w = _matrices(B, T, P, B + T + P)
    c, best, bp, elw = eng.rell(s, w)
    rbest, rbp, relw = RR.reductions(c)
    assert np.array_equal(best, rbest)
    assert np.array_equal(bp, rbp)
    print(f"B={B} T={T} P={P}: elw error {float(np.abs(elw - relw).max()):.2e}")
    assert np.all(np.abs(elw - relw) <= 1e-12)
    assert abs(float(np.sum(elw.astype(LD))) - 1.0) <= 1e-12
    # without the [B][T] output: the engine's workspace holds the product
    none, best2, bp2, elw2 = eng.rell(s, w, replicate_log_likelihoods=False)
    assert none is None and np.array_equal(best2, best) and np.array_equal(bp2, bp) and np.array_equal(elw2, elw)


def test_device_entry_equals_host_call(eng):
    import torch
    B, T, P = 33, 19, 131
    s, w = _matrices(B, T, P, 5)
    c, best, bp, elw = eng.rell(s, w)
    dev = torch.device("cuda", 0)
    d_s, d_w = torch.from_numpy(s).to(dev), torch.from_numpy(w).to(dev)
    d_c = torch.empty((B, T), dtype=torch.float64, device=dev)
    d_best = torch.empty(B, dtype=torch.int32, device=dev)
    d_bp, d_elw = (torch.empty(T, dtype=torch.float64, device=dev) for _ in range(2))
    eng.reserve_rell(B, T, P)
    stream = torch.cuda.current_stream().cuda_stream
    for _ in range(2):
        eng.rell_device(stream, B, T, P, d_s.data_ptr(), d_w.data_ptr(), d_bp.data_ptr(),
                        out_replicate_ll=d_c.data_ptr(), out_best=d_best.data_ptr(), out_elw=d_elw.data_ptr())
        eng.check_status(stream)
        assert np.array_equal(d_c.cpu().numpy(), c) and np.array_equal(d_best.cpu().numpy(), best)
        assert np.array_equal(d_bp.cpu().numpy(), bp) and np.array_equal(d_elw.cpu().numpy(), elw)


# ---- 4. end to end against the oracle ----

@pytest.mark.parametrize("n,P,K,B,seed", [(5, 13, 1, 33, 2), (8, 70, 4, 64, 1), (12, 131, 6, 100, 3),
                                          (12, 67, 2, 50, 5)])
def test_bootstrap_matches_oracle(n, P, K, B, seed):
    import libsbn_amd as L
    tips, w, pids, bls, W, spec, pr = RR.bootstrap_case(n, P, K, B, seed)
    T = len(pids)
    s_ref = RR.pattern_log_likelihoods(spec, tips, pids, bls, pr)
    c_ref, best_ref, bp_ref, elw_ref = RR.rell(s_ref, W)
    gap = RR.top_two_gap(c_ref)
    print(f"n={n} P={P} K={K} B={B}: T={T}, smallest top-two gap {gap.min():.2e}, "
          f"trees with support {int((bp_ref > 0).sum())}")
    assert np.all(gap > 1e-8)  # a condition on the inputs: every replicate's order is decided
    eng = L.Engine(L.PhyloModelSpecification("JC69", RR.site(K), "strict"), tips, w, device=0)
    r = eng.rell_bootstrap(pids, bls, W, pr)
    assert " pattern_ll" in eng.last_call_path() and eng.last_call_info()[1] == T
    assert np.array_equal(r.log_likelihood, eng.log_likelihoods(pids, bls, pr))
    assert np.all(np.abs(r.pattern_log_likelihood - s_ref) <= 1e-10 * np.abs(s_ref))
    assert np.array_equal(r.best_tree, best_ref)
    assert np.array_equal(r.bootstrap_proportion, bp_ref)
    c_err = np.abs(r.replicate_log_likelihood.astype(LD) - c_ref)
    assert np.all(c_err <= 1e-10 * np.abs(c_ref)), float((c_err / np.abs(c_ref)).max())
    assert np.all(np.abs(r.expected_likelihood_weight - elw_ref) <= 1e-8)
    # the two calls it is made of give the same bits
    ll, s = eng.pattern_log_likelihoods(pids, bls, pr)
    c, best, bp, elw = eng.rell(s, W)
    assert np.array_equal(s, r.pattern_log_likelihood) and np.array_equal(c, r.replicate_log_likelihood)
    assert np.array_equal(best, r.best_tree) and np.array_equal(elw, r.expected_likelihood_weight)


def test_bootstrap_refuses_a_sharded_handle():
    import libsbn_amd as L
    tips, w, pids, bls, W, spec, pr = RR.bootstrap_case(5, 13, 1, 4, 2)
    sharded = L.Engine(L.PhyloModelSpecification("JC69", "constant", "strict"), tips, w, device=0,
                       shard_devices=[0, 0], shard_mode="trees")
    with pytest.raises(RuntimeError, match="single-device"):
        sharded.rell_bootstrap(pids, bls, W, pr)
    # ... while the matrix calls let its first shard do the work
    s, wm = _matrices(5, 3, 13, 1)
    assert sharded.rell(s, wm)[0].shape == (5, 3)


# ---- 5. the mixture marginal ----

@pytest.mark.parametrize("T,P", [(1, 13), (3, 65), (32, 131), (19, 300)])
def test_mixture_matches_long_double_logsumexp(eng, T, P):
    rng = np.random.default_rng(T + P)
    s = rng.uniform(-60.0, -4.0, size=(T, P))
    pw = rng.integers(0, 6, size=P).astype(np.float64)
    lw = np.log(rng.dirichlet(np.ones(T)))
    for weights in (lw, None):
        per, total = eng.pattern_mixture(s, pw, weights)
        rper, rtotal = RR.mixture(s, pw, weights)
        assert np.all(np.abs(per.astype(LD) - rper) <= 1e-13 * np.abs(rper))
        gpu_sum = (pw.astype(LD) * per.astype(LD)).sum()  # the scalar against the GPU's own per-pattern values
        assert abs(LD(total) - gpu_sum) <= P * 2.0 ** -52 * abs(gpu_sum)
        assert abs(LD(total) - rtotal) <= (P * 2.0 ** -52 + 1e-13) * abs(rtotal)


def test_mixture_of_copies_is_the_tree():
    import libsbn_amd as L
    tips, w, pids, bls, spec, pr = RR.case("random12", 131, "GTR", 4, 31)
    eng = L.Engine(L.PhyloModelSpecification("GTR", "weibull+4", "strict"), tips, w, device=0)
    T = 5
    ll, s = eng.pattern_log_likelihoods(np.stack([pids[0]] * T), np.stack([bls[0]] * T), np.stack([pr[0]] * T))
    assert np.all(s == s[0]) and np.all(ll == ll[0])
    per, total = eng.pattern_mixture(s, w)
    assert np.all(np.abs(per - s[0]) <= 2 * np.spacing(np.abs(s[0])))
    assert abs(total - ll[0]) <= 131 * 2.0 ** -52 * abs(ll[0])


# ---- 6. the C++ adapter ----

def test_cpp_adapter_gives_the_python_call_bit_for_bit(tmp_path):
    import libsbn_amd as L
    exe = tmp_path / "rell_example"
    lib = os.path.join(REPO, "libsbn_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(REPO, "tests/cpp/rell_example.cpp"),
                    "-L" + lib, "-lmi_phylo", "-lmi_phylo_host", "-Wl,-rpath," + lib, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe), os.path.join(REPO, "tests/golden/data")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    got, shape = {}, None
    for line in out.stdout.splitlines():
        name, *rest = line.split()
        if name == "shape":
            shape = tuple(int(x) for x in rest)
        else:
            got.setdefault(name, []).append(int(rest[1]) if name == "rell.best" else float.fromhex(rest[1]))
    tips, w, pids, bls = O.struct_arrays(O.load_struct("hello"))
    T, P, B = len(pids), tips.shape[1], 9
    assert shape == (T, P, B)
    eng = L.Engine(L.PhyloModelSpecification("JC69", "weibull+4", "strict"), tips, w, device=0)
    pr = np.zeros((T, eng.param_count))
    pr[:, eng.block_specification()["Weibull shape"][0]] = 0.8
    W = np.array([[(7 * b + 3 * p) % 5 for p in range(P)] for b in range(B)], dtype=np.float64)
    ll, s = eng.pattern_log_likelihoods(pids, bls, pr)
    r = eng.rell_bootstrap(pids, bls, W, pr)
    assert np.array_equal(got["pattern_ll.ll"], ll) and np.array_equal(got["pattern_ll.s"], s.reshape(-1))
    assert np.array_equal(got["rell.ll"], r.log_likelihood)
    assert np.array_equal(got["rell.s"], r.pattern_log_likelihood.reshape(-1))
    assert np.array_equal(got["rell.c"], r.replicate_log_likelihood.reshape(-1))
    assert np.array_equal(got["rell.best"], r.best_tree)
    assert np.array_equal(got["rell.bp"], r.bootstrap_proportion)
    assert np.array_equal(got["rell.elw"], r.expected_likelihood_weight)
