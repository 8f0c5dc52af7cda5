"""Sampling from an SBN and the topology gradient on the GPU against
tests/sbn_vi_ref.py: the descent table byte for byte, the CDF, the sampler bit for bit (the
reference sampler reads the device's own CDF, so no exp has to match between host and device), its
consistency with the index and log_prob calls, the frequencies of 65 536 draws, the gradient's
known answers (the reference's doctest) and the brute force, the errors, the device forms from one
captured graph and the C++ adapter.  Taxon counts as tests/test_sbn_gpu.py: 3, 4, 5, the word
boundaries 32 | 33 and 64 | 65, DS1's 27, and 257 (node arrays in memory instead of LDS)."""
import dataclasses
import json
import math
import os
import subprocess

import numpy as np
import pytest

import sbn_ref as R
import sbn_vi_ref as V
import splits_ref as SR

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG_INF = float("-inf")


def _engine(**kw):
    """Any engine serves: the SBN calls take their taxon count as an argument."""
    import libsbn_amd as L
    tips = np.random.default_rng(5).integers(0, 4, size=(4, 7)).astype(np.int32)
    return L.Engine(L.PhyloModelSpecification("JC69", "constant", "strict"), tips, np.ones(7), **kw)


@pytest.fixture(scope="module")
def eng():
    return _engine()


def _golden(name):
    with open(os.path.join(REPO, "tests", "golden", name)) as f:
        return json.load(f)


_CACHE = {}


def _batch(n, T):
    """(parent ids, the reference's support, its descent table): computed once, never changed.
    Random trees and, from 7 trees on, the caterpillar and a balanced tree (tests/test_sbn_gpu.py)."""
    key = ("batch", n, T)
    if key not in _CACHE:
        pids, _ = SR.random_batch(n, T, np.random.default_rng(7000 * n + T))
        if T >= 7:
            pids[2], pids[3] = R.caterpillar(n), R.balanced(n)
        pids.setflags(write=False)
        ref = R.Support(pids)
        _CACHE[key] = (pids, ref, V.descent_table(ref))
    return _CACHE[key]


def _ds1(T0=None):
    key = ("ds1", T0)
    if key not in _CACHE:
        pids = np.array([t["parent_ids"] for t in _golden("ds1_top100.struct.json")["trees"]], np.int32)
        ref = R.Support(pids, support_tree_count=T0)
        _CACHE[key] = (pids, ref, V.descent_table(ref))
    return _CACHE[key]


def _five():
    if "five" not in _CACHE:
        pids = np.array([t["parent_ids"] for t in _golden("five_taxon.struct.json")["trees"]], np.int32)
        ref = R.Support(pids)
        _CACHE["five"] = (pids, ref, V.descent_table(ref))
    return _CACHE["five"]


SHAPES = [(n, 7) for n in (3, 4, 5, 27, 32, 33, 64, 65)] + [(257, 2)]


def _random_params(ref, seed, holes=True):
    """Unnormalised parameters; with holes, some -inf entries, never a block's first (every block
    keeps a finite entry: no sample can reach an empty one)."""
    rng = np.random.default_rng(seed)
    phi = rng.normal(0.0, 2.0, ref.P)
    if holes:
        firsts = {b for b, _ in ref.blocks()}
        for j in rng.choice(ref.P, max(1, ref.P // 10), replace=False):
            if int(j) not in firsts:
                phi[j] = NEG_INF
    return phi


# ---- the descent table ----
@pytest.mark.parametrize("n,T", SHAPES)
def test_descent_is_the_references(eng, n, T):
    pids, ref, table = _batch(n, T)
    got = eng.sbn_descent(eng.sbn_index(pids))
    assert eng.last_call_path() == f"sbn n={n} store={'lds' if n <= 214 else 'global'}"
    assert got.dtype == np.int32 and got.tobytes() == np.array(table, np.int32).tobytes()


def test_descent_of_ds1_and_of_a_part_of_it(eng):
    for T0 in (None, 50):
        pids, ref, table = _ds1(T0)
        sup = eng.sbn_index(pids, support_tree_count=T0)
        assert eng.sbn_descent(sup).tobytes() == np.array(table, np.int32).tobytes()


def test_descent_refuses_a_sentinel_in_a_support_tree(eng):
    pids, ref, _ = _ds1(50)
    sup = eng.sbn_index(pids, support_tree_count=50)
    outside = [t for t in range(100) if any(ref.P in r for r in ref.reps[t])]
    with pytest.raises(RuntimeError, match=r"SBN descent: a support tree.*outside the support \(tree (\d+)\)") as err:
        eng.sbn_descent(dataclasses.replace(sup, support_tree_count=100))
    assert int(str(err.value).rsplit("tree ", 1)[1].rstrip(")")) in outside
    eng.sbn_descent(sup)  # (the status word is clear again)


# ---- the CDF and the sampler ----
def _check_cdf(cdf, phi, ref):
    want = V.cdf([float(x) for x in phi], ref.blocks())
    for b, e in ref.blocks():
        assert e - b <= 1000
        assert np.all(np.diff(cdf[b:e]) >= 0.0)                 # non-decreasing, exactly
        for j in range(b, e):
            if phi[j] == NEG_INF:
                assert cdf[j] == (cdf[j - 1] if j > b else 0.0)  # repeats the predecessor
            assert abs(cdf[j] - want[j]) <= 1e-12 * want[j]


def _reference_samples(ref, table, cdf, seed, first_sample, K):
    """The reference sampler over the device's CDF: [(parent ids, root edge, sampled parameters)]."""
    return [V.sample(ref.n, ref.S, ref.parent_range, table, cdf, seed, first_sample + k) for k in range(K)]


def _check_samples(got, want):
    """Equality of every integer output of EVERY sample."""
    pid, edge, params = got[:3]
    assert pid.shape[0] == len(want)
    assert pid.tolist() == [w[0] for w in want]
    assert edge.tolist() == [w[1] for w in want]
    assert params.tolist() == [w[2] for w in want]


def _params(eng, sup, ref, which, seed):
    """The three parameter sets: SA-trained, random unnormalised, random with -inf entries."""
    if which == "sa":
        return eng.sbn_train(sup, "sa")[0]
    return _random_params(ref, seed, holes=which == "holes")


# K = 1000 at every taxon count but 257, where the reference sampler (a Python recursion over 256
# draws and a renumbering of 511 nodes per sample) allows 130 in the time a test may take: 130
# samples are still nine waves at 16 samples per wave, the last of them partly filled, which is all
# the global store adds to the LDS form (a wave's arrays lie at its block's offset).
@pytest.mark.parametrize("which", ["sa", "random", "holes"])
@pytest.mark.parametrize("n,T", SHAPES)
def test_sampler_is_the_references(eng, n, T, which):
    pids, ref, table = _batch(n, T)
    sup = eng.sbn_index(pids)
    desc = eng.sbn_descent(sup)
    phi = _params(eng, sup, ref, which, 31 * n)
    seed, most = 1000 + n, 1000 if n <= 65 else 130
    whole = eng.sbn_sample(sup, desc, phi, most, seed, cdf=True)
    assert eng.last_call_path() == f"sbn n={n} store={'lds' if n <= 214 else 'global'}"
    _check_cdf(whole[4], phi, ref)
    want = _reference_samples(ref, table, whole[4], seed, 0, most)
    _check_samples(whole, want)
    # K = 1, 7 and 65 against the reference, from the start and from inside the batch: a sample
    # depends on (seed, first_sample + k) alone
    for K, first in ((1, 0), (1, 40), (7, 0), (7, 58), (65, 0), (65, most - 65)):
        part = eng.sbn_sample(sup, desc, phi, K, seed, first_sample=first, cdf=True)
        assert part[4].tobytes() == whole[4].tobytes()
        _check_samples(part, want[first:first + K])
        assert part[3].tobytes() == whole[3][first:first + K].tobytes()
    # the log probability is that of the sampled parameters
    lp = [V.log_prob_of_sample(list(phi), ref.blocks(), w[2]) for w in want[:65]]
    assert np.all(np.abs(whole[3][:65] - lp) <= 1e-10 * np.maximum(1.0, np.abs(lp)))


@pytest.mark.parametrize("which", ["sa", "random", "holes"])
def test_sampler_on_ds1_in_a_thousand(eng, which):
    pids, ref, table = _ds1()
    sup = eng.sbn_index(pids)
    desc = eng.sbn_descent(sup)
    phi = _params(eng, sup, ref, which, 77)
    seed, first = 2 ** 63 + 12345, 2 ** 32 - 300   # (a seed with its top bit set, sample numbers across 2^32)
    whole = eng.sbn_sample(sup, desc, phi, 1000, seed, first_sample=first, cdf=True)
    _check_cdf(whole[4], phi, ref)
    _check_samples(whole, _reference_samples(ref, table, whole[4], seed, first, 1000))
    # 1000 = 300 + 700, and run to run
    a = eng.sbn_sample(sup, desc, phi, 300, seed, first_sample=first)
    b = eng.sbn_sample(sup, desc, phi, 700, seed, first_sample=2 ** 32)
    again = eng.sbn_sample(sup, desc, phi, 1000, seed, first_sample=first, cdf=True)
    for x, y, w, z in zip(a, b, whole, again):
        assert np.concatenate([x, y]).tobytes() == w.tobytes() == z.tobytes()


def test_sampler_bits_do_not_depend_on_trees_per_wave(monkeypatch):
    runs = []
    for n, T, K in ((65, 7, 70), (27, 7, 200)):   # (65 taxa: in LDS at 16 and 32 per wave, in memory at 64)
        pids, ref, table = _batch(n, T)
        phi = _random_params(ref, 5 * n)
        per = []
        for tpw in ("16", "32", "64"):
            monkeypatch.setenv("MI_PHYLO_SBN_TREES_PER_WAVE", tpw)
            e = _engine()
            sup = e.sbn_index(pids)
            desc = e.sbn_descent(sup)
            assert desc.tobytes() == np.array(table, np.int32).tobytes()
            per.append(e.sbn_sample(sup, desc, phi, K, 99, cdf=True))
            runs.append(e.last_call_path())
        for other in per[1:]:
            for a, b in zip(per[0], other):
                assert a.tobytes() == b.tobytes()
    assert runs[:3] == ["sbn n=65 store=lds", "sbn n=65 store=lds", "sbn n=65 store=global"]


@pytest.mark.parametrize("n,T", [(5, 7), (27, 7), (65, 7), (257, 2)])
def test_samples_are_consistent_with_index_and_log_prob(eng, n, T):
    import libsbn_amd as L
    pids, ref, _ = _batch(n, T)
    sup = eng.sbn_index(pids)
    desc = eng.sbn_descent(sup)
    phi = _random_params(ref, 13 * n)
    K = 33 if n <= 65 else 4
    pid, edge, params, lp = eng.sbn_sample(sup, desc, phi, K, 4242)
    assert eng.split_index(pid).split_index.shape == (K, 2 * n - 1)       # every sample is a tree the split table takes
    both = eng.sbn_index(np.concatenate([pids, pid]), support_tree_count=T)
    assert both.parameter_count == ref.P
    rooting, _ = eng.sbn_log_prob(both, phi, trees=slice(T, T + K))
    for k in range(K):
        assert np.all(both.root_index[T + k] < ref.S) and np.all(both.slot_index[T + k] < ref.P)  # inside the support
        rep = L.sbn_rooted_representations(both, T + k)[int(edge[k])]
        assert rep[0] == params[k][0] and sorted(rep) == sorted(params[k].tolist())
        want = rooting[k][int(edge[k])]
        assert abs(lp[k] - want) <= 1e-10 * max(1.0, abs(want))


def test_sample_frequencies_follow_q(eng):
    pids, ref, _ = _five()
    sup = eng.sbn_index(pids)
    desc = eng.sbn_descent(sup)
    theta, _ = eng.sbn_train(sup, "sa")
    K = 65536
    pid, edge, params, lp = eng.sbn_sample(sup, desc, theta, K, 20261020, first_sample=0)
    vectors, counts = np.unique(pid, axis=0, return_counts=True)
    both = eng.sbn_index(np.concatenate([pids, vectors]), support_tree_count=len(pids))
    _, lq = eng.sbn_log_prob(both, theta, trees=slice(len(pids), None), normalized=True)
    share = {}
    for v in range(len(vectors)):   # (an unrooted topology is its set of splits)
        entry = share.setdefault(frozenset(both.root_index[len(pids) + v].tolist()), [0, lq[v]])
        entry[0] += int(counts[v])
        assert entry[1] == lq[v]
    worst = max(abs(c / K - math.exp(q)) for c, q in share.values())
    print("topologies", len(share), "parent vectors", len(vectors), "largest deviation", worst)
    assert worst < 5 * 0.5 / math.sqrt(K)
    assert abs(sum(math.exp(q) for _, q in share.values()) - 1.0) < 1e-9


# ---- the gradient ----
def _kat_support(eng):
    k = _golden("sbn_vi_kats.json")
    trees = k["gradient_test"]["support_parent_ids"]
    both = eng.sbn_index(np.array(trees + [k["uniform"]["tau_parent_ids"]], np.int32), support_tree_count=2)
    assert (both.rootsplit_count, both.pcsp_count) == (k["gradient_test"]["rootsplit_count"], k["gradient_test"]["pcsp_count"])
    return k, both


def test_gradient_known_answers(eng):
    import libsbn_amd as L
    k, both = _kat_support(eng)
    S, P = both.rootsplit_count, both.parameter_count
    u = k["uniform"]
    grad, factors, lq = eng.sbn_topology_gradient(both, np.zeros(P), [1.0], "given", trees=[2])
    assert factors.tolist() == [1.0] and abs(math.exp(lq[0]) - u["q"]) < u["tolerance"]
    assert np.allclose(np.sort(grad[:S]), u["sorted_rootsplit_gradient"], rtol=0, atol=u["tolerance"])
    want = []
    for part in ("low", "zero", "high"):
        want += [u["sorted_pcsp_gradient_" + part]["value"]] * u["sorted_pcsp_gradient_" + part]["count"]
    assert np.allclose(np.sort(grad[S:]), want, rtol=0, atol=u["tolerance"])
    # s and s'
    c = k["s_and_s_prime"]
    strings = L.sbn_strings(both)
    s, sp = strings.index(c["s"]), strings.index(c["s_prime"])
    phi = np.zeros(P)
    phi[s], phi[sp] = c["phi_s"], c["phi_s_prime"]
    theta = eng.sbn_normalize(both, phi)
    grad, _, lq = eng.sbn_topology_gradient(both, phi, [1.0], "given", trees=[2])
    p_tau_rho, q = c["rooting_rootsplit_prior"] * math.exp(theta[s]), math.exp(lq[0])
    assert abs(grad[s] - p_tau_rho / q * (1 - math.exp(theta[s]))) < c["tolerance"]
    assert abs(grad[sp] - p_tau_rho / q * -math.exp(theta[sp])) < c["tolerance"]
    # the factors
    f = k["factors"]
    four = [0, 1, 2, 1]
    _, plain, _ = eng.sbn_topology_gradient(both, phi, f["log_f"], "plain", trees=four)
    _, vimco, _ = eng.sbn_topology_gradient(both, phi, f["log_f"], "vimco", trees=four)
    assert np.allclose(plain, f["plain"], rtol=0, atol=f["plain_tolerance"])
    assert np.allclose(vimco, f["vimco"], rtol=0, atol=f["vimco_tolerance"])


def _check_gradient(eng, sup, ref, reps, trees, phi, seed):
    rng = np.random.default_rng(seed)
    K = len(reps)
    theta = R.normalize([float(x) for x in phi], ref.blocks())
    log_f = rng.normal(-80.0, 3.0, K)
    for estimator, factors in (("plain", V.plain_factors(list(log_f))), ("vimco", V.vimco_factors(list(log_f))),
                               ("given", list(rng.normal(0.0, 2.0, K)))):
        arg = factors if estimator == "given" else log_f
        grad, got_factors, lq = eng.sbn_topology_gradient(sup, phi, arg, estimator, trees=trees)
        want, want_lq = V.topology_gradient(reps, theta, ref.blocks(), factors)
        assert not np.any(np.isnan(grad)) and not np.any(np.isnan(lq))
        assert np.allclose(got_factors, factors, rtol=0, atol=1e-10 * max(1.0, np.abs(factors).max()))
        for a, b in zip(lq, want_lq):
            assert a == b == NEG_INF or abs(a - b) <= 1e-10 * max(1.0, abs(b))
        bound = 1e-10 * max(1.0, float(np.abs(factors).sum()))
        print(estimator, "largest difference", np.abs(grad - want).max(), "bound", bound)
        assert np.all(np.abs(grad - want) <= bound)
        theta_dev = eng.sbn_normalize(sup, phi)
        grad2, _, _ = eng.sbn_topology_gradient(sup, theta_dev, arg, estimator, trees=trees, normalized=True)
        assert grad2.tobytes() == grad.tobytes()   # (and run to run)


@pytest.mark.parametrize("n,T", [(5, 7), (65, 7)])
def test_gradient_is_the_brute_force(eng, n, T):
    pids, ref, _ = _batch(n, T)
    sup = eng.sbn_index(pids)
    _check_gradient(eng, sup, ref, ref.reps, None, _random_params(ref, 17 * n), n)


def test_gradient_with_trees_outside_the_support(eng):
    pids, ref, _ = _ds1(50)
    sup = eng.sbn_index(pids, support_tree_count=50)
    phi = _random_params(ref, 3)
    trees = list(range(50, 100))
    reps = [ref.reps[t] for t in trees]
    lq = R.log_prob(reps, R.normalize([float(x) for x in phi], ref.blocks()))[1]
    assert NEG_INF in lq and any(x != NEG_INF for x in lq)   # some trees add nothing, some do
    _check_gradient(eng, sup, ref, reps, trees, phi, 8)


def test_gradient_of_one_tree_is_built_from_the_expected_counts(eng):
    pids, ref, _ = _ds1()
    sup = eng.sbn_index(pids)
    phi = _random_params(ref, 21)
    theta = eng.sbn_normalize(sup, phi)
    for t in (0, 57):
        grad, _, lq = eng.sbn_topology_gradient(sup, phi, [1.0], "given", trees=[t])
        _, lq2, counts = eng.sbn_log_prob(sup, phi, trees=[t], expected_counts=True)
        assert lq.tobytes() == lq2.tobytes()
        G = np.exp(counts)
        want = G.copy()
        for b, e in ref.blocks():
            want[b:e] -= np.where(theta[b:e] == NEG_INF, 0.0, np.exp(theta[b:e])) * math.fsum(G[b:e])
        assert np.all(np.abs(grad - want) <= 1e-10)


# ---- errors ----
def test_an_empty_block_names_its_sample_and_block(eng):
    pids, ref, table = _five()
    sup = eng.sbn_index(pids)
    desc = eng.sbn_descent(sup)
    j = next(j for j in range(ref.S) if table[j][0] >= 0)
    block = table[j][0]
    phi = np.zeros(ref.P)
    phi[:ref.S] = NEG_INF
    phi[j] = 0.0                                  # every sample takes rootsplit j ...
    b, e = ref.parent_range[block]
    phi[b:e] = NEG_INF                            # ... and then finds its first block empty
    with pytest.raises(RuntimeError, match=rf"all -inf \(sample 0, block {block}\)"):
        eng.sbn_sample(sup, desc, phi, 1, 3)
    phi[:] = NEG_INF
    with pytest.raises(RuntimeError, match=r"all -inf \(sample 0, block -1\)"):
        eng.sbn_sample(sup, desc, phi, 1, 3)
    pid, edge, params, lp = eng.sbn_sample(sup, desc, np.zeros(ref.P), 3, 3)   # (the status word is clear again)
    assert np.all(pid >= 5) and not np.any(np.isnan(lp))


def test_bad_inputs_are_refused(eng, monkeypatch):
    pids, ref, _ = _batch(5, 7)
    sup = eng.sbn_index(pids)
    desc = eng.sbn_descent(sup)
    phi = np.zeros(ref.P)
    for bad in (np.nan, np.inf):
        phi[3] = bad
        with pytest.raises(RuntimeError, match=r"finite or -inf \(parameter 3\)"):
            eng.sbn_sample(sup, desc, phi, 4, 1)
        with pytest.raises(RuntimeError, match=r"finite or -inf \(parameter 3\)"):
            eng.sbn_topology_gradient(sup, phi, np.zeros(7), "plain")
    phi[3] = 0.0
    with pytest.raises(RuntimeError, match="at least 2 trees"):
        eng.sbn_topology_gradient(sup, phi, [0.0], "vimco", trees=[0])
    with pytest.raises(RuntimeError, match="estimator"):
        eng.sbn_topology_gradient(sup, phi, np.zeros(7), "mean")
    with pytest.raises(RuntimeError, match="estimator"):   # (the device form checks before it touches a pointer)
        eng.sbn_topology_gradient_device(None, 7, 5, *([None] * 3), ref.S, ref.C, sup.parent_count, None, None, False,
                                         None, "mean", None, None, None)
    with pytest.raises(RuntimeError, match="tree_count must be positive"):
        eng.sbn_sample(sup, desc, phi, 0, 1)
    wrong = desc.copy()
    wrong[:, 1] = 0                               # every entry 1 a block: more than n - 1 draws
    with pytest.raises(RuntimeError, match=r"descent table.*\(sample \d+\)"):
        eng.sbn_sample(sup, wrong, phi, 4, 1)
    monkeypatch.setenv("MI_PHYLO_PLV_BYTES", "100000")
    small = _engine()
    big, big_ref, _ = _batch(33, 7)
    big_sup = eng.sbn_index(big[:1])
    with pytest.raises(RuntimeError, match=r"2000 trees of 33 taxa need \d+ bytes.*not chunked"):
        small.sbn_sample(big_sup, eng.sbn_descent(big_sup), np.zeros(big_sup.parameter_count), 2000, 1)
    with pytest.raises(RuntimeError, match=r"2000 trees of 33 taxa need \d+ bytes.*not chunked"):
        small.sbn_topology_gradient(big_sup, np.zeros(big_sup.parameter_count), np.zeros(2000), "plain",
                                    trees=[0] * 2000)


# ---- one step from a captured graph ----
def test_a_step_replays_from_one_graph():
    import torch
    n, T0, K = 27, 20, 64
    pids, ref, _ = _ds1()
    pids = pids[:T0]
    first = _engine()
    sup = first.sbn_index(pids)
    S, C, parents, P, E = sup.rootsplit_count, sup.pcsp_count, sup.parent_count, sup.parameter_count, 2 * n - 3
    desc = first.sbn_descent(sup)
    phi = np.random.default_rng(4).normal(0.0, 1.0, P)
    log_f = np.random.default_rng(5).normal(-90.0, 2.0, K)
    seed, first_sample = 777, 10 ** 6
    # eager, through the host forms
    s_pid, s_edge, s_params, s_lp = first.sbn_sample(sup, desc, phi, K, seed, first_sample=first_sample)
    both = first.sbn_index(np.concatenate([pids, s_pid]), support_tree_count=T0)
    want_rooting, want_lq = first.sbn_log_prob(both, phi, trees=slice(T0, None))
    want_grad, want_factors, want_glq = first.sbn_topology_gradient(both, phi, log_f, "vimco", trees=slice(T0, None))
    dev = torch.device("cuda:0")
    i32, f64 = torch.int32, torch.float64
    d_range, d_desc = (torch.tensor(np.ascontiguousarray(x), device=dev) for x in (sup.parent_range, desc))
    d_phi, d_f = torch.tensor(phi, device=dev), torch.tensor(log_f, device=dev)
    all_pid = torch.zeros((T0 + K, E), dtype=i32, device=dev)
    all_pid[:T0] = torch.tensor(pids, device=dev)
    o_edge, o_params = torch.zeros(K, dtype=i32, device=dev), torch.zeros((K, n - 1), dtype=i32, device=dev)
    o_lp = torch.zeros(K, dtype=f64, device=dev)
    o_root, o_slot = torch.zeros((T0 + K, E), dtype=i32, device=dev), torch.zeros((T0 + K, 2 * E, 3), dtype=i32, device=dev)
    o_counts = torch.zeros(3, dtype=i32, device=dev)
    W = (n + 31) // 32
    o_bits = torch.zeros((S, W), dtype=i32, device=dev)
    o_clades, o_prange, o_parent = (torch.zeros(shape, dtype=i32, device=dev) for shape in ((C, 3), (C, 2), (C,)))
    o_rooting, o_lq = torch.zeros((K, E), dtype=f64, device=dev), torch.zeros(K, dtype=f64, device=dev)
    o_grad, o_factors, o_glq = (torch.zeros(m, dtype=f64, device=dev) for m in (P, K, K))
    outputs = (all_pid[T0:], o_edge, o_params, o_lp, o_root, o_slot, o_rooting, o_lq, o_grad, o_factors, o_glq)

    def step(stream, e):
        e.sbn_sample_device(stream, K, n, S, C, parents, d_range.data_ptr(), d_desc.data_ptr(), d_phi.data_ptr(),
                            seed, first_sample, all_pid[T0:].data_ptr(), o_edge.data_ptr(), o_params.data_ptr(),
                            o_lp.data_ptr())
        e.sbn_index_device(stream, T0 + K, n, all_pid.data_ptr(), T0, S, C, o_root.data_ptr(), o_slot.data_ptr(),
                           o_counts.data_ptr(), o_bits.data_ptr(), o_clades.data_ptr(), o_prange.data_ptr(),
                           o_parent.data_ptr())
        e.sbn_log_prob_device(stream, K, n, all_pid[T0:].data_ptr(), o_root[T0:].data_ptr(), o_slot[T0:].data_ptr(),
                              S, C, parents, d_range.data_ptr(), d_phi.data_ptr(), False, o_rooting.data_ptr(),
                              o_lq.data_ptr())
        e.sbn_topology_gradient_device(stream, K, n, all_pid[T0:].data_ptr(), o_root[T0:].data_ptr(),
                                       o_slot[T0:].data_ptr(), S, C, parents, d_range.data_ptr(), d_phi.data_ptr(),
                                       False, d_f.data_ptr(), "vimco", o_grad.data_ptr(), o_factors.data_ptr(),
                                       o_glq.data_ptr())

    def check():
        torch.cuda.synchronize()
        assert all_pid[T0:].cpu().numpy().tobytes() == s_pid.tobytes()
        assert o_edge.cpu().numpy().tobytes() == s_edge.tobytes()
        assert o_params.cpu().numpy().tobytes() == s_params.tobytes()
        assert o_lp.cpu().numpy().tobytes() == s_lp.tobytes()
        assert o_counts.cpu().numpy().tolist() == [S, C, parents]
        assert o_root.cpu().numpy().tobytes() == both.root_index.tobytes()
        assert o_slot.cpu().numpy().tobytes() == both.slot_index.tobytes()
        assert o_rooting.cpu().numpy().tobytes() == want_rooting.tobytes()
        assert o_lq.cpu().numpy().tobytes() == want_lq.tobytes() == o_glq.cpu().numpy().tobytes() == want_glq.tobytes()
        assert o_factors.cpu().numpy().tobytes() == want_factors.tobytes()
        assert o_grad.cpu().numpy().tobytes() == want_grad.tobytes()

    gs = torch.cuda.Stream()
    step(gs.cuda_stream, first)  # (the kernels' code objects are loaded at their first launch)
    check()
    fresh = _engine()
    fresh.reserve_sbn(T0 + K, n)
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info(0)[0]
    with torch.cuda.stream(gs):
        step(gs.cuda_stream, fresh)
    check()
    assert torch.cuda.mem_get_info(0)[0] == free_before  # (reserved: the calls allocated nothing)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=gs):
        step(torch.cuda.current_stream().cuda_stream, fresh)
    for _ in range(2):
        for o in outputs:
            o.zero_()
        graph.replay()
        check()
    fresh.check_status()


def test_cpp_adapter(tmp_path, eng):
    """tests/cpp/sbn_vi_example.cpp: 64 trees drawn and a gradient through Engine::SbnDescent,
    SbnSample, SbnIndex and SbnTopologyGradient; its printed numbers are the Python call's."""
    exe = tmp_path / "sbn_vi_example"
    lib = os.path.join(REPO, "libsbn_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(REPO, "tests/cpp/sbn_vi_example.cpp"),
                    "-L" + lib, "-lmi_phylo", "-lmi_phylo_host", "-Wl,-rpath," + lib, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe), os.path.join(REPO, "tests/golden/data")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = dict(line.split(" ", 1) for line in out.stdout.strip().splitlines())
    assert lines["status"] == "all checks passed"
    pids = np.array([int(x) for x in lines["support"].split()], np.int32).reshape(-1, 7)
    theta = np.array([float.fromhex(x) for x in lines["log_params"].split()])
    sup = eng.sbn_index(pids)
    pid, edge, params, lp = eng.sbn_sample(sup, eng.sbn_descent(sup), theta, 64, 20261020)
    both = eng.sbn_index(np.concatenate([pids, pid]), support_tree_count=len(pids))
    log_f = -70.0 - 0.25 * np.arange(64)
    grad, factors, lq = eng.sbn_topology_gradient(both, theta, log_f, "vimco", trees=slice(len(pids), None))
    assert [int(x) for x in lines["first_tree"].split()] == pid[0].tolist()
    assert [int(x) for x in lines["root_edges"].split()] == edge.tolist()
    assert np.array([float.fromhex(x) for x in lines["gradient"].split()]).tobytes() == grad.tobytes()
    assert np.array([float.fromhex(x) for x in lines["log_prob"].split()]).tobytes() == lp.tobytes()
