"""Subsplit Bayesian networks on the GPU against tests/sbn_ref.py, the brute-force
restatement of the reference: the support with its numbering and every tree's slots, the look-up of
trees outside the support, the probabilities of all rootings with the expected usages, the
log-normalisation, simple-average and EM training (the reference's four known-answer vectors on
DS1), the device forms from a captured graph, and the errors.  Taxon counts: 3 (no k != 0 slot),
4, 5, the word boundaries 32 | 33 and 64 | 65 of the split table underneath, DS1's 27, and 257
(the node arrays in memory instead of LDS)."""
import json
import os
import subprocess

import numpy as np
import pytest

import sbn_ref as R
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
    """(parent ids, the reference's support of the whole batch): computed once, never changed.
    Random trees, a duplicate of tree 0 and another rooting of it (splits_ref.random_batch), and
    from 7 trees on the caterpillar (the deepest chain) and a balanced tree."""
    key = ("batch", n, T)
    if key not in _CACHE:
        pids, _ = SR.random_batch(n, T, np.random.default_rng(7000 * n + T))
        if T >= 7:
            pids[2], pids[3] = R.caterpillar(n), R.balanced(n)
        pids.setflags(write=False)
        _CACHE[key] = (pids, R.Support(pids))
    return _CACHE[key]


def _ds1():
    if "ds1" not in _CACHE:
        pids = np.array([t["parent_ids"] for t in _golden("ds1_top100.struct.json")["trees"]], np.int32)
        _CACHE["ds1"] = (pids, R.Support(pids))
    return _CACHE["ds1"]


def _ds1_half():
    """Support of the first 50 DS1 trees, all 100 looked up."""
    if "ds1_half" not in _CACHE:
        pids = _ds1()[0]
        _CACHE["ds1_half"] = (pids, R.Support(pids, support_tree_count=50))
    return _CACHE["ds1_half"]


def _check_support(got, ref, trees=None):
    import libsbn_amd as L
    assert (got.rootsplit_count, got.pcsp_count, got.parent_count) == (ref.S, ref.C, len(ref.parent_range))
    strings = L.sbn_strings(got)
    assert set(strings) == set(ref.strings())
    assert strings == ref.strings()  # (the numbering rule is the header's: the same order)
    assert got.parent_range.tolist() == [list(r) for r in ref.parent_range]
    assert got.pcsp_parent.tolist() == ref.pcsp_parent
    T = got.parent_ids.shape[0]
    for t in (range(T) if trees is None else trees):
        reps = L.sbn_rooted_representations(got, t)
        assert [sorted(r) for r in reps] == [sorted(r) for r in ref.reps[t]], t
        assert [r[0] for r in reps] == [r[0] for r in ref.reps[t]]


SHAPES = [(n, T) for n in (3, 4, 5, 27, 32, 33, 64, 65) for T in (1, 7, 65)] + [(257, 2)]


@pytest.mark.parametrize("n,T", SHAPES)
def test_index_is_the_references(eng, n, T):
    pids, ref = _batch(n, T)
    got = eng.sbn_index(pids)
    assert eng.last_call_path() == f"sbn n={n} store={'lds' if n <= 214 else 'global'}"
    _check_support(got, ref, trees=None if T <= 7 or n <= 5 else (0, 1, 2, 3, T - 1))
    E, P = 2 * n - 3, ref.P
    # slots exist exactly where the focal clade has two taxa and the far node is internal
    slot = got.slot_index
    assert np.all(slot[:, 0:2 * n:2, :] == -1)                       # below a leaf: no focal pair
    assert np.all(slot[:, 1::2, 0] >= 0) and np.all(slot[:, 1:2 * n:2, 1:] == -1)   # above a leaf: k = 0 only
    assert np.all(slot[:, 2 * n:, :] >= 0) and np.all(slot < P) and np.all(got.root_index < ref.S)
    if n == 3:
        assert not np.any(slot[:, :, 1:] >= 0)
    # blocks are contiguous, in order of the parents' first occurrences, children by their own
    order = {}
    for t in range(T):
        for j in slot[t].reshape(-1):
            if j >= 0:
                order.setdefault(int(j), len(order))
    firsts = [order[j] for j in range(ref.S, P)]
    for b, e in got.parent_range:
        block = firsts[b - ref.S:e - ref.S]
        assert block == sorted(block)
    heads = [firsts[b - ref.S] for b, _ in got.parent_range]
    assert heads == sorted(heads)
    # the duplicate of tree 0 shares its slots; the other rooting of it its features
    if T >= 3:
        assert np.array_equal(slot[T - 1], slot[0]) and np.array_equal(got.root_index[T - 1], got.root_index[0])
    if T >= 2 and n >= 4:
        assert set(slot[1].reshape(-1)) == set(slot[0].reshape(-1))


def test_collision_path_gives_the_same_bytes(monkeypatch):
    pids, ref = _batch(12, 7)
    want = _engine().sbn_index(pids)
    for bits in ("0", "4"):
        monkeypatch.setenv("MI_PHYLO_SPLIT_HASH_BITS", bits)
        got = _engine().sbn_index(pids)
        for name in ("root_index", "slot_index", "split_bits", "pcsp_clades", "parent_range", "pcsp_parent"):
            assert getattr(got, name).tobytes() == getattr(want, name).tobytes(), (bits, name)
    _check_support(want, ref)


def test_five_taxon_known_answers(eng):
    import libsbn_amd as L
    kats = _golden("sbn_kats.json")
    trees = [t["parent_ids"] for t in _golden("five_taxon.struct.json")["trees"]]
    queries = [kats[k]["parent_ids"] for k in ("five_taxon_representation_1", "five_taxon_representation_2")]
    got = eng.sbn_index(np.array(trees + queries, np.int32), support_tree_count=4)
    strings = L.sbn_strings(got)
    assert got.rootsplit_count == 12
    assert set(strings[:12]) == set(_golden("split_kats.json")["five_taxon_rootsplits"]["strings"])
    block = sorted(strings.index(s) for s in kats["five_taxon_pcsp_block"]["strings"])
    assert [block[0], block[0] + 4] in got.parent_range.tolist() and block == list(range(block[0], block[0] + 4))
    for q, name in enumerate(("five_taxon_representation_1", "five_taxon_representation_2")):
        reps = L.sbn_rooted_representations(got, 4 + q)
        assert [{strings[j] for j in r} for r in reps] == [set(r) for r in kats[name]["rootings"]]
    _check_support(got, R.Support(trees + queries, support_tree_count=4))


def test_index_errors(eng):
    pids, ref = _batch(5, 7)
    bad = np.array(pids)
    bad[4] = bad[4][::-1]
    with pytest.raises(RuntimeError, match=r"\(tree 4\)"):
        eng.sbn_index(bad)
    arity = np.array(pids)
    arity[5] = [5, 5, 5, 6, 6, 7, 7]
    with pytest.raises(RuntimeError, match=r"bifurcating.*\(tree 5\)"):
        eng.sbn_index(arity)
    with pytest.raises(RuntimeError, match=rf"capacities \(S = {ref.S}, C = {ref.C}\)"):
        eng.sbn_index(pids, rootsplit_capacity=ref.S - 1)
    with pytest.raises(RuntimeError, match=rf"capacities \(S = {ref.S}, C = {ref.C}\)"):
        eng.sbn_index(pids, pcsp_capacity=ref.C - 1)
    exact = eng.sbn_index(pids, rootsplit_capacity=ref.S, pcsp_capacity=ref.C)
    _check_support(exact, ref)
    with pytest.raises(RuntimeError, match="support_tree_count"):
        eng.sbn_index(pids, support_tree_count=8)


def test_index_over_the_budget_is_refused(monkeypatch):
    monkeypatch.setenv("MI_PHYLO_PLV_BYTES", "100000")
    pids, _ = _batch(33, 65)
    with pytest.raises(RuntimeError, match=r"65 trees of 33 taxa need \d+ bytes.*not chunked"):
        _engine().sbn_index(pids)


# ---- look-up ----
@pytest.fixture(scope="module")
def half(eng):
    pids, ref = _ds1_half()
    return eng.sbn_index(pids, support_tree_count=50), ref


def test_lookup_places_the_sentinel_exactly(half):
    got, ref = half
    _check_support(got, ref, trees=range(0, 100, 7))
    P = ref.P
    outside = [t for t in range(100) if any(P in r for r in ref.reps[t])]
    assert outside and min(outside) >= 50
    for t in range(100):
        assert (P in got.slot_index[t] or P in got.root_index[t]) == (t in outside)


def test_lookup_probabilities(eng, half):
    got, ref = half
    theta, _ = R.train(ref, method="sa", T0=50)
    lp, lq = eng.sbn_log_prob(got, theta, normalized=True)
    rlp, rlq = R.log_prob(ref.reps, theta)
    assert not np.any(np.isnan(lp)) and not np.any(np.isnan(lq))
    nowhere = [t for t in range(100) if rlq[t] == NEG_INF]
    partly = [t for t in range(100) if rlq[t] != NEG_INF and NEG_INF in rlp[t]]
    assert nowhere and partly
    for t in range(100):
        for a, b in zip(lp[t], rlp[t]):
            assert a == b == NEG_INF or abs(a - b) <= 1e-10 * max(1.0, abs(b))
        assert lq[t] == rlq[t] == NEG_INF or abs(lq[t] - rlq[t]) <= 1e-10 * max(1.0, abs(rlq[t]))
    # the trees without a rooting in the support contribute nothing
    w = np.linspace(0.5, 2.0, 100)
    _, _, counts = eng.sbn_log_prob(got, theta, normalized=True, tree_weights=w, expected_counts=True)
    want = R.log_expected_counts(ref.reps, theta, w)
    assert not np.any(np.isnan(counts))
    for a, b in zip(counts, want):
        assert a == b == NEG_INF or abs(a - b) <= 1e-10 * max(1.0, abs(b))


# ---- log_prob ----
def _random_params(ref, seed):
    rng = np.random.default_rng(seed)
    theta = rng.normal(0.0, 2.0, ref.P)
    theta[rng.choice(ref.P, max(1, ref.P // 40), replace=False)] = NEG_INF
    return theta


def _close(got, want):
    got, want = np.asarray(got, float).reshape(-1), np.asarray(want, float).reshape(-1)
    both = (got == NEG_INF) & (want == NEG_INF)
    assert not np.any(np.isnan(got))
    assert np.array_equal(got == NEG_INF, want == NEG_INF)
    err = np.abs(got[~both] - want[~both]) / np.maximum(1.0, np.abs(want[~both]))
    print("largest scaled difference", err.max() if err.size else 0.0)
    assert np.all(err <= 1e-10)


@pytest.mark.parametrize("n,T", [(5, 7), (27, 65), (33, 7), (65, 7), (257, 2)])
def test_log_prob_is_the_references(eng, n, T):
    pids, ref = _batch(n, T)
    got = eng.sbn_index(pids)
    theta = _random_params(ref, n)
    w = np.random.default_rng(T).uniform(0.1, 3.0, T)
    norm = R.normalize(list(theta), ref.blocks())
    _close(eng.sbn_normalize(got, theta), norm)
    rlp, rlq = R.log_prob(ref.reps, norm)
    want = R.log_expected_counts(ref.reps, norm, w)
    for normalized, params in ((False, theta), (True, norm)):
        lp, lq, counts = eng.sbn_log_prob(got, params, normalized=normalized, tree_weights=w, expected_counts=True)
        _close(lp, rlp)
        _close(lq, rlq)
        _close(counts, want)
    assert eng.last_call_path() == f"sbn n={n} store={'lds' if n <= 214 else 'global'}"


def test_log_prob_bits_repeat(eng):
    pids, ref = _batch(27, 65)
    got = eng.sbn_index(pids)
    theta = np.array(R.normalize(list(_random_params(ref, 3)), ref.blocks()))
    first = eng.sbn_log_prob(got, theta, normalized=True, expected_counts=True)
    again = eng.sbn_log_prob(got, theta, normalized=True, expected_counts=True)
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()
    # a permuted batch: every tree keeps its bits
    perm = np.random.default_rng(9).permutation(65)
    lp, lq = eng.sbn_log_prob(got, theta, trees=perm, normalized=True)
    assert lp.tobytes() == first[0][perm].tobytes() and lq.tobytes() == first[1][perm].tobytes()
    # a tree alone
    for t in (0, 17, 64):
        lp, lq = eng.sbn_log_prob(got, theta, trees=[t], normalized=True)
        assert lp.tobytes() == first[0][t:t + 1].tobytes() and lq.tobytes() == first[1][t:t + 1].tobytes()


def test_log_prob_refuses_bad_inputs(eng):
    pids, ref = _batch(5, 7)
    got = eng.sbn_index(pids)
    theta = np.zeros(ref.P)
    for bad in (np.nan, np.inf):
        theta[3] = bad
        with pytest.raises(RuntimeError, match=r"finite or -inf \(parameter 3\)"):
            eng.sbn_log_prob(got, theta)
    theta[3] = 0.0
    with pytest.raises(RuntimeError, match=r"weights.*\(tree 2\)"):
        eng.sbn_log_prob(got, theta, tree_weights=[1, 1, -1, 1, 1, 1, 1], expected_counts=True)


def test_device_forms_replay_from_a_graph():
    import torch
    n, T = 27, 65
    pids, ref = _batch(n, T)
    first = _engine()
    sup = first.sbn_index(pids)
    theta = _random_params(ref, 11)
    w = np.random.default_rng(2).uniform(0.5, 2.0, T)
    want = first.sbn_log_prob(sup, theta, tree_weights=w, expected_counts=True)
    dev = torch.device("cuda:0")
    E, P = 2 * n - 3, ref.P
    d = {k: torch.tensor(np.ascontiguousarray(v), device=dev) for k, v in (
        ("pid", sup.parent_ids), ("root", sup.root_index), ("slot", sup.slot_index), ("range", sup.parent_range),
        ("theta", theta), ("w", w))}
    o_lp = torch.zeros((T, E), dtype=torch.float64, device=dev)
    o_lq = torch.zeros(T, dtype=torch.float64, device=dev)
    o_counts, o_norm = (torch.zeros(P, dtype=torch.float64, device=dev) for _ in range(2))
    gs = torch.cuda.Stream()

    def call(stream, engine):
        engine.sbn_normalize_device(stream, ref.S, ref.C, sup.parent_count, d["range"].data_ptr(),
                                    d["theta"].data_ptr(), o_norm.data_ptr())
        engine.sbn_log_prob_device(stream, T, n, d["pid"].data_ptr(), d["root"].data_ptr(), d["slot"].data_ptr(),
                                   ref.S, ref.C, sup.parent_count, d["range"].data_ptr(), d["theta"].data_ptr(), False,
                                   o_lp.data_ptr(), o_lq.data_ptr(), o_counts.data_ptr(), d["w"].data_ptr())

    call(gs.cuda_stream, first)  # (the kernels' code objects are loaded at their first launch)
    torch.cuda.synchronize()
    fresh = _engine()
    fresh.reserve_sbn(T, n)
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info(0)[0]
    with torch.cuda.stream(gs):
        call(gs.cuda_stream, fresh)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info(0)[0] == free_before  # (reserved: the calls allocated nothing)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=gs):
        call(torch.cuda.current_stream().cuda_stream, fresh)
    for _ in range(2):
        for o in (o_lp, o_lq, o_counts, o_norm):
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert o_lp.cpu().numpy().tobytes() == want[0].tobytes()
        assert o_lq.cpu().numpy().tobytes() == want[1].tobytes()
        assert o_counts.cpu().numpy().tobytes() == want[2].tobytes()
        assert o_norm.cpu().numpy().tobytes() == first.sbn_normalize(sup, theta).tobytes()
    fresh.check_status()


# ---- training ----
@pytest.fixture(scope="module")
def ds1(eng):
    pids, ref = _ds1()
    got = eng.sbn_index(pids)
    assert (got.rootsplit_count, got.pcsp_count, got.parent_count) == (69, 554, 369)
    return got, ref


@pytest.mark.parametrize("name,method,alpha,iters", [
    ("sa", "sa", 0.0, 0), ("em_alpha0_iter1", "em", 0.0, 1), ("em_alpha0_iter23", "em", 0.0, 23),
    ("em_alpha05_iter100", "em", 0.5, 100)])
def test_training_known_answers(eng, ds1, name, method, alpha, iters):
    got, ref = ds1
    k = _golden("sbn_kats.json")["ds1_probabilities"]
    theta, history = eng.sbn_train(got, method=method, alpha=alpha, max_iter=iters)
    assert len(history) == iters
    _, lq = eng.sbn_log_prob(got, theta, normalized=True)
    worst = np.max(np.abs(np.exp(lq) - np.array(k[name]["values"])))
    print(name, "largest difference", worst)
    assert len(lq) == 100 and worst <= k["tolerances"][name]
    assert all(b >= a - 1e-10 * abs(a) for a, b in zip(history, history[1:]))  # the score is monotone
    if iters in (0, 1, 23):
        want, rh = R.train(ref, method=method, alpha=alpha, max_iter=iters)
        _close(theta, want)
        _close(history, rh)


def test_training_weights_are_duplicates(eng):
    pids, ref = _batch(27, 7)
    got = eng.sbn_index(pids[:6])
    w = np.array([2.0, 1, 1, 1, 1, 1])
    twice = eng.sbn_index(np.concatenate([pids[:6], pids[:1]]))
    for method, iters in (("sa", 0), ("em", 3)):
        a, ha = eng.sbn_train(got, method=method, tree_weights=w, max_iter=iters)
        b, hb = eng.sbn_train(twice, method=method, max_iter=iters)
        _close(a, b)
        _close(ha, hb)
        ref6 = R.Support(pids[:6])
        _close(a, R.train(ref6, weights=w, method=method, max_iter=iters)[0])


def test_training_stops_on_score_epsilon(eng, ds1):
    got, ref = ds1
    _, full = eng.sbn_train(got, method="em", max_iter=12)
    gains = [abs((b - a) / a) for a, b in zip(full, full[1:])]
    # (the gains need not fall from iteration to iteration) a threshold that only the smallest is below
    order = np.argsort(gains)
    stop, eps = int(order[0]), 0.5 * (gains[order[0]] + gains[order[1]])
    assert stop + 2 < 12 and gains[order[1]] > 1.05 * gains[order[0]]
    theta, history = eng.sbn_train(got, method="em", max_iter=12, score_epsilon=eps)
    assert len(history) == stop + 2 and history.tobytes() == full[:stop + 2].tobytes()
    _close(theta, R.train(ref, method="em", max_iter=12, score_epsilon=eps)[0])


def test_training_errors(eng, half):
    got, ref = half
    with pytest.raises(RuntimeError, match="alpha"):
        eng.sbn_train(got, method="em", alpha=-0.5, max_iter=2)
    outside = min(t for t in range(100) if any(ref.P in r for r in ref.reps[t]))
    with pytest.raises(RuntimeError, match=r"outside the support \(tree 50\)"):
        eng.sbn_train(got, method="sa", trees=list(range(50)) + [outside])
    with pytest.raises(RuntimeError, match="method"):
        eng.sbn_train(got, method="mle")


def test_cpp_adapter(tmp_path):
    exe = tmp_path / "sbn_example"
    lib = os.path.join(REPO, "libsbn_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(REPO, "tests/cpp/sbn_example.cpp"),
                    "-L" + lib, "-lmi_phylo", "-lmi_phylo_host", "-Wl,-rpath," + lib, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe), os.path.join(REPO, "tests/golden/data")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
