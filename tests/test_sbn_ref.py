"""tests/sbn_ref.py (the brute-force restatement of the reference's SBN code) against the
reference's known answers (tests/golden/sbn_kats.json, at the reference's own tolerances), and the
linear-time slot and region-sum formulation (tests/sbn_slots.py: what the kernels do) against the
brute force on every DS1 tree.  No GPU."""
import json
import math
import os

import pytest

import sbn_ref as R
import sbn_slots as SL

HERE = os.path.dirname(os.path.abspath(__file__))


def _golden(name):
    with open(os.path.join(HERE, "golden", name)) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def kats():
    return _golden("sbn_kats.json")


@pytest.fixture(scope="module")
def ds1():
    return R.Support([t["parent_ids"] for t in _golden("ds1_top100.struct.json")["trees"]])


@pytest.fixture(scope="module")
def five():
    return R.Support([t["parent_ids"] for t in _golden("five_taxon.struct.json")["trees"]])


def test_ds1_support_sizes(ds1):
    assert (ds1.S, ds1.C, len(ds1.parent_range)) == (69, 554, 369)
    assert sum(len(r) for rep in ds1.reps for r in rep) == 132600
    # blocks are contiguous, cover S .. P and follow the parents' first occurrences
    assert [b for b, _ in ds1.parent_range] == [ds1.S] + [e for _, e in ds1.parent_range[:-1]]
    assert ds1.parent_range[-1][1] == ds1.P
    for (b, e), k in zip(ds1.parent_range, range(len(ds1.parent_range))):
        assert all(ds1.pcsp_parent[j - ds1.S] == k and ds1.pcsps[j - ds1.S][:2] == ds1.pcsps[b - ds1.S][:2]
                   for j in range(b, e))


def test_five_taxon_known_answers(five, kats):
    strings = five.strings()
    assert five.S == 12
    assert set(strings[:12]) == set(_golden("split_kats.json")["five_taxon_rootsplits"]["strings"])
    assert set(kats["five_taxon_pcsp_block"]["strings"]) <= set(strings[12:])
    block = [strings.index(s) for s in kats["five_taxon_pcsp_block"]["strings"]]
    assert sorted(block) == list(range(min(block), min(block) + 4))
    assert (min(block), min(block) + 4) in five.parent_range
    trees = [t["parent_ids"] for t in _golden("five_taxon.struct.json")["trees"]]
    for name in ("five_taxon_representation_1", "five_taxon_representation_2"):
        query = R.Support(trees + [kats[name]["parent_ids"]], support_tree_count=4)
        assert query.strings() == strings
        got = [{strings[j] for j in r} for r in query.reps[4]]
        assert got == [set(r) for r in kats[name]["rootings"]]


@pytest.mark.parametrize("name,method,alpha,iters", [
    ("sa", "sa", 0.0, 0), ("em_alpha0_iter1", "em", 0.0, 1), ("em_alpha0_iter23", "em", 0.0, 23),
    ("em_alpha05_iter100", "em", 0.5, 100)])
def test_training_known_answers(ds1, kats, name, method, alpha, iters):
    k = kats["ds1_probabilities"]
    theta, history = R.train(ds1, method=method, alpha=alpha, max_iter=iters)
    _, lq = R.log_prob(ds1.reps, theta)
    assert len(lq) == 100 == len(k[name]["values"])
    worst = max(abs(math.exp(x) - y) for x, y in zip(lq, k[name]["values"]))
    print(name, "largest difference", worst)
    assert worst <= k["tolerances"][name]
    assert all(b >= a - 1e-10 * abs(a) for a, b in zip(history, history[1:]))
    for b, e in ds1.blocks():
        assert abs(R.logsumexp(theta[b:e])) < 1e-12


def test_slot_formulation_is_the_brute_force(ds1):
    theta, _ = R.train(ds1, method="sa")
    for t, pid in enumerate(ds1.pids):
        tree = SL.Tree(pid)
        slots = tree.slots()
        assert {(d, k): f for d, k, f in R.ordered_pcsps(pid)} == slots
        feats = R.tree_features(pid)
        assert {f for r in feats for f in r[1:]} == set(slots.values())
        # probabilities of the rootings
        root_theta = [theta[ds1.number[r[0]]] for r in feats]
        slot_theta = {dk: theta[ds1.number[f]] for dk, f in slots.items()}
        lp = tree.walk(root_theta, slot_theta)
        ref = R.rooting_log_probs(ds1.reps[t], theta)
        assert max(abs(a - b) for a, b in zip(lp, ref)) < 1e-12
        # usages: with rho = 1 the integer rooting counts, then the posterior weights
        for log_rho in ([0.0] * len(pid), [x - R.logsumexp(ref) for x in ref]):
            _, use = tree.usage(log_rho)
            want = {}
            for v, r in enumerate(feats):
                for f in r[1:]:
                    want.setdefault(f, []).append(log_rho[v])
            for dk, f in slots.items():
                assert abs(use[dk] - R.logsumexp(want[f])) < 1e-12


def test_sentinel_and_minus_infinity():
    trees = [t["parent_ids"] for t in _golden("five_taxon.struct.json")["trees"]]
    s = R.Support(trees, support_tree_count=1)
    theta, _ = R.train(s, method="sa", T0=1)
    lp, lq = R.log_prob(s.reps, theta)
    assert lq[0] == pytest.approx(0.0, abs=1e-12)
    assert all(x == R.NEG_INF for x in lq[1:]) and not any(math.isnan(x) for row in lp for x in row)
    counts = R.log_expected_counts(s.reps, theta, [1.0] * 4)
    assert not any(math.isnan(x) for x in counts)
