"""The plain-Python reference of the SBN sampler and the topology gradient (tests/sbn_vi_ref.py)
pinned on the CPU: Philox4x32-10's known answers, the reference's gradient doctest
(tests/golden/sbn_vi_kats.json), the closure of the descent table, the sampler's invariants and
the gradient of log q against central differences of the brute-force log q."""
import json
import math
import os

import numpy as np
import pytest

import sbn_ref as R
import sbn_vi_ref as V
import tree_utils as TU

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _golden(name):
    with open(os.path.join(REPO, "tests", "golden", name)) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def kats():
    return _golden("sbn_vi_kats.json")


@pytest.fixture(scope="module")
def five():
    return R.Support([t["parent_ids"] for t in _golden("five_taxon.struct.json")["trees"]])


@pytest.fixture(scope="module")
def ds1_20():
    return R.Support([t["parent_ids"] for t in _golden("ds1_top100.struct.json")["trees"][:20]])


@pytest.mark.parametrize("counter,key,want", [
    ([0, 0, 0, 0], [0, 0], "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ([0xffffffff] * 4, [0xffffffff] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0],
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    assert " ".join(f"{w:08x}" for w in V.philox4x32_10(counter, key)) == want


def test_uniform_is_in_the_unit_interval_and_keyed_by_seed_and_sample():
    us = [V.uniform(7, t, i) for t in range(4) for i in range(4)]
    assert all(0.0 <= u < 1.0 for u in us) and len(set(us)) == 16
    assert V.uniform(7, 2 ** 40 + 1, 3) != V.uniform(7, 1, 3)
    assert V.uniform(2 ** 63 + 5, 1, 3) != V.uniform(5, 1, 3)


def test_descent_table_closes(five, ds1_20):
    assert (five.S, five.C, len(five.parent_range)) == (12, 65, 49)
    assert (ds1_20.S, ds1_20.C, len(ds1_20.parent_range)) == (61, 359, 275)
    for sup in (five, ds1_20):
        table = V.descent_table(sup)   # (KeyError if a pair does not resolve)
        assert len(table) == sup.P
        for row in table:
            for e in row:
                assert -sup.n <= e < len(sup.parent_range)


def _uniform_case(kats):
    sup = R.Support(kats["gradient_test"]["support_parent_ids"])
    assert (sup.S, sup.C) == (kats["gradient_test"]["rootsplit_count"], kats["gradient_test"]["pcsp_count"])
    tau = R.Support(kats["gradient_test"]["support_parent_ids"] + [kats["uniform"]["tau_parent_ids"]], 2)
    return sup, tau.reps[2]


def test_reference_gradient_doctest_uniform(kats):
    sup, rep = _uniform_case(kats)
    k = kats["uniform"]
    theta = R.normalize([0.0] * sup.P, sup.blocks())
    grad, lq = V.grad_log_q(rep, theta, sup.blocks())
    assert abs(math.exp(lq) - k["q"]) < k["tolerance"]
    assert np.allclose(sorted(grad[:sup.S]), k["sorted_rootsplit_gradient"], rtol=0, atol=k["tolerance"])
    want = []
    for part in ("low", "zero", "high"):
        want += [k["sorted_pcsp_gradient_" + part]["value"]] * k["sorted_pcsp_gradient_" + part]["count"]
    assert np.allclose(sorted(grad[sup.S:]), want, rtol=0, atol=k["tolerance"])


def test_reference_gradient_doctest_s_and_s_prime(kats):
    sup, rep = _uniform_case(kats)
    k = kats["s_and_s_prime"]
    strings = sup.strings()
    s, sp = strings.index(k["s"]), strings.index(k["s_prime"])
    phi = [0.0] * sup.P
    phi[s], phi[sp] = k["phi_s"], k["phi_s_prime"]
    theta = R.normalize(phi, sup.blocks())
    grad, lq = V.grad_log_q(rep, theta, sup.blocks())
    p_tau_rho = k["rooting_rootsplit_prior"] * math.exp(theta[s])
    q = math.exp(lq)
    assert abs(grad[s] - p_tau_rho / q * (1 - math.exp(theta[s]))) < k["tolerance"]
    assert abs(grad[sp] - p_tau_rho / q * -math.exp(theta[sp])) < k["tolerance"]


def test_reference_factors(kats):
    k = kats["factors"]
    assert np.allclose(V.plain_factors(k["log_f"]), k["plain"], rtol=0, atol=k["plain_tolerance"])
    assert np.allclose(V.vimco_factors(k["log_f"]), k["vimco"], rtol=0, atol=k["vimco_tolerance"])


def test_gradient_is_the_central_difference_of_log_q(five):
    rng = np.random.default_rng(11)
    phi = list(rng.normal(size=five.P))
    blocks = five.blocks()
    rep = five.reps[1]
    grad, _ = V.grad_log_q(rep, R.normalize(phi, blocks), blocks)
    h = 1e-5
    for j in (0, 3, five.S, five.S + 7, five.P - 1) + tuple(rep[0][:3]):
        up, down = list(phi), list(phi)
        up[j] += h
        down[j] -= h
        lq_up = R.log_prob([rep], R.normalize(up, blocks))[1][0]
        lq_down = R.log_prob([rep], R.normalize(down, blocks))[1][0]
        assert abs((lq_up - lq_down) / (2 * h) - grad[j]) < 1e-8, j


def test_sampler_invariants(five):
    """Every sample is a tree of the support's closure whose chosen rooting expands to the sampled
    parameters; the numbering is tree_utils._polish's; frequencies follow q."""
    theta, _ = R.train(five, method="sa")
    blocks = five.blocks()
    table, c = V.descent_table(five), V.cdf(theta, blocks)
    K, seen = 4096, {}
    for t in range(K):
        pid, edge, chosen = V.sample(five.n, five.S, five.parent_range, table, c, 20261020, t)
        key = tuple(pid)
        seen.setdefault(key, [0, edge, chosen])[0] += 1
    assert len(seen) <= 12
    reps = R.Support(five.pids + [list(k) for k in seen], len(five.pids)).reps[len(five.pids):]
    share = {}
    for (pid, (count, edge, chosen)), rep in zip(seen.items(), reps):
        assert sorted(rep[edge]) == sorted(chosen) and rep[edge][0] == chosen[0]
        assert len(chosen) == five.n - 1
        lq = R.log_prob([rep], theta)[1][0]
        topology = frozenset(r[0] for r in rep)   # (an unrooted topology is its set of splits)
        share.setdefault(topology, [0, lq])[0] += count
    assert len(share) == 4 and abs(sum(math.exp(lq) for _, lq in share.values()) - 1.0) < 1e-9
    for count, lq in share.values():
        assert abs(count / K - math.exp(lq)) < 5 * 0.5 / math.sqrt(K)


def test_polish_is_tree_utils_polish():
    tree = (((0, 3), 1), (2, 5), (4, (6, 7)))
    pid, top = V.polish(tree, 8)
    assert pid == TU._polish(tree, 8).tolist()
    assert sorted(i for _, i in top) == sorted(v for v, p in enumerate(pid) if p == len(pid))
