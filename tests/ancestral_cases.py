"""The inputs of tests/test_ancestral_gpu.py and their ancestral_ref references (TEST
INFRASTRUCTURE ONLY).  tests/test_ancestral_ref.py reads the same inputs on the CPU: it measures
the float64-against-longdouble floor on them and holds the map-state exclusions to their cap.
Category rates and weights are the oracle's (oracle_lib.model_set); everything else is numpy."""
import functools
from types import SimpleNamespace

import numpy as np

import ancestral_ref as A
import oracle_lib as O
import tree_utils as TU

SHAPES = ("n4", "n5", "balanced8", "ladder9", "random12")
SUBSTS = ("JC69", "GTR")
KS = (1, 2, 4, 6)
PS = (13, 63, 64, 65, 129)
T = 3


def site(K):
    return "constant" if K == 1 else f"weibull+{K}"


def topologies(name, rng):
    if name == "n4":
        return np.stack([TU.random_topology(4, rng) for _ in range(T)])
    if name == "n5":
        return np.stack([TU.random_topology(5, rng) for _ in range(T)])
    if name == "balanced8":
        return np.stack([TU.balanced_topology(8)] * T)
    if name == "ladder9":
        return np.stack([TU.ladder_topology(9)] * T)
    assert name == "random12"
    return np.stack([TU.random_topology(12, rng) for _ in range(T)])


def params(spec, subst, K, trees, rng):
    """(params [T][param_count], GTR rates [T][6], frequencies [T][4]); JC69: ones and quarters."""
    lay = O.param_layout(spec)
    pr = np.zeros((trees, O.param_count(spec)))
    rates, freqs = np.ones((trees, 6)), np.full((trees, 4), 0.25)
    if subst == "GTR":
        rates, freqs = TU.random_gtr_params(trees, rng)
        pr[:, lay["GTR rates"]:lay["GTR rates"] + 6] = rates
        pr[:, lay["frequencies"]:lay["frequencies"] + 4] = freqs
    if K > 1:
        pr[:, lay["Weibull shape"]] = rng.uniform(0.4, 1.6, size=trees)
    pr[:, lay["clock rate"]] = 1.0
    return pr, rates, freqs


def _finish(name, subst, K, states, vectors, w, pids, bls, rng):
    n, P = vectors.shape[:2]
    spec = O.make_spec(n, P, subst, site(K))
    pr, rates, freqs = params(spec, subst, K, len(pids), rng)
    return SimpleNamespace(name=name, subst=subst, K=K, n=n, P=P, states=states, vectors=vectors, w=w, pids=pids,
                           bls=bls, spec=spec, pr=pr, rates=rates, freqs=freqs)


@functools.lru_cache(maxsize=None)
def parity(name, subst, K, P):
    """Compact tip states with gaps (no all-gap column: under JC69 it ties four ways exactly),
    random unequal branch lengths.  Treat as read-only."""
    seed = 7000 + 1000 * SHAPES.index(name) + 100 * SUBSTS.index(subst) + 10 * K + PS.index(P)
    rng = np.random.default_rng(seed)
    pids = topologies(name, rng)
    n = (pids.shape[1] + 3) // 2
    states, w = TU.random_alignment(n, P, rng)
    for p in np.nonzero(np.all(states > 3, axis=0))[0]:
        states[0, p] = p % 4
    assert np.any(states > 3)
    bls = rng.uniform(0.01, 0.5, size=(T, 2 * n - 2))
    bls[:, -1] = 0.0
    return _finish(name, subst, K, states, A.tip_vectors(states, np.float64), w, pids, bls, rng)


@functools.lru_cache(maxsize=None)
def partials(name, subst, K, form):
    """Tip vectors through tip_partials: `masks` -- a fifth of the one-hot vectors get one or two
    more states --, or `real` -- three tips with every entry in (0.05, 1]."""
    P = 70
    seed = 8000 + 1000 * SHAPES.index(name) + 100 * SUBSTS.index(subst) + 10 * K + (form == "real")
    rng = np.random.default_rng(seed)
    pids = topologies(name, rng)
    n = (pids.shape[1] + 3) // 2
    states = rng.integers(0, 4, size=(n, P)).astype(np.int32)
    w = rng.integers(1, 6, size=P).astype(np.float64)
    vec = A.tip_vectors(states, np.float64)
    if form == "masks":
        for i, p in zip(*np.nonzero(rng.random((n, P)) < 0.2)):
            extra = rng.choice([s for s in range(4) if s != states[i, p]], size=rng.integers(1, 3), replace=False)
            vec[i, p, extra] = 1.0
        counts = vec.sum(axis=2)
        assert np.any(counts == 2) and np.any(counts == 3)
    else:
        vec[:3] = 1.0 - rng.uniform(0.0, 0.95, size=vec[:3].shape)
    bls = rng.uniform(0.01, 0.5, size=(T, 2 * n - 2))
    bls[:, -1] = 0.0
    return _finish(name, subst, K, None, vec, w, pids, bls, rng)


@functools.lru_cache(maxsize=None)
def ladder200():
    """A 200-taxon ladder x 40 patterns, JC69 + Weibull-4 (pattern likelihoods down to 1e-126)."""
    rng = np.random.default_rng(9001)
    n, P = 200, 40
    states, w = TU.random_alignment(n, P, rng)
    pids = np.stack([TU.ladder_topology(n)])
    bls = rng.uniform(0.01, 0.5, size=(1, 2 * n - 2))
    bls[:, -1] = 0.0
    return _finish("ladder200", "JC69", 4, states, A.tip_vectors(states, np.float64), w, pids, bls, rng)


def model(x, t, dtype=A.LD):
    """Q, pi of tree t (dense_ref's) and its category rates and weights (the oracle's)."""
    Q, pi = A.gtr_q(x.rates[t], x.freqs[t], dtype)
    m = O.model_set(x.spec, x.pr[t])
    return Q, pi, np.array(m.cat_rates[:x.K]), np.array(m.cat_weights[:x.K])


def reference(x, dtype=A.LD, with_tips=True):
    """ancestral_ref of every tree of a case."""
    return [A.ancestral(x.pids[t], x.bls[t], *model(x, t, dtype), x.vectors, dtype=dtype, with_tips=with_tips)
            for t in range(len(x.pids))]


@functools.lru_cache(maxsize=None)
def parity_reference(name, subst, K, P):
    return reference(parity(name, subst, K, P))


@functools.lru_cache(maxsize=None)
def partials_reference(name, subst, K, form):
    return reference(partials(name, subst, K, form))


def engine(x, **kw):
    """The engine of a case on device 0: compact states where the case has them, else tip partials."""
    import libsbn_amd as L
    spec = L.PhyloModelSpecification(x.subst, site(x.K), "strict")
    if x.states is not None:
        return L.Engine(spec, x.states, x.w, device=0, **kw)
    return L.Engine(spec, None, x.w, device=0, use_tip_states=False, tip_partials=x.vectors, **kw)


def check_all(res, x, refs, label, tips=True):
    """Every output of an Engine.ancestral_states result against the references of its case."""
    K = x.K
    worst = dict(rel=0.0, low=0.0, rows=0.0, excluded=0.0)

    def note(pair=None, rows=None, excluded=None):
        if pair:
            worst["rel"], worst["low"] = max(worst["rel"], pair[0]), max(worst["low"], pair[1])
        worst["rows"] = max(worst["rows"], rows or 0.0)
        worst["excluded"] = max(worst["excluded"], excluded or 0.0)

    for t, ref in enumerate(refs):
        tag = f"{label} tree {t}"
        assert np.all(np.isfinite(res.state_posteriors[t])), tag
        note(A.check(res.state_posteriors[t], ref.state_post, tag + " state"))
        note(rows=A.check_rows(res.state_posteriors[t], A.ROW_SUM, tag + " state rows"))
        note(excluded=A.check_map(res.map_states[t], ref, tag + " map"))
        # (the map state is the argmax of the row as delivered, the lowest state among equals)
        assert np.array_equal(res.map_states[t], np.argmax(res.state_posteriors[t], axis=-1)), tag
        note(A.check(res.category_posteriors[t], ref.cat_post, tag + " cat"))
        note(rows=A.check_rows(res.category_posteriors[t], A.cat_row_sum(K), tag + " cat rows"))
        note(A.check(res.pattern_rates[t], ref.pattern_rate, tag + " rate"))
        if tips:
            note(A.check(res.tip_posteriors[t], ref.tip_post, tag + " tip"))
            note(rows=A.check_rows(res.tip_posteriors[t], A.ROW_SUM, tag + " tip rows"))
        ll = float(np.sum(np.asarray(x.w, A.LD) * np.log(ref.lik)))
        assert abs(res.log_likelihoods[t] - ll) <= A.REL * abs(ll), tag
    print(f"{label}: relative {worst['rel']:.2e}, absolute below {A.SMALL} {worst['low']:.2e}, "
          f"|row sum - 1| {worst['rows']:.2e}, map states left out {100 * worst['excluded']:.3f} %")
