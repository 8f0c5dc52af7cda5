"""The inputs of tests/test_spr_scan_gpu.py and their references (TEST INFRASTRUCTURE ONLY), in
the manner of ancestral_cases.py, whose model rows they use.  tests/test_spr_ref.py reads the
same inputs on the CPU.  The reference of a case is the oracle's log-likelihood of every spr_ref
neighbour; where the tips are real-valued vectors, which the oracle does not take, spr_ref's own
pruning in longdouble."""
import functools

import numpy as np

import ancestral_cases as AC
import oracle_lib as O
import spr_ref as R
import tree_utils as TU

T = 3
# (shape, patterns, categories, model, tips, rescaling): every n, P, K and model; at every K both
# settings of both template parameters of the family (rescaling; tip vectors instead of states)
SMALL = (
    ("n3", 1, 1, "JC69", "states", False),
    ("n8", 129, 1, "GTR", "onehot", True),
    ("n4", 63, 2, "GTR", "states", True),
    ("n12", 65, 2, "JC69", "onehot", False),
    ("n5", 64, 4, "JC69", "real", False),
    ("ladder12", 129, 4, "GTR", "states", True),
    ("n6", 65, 6, "GTR", "real", True),
    ("n12", 63, 6, "JC69", "states", False),
)
RADIUS = (("n12", 65, 2, "JC69", "onehot", False), ("ladder12", 129, 4, "GTR", "states", True))
SHAPES = ("n3", "n4", "n5", "n6", "n8", "n12", "ladder12")


def case_id(c):
    return "-".join(map(str, c))


def topologies(name, rng, count=T):
    if name == "n3":
        return np.stack([np.array([3, 3, 3], np.int32)] * count)
    if name.startswith("ladder"):
        return np.stack([TU.ladder_topology(int(name[6:]))] * count)
    return np.stack([TU.random_topology(int(name[1:]), rng) for _ in range(count)])


def weights(P, rng):
    """Pattern weights with zeros and non-integers among them."""
    w = rng.choice([0.0, 1.0, 1.0, 2.0, 3.0, 0.5, 2.25], size=P)
    w[0] = 1.0
    if P > 2:
        w[1], w[2] = 0.0, 0.75
    return w


@functools.lru_cache(maxsize=None)
def case(name, P, K, subst, tips, rescaling, count=T, seed_offset=0):
    seed = 23000 + 1000 * SHAPES.index(name) + 100 * (subst == "GTR") + 10 * K + P % 7 + seed_offset
    rng = np.random.default_rng(seed)
    pids = topologies(name, rng, count)
    n = (pids.shape[1] + 3) // 2
    states, _ = TU.random_alignment(n, P, rng, gap_fraction=0.1)
    w = weights(P, rng)
    vectors = AC.A.tip_vectors(states, np.float64)
    if tips == "real":
        vectors[:3] = 1.0 - rng.uniform(0.0, 0.95, size=vectors[:3].shape)
    bls = rng.uniform(0.01, 0.5, size=(count, 2 * n - 2))
    bls[:, -1] = 0.0
    x = AC._finish(name, subst, K, states if tips != "real" else None, vectors, w, pids, bls, rng)
    x.tips, x.rescaling = tips, rescaling
    return x


def engine(x, **kw):
    """The engine of a case on device 0: compact states, or the tip vectors as tip partials."""
    import libsbn_amd as L
    spec = L.PhyloModelSpecification(x.subst, AC.site(x.K), "strict")
    if x.tips == "states":
        return L.Engine(spec, x.states, x.w, device=0, **kw)
    return L.Engine(spec, None, x.w, device=0, use_tip_states=False, tip_partials=x.vectors, **kw)


def log_likelihoods(x, t, pids, bls, variant="f64"):
    """Reference log-likelihoods of trees under tree t's model row: the oracle's (`variant`), or
    for real-valued tips spr_ref's pruning in longdouble."""
    if x.states is None:
        Q, pi, r, c = AC.model(x, t)
        memo = {}
        return np.array([float(R.log_likelihood(p, b, Q, pi, r, c, x.vectors, x.w, memo=memo))
                         for p, b in zip(pids, bls)])
    O.select(variant)
    try:
        return O.unrooted_log_likelihoods(x.spec, x.states, x.w, pids, bls,
                                          np.repeat(x.pr[t][None], len(pids), axis=0), x.rescaling, 4)
    finally:
        O.select("f64")


def reference(x, t, chosen=None, variant="f64"):
    """(logL of tree t, moves, logL of each move's neighbour): all moves, or the `chosen` ones."""
    mv = R.moves(x.n, x.pids[t]) if chosen is None else chosen
    ll = float(log_likelihoods(x, t, x.pids[t][None], x.bls[t][None], variant)[0])
    if not mv:
        return ll, mv, np.zeros(0)
    nb = [R.neighbour(x.n, x.pids[t], x.bls[t], m[0], m[1], m[2], known_move=True) for m in mv]
    return ll, mv, log_likelihoods(x, t, np.stack([a for a, _ in nb]), np.stack([b for _, b in nb]), variant)


@functools.lru_cache(maxsize=None)
def small_reference(c, variant="f64"):
    x = case(*c)
    return [reference(x, t, variant=variant) for t in range(len(x.pids))]


def check_tree(res, t, x, ref, radius=0, label=""):
    """One tree of an SprScan with the whole table against its reference: logL, logL + delta, -inf
    and -1 exactly where the definition has no move within the radius, best targets and best move
    equal to the reference's.  Returns the largest relative error."""
    ll, mv, nll = ref
    E = 2 * x.n - 3
    keep = [i for i, m in enumerate(mv) if radius == 0 or m[3] <= radius]
    want = R.table(x.n, [mv[i] for i in keep], nll[keep] - ll)
    got = res.delta[t]
    assert got.shape == (E, 2, E)
    assert abs(res.log_likelihoods[t] - ll) <= R.REL * abs(ll), (label, t)
    there = ~np.isneginf(want)
    assert np.array_equal(np.isneginf(got), ~there), (label, t, "where the moves are")
    worst = 0.0
    if there.any():
        total = res.log_likelihoods[t] + got[there]
        worst = float(np.max(np.abs(total - (ll + want[there])) / np.abs(ll + want[there])))
    target, best, _, move, _ = R.decisions(want)
    assert np.array_equal(res.best_target[t], target), (label, t, "best targets")
    assert np.array_equal(np.isneginf(res.best_delta[t]), target < 0), (label, t)
    rows = target >= 0
    assert np.array_equal(res.best_delta[t][rows], np.max(got, axis=2)[rows]), (label, t)
    assert tuple(int(v) for v in res.best_move[t]) == move, (label, t, res.best_move[t], move)
    return worst


# ---- 70 taxa, rescaling on: the stored exponents at work ----

BIG = ("ladder70", "random70")


@functools.lru_cache(maxsize=None)
def big(name):
    """One 70-taxon tree, 65 patterns, four categories, rescaling on."""
    rng = np.random.default_rng(29000 + BIG.index(name))
    n, P = 70, 65
    pids = np.stack([TU.ladder_topology(n) if name == "ladder70" else TU.random_topology(n, rng)])
    states, _ = TU.random_alignment(n, P, rng, gap_fraction=0.1)
    w = weights(P, rng)
    bls = rng.uniform(0.01, 0.5, size=(1, 2 * n - 2))
    bls[:, -1] = 0.0
    subst = "JC69" if name == "ladder70" else "GTR"
    x = AC._finish(name, subst, 4, states, AC.A.tip_vectors(states, np.float64), w, pids, bls, rng)
    x.tips, x.rescaling = "states", True
    return x


@functools.lru_cache(maxsize=None)
def big_radius3_reference(name, variant="f64"):
    x = big(name)
    return reference(x, 0, R.moves(x.n, x.pids[0], 3), variant)


@functools.lru_cache(maxsize=None)
def big_sample(name):
    """A fixed-seed sample of at least 300 moves of any distance, drawn by whole rows (s, dir) so
    that the reference's best target of every sampled (s, dir) is known: [(s, d, f, distance)]."""
    x = big(name)
    rng = np.random.default_rng(29100 + BIG.index(name))
    E = 2 * x.n - 3
    out = []
    for code in rng.permutation(2 * E):
        reach = R.targets(x.n, x.pids[0], int(code) // 2, int(code) % 2)
        out += [(int(code) // 2, int(code) % 2, f, reach[f]) for f in sorted(reach)]
        if len(out) >= 300:
            break
    return out


@functools.lru_cache(maxsize=None)
def big_sample_reference(name, variant="f64"):
    return reference(big(name), 0, big_sample(name), variant)


def check_rows(res, x, ref, rows_complete, label=""):
    """Tree 0 of an SprScan with the whole table against a reference that holds some of its moves:
    logL + delta on those, and the best target of every (s, dir) of `rows_complete`, whose moves the
    reference holds all of.  Returns the largest relative error."""
    ll, mv, nll = ref
    got = res.delta[0]
    assert abs(res.log_likelihoods[0] - ll) <= R.REL * abs(ll), label
    idx = tuple(np.array([m[:3] for m in mv]).T)
    total = res.log_likelihoods[0] + got[idx]
    assert np.all(np.isfinite(total)), label
    worst = float(np.max(np.abs(total - nll) / np.abs(nll)))
    want = R.table(x.n, mv, nll - ll)
    target = R.decisions(want)[0]
    for s, d in rows_complete:
        assert res.best_target[0][s, d] == target[s, d], (label, s, d)
        assert res.best_delta[0][s, d] == got[s, d, target[s, d]], (label, s, d)
    return worst
