"""The inputs of tests/test_branch_hessian_edges_gpu.py, and their dense_ref references
(TEST INFRASTRUCTURE ONLY).  tests/test_dense_ref.py reads the same inputs on the CPU: an FP64
evaluator has to sit a factor of 100 inside the GPU tolerances on exactly these.

Every case: GTR with per-tree rates and frequencies, Weibull shape in [0.4, 1.6] (K = 1: the
constant site model), three trees (random, ladder, balanced) unless it says otherwise, branch
lengths drawn from LENGTHS with exactly one internal branch per tree set to 0.

One constraint on the draw: a group of tips held together by branches of at most 0.03 has no
tiny branch (0, 1e-8, 1e-4) inside it.  Where it has, and the tips' states differ, a pattern's
likelihood is an off-diagonal P_ab(t) ~ t of the tiny branch itself, which BEAGLE's form
P = V exp(L t) V^-1 (the oracle's transition mode 0) delivers with an ABSOLUTE error of 1e-16:
1e-8 relative at t = 1e-8, and the f64 oracle then misses the tolerance form by up to 3e4 (0.03
counts: in a slow rate category it is a tiny length too).  The bound stays and the inputs give
way: a branch of such a group is redrawn from 0.3, 2, 10 until no group is left.  (Real data put
equal states at the two ends of such a path: the DS1 case here and the optimiser's own case in
test_branch_opt_gpu.py.)"""
import functools
import zlib
from types import SimpleNamespace

import numpy as np

import dense_ref as D
import oracle_lib as O
import tree_utils as TU

WALK = "gradient_walk_hess_kernel"  # K <= 4 with tip masks
HBM = "gradient_hbm_hess_kernel"    # everything else, and MI_PHYLO_GRADIENT_PATH=hbm
LENGTHS = (1e-8, 1e-4, 0.03, 0.3, 2.0, 10.0)
WEIGHTS = (1e-3, 0.25, 1.0, 7.0, 1e6)
EPS = 1e-10  # the project's parity bound (README)

# the walk takes kLlR 16/Kp = 48, 24, 12 patterns per wave for K = 1, 2, >= 3 (whole-word tip
# path for K >= 3 when tile_first + 12 <= P); gradient_hbm_hess_kernel 64 patterns per tile
WALK_KP = [(1, 1), (1, 47), (1, 48), (1, 49), (2, 23), (2, 24), (2, 25), (3, 11), (3, 12), (3, 13),
           (4, 1), (4, 11), (4, 12), (4, 13), (4, 25)]


def _case(name, n, P, K, kernel=WALK, store="lds", env=(), form="states", weights="integer",
          trees="three", rescaling=(False, True)):
    return SimpleNamespace(name=name, n=n, P=P, K=K, kernel=kernel, store=store, env=dict(env),
                           form=form, weights=weights, trees=trees, rescaling=rescaling)


CASES = [_case(f"walk-n{n}-K{K}-P{P}", n, P, K) for n in (4, 5, 9) for K, P in WALK_KP]
CASES += [_case(f"arena-n40-K{K}-P{P}", 40, P, K, store="arena",
                env={"MI_PHYLO_GRADIENT_STORE": "arena"}) for K, P in ((4, 12), (4, 13), (1, 49))]
CASES += [_case(f"hbm-n6-K6-P{P}", 6, P, 6, kernel=HBM, store="hbm") for P in (63, 64, 65)]
CASES += [_case("hbm-forced-n6-K4-P65", 6, 65, 4, kernel=HBM, store="hbm",
                env={"MI_PHYLO_GRADIENT_PATH": "hbm"})]
CASES += [_case("deep-ladder-n100-K4-P13", 100, 13, 4, store="lds", trees="ladder", rescaling=(True,))]
# tip forms: gaps; an all-gap column and a column of one state; 0/1 ambiguity masks and
# real-valued vectors through tip_partials (masks keep the walk, real values take the HBM kernel)
CASES += [_case("tips-gaps", 8, 25, 4, form="gaps"), _case("tips-columns", 8, 25, 4, form="columns"),
          _case("tips-masks", 8, 25, 4, form="masks"),
          _case("tips-real", 8, 25, 4, form="real", kernel=HBM, store="hbm")]
CASES += [_case(f"weights-K{K}{z}", 8, 25, K, weights="spread" + z) for K in (1, 4) for z in ("", "-zeros")]
CASES += [_case("ds1-own-lengths", 27, 200, 4, trees="ds1")]
BY_NAME = {c.name: c for c in CASES}
ZEROED = (3, 17)  # the patterns whose weight the "-zeros" cases set to 0


@functools.lru_cache(maxsize=None)
def _ds1():
    """states, weights, parent ids, branch lengths of the ds1_top100 fixture."""
    return O.struct_arrays(O.load_struct("ds1_top100"))


def _trees(c, rng):
    """Parent ids and lengths; drawn again as a whole until the case holds a branch each of 0,
    1e-8 and 10 (the redraw of tight groups can take the last 1e-8 out of a small tree)."""
    if c.trees == "ds1":
        _, _, pids, bls = _ds1()
        return pids[:2], bls[:2]
    while True:
        pids, bls = _draw_trees(c, rng)
        if all(np.any(bls[:, :-1] == v) for v in (0.0, 1e-8, 10.0)):
            return pids, bls


def _draw_trees(c, rng):
    n = c.n
    pids = np.stack([TU.ladder_topology(n)] if c.trees == "ladder" else
                    [TU.random_topology(n, rng), TU.ladder_topology(n), TU.balanced_topology(n)])
    bls = rng.choice(LENGTHS, size=(len(pids), 2 * n - 2))
    for t in range(len(pids)):
        bls[t, rng.integers(n, 2 * n - 3)] = 0.0  # one internal branch (nodes n .. 2n-4)
        while True:
            closing = _tight_groups_with_a_tiny_branch(pids[t], bls[t], n)
            if not closing:
                break
            bls[t, rng.choice(closing)] = rng.choice(LENGTHS[3:])
    bls[:, -1] = 0.0
    return pids, bls


def _tight_groups_with_a_tiny_branch(pid, bl, n):
    """The branches of 1e-8 to 0.03 in a component of branches <= 0.03 that holds two tips or
    more and a branch <= 1e-4."""
    comp = list(range(len(pid) + 1))

    def find(v):
        while comp[v] != v:
            v = comp[v]
        return v

    tight = [j for j in range(len(pid)) if bl[j] <= 0.03]
    for j in tight:
        comp[find(j)] = find(pid[j])
    tips = [find(v) for v in range(n)]
    bad = {find(j) for j in tight if bl[j] <= 1e-4 and tips.count(find(j)) > 1}
    return [j for j in tight if bl[j] > 0 and find(j) in bad]


def _tips(c, rng):
    """(states [n][P] or None, tip vectors [n][P][4] float64)."""
    n, P = c.n, c.P
    if c.trees == "ds1":
        states = np.ascontiguousarray(_ds1()[0][:, :P])
        return states, D.tip_vectors(states, np.float64)
    states = rng.integers(0, 4, size=(n, P)).astype(np.int32)
    if c.form == "gaps":
        states[rng.random((n, P)) < 0.05] = 4
        assert np.any(states == 4)
    if c.form == "columns":
        states[:, 5] = 4
        states[:, 11] = 2
    vec = D.tip_vectors(states, np.float64)
    if c.form == "masks":  # a fifth of the vectors get one or two more states
        for i, p in zip(*np.nonzero(rng.random((n, P)) < 0.2)):
            extra = rng.choice([s for s in range(4) if s != states[i, p]], size=rng.integers(1, 3),
                               replace=False)
            vec[i, p, extra] = 1.0
        counts = vec.sum(axis=2)
        assert np.any(counts == 2) and np.any(counts == 3)
        return None, vec
    if c.form == "real":  # three tips: every entry in (0.05, 1]
        vec[:3] = 1.0 - rng.uniform(0.0, 0.95, size=vec[:3].shape)
        return None, vec
    return states, vec


@functools.lru_cache(maxsize=None)
def inputs(name):
    """Everything a case feeds the engine (and the oracle).  Treat as read-only."""
    c = BY_NAME[name]
    seed = zlib.crc32(name.replace("-zeros", "").encode())  # (the "-zeros" twin: same draws)
    rng = np.random.default_rng(seed)
    pids, bls = _trees(c, rng)
    T = len(pids)
    states, vec = _tips(c, rng)
    w = rng.integers(1, 6, size=c.P).astype(np.float64)
    if c.trees == "ds1":
        w = _ds1()[1][:c.P].copy()
    if c.weights.startswith("spread"):
        w = rng.choice(WEIGHTS, size=c.P)
        assert set(w) == set(WEIGHTS)
        if c.weights.endswith("zeros"):
            w[list(ZEROED)] = 0.0
    site = "constant" if c.K == 1 else f"weibull+{c.K}"
    spec = O.make_spec(c.n, c.P, "GTR", site)
    rates, freqs = TU.random_gtr_params(T, rng)
    shapes = rng.uniform(0.4, 1.6, size=T)
    lay = O.param_layout(spec)
    pr = np.zeros((T, O.param_count(spec)))
    pr[:, lay["GTR rates"]:lay["GTR rates"] + 6] = rates
    pr[:, lay["frequencies"]:lay["frequencies"] + 4] = freqs
    if c.K > 1:
        pr[:, lay["Weibull shape"]] = shapes
    pr[:, lay["clock rate"]] = 1.0
    return SimpleNamespace(case=c, site=site, spec=spec, states=states, vectors=vec, w=w, pids=pids,
                           bls=bls, pr=pr, rates=rates, freqs=freqs)


def model(x, t, dtype=D.LD):
    """Q, pi of tree t (built by dense_ref) and its category rates and weights (the oracle's)."""
    Q, pi = D.gtr_q(x.rates[t], x.freqs[t], dtype)
    m = O.model_set(x.spec, x.pr[t])
    K = x.case.K
    return Q, pi, np.array(m.cat_rates[:K]), np.array(m.cat_weights[:K])


@functools.lru_cache(maxsize=None)
def references(name, dtype=D.LD):
    """dense_ref of every tree of a case (patterns of weight 0 removed: they must not count)."""
    x = inputs(name)
    keep = x.w > 0
    return [D.branch_derivatives(x.pids[t], x.bls[t], *model(x, t, dtype), x.vectors[:, keep], x.w[keep],
                                 dtype=dtype) for t in range(len(x.pids))]


def ratios(refs, ll, g, h, s):
    """max_j |error_j| / tolerance_j of the outputs of a Hessian call, per quantity, over the
    trees of a case; asserts that every output is finite and that root and fixed entries are
    exactly 0.  (The maxima are numpy's, which hand a NaN on; Python's max(x, nan) is x.)"""
    T = len(refs)
    for key, got in (("logL", ll), ("g", g), ("H", h), ("S", s)):
        got = np.asarray(got)
        assert len(got) == T and np.all(np.isfinite(got)), (key, got)
    per_tree = dict(logL=[], g=[], S=[], H=[])
    for t, ref in enumerate(refs):
        tol = D.tolerances(ref, EPS)
        per_tree["logL"].append(abs(ll[t] - ref.log_likelihood) / (EPS * abs(ref.log_likelihood)))
        for key, got, want, bound in (("g", g, ref.g, tol.g), ("S", s, ref.S, tol.S), ("H", h, ref.H, tol.H)):
            assert np.all(got[t, -2:] == 0), (key, got[t, -2:])
            per_tree[key].append(np.max(np.abs(got[t, :-2] - want[:-2]) / bound[:-2]))
    return {key: float(np.max(np.array(v, dtype=D.LD))) for key, v in per_tree.items()}


def within(r):
    """True where every ratio of ratios() is at most 1 (a NaN is not)."""
    v = np.array(list(r.values()))
    return bool(np.all(v <= 1.0))
