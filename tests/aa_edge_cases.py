"""The inputs of tests/test_aa_edges_gpu.py, their dense_ref references, and the kernel forms the
20-state engine is run in (TEST INFRASTRUCTURE ONLY).  tests/test_dense_ref.py reads the same
inputs on the CPU: the FP64 oracle in its expm1 form has to sit a factor of 10 inside the GPU
bounds on exactly these.

Every case unless it says otherwise: three trees (random, ladder, balanced), branch lengths drawn
from LENGTHS with exactly one internal branch per tree set to 0, drawn again until a 0, a 1e-8 and
a 10 are present; one Weibull shape per tree from [0.3, 2] (K = 1: the constant site model); 5 %
of the tip codes gaps (code 20); integer weights 1..5; WAG for the even entries of CASES and
aa_utils.random_reversible_model for the odd ones.  The window, ladder and balanced cases of 129
taxa and more draw from DEEP_LENGTHS and get one 0, one 1e-8 and one 10 each.

A pattern of likelihood 0 cannot occur: the only branch of length 0 joins two internal nodes, and
an internal node's vector is positive in every state because all the branches below it are
positive and every exchangeability is (dense_ref asserts it all the same).

The shapes are the smallest at which each mechanism of kernels_aa.hip can go wrong: see the
comments at CASES."""
import functools
import zlib
from types import SimpleNamespace

import numpy as np

import aa_utils as A
import dense_ref as D
import oracle_lib as O
import tree_utils as TU

S = 20
LENGTHS = (1e-8, 1e-4, 0.03, 0.3, 2.0, 10.0)
DEEP_LENGTHS = (0.03, 0.1, 0.3)
WEIGHTS = (1e-3, 0.25, 1.0, 7.0, 1e6)
ZEROED = (3, 17)  # the patterns whose weight the "-zeros" case sets to 0
EPS = 1e-10  # the project's parity bound (README)
CLOCK_RATE = 0.7

# kernels_aa.hip / mi_phylo_kernels.h
TILE = 16              # kAaTile: patterns per tile
TILE_DOUBLES = 320     # kAaTileDoubles
POST_WAVES = 4         # kPostWaves: waves of a post-order workgroup
RING_LDS = 135 * 1024  # what a forced post-order ring may take of a CU's LDS


def _case(name, n, P, K, trees="three", lengths="all", tips="gaps5", weights="integer",
          launches=False, rooted=False, draws=None):
    return SimpleNamespace(name=name, n=n, P=P, K=K, trees=trees, lengths=lengths, tips=tips,
                           weights=weights, launches=launches, rooted=rooted, draws=draws or name)


# Tile and workgroup edges.  aa_tiles pads to four 16-pattern tiles: P = 1, 15, 16, 17 the padded
# tail of the first group; 63, 64, 65 the step from one group to two; 129 (12 tiles) a half-idle
# last workgroup at two tiles per wave and one padding wave at four; 257 (20 tiles) a workgroup
# with three padding waves at four tiles, and 10 pre-order blocks that aa_reduce_kernel splits
# 2, 3, 2, 3 over its four parts.
CASES = [_case(f"tile-n{n}-K{K}-P{P}", n, P, K) for n in (5, 9) for K in (1, 2, 4)
         for P in (1, 15, 16, 17, 63, 64, 65, 129, 257)]
CASES += [_case("tile-n9-K8-P65", 9, 65, 8)]
# XCD interleave (aa_unit): 3 trees x K = 1 x 3 workgroups at one tile per wave = 9 work items,
# no multiple of 8
CASES += [_case("xcd-n6-K1-P129", 6, 129, 1)]
# Schedule window (kSchedWindow = 128 visits): n = 129 fills it exactly once, 130 refills it once
# (forwards and backwards), 258 twice; on the ladder every visit takes its child from registers.
# N = 257, 259, 515 are also edge blocks of aa_reduce_kernel's 64-edge workgroups, and 258 taxa
# underflow FP64 unscaled (20^-258): the rescaling case.
CASES += [_case(f"window-n{n}-K4-P17", n, 17, 4, trees="random", lengths="deep") for n in (129, 130, 258)]
CASES += [_case("window-ladder-n130-K1-P16", 130, 16, 1, trees="ladder", lengths="deep"),
          _case("window-balanced-n130-K4-P17", 130, 17, 4, trees="balanced", lengths="deep")]
# aa_reduce_kernel's edge blocks: N = 63 and 65
CASES += [_case(f"reduce-n{n}-K4-P17", n, 17, 4) for n in (32, 33)]
# ... and its loop over four pattern blocks at a time, which a wave enters from 16 pre-order
# blocks on: P = 513 is 36 tiles, 18 blocks, split 4, 5, 4, 5 (one round of four, and a tail of one)
CASES += [_case("reduce-blocks-n5-K2-P513", 5, 513, 2)]
# Ring spill: the vector stack of a balanced 64-taxon tree is deeper than a four-entry ring
CASES += [_case("spill-balanced-n64-K2-P33", 64, 33, 2, trees="balanced")]
# Tips: an all-gap column and a column of one state; 20 % gaps; the same alignment as one-hot
# tip_partials (use_tip_states=False)
CASES += [_case("tips-columns", 8, 25, 4, tips="columns"), _case("tips-gaps20", 8, 25, 4, tips="gaps20"),
          _case("tips-gaps20-onehot", 8, 25, 4, tips="gaps20-onehot", draws="tips-gaps20")]
# Weights from 1e-3 to 1e6, and the same with two patterns of weight 0
CASES += [_case(f"weights-K{K}{z}", 8, 25, K, weights="spread" + z, draws=f"weights-K{K}")
          for K in (1, 4) for z in ("", "-zeros")]
# Several launches: five trees, an arena budget of two and a half evaluations
CASES += [_case("launches-n9-K4-P65", 9, 65, 4, trees="five", launches=True)]
# Rooted, strict clock
CASES += [_case("rooted-n9-K4-P33", 9, 33, 4, trees="rooted", lengths="own", rooted=True)]
for _i, _c in enumerate(CASES):
    _c.model = "WAG" if _i % 2 == 0 else "random"
BY_NAME = {c.name: c for c in CASES}
for _c in CASES:
    _c.model = BY_NAME[_c.draws].model  # (twins share everything but what their names say)


def _topologies(c, rng):
    n = c.n
    if c.trees == "random":
        return [TU.random_topology(n, rng)]
    if c.trees == "ladder":
        return [TU.ladder_topology(n)]
    if c.trees == "balanced":
        return [TU.balanced_topology(n)]
    three = [TU.random_topology(n, rng), TU.ladder_topology(n), TU.balanced_topology(n)]
    if c.trees == "five":
        three += [TU.random_topology(n, rng), TU.random_topology(n, rng)]
    return three


def _draw_trees(c, rng):
    n = c.n
    pids = np.stack(_topologies(c, rng))
    T = len(pids)
    if c.lengths == "deep":
        bls = rng.choice(DEEP_LENGTHS, size=(T, 2 * n - 2))
        for t in range(T):
            zero = rng.integers(n, 2 * n - 3)
            others = rng.choice([j for j in range(2 * n - 3) if j != zero], size=2, replace=False)
            bls[t, zero], bls[t, others[0]], bls[t, others[1]] = 0.0, 1e-8, 10.0
    else:
        bls = rng.choice(LENGTHS, size=(T, 2 * n - 2))
        for t in range(T):
            bls[t, rng.integers(n, 2 * n - 3)] = 0.0  # one internal branch (nodes n .. 2n-4)
    bls[:, -1] = 0.0
    return pids, bls


def _trees(c, rng):
    """Parent ids and lengths, drawn again as a whole until the case holds a branch each of 0,
    1e-8 and 10."""
    while True:
        pids, bls = _draw_trees(c, rng)
        if all(np.any(bls[:, :-1] == v) for v in (0.0, 1e-8, 10.0)):
            return pids, bls


def _states(c, rng):
    n, P = c.n, c.P
    states = rng.integers(0, S, size=(n, P)).astype(np.int32)
    states[rng.random((n, P)) < (0.2 if c.tips.startswith("gaps20") else 0.05)] = S
    if c.tips == "columns":
        states[:, 5] = S
        states[:, 11] = 7
    return states


def _weights(c, rng):
    if not c.weights.startswith("spread"):
        return rng.integers(1, 6, size=c.P).astype(np.float64)
    while True:
        w = rng.choice(WEIGHTS, size=c.P)
        if set(w) == set(WEIGHTS):
            break
    if c.weights.endswith("zeros"):
        w[list(ZEROED)] = 0.0
    return w


@functools.lru_cache(maxsize=None)
def wag():
    import libsbn_amd.engine as E
    return E.wag_model()


@functools.lru_cache(maxsize=None)
def inputs(name):
    """Everything a case feeds the engine (and the oracle).  Treat as read-only."""
    c = BY_NAME[name]
    rng = np.random.default_rng(zlib.crc32(c.draws.encode()))
    x = SimpleNamespace(case=c, site="constant" if c.K == 1 else f"weibull+{c.K}")
    if c.rooted:
        x.pids, x.bls, dates = (np.stack([a]) for a in TU.clocklike_rooted_tree(c.n, rng))
        x.heights, x.bounds, x.ratios = (np.stack([a]) for a in
                                         O.time_tree_init(c.n, x.pids[0], x.bls[0], dates[0]))
        x.rates = np.full((1, 2 * c.n - 2), CLOCK_RATE)
        x.rate_counts = np.ones(1, np.int32)
    else:
        x.pids, x.bls = _trees(c, rng)
    T = len(x.pids)
    x.states = _states(c, rng)
    x.partials = D.tip_vectors(x.states, np.float64, S) if c.tips.endswith("onehot") else None
    x.w = _weights(c, rng)
    x.model = wag() if c.model == "WAG" else A.random_reversible_model(rng)
    x.shapes = rng.uniform(0.3, 2.0, size=T)
    x.pr = np.full((T, 1), CLOCK_RATE if c.rooted else 1.0)
    if c.K > 1:
        x.pr = np.column_stack([x.shapes, x.pr[:, 0]])
    x.spec = A.oracle_spec(c.n, c.P, x.site)
    return x


def effective_lengths(x, t):
    """The lengths the likelihood of tree t is a function of: rate x time on the rooted case."""
    return x.bls[t] * CLOCK_RATE if x.case.rooted else x.bls[t]


def log_det_jacobian(x, t):
    """log |d heights / d ratios| of rooted tree t, which the rooted calls add to log L: the sum
    over the internal nodes below the root of log(height of the parent - bound of the node)."""
    n = x.case.n
    v = np.arange(n, 2 * n - 2)
    return np.sum(np.log(x.heights[t, x.pids[t, v]].astype(D.LD) - x.bounds[t, v].astype(D.LD)))


@functools.lru_cache(maxsize=None)
def references(name):
    """dense_ref of every tree of a case (patterns of weight 0 removed: they must not count),
    the Weibull rates and their derivatives computed in long double by dense_ref.weibull."""
    x = inputs(name)
    K = x.case.K
    keep = x.w > 0
    Q, pi = D.reversible_q(*x.model)
    vec = D.tip_vectors(x.states[:, keep], s=S)
    refs = []
    for t in range(len(x.pids)):
        r, c, dr = D.weibull(K, x.shapes[t])
        refs.append(D.branch_derivatives(x.pids[t], effective_lengths(x, t), Q, pi, r, c, vec, x.w[keep],
                                         cat_rate_derivs=dr if K > 1 else None, hessian=False))
    return refs


def bounds(refs, x, t):
    """The bounds of tree t: log L relative; g_j dense_ref.tolerances; the shape derivative
    EPS (A_site + W rho_site sum_j t_j), t_j the effective lengths; the clock-rate derivative
    sum_j t_j g_j, t_j the times, EPS sum_j t_j (A1_j + W rho)."""
    ref = refs[t]
    b = SimpleNamespace(logL=D.LD(EPS) * abs(ref.log_likelihood), g=D.tolerances(ref, EPS).g)
    b.clock = np.sum(np.asarray(x.bls[t], D.LD) * b.g[:len(x.bls[t])])
    if hasattr(ref, "g_site"):
        total = np.sum(effective_lengths(x, t).astype(D.LD))
        b.site = D.LD(EPS) * (ref.A_site + ref.W * ref.rho_site * total)
    return b


def ratios(refs, x, ll, g=None, site=None, clock=None, trees=None, jacobian=None):
    """max_j |error_j| / bound_j of the outputs of a call, per quantity, over the trees of a case
    (`trees`: the indices the outputs are of; default all).  g: [T][nodes + 1] branch gradients,
    site: [T] shape derivatives, clock: [T] clock-rate derivatives (d log L / d rate =
    sum_j t_j g_j, g_j at the effective lengths rate t_j).  Asserts that every
    output is finite and that root and fixed entries are exactly 0.  `jacobian`: ll carries
    log_det_jacobian, which is taken off it first (default: the rooted case; rooted_log_likelihoods
    adds it, the log L that rooted_gradients returns is without it).  (The maxima are numpy's,
    which hand a NaN on.)"""
    trees = list(range(len(refs))) if trees is None else list(trees)
    out = {}
    if x.case.rooted if jacobian is None else jacobian:
        ll = np.asarray(ll, D.LD) - np.array([log_det_jacobian(x, t) for t in trees])
    for key, got in (("logL", ll), ("g", g), ("site", site), ("clock", clock)):
        if got is None:
            continue
        got = np.asarray(got)
        assert len(got) == len(trees) and np.all(np.isfinite(got)), (key, got)
        worst = []
        for i, t in enumerate(trees):
            ref, b = refs[t], bounds(refs, x, t)
            if key == "logL":
                worst.append(abs(got[i] - ref.log_likelihood) / b.logL)
            elif key == "g":
                assert got.shape[1] == len(ref.g) and np.all(got[i, -2:] == 0), (key, got[i, -2:])
                worst.append(np.max(np.abs(got[i, :-2] - ref.g[:-2]) / b.g[:-2]))
            elif key == "site":
                worst.append(abs(got[i] - ref.g_site) / b.site)
            else:
                want = np.sum(x.bls[t] * ref.g[:len(x.bls[t])])  # d/d rate of log L(rate t_j)
                worst.append(abs(got[i] - want) / b.clock)
        out[key] = float(np.max(np.array(worst, dtype=D.LD)))
    return out


def within(r, limit=1.0):
    """True where every ratio of ratios() is at most `limit` (a NaN is not)."""
    return bool(np.all(np.array(list(r.values())) <= limit))


# ---------------------------------------------------------------------------------------------
# The kernel forms: MI_PHYLO_<switch> settings, read once when an engine is made.
SWITCHES = ("AA_POST", "AA_POST_TILES", "AA_RING", "AA_PRE", "AA_PRE_RING", "AA_POST_ONE_TILE_BELOW")


def _form(name, post="", tiles="", ring="", pre="", pre_ring="", below=""):
    return SimpleNamespace(name=name, env=dict(zip(SWITCHES, (post, tiles, ring, pre, pre_ring, below))))


FORMS = [_form("auto"), _form("t1-r0", tiles="1", ring="0"), _form("t1-r4", tiles="1", ring="4"),
         _form("t2-r1", tiles="2", ring="1"),  # the default of a large launch
         _form("t2-r0", tiles="2", ring="0"), _form("t2-r2", tiles="2", ring="2"),
         _form("t4-r1", tiles="4", ring="1"), _form("t4-r2", tiles="4", ring="2"),
         _form("wave-t2", post="wave", tiles="2"), _form("wave-t4", post="wave", tiles="4"),
         _form("pre-wave", pre="wave"), _form("pre-r0", pre_ring="0"), _form("pre-r2", pre_ring="2"),
         _form("both-wave", post="wave", pre="wave"),
         _form("auto-two-tiles", below="0")]  # the automatic choice takes two tiles at any size


def aa_tiles(P):
    """16-pattern tiles, padded to a multiple of four (aa_tiles of kernels_aa.hip)."""
    return ((P + TILE - 1) // TILE + 3) // 4 * 4


def arena_bytes(c, gradient):
    """The arena of one evaluation: a vector per internal node (gradient call) or per slot of the
    post-order stack, floor(log2 n) + 1 (log-likelihood call)."""
    nodes = c.n - 1 if gradient else int(np.floor(np.log2(c.n))) + 1
    return nodes * c.K * aa_tiles(c.P) * TILE_DOUBLES * 8


def expected(form, c, evals, compute_units, gradient):
    """What last_call_path() and last_call_info()[0] must say of a call of `evals` evaluations in
    its first launch, by the rules of aa_post_tiles, aa_post_ring_entries and aa_pre_ring_entries
    (kernels_aa.hip): (kernel name, the path's fields after the kernel and store)."""
    e = form.env
    tiles = aa_tiles(c.P)
    m = int(e["AA_POST_TILES"]) if e["AA_POST_TILES"] else None
    if m is None:  # one tile where the launch is short of work, else two
        threshold = int(e["AA_POST_ONE_TILE_BELOW"]) if e["AA_POST_ONE_TILE_BELOW"] else 2 * compute_units
        m = 1 if (tiles // 2 + 3) // 4 * evals * c.K < threshold else 2
    post_wave, pre_wave = e["AA_POST"] == "wave", e["AA_PRE"] == "wave"
    if post_wave:
        post_tiles, ring = max(2, m), 0  # (the wave form has two and four tiles, and no ring)
    else:
        post_tiles = m
        workgroups = (tiles // m + POST_WAVES - 1) // POST_WAVES * evals * c.K
        grid = (workgroups + 7) // 8 * 8
        ring = int(e["AA_RING"]) if e["AA_RING"] else (4 if grid < 2 * compute_units else 1)
        while ring > 0 and 8 * POST_WAVES * ring * m * (TILE_DOUBLES + 8) > RING_LDS:
            ring >>= 1
    fields = f" store=hbm-arena post-tiles={post_tiles} post-ring={ring}"
    if gradient:
        pre_ring = 0 if pre_wave else int(e["AA_PRE_RING"]) if e["AA_PRE_RING"] else 1
        fields += f" pre-ring={pre_ring}"
        kernel = "aa_pre_kernel" if pre_wave else "aa_pre_wg_kernel"
    else:
        kernel = "aa_post_kernel" if post_wave else "aa_post_wg_kernel"
    return kernel, fields + f" states=20 K={c.K}"
