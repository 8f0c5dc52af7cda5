"""An independent reference for the SPR hill-climbing search (mi_engine_spr_search_unrooted,
DESIGN.md 4.19), and the cases the tests run it on.

Per round and tree: the reference optimum of the branch lengths on the oracle
(branch_opt_ref.reference_optimum), the oracle's log-likelihood of every neighbour tree
(spr_ref.neighbour of spr_ref.moves, within the radius) at those lengths, and the public decision
rule.  Nothing of the library is used.  Every decision comes with its margin, min(best delta -
second-best delta, |best delta - min_gain|): how far the deltas would have to move for the
search to go another way.  tests/test_spr_search_ref.py checks on the CPU that the margins of
the committed cases are at least ten times what the deltas move by when the optimiser stops 100
times earlier."""
import functools

import numpy as np

import nni_search_ref as NS
import oracle_lib as O
import spr_ref as SR
import tree_utils as TU

LOCAL_OPTIMUM, MOVE_LIMIT = 0, 1
MIN_GAIN = NS.MIN_GAIN  # the call's default
TIGHT, LOOSE = NS.TIGHT, NS.LOOSE


class Decision:
    """One round of one tree: the moves (s, dir, f, distance) in code order with their deltas, the
    triple taken ((-1, -1, -1): none to take)."""

    def __init__(self, moves, delta, min_gain, log_likelihood):
        self.moves, self.delta, self.log_likelihood = moves, delta, log_likelihood
        self.move, self.index, self.best, self.margin = (-1, -1, -1), -1, 0.0, np.inf
        if len(delta):
            k = int(np.argmax(delta))  # (the first of equals: the lowest code)
            self.move, self.index, self.best = tuple(moves[k][:3]), k, float(delta[k])
            self.margin = abs(self.best - min_gain)
            if len(delta) > 1:
                self.margin = min(self.margin, self.best - float(np.delete(delta, k).max()))


class SearchResult:
    def __init__(self):
        self.moves, self.gains, self.decisions = [], [], []
        self.parent_ids = self.branch_lengths = None
        self.log_likelihood, self.best_delta, self.status = 0.0, 0.0, LOCAL_OPTIMUM


def neighbourhood(spec, tips, w, pid, x, params, rescaling=False, radius=0):
    """(moves, neighbour trees, their oracle log-likelihoods) of one tree at lengths x."""
    n = spec.taxon_count
    moves = SR.moves(n, pid, radius)
    if not moves:
        return moves, [], np.empty(0)
    nb = [SR.neighbour(n, pid, x, s, d, f, known_move=True) for s, d, f, _ in moves]
    lls = O.unrooted_log_likelihoods(spec, tips, w, np.stack([p for p, _ in nb]), np.stack([b for _, b in nb]),
                                     np.repeat(np.asarray(params, float).reshape(1, -1), len(nb), axis=0),
                                     rescaling, min(8, len(nb)))
    return moves, nb, lls


def reference_search(spec, tips, w, pid, start, params, rescaling=False, min_gain=MIN_GAIN,
                     max_moves=100, radius=0, tol=TIGHT):
    """The search from one tree (pid [2n-3], start [2n-2], params [C]) -> SearchResult."""
    pid, bl = np.array(pid, np.int32), np.array(start, float)
    out = SearchResult()
    while True:
        x, ll = NS._optimum(spec, tips, w, pid, bl, params, rescaling, tol)
        moves, nb, lls = neighbourhood(spec, tips, w, pid, x, params, rescaling, radius)
        d = Decision(moves, lls - ll, min_gain, ll)
        out.decisions.append(d)
        better = d.move[0] >= 0 and d.best > min_gain
        if better and len(out.moves) < max_moves:
            out.moves.append(d.move)
            out.gains.append(d.best)
            pid, bl = nb[d.index]
            pid = np.asarray(pid, np.int32)
            continue
        out.parent_ids, out.branch_lengths = pid, x
        out.log_likelihood, out.best_delta = ll, d.best
        out.status = MOVE_LIMIT if better else LOCAL_OPTIMUM
        return out


# ---- the cases ----

def random_spr_walk(n, pid, bl, steps, rng):
    """`steps` random SPR moves away from a tree (spr_ref.neighbour)."""
    for _ in range(steps):
        moves = SR.moves(n, pid)
        s, d, f, _ = moves[int(rng.integers(0, len(moves)))]
        pid, bl = SR.neighbour(n, pid, bl, s, d, f, known_move=True)
    return np.asarray(pid, np.int32), bl


class Case:
    """An alignment evolved down a random tree, and start trees `away` random SPR moves from it."""

    def __init__(self, name, n, P, subst, site, seed, away, radius=0):
        self.name, self.n, self.P, self.subst, self.site, self.seed = name, n, P, subst, site, seed
        self.away, self.radius = away, radius

    def __repr__(self):
        return self.name

    @functools.lru_cache(maxsize=None)
    def build(self):
        """(spec, tips, weights, parent ids [T][2n-3], start lengths [T][2n-2], params [T][C])"""
        n, rng = self.n, np.random.default_rng(self.seed)
        true_pid = TU.random_topology(n, rng)
        tips, w = NS.evolved_alignment(true_pid, n, self.P, rng)
        start = np.full(2 * n - 2, 0.1)
        start[-1] = 0.0
        pids = np.stack([random_spr_walk(n, true_pid, start, k, rng)[0] for k in self.away])
        T = len(self.away)
        spec = O.make_spec(n, self.P, self.subst, self.site)
        pr = np.zeros((T, O.param_count(spec)))
        lay = O.param_layout(spec)
        if self.subst == "GTR":
            gr, gf = TU.random_gtr_params(T, rng)
            pr[:, lay["GTR rates"]:lay["GTR rates"] + 6] = gr
            pr[:, lay["frequencies"]:lay["frequencies"] + 4] = gf
        if self.site != "constant":
            pr[:, lay["Weibull shape"]] = rng.uniform(0.4, 1.6, size=T)
        if lay["clock rate"] >= 0:
            pr[:, lay["clock rate"]] = 1.0
        return spec, tips, w, pids, np.tile(start, (T, 1)), pr

    @functools.lru_cache(maxsize=None)
    def reference(self, tol=TIGHT, max_moves=100):
        """The reference search of every tree of the case (computed once, shared by the tests)."""
        spec, tips, w, pids, start, pr = self.build()
        return [reference_search(spec, tips, w, pids[t], start[t], pr[t], tol=tol, max_moves=max_moves,
                                 radius=self.radius)
                for t in range(len(pids))]


# n = 4 (three moves in all, the hub often the root), 5, 8, 12; one and four categories; JC69 and
# GTR; 100 to 300 patterns; one case at radius 2.  SPR neighbourhoods hold near-ties (an edge on
# its lower bound makes the targets on either side of it near-equal): a seed whose case fails the
# margin check of tests/test_spr_search_ref.py is replaced here, never skipped at run time.
CASES = [
    Case("n4-jc-k1", 4, 100, "JC69", "constant", 301, (0, 1, 1)),
    Case("n5-jc-k4", 5, 150, "JC69", "weibull+4", 302, (0, 1, 2)),
    Case("n8-gtr-k1", 8, 200, "GTR", "constant", 303, (0, 1, 2)),
    Case("n8-jc-k4-r2", 8, 250, "JC69", "weibull+4", 304, (1, 2, 3), radius=2),
    Case("n12-gtr-k4", 12, 300, "GTR", "weibull+4", 305, (0, 2, 3)),
    Case("n12-jc-k1", 12, 200, "JC69", "constant", 306, (1, 2, 3)),
]

# One start, four random SPR moves from the tree the alignment evolved down, from which NNI hill
# climbing (nni_search_ref.reference_search) takes one move and stops far below where the SPR
# search ends after two: the optimised tree has inner edges on the lower bound, across which
# both NNI neighbours score as the tree itself.
NNI_BELOW_SPR = Case("nni-below-spr", 8, 200, "JC69", "constant", 404, (4,))
