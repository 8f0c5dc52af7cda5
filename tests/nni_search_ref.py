"""An independent reference for the NNI hill-climbing search (mi_engine_nni_search_unrooted,
DESIGN.md 4.11), and the cases the tests run it on.

Per round and tree: the reference optimum of the branch lengths on the oracle
(branch_opt_ref.reference_optimum), the oracle's log-likelihood of every neighbour tree
(nni_ref.all_neighbours) at those lengths, and the public decision rule.  Nothing of the
library is used.  Every decision comes with its margin, min(best delta - second-best delta,
|best delta - min_gain|): how far the deltas would have to move for the search to go another
way.  tests/test_nni_search_ref.py checks on the CPU that the margins of the committed cases
are at least ten times what the deltas move by when the optimiser stops 100 times earlier."""
import functools

import numpy as np

import branch_opt_ref as R
import nni_ref as NR
import oracle_lib as O
import tree_utils as TU

LOCAL_OPTIMUM, MOVE_LIMIT = 0, 1
MIN_GAIN, LO, HI = 1e-3, 1e-8, 10.0  # the call's defaults
TIGHT, LOOSE = 1e-9, 1e-7            # the reference optimiser's criterion, and 100 times looser


class Decision:
    """One round of one tree: the deltas in code order from 2n, the move taken (-1: stopped)."""

    def __init__(self, n, delta, min_gain, log_likelihood):
        self.delta, self.log_likelihood = delta, log_likelihood
        self.code, self.best, self.margin = -1, 0.0, np.inf
        if len(delta):
            k = int(np.argmax(delta))  # (the first of equals: the lowest code)
            self.code, self.best = 2 * n + k, float(delta[k])
            rest = np.delete(delta, k)
            self.margin = min(self.best - float(rest.max()), abs(self.best - min_gain))


class SearchResult:
    def __init__(self):
        self.moves, self.gains, self.decisions = [], [], []
        self.parent_ids = self.branch_lengths = None
        self.log_likelihood, self.best_delta, self.status = 0.0, 0.0, LOCAL_OPTIMUM


def _optimum(spec, tips, w, pid, start, params, rescaling, tol):
    """Maximum-likelihood lengths of one tree: reference_optimum at the tight criterion; at a
    looser one its numpy method stopped there."""
    if tol == TIGHT:
        x, ll, _, _ = R.reference_optimum(spec, tips, w, pid, start, params, rescaling, LO, HI)
        return x, ll
    f = R.OracleTree(spec, tips, w, pid, params, rescaling, fixed_entry=start[-1])
    x = R._newton(f, np.clip(start[:-1], LO, HI), LO, HI, tol=tol)
    return np.append(x, start[-1]), float(f(x)[0][0])


def reference_search(spec, tips, w, pid, start, params, rescaling=False, min_gain=MIN_GAIN,
                     max_moves=100, tol=TIGHT):
    """The search from one tree (pid [2n-3], start [2n-2], params [C]) -> SearchResult."""
    n = spec.taxon_count
    pid, bl = np.array(pid, np.int32), np.array(start, float)
    out = SearchResult()
    while True:
        x, ll = _optimum(spec, tips, w, pid, bl, params, rescaling, tol)
        nb = NR.all_neighbours(n, pid, x)
        delta = np.empty(0)
        if nb:
            lls = O.unrooted_log_likelihoods(spec, tips, w, np.stack([p for _, _, p, _ in nb]),
                                             np.stack([b for _, _, _, b in nb]),
                                             np.repeat(np.asarray(params, float).reshape(1, -1), len(nb), axis=0),
                                             rescaling, min(8, len(nb)))
            delta = lls - ll
        d = Decision(n, delta, min_gain, ll)
        out.decisions.append(d)
        better = d.code >= 0 and d.best > min_gain
        if better and len(out.moves) < max_moves:
            out.moves.append(d.code)
            out.gains.append(d.best)
            _, _, pid, bl = nb[d.code - 2 * n]
            continue
        out.parent_ids, out.branch_lengths = pid, x
        out.log_likelihood, out.best_delta = ll, d.best
        out.status = MOVE_LIMIT if better else LOCAL_OPTIMUM
        return out


# ---- the cases ----

def evolved_alignment(pids, n, P, rng, change=0.08):
    """Tip states evolved down the tree (a state changes with probability `change` per branch),
    integer pattern weights: as tests/test_branch_opt_gpu.py builds its evolved cases."""
    root = 2 * n - 3
    states = np.zeros((root + 1, P), np.int32)
    states[root] = rng.integers(0, 4, size=P)
    for v in range(root - 1, -1, -1):
        flip = rng.random(P) < change
        states[v] = np.where(flip, rng.integers(0, 4, size=P), states[pids[v]])
    return states[:n].copy(), rng.integers(1, 6, size=P).astype(np.float64)


def random_nni_walk(n, pid, bl, steps, rng):
    """`steps` random NNI moves away from a tree (nni_ref.neighbour)."""
    for _ in range(steps):
        v = int(rng.integers(n, 2 * n - 3))
        pid, bl = NR.neighbour(n, pid, bl, v, int(rng.integers(0, 2)))
    return pid, bl


class Case:
    """An alignment evolved down a random tree, and start trees `away` random NNI moves from it."""

    def __init__(self, name, n, P, subst, site, seed, away):
        self.name, self.n, self.P, self.subst, self.site, self.seed, self.away = name, n, P, subst, site, seed, away

    def __repr__(self):
        return self.name

    @functools.lru_cache(maxsize=None)
    def build(self):
        """(spec, tips, weights, parent ids [T][2n-3], start lengths [T][2n-2], params [T][C])"""
        n, rng = self.n, np.random.default_rng(self.seed)
        true_pid = TU.random_topology(n, rng)
        tips, w = evolved_alignment(true_pid, n, self.P, rng)
        start = np.full(2 * n - 2, 0.1)
        start[-1] = 0.0
        pids = np.stack([random_nni_walk(n, true_pid, start, k, rng)[0] for k in self.away])
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
        return [reference_search(spec, tips, w, pids[t], start[t], pr[t], tol=tol, max_moves=max_moves)
                for t in range(len(pids))]


# n = 4 (one inner edge, u is the root), 5, 8, 12; one and four categories; JC69 and GTR; 100 to
# 300 patterns.  A seed whose case fails the margin check of tests/test_nni_search_ref.py is
# replaced here, never skipped at run time.
CASES = [
    Case("n4-jc-k1", 4, 100, "JC69", "constant", 101, (0, 1, 1)),
    Case("n5-jc-k4", 5, 150, "JC69", "weibull+4", 102, (0, 1, 2)),
    Case("n8-gtr-k1", 8, 200, "GTR", "constant", 103, (0, 2, 3)),
    Case("n8-jc-k4", 8, 250, "JC69", "weibull+4", 104, (1, 2, 4)),
    Case("n12-gtr-k4", 12, 300, "GTR", "weibull+4", 105, (0, 3, 5)),
    Case("n12-jc-k1", 12, 200, "JC69", "constant", 201, (2, 4, 6)),
]
