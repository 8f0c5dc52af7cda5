"""The inputs of tests/test_placement_gpu.py and their placement_ref references (TEST
INFRASTRUCTURE ONLY), in the manner of ancestral_cases.py, whose trees, model rows and engines
they use.  tests/test_placement_ref.py reads the same inputs on the CPU."""
import functools
from types import SimpleNamespace

import numpy as np

import ancestral_cases as AC
import placement_ref as R
import tree_utils as TU

SHAPES = ("n3", "n4", "n5", "balanced8", "ladder9", "random12")
SUBSTS = ("JC69", "GTR")
KS = (1, 4)
PS = (13, 64, 65, 129)
T = 3
Q = 67  # one wave-multiple plus a tail
PENDANTS = (0.02, 0.3)


def topologies(name, rng):
    if name == "n3":
        return np.stack([np.array([3, 3, 3], np.int32)] * T)
    return AC.topologies(name, rng)


def queries(x, rng, count, col):
    """[count][C] int8: row 0 copies taxon 0, row 1 is all gaps, row 2 one state throughout, the
    others random with a tenth of gaps."""
    C = len(col)
    q = rng.integers(0, 4, size=(count, C)).astype(np.int8)
    q[rng.random((count, C)) < 0.1] = 4
    taxon0 = x.states[0] if x.states is not None else np.argmax(x.vectors[0], axis=1)
    q[0] = np.minimum(taxon0[col], 4)
    if count > 1:
        q[1] = 4
    if count > 2:
        q[2] = 2
    return q


def all_gap(q):
    """[Q] bool: the query rows that are gaps throughout."""
    q = np.asarray(q)
    return np.all((q < 0) | (q > 3), axis=1)


def site_map(P, rng):
    """A site-level column map with C = 2 P + 7: patterns repeat, pattern P // 2 is never
    referenced, some weights are 0 or non-integer."""
    C = 2 * P + 7
    allowed = np.array([p for p in range(P) if p != P // 2], np.int32)
    col = rng.choice(allowed, size=C).astype(np.int32)
    col[:len(allowed)] = rng.permutation(allowed)  # every other pattern at least once
    w = rng.choice([0.0, 1.0, 1.0, 2.0, 0.5, 2.25], size=C)
    w[:3] = (0.0, 1.0, 0.75)
    return col, w


def _with_queries(x, rng, count=Q):
    x.col_site, x.w_site = site_map(x.P, rng)
    x.q_identity = queries(x, rng, count, np.arange(x.P))
    x.q_site = queries(x, rng, count, x.col_site)
    x.pendants = np.array(PENDANTS)
    return x


@functools.lru_cache(maxsize=None)
def parity(name, subst, K, P):
    """Compact tip states with gaps, random unequal branch lengths, T trees.  Read-only."""
    seed = 17000 + 1000 * SHAPES.index(name) + 100 * SUBSTS.index(subst) + 10 * K + PS.index(P)
    rng = np.random.default_rng(seed)
    pids = topologies(name, rng)
    n = (pids.shape[1] + 3) // 2
    states, w = TU.random_alignment(n, P, rng)
    bls = rng.uniform(0.01, 0.5, size=(T, 2 * n - 2))
    bls[:, -1] = 0.0
    x = AC._finish(name, subst, K, states, R.tip_vectors(states, np.float64), w, pids, bls, rng)
    return _with_queries(x, rng)


@functools.lru_cache(maxsize=None)
def partials(name, form):
    """ancestral_cases.partials' tip vectors (0/1 masks, real values), GTR, four categories."""
    x = SimpleNamespace(**vars(AC.partials(name, "GTR", 4, form)))
    return _with_queries(x, np.random.default_rng(18000 + SHAPES.index(name) + 10 * (form == "real")))


@functools.lru_cache(maxsize=None)
def ladder200():
    x = SimpleNamespace(**vars(AC.ladder200()))
    return _with_queries(x, np.random.default_rng(19001), count=3)


def maps(x):
    """(label, queries, column_pattern or None, column_weights or None) of the two column maps."""
    return (("identity", x.q_identity, None, None), ("site", x.q_site, x.col_site, x.w_site))


def resolved(x, col, w):
    """The column map and weights a call with (col, w) uses."""
    return (np.arange(x.P), x.w) if col is None else (col, w)


def tables(x, t, pendants=None, dtype=R.LD, form="insertion"):
    pend = x.pendants if pendants is None else pendants
    args = (x.pids[t], x.bls[t], *AC.model(x, t, dtype), x.vectors, pend)
    if form == "insertion":
        return R.insertion_tables(*args, dtype=dtype)[0]
    return R.formula_tables(*args, dtype=dtype)[0]


@functools.lru_cache(maxsize=None)
def parity_tables(name, subst, K, P):
    x = parity(name, subst, K, P)
    return [tables(x, t) for t in range(T)]


@functools.lru_cache(maxsize=None)
def partials_tables(name, form):
    x = partials(name, form)
    return [tables(x, t) for t in range(len(x.pids))]


def log_likelihood(x, t):
    lik = R.pattern_lik(x.pids[t], x.bls[t], *AC.model(x, t), x.vectors)
    return float(np.sum(np.asarray(x.w, R.LD) * np.log(lik)))


def check_result(res, x, S, queries_, col, w, label, tables_out=True):
    """A Placement of one case and column map against the reference tables S (per tree).  Prints
    the figures, then asserts.  Returns the share of best_edge / pendant_index entries left out."""
    col, w = resolved(x, col, w)
    worst = dict(ll=0.0, tab=0.0, lwr=0.0, rows=0.0, out=0.0)
    fails = []
    for t in range(len(S)):
        ref_ll = R.score(S[t], queries_, col, w)
        ref = R.summarise(ref_ll)
        scale = float(np.max(np.abs(ref.edge_ll)))
        delta = R.REL * scale
        got = res.edge_log_likelihoods[t]
        err = float(np.max(np.abs(got - ref.edge_ll) / np.abs(ref.edge_ll)))
        worst["ll"] = max(worst["ll"], err)
        if not err <= R.REL:
            fails.append(f"{label} tree {t}: edge_ll off by {err:.3e} relative")
        if tables_out and res.tables is not None:
            finite = np.isfinite(S[t])
            terr = float(np.max(np.abs(res.tables[t][finite] - S[t][finite]) / np.abs(S[t][finite])))
            worst["tab"] = max(worst["tab"], terr)
            if not (terr <= R.REL and np.array_equal(res.tables[t][~finite], S[t][~finite].astype(np.float64))):
                fails.append(f"{label} tree {t}: table off by {terr:.3e} relative")
        # The ranks wherever the reference's top two differ by more than the tolerance implies.
        # An all-gap query is apart: by definition it scores sum_c w_c s on every edge and pendant
        # length, an exact tie, so its row must come back as one value bit for bit, with the lowest
        # index as pendant length and as best edge; it is neither compared by margin nor counted.
        tied = all_gap(queries_)
        if not (np.all(got[tied] == got[tied][:, :1]) and np.all(res.best_edge[t][tied] == 0) and
                (res.pendant_index is None or np.all(res.pendant_index[t][tied] == 0))):
            fails.append(f"{label} tree {t}: an all-gap query is no exact tie resolved to index 0")
        sure_e = (ref.edge_gap > 2 * delta) & ~tied
        sure_g = (ref.pendant_gap > 2 * delta) & ~tied[:, None]
        left = max(1.0 - np.mean(sure_e[~tied]), 1.0 - np.mean(sure_g[~tied]))
        worst["out"] = max(worst["out"], float(left))
        if not np.array_equal(res.best_edge[t][sure_e], ref.best_edge[sure_e]):
            fails.append(f"{label} tree {t}: best_edge differs")
        if res.pendant_index is not None and \
                not np.array_equal(res.pendant_index[t][sure_g], ref.pendant_index[sure_g]):
            fails.append(f"{label} tree {t}: pendant_index differs")
        if res.lwr is not None:
            lref = ref.lwr.astype(np.float64)
            over = np.abs(res.lwr[t] - lref) - (2 * delta * lref + 2.0 ** -50)
            worst["lwr"] = max(worst["lwr"], float(np.max(np.abs(res.lwr[t] - lref))))
            rows = float(np.max(np.abs(np.sum(res.lwr[t], axis=1) - 1.0)))
            worst["rows"] = max(worst["rows"], rows)
            if not np.all(over <= 0):
                fails.append(f"{label} tree {t}: lwr beyond 2 delta ref + 2^-50 by {float(np.max(over)):.3e}")
            if not rows <= 2 * ref.edge_ll.shape[1] * 2.0 ** -53:
                fails.append(f"{label} tree {t}: lwr rows sum to 1 +- {rows:.3e}")
        ll = log_likelihood(x, t)
        if not abs(res.log_likelihoods[t] - ll) <= R.REL * abs(ll):
            fails.append(f"{label} tree {t}: log-likelihood {res.log_likelihoods[t]} against {ll}")
    print(f"{label}: edge_ll relative {worst['ll']:.2e}, table relative {worst['tab']:.2e}, |lwr - ref| "
          f"{worst['lwr']:.2e}, |row sum - 1| {worst['rows']:.2e}, ranks left out {100 * worst['out']:.3f} %")
    assert worst["out"] <= R.EXCLUDED, label
    assert not fails, fails
    return worst["out"]
