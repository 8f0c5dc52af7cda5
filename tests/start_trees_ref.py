"""A plain reference for the starting-tree calls (TEST INFRASTRUCTURE ONLY; numpy only):
substitution counts of all pairs of taxa by integer arithmetic, the pair likelihood l(t) and its
two derivatives in np.longdouble with the transition matrices of tests/dense_ref.py (Taylor
series, no eigensystem), its maximiser, and neighbour joining by the rule of include/mi_phylo.h
in IEEE doubles, numbered by tree_utils._polish."""
import sys

import numpy as np

import dense_ref as D
import tree_utils as TU

LD = np.longdouble


# ---- counts ----

def codes_from_partials(partials):
    """[n][P][4] tip vectors -> [n][P] codes: a where the vector is exactly the unit vector e_a,
    4 (missing) for everything else (gaps, 0/1 masks, real values)."""
    p = np.asarray(partials, np.float64)
    unit = ((p == 1.0).sum(-1) == 1) & ((p == 0.0).sum(-1) == 3)
    return np.where(unit, np.argmax(p, -1), 4).astype(np.int64)


def pair_counts(codes, W):
    """codes [n][P] (0..3, anything else missing), W [B][P] integer weights -> int64
    [B][n(n-1)/2][4][4]: N[r][(i, j)][a][b] = sum_p W[r][p] [code_i(p) = a][code_j(p) = b], pairs
    in lexicographic (i, j) order."""
    codes = np.asarray(codes)
    W = np.asarray(W)
    assert np.array_equal(W, np.rint(W))
    Wi = W.astype(np.int64)
    n = codes.shape[0]
    onehot = np.stack([(codes == a) for a in range(4)], 1).astype(np.int64)  # [n][4][P]
    out = np.zeros((Wi.shape[0], n * (n - 1) // 2, 4, 4), np.int64)
    q = 0
    for i in range(n):
        for j in range(i + 1, n):
            # [B][4][4] = sum_p W[b][p] X_i[a][p] X_j[b][p]
            out[:, q] = np.einsum("rp,ap,bp->rab", Wi, onehot[i], onehot[j])
            q += 1
    return out


def pair_index(n):
    return [(i, j) for i in range(n) for j in range(i + 1, n)]


# ---- the pair likelihood ----

def weibull_categories(K, shape):
    """Rates and weights of the discretised Weibull site model (mean rate 1): the quantile
    midpoints (2 i + 1) / (2 K)."""
    q = (2.0 * np.arange(K) + 1.0) / (2.0 * K)
    r = (-np.log(1.0 - q)) ** (1.0 / shape)
    return r / r.mean(), np.full(K, 1.0 / K)


class PairLikelihood:
    """l(t) = sum_ab N[a][b] log sum_k c_k P_ab(r_k t) with its first two derivatives, long double."""

    def __init__(self, rates6, freqs4, cat_rates, cat_weights):
        self.Q, _ = D.gtr_q(rates6, freqs4)
        self.r = np.asarray(cat_rates, LD)
        self.c = np.asarray(cat_weights, LD)

    def matrices(self, t):
        """(L, L', L'') [4][4] at t."""
        t = LD(t)
        L = np.zeros((4, 4), LD)
        L1, L2 = L.copy(), L.copy()
        for r, c in zip(self.r, self.c):
            P = D.expm(self.Q * (r * t))
            rq = self.Q * r
            L += c * P
            L1 += c * (rq @ P)
            L2 += c * (rq @ rq @ P)
        return L, L1, L2

    @staticmethod
    def from_matrices(N, mats):
        """(l, l', l'') of one count matrix (zero counts add nothing)."""
        L, L1, L2 = mats
        N = np.asarray(N, LD).reshape(4, 4)
        on = N != 0
        q = L1[on] / L[on]
        return (np.sum(N[on] * np.log(L[on])), np.sum(N[on] * q), np.sum(N[on] * (L2[on] / L[on] - q * q)))

    def derivatives(self, N, t):
        return self.from_matrices(N, self.matrices(t))

    def maximiser(self, N, tmin=1e-8, tmax=10.0):
        """argmax of l over [tmin, tmax] by bisection on the sign of l' with Newton steps where they
        stay inside, to long-double precision; a bound where l' does not change sign; tmax
        without data."""
        N = np.asarray(N, LD)
        if N.sum() == 0:
            return LD(tmax)
        if self.derivatives(N, tmin)[1] <= 0:
            return LD(tmin)
        if self.derivatives(N, tmax)[1] >= 0:
            return LD(tmax)
        lo, hi = LD(tmin), LD(tmax)
        t = LD(0.5) * (lo + hi)
        for _ in range(200):
            _, g, h = self.derivatives(N, t)
            if g > 0:
                lo = t
            elif g < 0:
                hi = t
            else:
                return t
            nxt = t - g / h if h < 0 else lo
            if not (lo < nxt < hi):
                nxt = LD(0.5) * (lo + hi)
            if abs(nxt - t) <= LD(1e-17) * t:
                return nxt
            t = nxt
        return t


def jc69_distance(share):
    """The closed form of the JC69 maximiser from the mismatch share (share < 3/4)."""
    return -0.75 * np.log1p(-LD(share) * 4 / 3)


# ---- neighbour joining ----

def neighbour_joining(d, min_length=1e-8, max_length=10.0, margins=None, fused=False):
    """One matrix [n][n] (i < j read) -> (parent ids [2n-3], branch lengths [2n-2]) by the rule of
    include/mi_phylo.h, numbered by tree_utils._polish; lengths clamped on the way out.
    margins: a list that receives per round the relative margin between the best and the
    second-best Q, (q2 - q1) / max over the two of ((r-2) d_ij + R_i + R_j).  (With four
    clusters left Q(a, b) = Q(c, d) identically, and either join gives the same unrooted tree:
    the complementary pair is not a rival there.)
    fused: NOT the rule -- (r-2) d - R_i rounded once, as a fused multiply-add computes it: what an
    implementation that contracts the product into the subtraction would return (small n only)."""
    d = np.asarray(d, np.float64)
    n = d.shape[0]
    D_ = np.triu(d, 1)
    D_ = D_ + D_.T
    live = list(range(n))
    sub = {i: i for i in range(n)}  # slot -> its cluster as nested tuples (what _polish numbers)
    label = {i: i for i in range(n)}  # slot -> its cluster's label: a leaf id, or n + join number
    kids, length = {}, {}             # by label: the two clusters joined, the raw branch length
    for r in range(n, 3, -1):
        idx = np.array(live)
        R = np.zeros(n)
        for k in live:  # ascending: one rounding per addition (k = i adds the diagonal's 0.0)
            R[idx] = R[idx] + D_[k, idx]
        sub_d = D_[np.ix_(idx, idx)]
        Q = ((r - 2.0) * sub_d - R[idx][:, None]) - R[idx][None, :]
        if fused:
            from fractions import Fraction
            Q = np.array([[float(Fraction(r - 2) * Fraction(float(sub_d[x, y])) - Fraction(float(R[idx[x]])))
                           for y in range(len(idx))] for x in range(len(idx))]) - R[idx][None, :]
        upper = np.triu(np.ones_like(Q, bool), 1)
        Qm = np.where(upper, Q, np.inf)
        flat = int(np.argmin(Qm))  # the first minimum in row-major order: the lowest (i, j)
        a, b = divmod(flat, len(idx))
        if margins is not None and upper.sum() > 1:
            scale = (r - 2.0) * sub_d + R[idx][:, None] + R[idx][None, :]
            rest = Qm.copy()
            rest[a, b] = np.inf
            if r == 4:
                c, e = (k for k in range(4) if k not in (a, b))
                rest[c, e] = np.inf
            a2, b2 = divmod(int(np.argmin(rest)), len(idx))
            margins.append((rest[a2, b2] - Qm[a, b]) / max(scale[a, b], scale[a2, b2], np.finfo(float).tiny))
        i, j = int(idx[a]), int(idx[b])
        dij = D_[i, j]
        di = dij / 2.0 + (R[i] - R[j]) / (2.0 * (r - 2.0))
        dj = dij - di
        length[label[i]], length[label[j]] = di, dj
        others = np.array([k for k in live if k != i and k != j])
        v = ((D_[i, others] + D_[j, others]) - dij) / 2.0
        D_[i, others] = v
        D_[others, i] = v
        sub[i] = (sub[i], sub[j])
        kids[2 * n - r] = (label[i], label[j])
        label[i] = 2 * n - r
        live.remove(j)
    a, b, c = live
    ab, ac, bc = D_[a, b], D_[a, c], D_[b, c]
    length[label[a]] = ((ab + ac) - bc) / 2.0
    length[label[b]] = ((bc + ab) - ac) / 2.0
    length[label[c]] = ((ac + bc) - ab) / 2.0
    tree = (sub[a], sub[b], sub[c])
    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(limit, 20 * n + 1000))
    try:
        pid = TU._polish(tree, n)
        # lengths by the final ids: walk the labelled tree the way _polish walks the nested one
        bl = np.zeros(2 * n - 2)
        next_id = [n]

        top = {}

        def maxleaf(lb):
            if lb not in top:
                top[lb] = lb if lb < n else max(maxleaf(k) for k in kids[lb])
            return top[lb]

        def visit(lb):
            if lb < n:
                me = lb
            else:
                for kid in sorted(kids[lb], key=maxleaf):
                    visit(kid)
                me = next_id[0]
                next_id[0] += 1
            bl[me] = length[lb]
            return me

        for lb in sorted((label[a], label[b], label[c]), key=maxleaf):
            visit(lb)
    finally:
        sys.setrecursionlimit(limit)
    bl[: 2 * n - 3] = np.clip(bl[: 2 * n - 3], min_length, max_length)
    return pid, bl



def first_join(d, fused=False):
    """The pair (i, j) the first round joins.  fused: (r-2) d - R_i rounded ONCE (exact rational
    arithmetic, then one rounding: what a fused multiply-add computes) instead of the rule's
    rounded product and rounded difference."""
    from fractions import Fraction
    d = np.asarray(d, np.float64)
    n = d.shape[0]
    R = np.zeros(n)
    for k in range(n):
        R = R + d[k]
    best = None
    for i in range(n):
        for j in range(i + 1, n):
            if fused:
                q1 = float(Fraction(n - 2) * Fraction(float(d[i, j])) - Fraction(float(R[i])))
            else:
                q1 = (n - 2.0) * d[i, j] - R[i]
            q = q1 - R[j]
            if best is None or q < best[0]:
                best = (q, i, j)
    return best[1:]


def path_lengths(parent_ids, bl):
    """The leaf-to-leaf path-length matrix [n][n] of an unrooted tree in the reference's form."""
    pid = np.asarray(parent_ids)
    n = (len(pid) + 3) // 2
    root = 2 * n - 3
    anc = []
    for leaf in range(n):
        chain, v, s = {}, leaf, 0.0
        while v != root:
            s += bl[v]
            v = int(pid[v])
            chain[v] = s
        anc.append(chain)
    d = np.zeros((n, n))
    for i in range(n):
        for j in range(i + 1, n):
            best = min(anc[i][v] + anc[j][v] for v in anc[i] if v in anc[j])
            d[i, j] = d[j, i] = best
    return d


def splits(parent_ids, bl):
    """The unrooted tree as {split: branch length}: per edge the set of leaves on the side that
    does not hold leaf 0 (where the trifurcation sits plays no part)."""
    pid = np.asarray(parent_ids)
    n = (len(pid) + 3) // 2
    below = [frozenset([v]) if v < n else frozenset() for v in range(2 * n - 2)]
    for v in range(2 * n - 3):  # a parent's id is above its children's
        below[int(pid[v])] = below[int(pid[v])] | below[v]
    everyone = frozenset(range(n))
    return {(everyone - below[v] if 0 in below[v] else below[v]): float(bl[v]) for v in range(2 * n - 3)}
