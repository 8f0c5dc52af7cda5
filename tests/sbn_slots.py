"""The linear-time slot and region-sum formulation of subsplit Bayesian networks (include/mi_phylo.h,
DESIGN.md 4.21) in plain Python: what the engine's kernels do, written a second time.  A tree's
PCSP occurrences are the slots (d, k) of its directed edges d = 2v + s; all 2n-3 rootings cost one
ascending and one descending pass, and so do the expected usages.  tests/test_sbn_ref.py holds it
against the brute force of tests/sbn_ref.py; the GPU tests compare with sbn_ref alone."""
import math

NEG_INF = float("-inf")


def _lse(*xs):
    m = max(xs)
    if m == NEG_INF:
        return NEG_INF
    return m + math.log(math.fsum(math.exp(x - m) for x in xs))


class Tree:
    def __init__(self, pid):
        self.pid = pid = [int(p) for p in pid]
        self.E = E = len(pid)
        self.n = n = (E + 3) // 2
        self.root = E
        self.kids = [[] for _ in range(E + 1)]
        for v in range(E):
            self.kids[pid[v]].append(v)
        self.below = [frozenset([v]) if v < n else frozenset() for v in range(E + 1)]
        for v in range(E):
            self.below[pid[v]] |= self.below[v]
        self.all = frozenset(range(n))

    def clade(self, d):
        v, s = d >> 1, d & 1
        return self.below[v] if s == 0 else self.all - self.below[v]

    def others(self, v):
        """The two other neighbours of parent(v), as directed edges away from it: the sibling then
        the edge above the parent; under the root the two siblings in ascending id."""
        p = self.pid[v]
        sibs = [2 * c for c in self.kids[p] if c != v]
        return sibs if p == self.root else sibs + [2 * p + 1]

    def focal_children(self, d):
        """The two child directed edges of d (empty for a leaf clade)."""
        v, s = d >> 1, d & 1
        if s == 0:
            return [2 * c for c in self.kids[v]]
        return self.others(v)

    def sisters(self, d):
        """[k] the sister's directed edge of slot (d, k), and the directed edge whose region uses
        the slot (None for k = 0: the rooting on the edge itself)."""
        v, s = d >> 1, d & 1
        if len(self.clade(d)) < 2:
            return []
        out = [(d ^ 1, None)]
        far = self.others(v) if s == 0 else [2 * c for c in self.kids[v]]
        if len(far) == 2:
            out += [(far[0], far[1]), (far[1], far[0])]
        return out

    def slots(self):
        """{(d, k): (sister, focal, child) as frozensets}."""
        out = {}
        for d in range(2 * self.E):
            for k, (sis, _) in enumerate(self.sisters(d)):
                c0, c1 = [self.clade(c) for c in self.focal_children(d)]
                focal = self.clade(d)
                child = c1 if min(focal) in c0 else c0
                out[(d, k)] = (self.clade(sis), focal, child)
        return out

    def sibling_slot(self, parent_d, c):
        """k_c: the slot of child directed edge c of parent_d whose sister is c's sibling."""
        sib = [x for x in self.focal_children(parent_d) if x != c][0]
        return [sis for sis, _ in self.sisters(c)].index(sib)

    def walk(self, root_theta, slot_theta):
        """log p of every rooting: root_theta [E], slot_theta {(d, k): theta}."""
        E = self.E
        B = [0.0] * (2 * E)
        order = [2 * v for v in range(E)] + [2 * v + 1 for v in reversed(range(E))]
        for d in order:
            if len(self.clade(d)) < 2:
                continue
            for c in self.focal_children(d):
                if len(self.clade(c)) >= 2:
                    B[d] += slot_theta[(c, self.sibling_slot(d, c))] + B[c]

        def A0(d):
            return slot_theta[(d, 0)] + B[d] if len(self.clade(d)) >= 2 else 0.0
        return [root_theta[v] + A0(2 * v) + A0(2 * v + 1) for v in range(E)]

    def usage(self, log_rho):
        """(root usage [E], {(d, k): log usage}) from the rootings' log weights: region sums."""
        E = self.E
        R = [NEG_INF] * (2 * E)  # log sum of rho over the edges of d's focal side, its own included
        for v in range(E):
            R[2 * v] = _lse(log_rho[v], *[R[2 * c] for c in self.kids[v]])
        for v in reversed(range(E)):
            R[2 * v + 1] = _lse(log_rho[v], *[R[x] for x in self.others(v)])
        out = {}
        for d in range(2 * E):
            for k, (_, region) in enumerate(self.sisters(d)):
                out[(d, k)] = log_rho[d >> 1] if region is None else R[region]
        return list(log_rho), out
