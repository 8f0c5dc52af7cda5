"""Subsplit Bayesian networks of unrooted trees in plain Python, by brute force:
a clade is a frozenset of leaves, every rooting of every tree is enumerated, features live in
dicts, sums are math.fsum.  Restates the reference's UnrootedSBNMaps (src/sbn_maps.cpp) and
SimpleAverage / ExpectationMaximization / ProbabilityOfSingle (src/sbn_probability.cpp) and
shares no structure with the engine's kernels: there are no slots and no region sums here.

A feature is ("r", split) for a rootsplit (the minorised split, never leaf 0) or
(sister, focal, child) for a PCSP.  The numbering is the engine's (include/mi_phylo.h): rootsplits
by first occurrence in (tree, edge) order; PCSPs in blocks per parent (sister | focal), blocks by
the parent's first occurrence in (tree, directed edge, sister) order, children within a block by
their own first occurrence."""
import math

NEG_INF = float("-inf")


def taxon_count(pid):
    return (len(pid) + 3) // 2


def _neighbours(pid):
    root = len(pid)
    adj = [[] for _ in range(root + 1)]
    for v in range(root):
        adj[v].append(int(pid[v]))
        adj[int(pid[v])].append(v)
    return adj


def _side(adj, n, x, up, memo=None):
    """The leaves reached from x without passing through `up` (memo: a dict per tree)."""
    if x < n:
        return frozenset([x])
    if memo is not None and (x, up) in memo:
        return memo[(x, up)]
    out = frozenset()
    for y in adj[x]:
        if y != up:
            out |= _side(adj, n, y, x, memo)
    if memo is not None:
        memo[(x, up)] = out
    return out


def _minor_child(c0, c1):
    """std::min of the two child bitsets (taxon 0 first): the one without the lowest taxon."""
    return c1 if min(c0) < min(c1) else c0


def _minorise(clade, n):
    return frozenset(range(n)) - clade if 0 in clade else clade


def rooted_features(pid, v, memo=None, adj=None):
    """The features of the tree rooted on edge v (between v and its parent): the rootsplit first,
    then the PCSPs (the reference's RootedIndexerRepresentation, as features)."""
    n = taxon_count(pid)
    adj = _neighbours(pid) if adj is None else adj
    p = int(pid[v])
    memo = {} if memo is None else memo
    below, above = _side(adj, n, v, p, memo), _side(adj, n, p, v, memo)
    out = [("r", _minorise(below, n))]

    def descend(x, up, sister):
        if x < n:
            return
        c0, c1 = [y for y in adj[x] if y != up]
        s0, s1 = _side(adj, n, c0, x, memo), _side(adj, n, c1, x, memo)
        out.append((sister, _side(adj, n, x, up, memo), _minor_child(s0, s1)))
        descend(c0, x, s1)
        descend(c1, x, s0)

    descend(v, p, above)
    descend(p, v, below)
    return out


def tree_features(pid):
    """[2n-3] feature lists, one per rooting (UnrootedIndexerRepresentation, as features)."""
    memo, adj = {}, _neighbours(pid)
    return [rooted_features(pid, v, memo, adj) for v in range(len(pid))]


def ordered_pcsps(pid):
    """Every PCSP occurrence of a tree in the header's (directed edge d = 2v + s, sister k) order,
    from the clade sets alone: [(d, k, feature)]."""
    n = taxon_count(pid)
    adj = _neighbours(pid)
    root = len(pid)
    out, memo = [], {}
    for v in range(root):
        p = int(pid[v])
        for s in (0, 1):
            focal_node, far = (v, p) if s == 0 else (p, v)
            focal = _side(adj, n, focal_node, far, memo)
            if len(focal) < 2:
                continue
            c0, c1 = [y for y in adj[focal_node] if y != far]
            child = _minor_child(_side(adj, n, c0, focal_node, memo), _side(adj, n, c1, focal_node, memo))
            sisters = [frozenset(range(n)) - focal]
            if far >= n:
                others = [y for y in adj[far] if y != focal_node]
                if s == 0 and far != root:
                    # the sibling, then the clade above the parent
                    others = [y for y in others if y != int(pid[far])] + [int(pid[far])]
                else:
                    others.sort()
                sisters += [_side(adj, n, y, far, memo) for y in others]
            for k, sister in enumerate(sisters):
                out.append((2 * v + s, k, (sister, focal, child)))
    return out


class Support:
    """The numbered support of trees 0 .. T0-1 and the representation of all T trees."""

    def __init__(self, pids, support_tree_count=None):
        self.pids = [list(map(int, p)) for p in pids]
        self.n = taxon_count(self.pids[0])
        T0 = len(self.pids) if support_tree_count is None else support_tree_count
        self.rootsplits = []                 # [S] frozensets
        number = {}
        first_parent, children = {}, {}      # parent -> order, parent -> [child feature]
        features = [tree_features(p) for p in self.pids]
        for t in range(T0):
            for feats in features[t]:
                if feats[0] not in number:
                    number[feats[0]] = len(self.rootsplits)
                    self.rootsplits.append(feats[0][1])
            for d, k, f in ordered_pcsps(self.pids[t]):
                parent = f[:2]
                if parent not in first_parent:
                    first_parent[parent] = len(first_parent)
                    children[parent] = []
                if f not in children[parent]:
                    children[parent].append(f)
        self.S = len(self.rootsplits)
        self.pcsps, self.parent_range, self.pcsp_parent = [], [], []
        for parent, _ in sorted(first_parent.items(), key=lambda kv: kv[1]):
            begin = self.S + len(self.pcsps)
            for f in children[parent]:
                number[f] = self.S + len(self.pcsps)
                self.pcsps.append(f)
                self.pcsp_parent.append(len(self.parent_range))
            self.parent_range.append((begin, self.S + len(self.pcsps)))
        self.C = len(self.pcsps)
        self.P = self.S + self.C
        self.number = number
        # [T][2n-3] index lists, the sentinel P for what the support lacks
        self.reps = [[[number.get(f, self.P) for f in feats] for feats in tree] for tree in features]

    def clade_string(self, clade):
        return "".join("1" if i in clade else "0" for i in range(self.n))

    def strings(self):
        """The reference's pretty indexer: "01110" and "00001|11110|01110"."""
        return [self.clade_string(s) for s in self.rootsplits] + \
               ["|".join(self.clade_string(c) for c in f) for f in self.pcsps]

    def blocks(self):
        return [(0, self.S)] + list(self.parent_range)


def logsumexp(xs):
    xs = list(xs)
    m = max(xs) if xs else NEG_INF
    if m == NEG_INF:
        return NEG_INF
    return m + math.log(math.fsum(math.exp(x - m) for x in xs))


def normalize(log_params, blocks):
    """ProbabilityNormalizeParamsInLog: every block minus its logsumexp."""
    out = list(log_params)
    for b, e in blocks:
        z = logsumexp(out[b:e])
        for j in range(b, e):
            out[j] = out[j] - z if z != NEG_INF else NEG_INF
    return out


def rooting_log_probs(rep, theta):
    """[2n-3] log p of every rooting; -inf where the rooting touches the sentinel."""
    P = len(theta)
    out = []
    for r in rep:
        if any(j == P or theta[j] == NEG_INF for j in r):
            out.append(NEG_INF)
        else:
            out.append(math.fsum(theta[j] for j in r))
    return out


def log_prob(reps, theta):
    """(rooting log probabilities [T][2n-3], log q [T])."""
    lp = [rooting_log_probs(rep, theta) for rep in reps]
    return lp, [logsumexp(row) for row in lp]


def log_expected_counts(reps, theta, weights):
    """[P] log sum_t w_t sum_v rho_tv [j in rep_tv]; a tree with log q = -inf adds nothing."""
    P = len(theta)
    terms = [[] for _ in range(P)]
    lp, lq = log_prob(reps, theta)
    for t, rep in enumerate(reps):
        if lq[t] == NEG_INF or weights[t] == 0:
            continue
        for v, r in enumerate(rep):
            if lp[t][v] == NEG_INF:
                continue
            x = lp[t][v] - lq[t] + math.log(weights[t])
            for j in r:
                terms[j].append(x)
    return [logsumexp(x) for x in terms]


def log_counts(reps, P, weights):
    """SetLogCounts: log of the weighted number of rootings that use each parameter."""
    counts = [0.0] * P
    for t, rep in enumerate(reps):
        for r in rep:
            for j in r:
                counts[j] += weights[t]
    return [math.log(c) if c > 0 else NEG_INF for c in counts]


def train(support, weights=None, method="sa", alpha=0.0, max_iter=1, score_epsilon=0.0, T0=None):
    """SimpleAverage / ExpectationMaximization on the support's own trees: (normalised log
    parameters [P], score history)."""
    reps = support.reps if T0 is None else support.reps[:T0]
    w = [1.0] * len(reps) if weights is None else [float(x) for x in weights]
    P, blocks = support.P, support.blocks()
    E = len(reps[0])
    log_m_tilde = log_counts(reps, P, w)
    if method == "sa":
        return normalize(log_m_tilde, blocks), []
    log_m_tilde = [x - math.log(E) for x in log_m_tilde]
    theta = normalize(log_m_tilde, blocks)
    if alpha > 0:
        log_m_tilde = [x + math.log(alpha) for x in log_m_tilde]
        m_tilde = [math.exp(x) for x in log_m_tilde]
    history = []
    for it in range(max_iter):
        _, lq = log_prob(reps, theta)
        score = math.fsum(w[t] * lq[t] for t in range(len(reps)))
        log_m_bar = log_expected_counts(reps, theta, w)
        if alpha > 0:
            log_m_bar = [logsumexp([a, b]) for a, b in zip(log_m_bar, log_m_tilde)]
        theta = normalize(log_m_bar, blocks)
        if alpha > 0:
            score += math.fsum(m * x for m, x in zip(m_tilde, theta) if m != 0.0)
        history.append(score)
        if it > 0:
            gain = (history[it] - history[it - 1]) / abs(history[it - 1])
            assert gain > -1e-10, "Score function decreased."
            if abs(gain) < score_epsilon:
                break
    return theta, history


def caterpillar(n):
    """Parent ids [2n-3] of the caterpillar ((..((0,1),2)..), n-2, n-1): the deepest chain."""
    pid = [0] * (2 * n - 3)
    if n == 3:
        return [3, 3, 3]
    pid[0] = pid[1] = n
    for i in range(2, n - 2):
        pid[i] = n + i - 1
        pid[n + i - 2] = n + i - 1
    pid[n - 2] = pid[n - 1] = pid[2 * n - 4] = 2 * n - 3
    return pid


def balanced(n):
    """Parent ids [2n-3] of a balanced tree: the two oldest open nodes are joined in turn."""
    pid, open_nodes, nxt = [0] * (2 * n - 3), list(range(n)), n
    while len(open_nodes) > 3:
        a, b = open_nodes.pop(0), open_nodes.pop(0)
        pid[a] = pid[b] = nxt
        open_nodes.append(nxt)
        nxt += 1
    for x in open_nodes:
        pid[x] = 2 * n - 3
    return pid
