"""Reference of the variational fit over the rooted trees of the subsplit DAG (TEST INFRASTRUCTURE
ONLY; DESIGN.md 4.29, include/mi_phylo.h): the log-normalisation, the branch draw by entry, the
map from rooted node to unrooted edge, the reparametrisation terms, the per-entry ordered sums, the
factors and the topology gradient in plain Python floats, every sum in the order the header states.
One step is the composition of the library's by-value host calls followed by vi_fit_ref's update,
as tests/vi_fit_ref.py does for the unrooted fit."""
import copy
import math

import numpy as np

import branch_model_ref as B
import gp_ref as GR
import gp_trees_ref as TR
import sbn_vi_ref as V
import vi_fit_ref as F

HALF_LOG_2PI = 0.91893853320467274178


# ---------------------------------------------------------------- the topology side
def log_normalize(d, phi):
    """(log q [G], q [G]): per block, l_e = (phi_e - m) - log(sum_i exp(phi_i - m)) with the sum in
    ascending entry order and one accumulator; a block that is all -inf gets -inf and 0."""
    lq, q = np.empty(d.G), np.empty(d.G)
    for lo, hi in TR.blocks(d):
        m = -math.inf
        for i in range(lo, hi):
            x = float(phi[i])
            if math.isnan(x) or x == math.inf:
                raise ValueError(f"log parameter {i} is NaN or +inf")
            if x > m:
                m = x
        if m == -math.inf:
            lq[lo:hi], q[lo:hi] = -math.inf, 0.0
            continue
        s = 0.0
        for i in range(lo, hi):
            s = s + math.exp(float(phi[i]) - m)
        ls = math.log(s)
        for i in range(lo, hi):
            lq[i] = (float(phi[i]) - m) - ls
            q[i] = math.exp(lq[i])
    return lq, q


def log_q_topology(q, entries):
    """sum over v ascending of log q[entries[v]], one accumulator; -inf at a zero parameter"""
    lp = 0.0
    for e in entries:
        x = float(q[e])
        lp = lp + (-math.inf if x == 0.0 else math.log(x))
    return lp


def factors(log_f, estimator):
    if estimator == "given":
        return [float(x) for x in log_f]
    return V.plain_factors(list(log_f)) if estimator == "plain" else V.vimco_factors(list(log_f))


def block_of(d):
    """[G] the index of every entry's block in TR.blocks(d)"""
    out = np.empty(d.G, np.int64)
    for b, (lo, hi) in enumerate(TR.blocks(d)):
        out[lo:hi] = b
    return out


def topology_gradient(d, q, entries, a):
    """out[j] = G_j - q_j sum_{i in block(j)} G_i; G_j = sum_t a_t [tree t uses j], ascending t, one
    accumulator; the block's sum in ascending entry order.  Also the sum of |terms| per entry."""
    usage, mass = np.zeros(d.G), np.zeros(d.G)
    for t, row in enumerate(entries):
        for e in row:
            if 0 <= e < d.G:
                usage[e] = usage[e] + float(a[t])
                mass[e] += abs(float(a[t]))
    out, scale = np.zeros(d.G), np.zeros(d.G)
    for lo, hi in TR.blocks(d):
        total, total_mass = 0.0, 0.0
        for i in range(lo, hi):
            total = total + usage[i]
            total_mass += mass[i]
        for i in range(lo, hi):
            out[i] = usage[i] - float(q[i]) * total
            scale[i] = mass[i] + float(q[i]) * total_mass
    return out, scale


def grad_log_q(d, q, entries_of_one_tree):
    """the gradient of log q(tau) with respect to the unnormalised log parameters"""
    return topology_gradient(d, q, [entries_of_one_tree], [1.0])[0]


# ---------------------------------------------------------------- the branch side
def branch_sample(entries, q_params, seed, first_sample, rate, epsilon=None):
    """(lengths [T][N], epsilon [T][N-1], log q [T], log prior [T]): node v < N-1 of tree t draws from
    the variable of its entry; the root's slot has no length."""
    entries = np.atleast_2d(entries)
    T, N = entries.shape
    bl, eps_out, lq, lp = np.zeros((T, N)), np.zeros((T, N - 1)), np.zeros(T), np.zeros(T)
    for t in range(T):
        sum_q, sum_theta = 0.0, 0.0
        for v in range(N - 1):
            mu, sigma = (float(x) for x in q_params[entries[t, v]])
            eps = float(epsilon[t][v]) if epsilon is not None else B.normal(seed, first_sample + t, v)
            x = mu + sigma * eps
            theta = math.exp(x)
            sum_q = sum_q + (((x + math.log(sigma)) + HALF_LOG_2PI) + 0.5 * (eps * eps))
            sum_theta = sum_theta + theta
            bl[t, v], eps_out[t, v] = theta, eps
        lq[t] = -sum_q
        lp[t] = float(N - 1) * math.log(rate) - rate * sum_theta
    return bl, eps_out, lq, lp


def deroot_mapped(pid, bl=None):
    """TR.deroot plus new_id [2n-1]: the unrooted id under which every rooted node's edge lands; both
    root children map to the root edge, the root to -1.  Written apart from TR.deroot: the ids come
    from a walk that records them per rooted node."""
    n, kids, taxa = GR._tree_nodes(pid)
    root = 2 * n - 2
    a, b = kids[root]
    x, y = (a, b) if n - 1 in taxa[a] else (b, a)
    if x < n:
        x, y = y, x
    new_id, out, counter = np.full(2 * n - 1, -1, np.int32), np.full(2 * n - 3, -1, np.int32), [n]

    def visit(v):
        if v < n:
            return v
        below = sorted(list(kids[v]) + ([y] if v == x else []), key=lambda k: max(taxa[k]))
        ids = [visit(k) for k in below]
        me = counter[0]
        counter[0] += 1
        for k, i in zip(below, ids):
            out[i] = me
            new_id[k] = i
        return me

    assert visit(x) == 2 * n - 3
    new_id[x] = new_id[y]
    lengths = None
    if bl is not None:
        lengths = np.zeros(2 * n - 2)
        for v in range(2 * n - 2):   # (ascending v: the root edge is bl[min(x, y)] + bl[max(x, y)], a commutative sum)
            lengths[new_id[v]] = lengths[new_id[v]] + float(bl[v])
    return out, lengths, int(new_id[y]), new_id


def branch_terms(entries, q_params, lengths, eps, new_id, branch_gradient, rate, weights=None):
    """(c0, c1) [T][N-1]: c0 = w ((d theta) + 1), c1 = w ((((d theta) eps) + eps) + (1 / sigma)),
    d = branch_gradient[new_id] - rate"""
    entries = np.atleast_2d(entries)
    T, N = entries.shape
    c0, c1 = np.zeros((T, N - 1)), np.zeros((T, N - 1))
    for t in range(T):
        w = 1.0 if weights is None else float(weights[t])
        for v in range(N - 1):
            sigma = float(q_params[entries[t, v]][1])
            d = float(branch_gradient[t][new_id[t][v]]) - rate
            dt, e = d * float(lengths[t][v]), float(eps[t][v])
            c0[t, v] = w * (dt + 1.0)
            c1[t, v] = w * ((dt * e + e) + 1.0 / sigma)
    return c0, c1


def ordered_sums(entries, G, c0, c1):
    """[G][2]: row j the sum of c0 resp. c1 over the positions (t, v), v < N-1, with entries == j, in
    ascending position with one accumulator"""
    out = np.zeros((G, 2))
    for t, row in enumerate(np.atleast_2d(entries)):
        for v in range(len(row) - 1):
            out[row[v], 0] = out[row[v], 0] + c0[t, v]
            out[row[v], 1] = out[row[v], 1] + c1[t, v]
    return out


def log_f(ll, lprior, lqt, lqb, beta):
    return np.array([((beta * float(a) + float(b)) - float(c)) - float(e) for a, b, c, e in zip(ll, lprior, lqt, lqb)])


# ---------------------------------------------------------------- one step from the by-value calls
class Composer:
    """One step from a GeneralizedPruning's by-value host calls and its engine's gradient call.  The
    draw needs the state's table in the object's place: the object's own q is put back."""

    def __init__(self, gp, options, model_params=None):
        self.gp, self.e, self.model_params = gp, gp.engine, model_params
        self.o = copy.copy(options)
        self.o.checked = None   # (every variable's sigma must stay positive)

    def particles(self, state):
        """(trees, draw, de-rooted trees with new_id) of step state.steps"""
        gp, o = self.gp, self.o
        base = state.first_sample + state.steps * o.particle_count
        _, q = gp.log_normalize(state.log_params)
        kept = gp.get_sbn_parameters()
        gp.set_sbn_parameters(q)
        try:
            trees = gp.sample_trees(o.particle_count, o.seed, first_sample=base)
        finally:
            gp.set_sbn_parameters(kept)
        draw = gp.branch_sample(trees.entries, state.q_params, o.seed, first_sample=base, prior_rate=o.prior_rate)
        un = self.e.deroot_trees_mapped(trees.parent_ids, draw.branch_lengths)
        return trees, draw, un

    def gradients(self, state):
        """(SBN gradient, q gradient, logL, log prior, log q topology, log q branch) of the step"""
        gp, e, o = self.gp, self.e, self.o
        trees, draw, un = self.particles(state)
        K, N = trees.entries.shape
        params = None if self.model_params is None else np.tile(self.model_params, (K, 1))
        grads = e.gradients(un.parent_ids, un.branch_lengths, params, gradient_blocks=("branch_lengths",))
        ll = np.array([x.log_likelihood for x in grads])
        g = np.zeros((K, N))
        for k, x in enumerate(grads):
            row = np.asarray(x.gradient["branch_lengths"], float)
            g[k, :len(row)] = row
        g_q, lf = gp.branch_gradient(trees.entries, state.q_params, draw, un.new_id, g, ll, log_q_topology=trees.log_q,
                                     beta=F.beta(state.steps, o.anneal_steps), prior_rate=o.prior_rate)
        g_sbn, _ = gp.topology_gradient(trees.entries, state.log_params, lf, estimator=o.estimator)
        return g_sbn, g_q, ll, draw.log_prior, trees.log_q, draw.log_q

    def step(self, state):
        """(state after the step, trace row)"""
        return F.update(state, self.o, *self.gradients(state))
