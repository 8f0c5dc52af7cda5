"""PSP indexing and the log-normal branch-length models in plain Python, on top
of tests/sbn_ref.py and tests/sbn_vi_ref.py: the PSP numbering and every tree's index rows from the
clade sets of the support (not from slots), the normal draw over sbn_vi_ref.philox4x32_10, and log
q, the prior and the gradient with math.fsum.  Restates the reference's PSPIndexer
(src/psp_indexer.cpp), vip/branch_model.py, vip/scalar_model.py and vip/priors.py and shares no
structure with the engine's kernels: no slots, no sort, no runs."""
import math

import sbn_ref as R
import sbn_vi_ref as V

M32 = 0xFFFFFFFF
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


# ---- PSP indexing ----
def psp_table(support):
    """(psp_of_pcsp [C], S, V) of a sbn_ref.Support: a PCSP is a PSP when its sister is the
    complement of its focal clade; PSPs are numbered from S in ascending parameter order."""
    everything = frozenset(range(support.n))
    out, nxt = [], support.S
    for sister, focal, _ in support.pcsps:
        if sister == everything - focal:
            out.append(nxt)
            nxt += 1
        else:
            out.append(-1)
    return out, support.S, nxt


def tree_psps(pid):
    """[2n-3] of (split, down, up) of every edge from the clade sets: the minorised split, and the
    (focal, child) pair below the edge (None for a pendant edge) and above it (PSPIndexer::
    RepresentationOf: down[v] = psp(children of v; leaves of v), up[v] = psp(the two other
    neighbours of v's parent; the complement of v's leaves))."""
    n = R.taxon_count(pid)
    adj, memo = R._neighbours(pid), {}
    out = []
    for v in range(len(pid)):
        p = int(pid[v])
        below, above = R._side(adj, n, v, p, memo), R._side(adj, n, p, v, memo)
        down = None
        if v >= n:
            c0, c1 = [R._side(adj, n, y, v, memo) for y in adj[v] if y != p]
            down = (below, R._minor_child(c0, c1))
        c0, c1 = [R._side(adj, n, y, p, memo) for y in adj[p] if y != v]
        out.append((R._minorise(below, n), down, (above, R._minor_child(c0, c1))))
    return out


def psp_index(support, pid, table, rows):
    """[rows][2n-3] variable indices of one tree against a support; V where there is none."""
    psp_of_pcsp, S, Vn = table
    everything = frozenset(range(support.n))

    def variable(pair):
        if pair is None:
            return Vn
        focal, child = pair
        j = support.number.get((everything - focal, focal, child), support.P)
        return psp_of_pcsp[j - S] if S <= j < support.P else Vn

    psps = tree_psps(pid)
    out = [[support.number.get(("r", s), Vn) for s, _, _ in psps]]
    if rows == 3:
        out.append([variable(d) for _, d, _ in psps])
        out.append([variable(u) for _, _, u in psps])
    return out


def psp_strings(support, table):
    """PSPIndexer::ToStringVector in this numbering: V + 1 strings, the last one empty."""
    psp_of_pcsp, S, Vn = table
    out = [support.clade_string(s) for s in support.rootsplits] + [""] * (Vn - S + 1)
    for (_, focal, child), j in zip(support.pcsps, psp_of_pcsp):
        if j >= 0:
            out[j] = support.clade_string(focal) + "|" + support.clade_string(child)
    return out


# ---- the log-normal models ----
def normal(seed, s, v):
    """The standard normal of edge v of sample s: key (seed lo, seed hi), counter (v, 1, s lo,
    s hi); Box-Muller's cosine branch from the two 53-bit uniforms of the four output words."""
    seed, s = int(seed) & (2 ** 64 - 1), int(s) & (2 ** 64 - 1)
    w = V.philox4x32_10([v, 1, s & M32, s >> 32], [seed & M32, seed >> 32])
    u1 = float((((w[0] << 32) | w[1]) >> 11) + 1) * 2.0 ** -53
    u2 = float(((w[2] << 32) | w[3]) >> 11) * 2.0 ** -53
    return math.sqrt(-2.0 * math.log(u1)) * math.cos(2.0 * math.pi * u2)


def edge_params(rows, q, v):
    """(mu, sigma) of edge v: the rows' parameters added in ascending row order; an index outside
    [0, V) adds nothing."""
    mu = sigma = 0.0
    for row in rows:
        j = int(row[v])
        if 0 <= j < len(q):
            mu, sigma = mu + float(q[j][0]), sigma + float(q[j][1])
    return mu, sigma


def log_q(xs, sigmas, eps):
    """-sum (x + log sigma + log(2 pi)/2 + eps^2 / 2)."""
    return -math.fsum(t for x, s, e in zip(xs, sigmas, eps) for t in (x, math.log(s), HALF_LOG_2PI, 0.5 * e * e))


def log_exp_prior(thetas, rate):
    """vip/priors.py: log(rate) * count - rate * sum."""
    return math.log(rate) * len(thetas) - rate * math.fsum(thetas)


def general_log_prob(values, mus, sigmas):
    """LogNormalModel.general_log_prob: the log density of `values`, from their logarithms."""
    logs = [math.log(x) for x in values]
    return -(math.fsum(logs) + math.fsum(math.log(s) for s in sigmas) + len(values) * HALF_LOG_2PI +
             math.fsum((lx - m) ** 2 / (2.0 * s * s) for lx, m, s in zip(logs, mus, sigmas)))


def sample(index, q, seed, first_sample, rate, epsilon=None):
    """(branch lengths [T][2n-2], epsilon [T][2n-3], log q [T], log prior [T])."""
    bls, epss, lqs, lps = [], [], [], []
    for t, rows in enumerate(index):
        E = len(rows[0])
        params = [edge_params(rows, q, v) for v in range(E)]
        eps = [float(epsilon[t][v]) if epsilon is not None else normal(seed, first_sample + t, v) for v in range(E)]
        xs = [m + s * e for (m, s), e in zip(params, eps)]
        theta = [math.exp(x) for x in xs]
        bls.append(theta + [0.0])
        epss.append(eps)
        lqs.append(log_q(xs, [s for _, s in params], eps))
        lps.append(log_exp_prior(theta, rate))
    return bls, epss, lqs, lps


def gradient(index, q, theta, eps, branch_gradient, weights, rate):
    """(gradient [V][2], sum of |terms| [V][2]): sum over the entries that name variable j of
    c0 = w (d theta + 1) and c1 = w (d theta eps + eps + 1 / sigma), d = g - rate."""
    terms = [([], []) for _ in q]
    for t, rows in enumerate(index):
        w = 1.0 if weights is None else float(weights[t])
        for v in range(len(rows[0])):
            _, sigma = edge_params(rows, q, v)
            d, th, e = float(branch_gradient[t][v]) - rate, float(theta[t][v]), float(eps[t][v])
            c0, c1 = w * (d * th + 1.0), w * (d * th * e + e + 1.0 / sigma)
            for row in rows:
                j = int(row[v])
                if 0 <= j < len(q):
                    terms[j][0].append(c0)
                    terms[j][1].append(c1)
    return ([[math.fsum(a), math.fsum(b)] for a, b in terms],
            [[math.fsum(map(abs, a)), math.fsum(map(abs, b))] for a, b in terms])


def log_f(log_likelihoods, log_prior, log_q_topology, log_q_branch, beta):
    """px_log_f of vip/burrito.py: beta scales the likelihood alone."""
    return [beta * ll + lp - (0.0 if log_q_topology is None else log_q_topology[t]) - lq
            for t, (ll, lp, lq) in enumerate(zip(log_likelihoods, log_prior, log_q_branch))]


def normal_cdf(x):
    return 0.5 * (1.0 + math.erf(x / math.sqrt(2.0)))


def moments_and_ks(draws):
    """(mean, variance, Kolmogorov-Smirnov statistic against the standard normal)."""
    xs = sorted(float(x) for x in draws)
    N = len(xs)
    mean = math.fsum(xs) / N
    var = math.fsum((x - mean) ** 2 for x in xs) / N
    ks = max(max((i + 1) / N - normal_cdf(x), normal_cdf(x) - i / N) for i, x in enumerate(xs))
    return mean, var, ks
