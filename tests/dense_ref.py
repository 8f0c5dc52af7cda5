"""A plain analytic reference for the branch-length gradient and Hessian calls (TEST
INFRASTRUCTURE ONLY; numpy only): log L, g, H, S of DESIGN.md 4.8 for one tree of any state count
(4 and 20 here), and the derivative by the Weibull shape, in np.longdouble.

Deliberately not the kernels' algorithm: there is no pre-order pass.  Per branch j the pruning is
repeated from j up to the root with P_j replaced by (r_k Q) P_j and by (r_k Q)^2 P_j, which gives
D1_p and D2_p directly; the transition matrices are exp(Q r_k t) by scaling-and-squaring Taylor
series (no eigensystem)."""
from types import SimpleNamespace

import numpy as np

LD = np.longdouble


def reversible_q(exchangeabilities, freqs, dtype=LD):
    """Q of a reversible model of s states from its s (s - 1) / 2 exchangeabilities (the upper
    triangle, row by row) and s frequencies, normalised to -sum_i pi_i Q_ii = 1."""
    rates, pi = np.asarray(exchangeabilities, dtype), np.asarray(freqs, dtype)
    s = len(pi)
    assert rates.shape == (s * (s - 1) // 2,)
    Q = np.zeros((s, s), dtype)
    r = 0
    for i in range(s):
        for j in range(i + 1, s):
            Q[i, j] = rates[r] * pi[j]
            Q[j, i] = rates[r] * pi[i]
            r += 1
    rows = Q.sum(axis=1)
    Q[np.diag_indices(s)] = -rows
    return Q / np.sum(rows * pi), pi


def gtr_q(rates, freqs, dtype=LD):
    """Q of GTR from its six rates (order AC AG AT CG CT GT) and frequencies: reversible_q at
    s = 4.  JC69 is rates = 1, freqs = 1/4."""
    return reversible_q(rates, freqs, dtype)


def tip_vectors(states, dtype=LD, s=4):
    """[n][P] state codes -> [n][P][s] tip vectors: one-hot, codes >= s (gaps) all ones."""
    states = np.asarray(states)
    v = np.ones(states.shape + (s,), dtype)
    known = states < s
    v[known] = np.eye(s, dtype=dtype)[states[known]]
    return v


def weibull(K, shape, dtype=LD):
    """Rates, weights and d rate / d shape of the K-category discretised Weibull site model
    (mean-one rates at the quantiles (2 i + 1) / (2 K)), in `dtype`.  K = 1 is the constant
    model: rate 1, derivative 0."""
    shape = dtype(shape)
    q = (2 * np.arange(K, dtype=dtype) + 1) / (2 * dtype(K))
    x = -np.log(1 - q)
    raw = x ** (1 / shape)
    du = -raw * np.log(x) / (shape * shape)
    mean, dmean = np.sum(raw) / K, np.sum(du) / K
    return raw / mean, np.full(K, 1 / dtype(K), dtype), (du * mean - raw * dmean) / (mean * mean)


def expm(A):
    """exp(A) of one small matrix: Taylor series of A / 2^s (norm at most 1/2), squared s times."""
    dtype = A.dtype
    norm = float(np.max(np.sum(np.abs(A), axis=1)))
    s = max(0, int(np.ceil(np.log2(norm))) + 1) if norm > 0 else 0
    B = A / dtype.type(2) ** s
    E = term = np.eye(A.shape[0], dtype=dtype)
    for i in range(1, 40):
        term = term @ B / dtype.type(i)
        E = E + term
        if np.max(np.abs(term)) < np.finfo(dtype).eps * 1e-3:
            break
    for _ in range(s):
        E = E @ E
    return E


def branch_derivatives(parent_ids, lengths, Q, pi, cat_rates, cat_weights, tips, weights, dtype=LD,
                       cat_rate_derivs=None, hessian=True):
    """One tree: parent ids (root = the last node, a parent's id above its children's; unrooted
    [2n-3] with three children of the root, rooted [2n-2] with two), lengths of every node (the
    root's entry 0), Q [s][s], pi [s], category rates and weights [K], tip vectors [n][P][s]
    (gaps, 0/1 masks or real values), pattern weights [P].

    Returns log_likelihood and, in the engine's node-id layout (the root's entry and one more
    after it, both 0), g_j = sum w D1/L and its scale A1_j = sum w |D1/L|; with `hessian` also
    S_j = sum w (D1/L)^2, H_j = sum w D2/L - S_j and A2_j = sum w |D2/L|; W = sum w and
    rho = r_max max_i sum_j |Q_ij| (what tolerances() needs).

    With cat_rate_derivs (d r_k / d alpha, [K]) also the derivative of log L by the site model's
    shape alpha, from the same per-category root vectors as g_j:
    g_site = sum_j t_j sum_p w_p (sum_k c_k dr_k [q.(Q P_j L_j)]_pk) / L_p, A_site the same sum
    with absolute values per pattern and branch, rho_site = max_k |dr_k| max_i sum_j |Q_ij|.
    Everything in `dtype`."""
    pid = np.asarray(parent_ids, int)
    root = len(pid)
    n = (root + 3) // 2
    t = np.asarray(lengths, dtype)
    Q, pi = np.asarray(Q, dtype), np.asarray(pi, dtype)
    r, c = np.asarray(cat_rates, dtype), np.asarray(cat_weights, dtype)
    tips, w = np.asarray(tips, dtype), np.asarray(weights, dtype)
    s = Q.shape[0]
    assert t.shape == (root + 1,) and t[root] == 0 and tips.shape[0] == n and tips.shape[2] == s
    assert np.all(pid > np.arange(root)) and np.all(pid <= root)
    K = len(r)
    kids = [[] for _ in range(root + 1)]
    for v, p in enumerate(pid):
        kids[p].append(v)

    Pm = np.stack([np.stack([expm(Q * (r[k] * t[v])) for k in range(K)]) for v in range(root)])
    rQ = r[:, None, None] * Q  # [K][s][s]

    # post-order: L[v][k][p][i], and the message of v to its parent, (P_v L_v)
    L = [None] * (root + 1)
    msg = [None] * root
    for v in range(root + 1):
        if v < n:
            L[v] = np.broadcast_to(tips[v], (K,) + tips[v].shape)
        else:
            L[v] = np.prod([msg[u] for u in kids[v]], axis=0)
        if v < root:
            msg[v] = np.einsum("kij,kpj->kpi", Pm[v], L[v])

    def site(x, cw=c):  # root vector [K][P][s] -> per-pattern value
        return np.einsum("k,kpi,i->p", cw, x, pi)

    def replaced(j, M):
        """Root vector [K][P][s] with P_j replaced by M [K][s][s]: pruned again from j up."""
        v, m = j, np.einsum("kij,kpj->kpi", M, L[j])
        while True:
            a = pid[v]
            x = m * np.prod([msg[u] for u in kids[a] if u != v], axis=0)
            if a == root:
                return x
            v, m = a, np.einsum("kij,kpj->kpi", Pm[a], x)

    lik = site(L[root])
    assert np.min(lik) > 0, "a pattern has likelihood 0 (zero-length branches joining different states?)"
    out = SimpleNamespace(log_likelihood=np.sum(w * np.log(lik)), W=np.sum(w),
                          rho=np.max(r) * np.max(np.sum(np.abs(Q), axis=1)))
    for name in ("g", "A1") + (("S", "H", "A2") if hessian else ()):
        setattr(out, name, np.zeros(root + 2, dtype))
    if cat_rate_derivs is not None:
        dr = np.asarray(cat_rate_derivs, dtype)
        assert dr.shape == r.shape and np.all(r > 0)
        out.g_site = out.A_site = dtype(0)
        out.rho_site = np.max(np.abs(dr)) * np.max(np.sum(np.abs(Q), axis=1))
    for j in range(root):
        x1 = replaced(j, rQ @ Pm[j])  # r_k [Q P_j L_j ...] per category
        d1 = site(x1) / lik
        out.g[j] = np.sum(w * d1)
        out.A1[j] = np.sum(w * np.abs(d1))
        if cat_rate_derivs is not None:
            ds = site(x1, c * dr / r) / lik
            out.g_site = out.g_site + t[j] * np.sum(w * ds)
            out.A_site = out.A_site + t[j] * np.sum(w * np.abs(ds))
        if hessian:
            d2 = site(replaced(j, rQ @ rQ @ Pm[j])) / lik
            out.S[j] = np.sum(w * d1 * d1)
            out.H[j] = np.sum(w * d2) - out.S[j]
            out.A2[j] = np.sum(w * np.abs(d2))
    return out


def tolerances(ref, eps):
    """Per-branch bounds for an FP64 evaluator compared with `ref`: eps times the size of the
    terms summed, plus W rho (W rho^2) -- on a saturated branch q.(Q L) cancels from terms of
    size rho, so an FP64 evaluator's absolute error there is ~ 1e-16 W rho whatever the value."""
    eps = LD(eps)
    tol = SimpleNamespace(g=eps * (ref.A1 + ref.W * ref.rho))
    if hasattr(ref, "H"):
        tol.S = eps * (ref.S + ref.W * ref.rho ** 2)
        tol.H = eps * (ref.A2 + ref.S + ref.W * ref.rho ** 2)
    return tol
