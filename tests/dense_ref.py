"""A plain analytic reference for the branch-length Hessian call (TEST INFRASTRUCTURE ONLY;
numpy only): log L, g, H, S of DESIGN.md 4.8 for one unrooted 4-state tree, in np.longdouble.

Deliberately not the kernels' algorithm: there is no pre-order pass.  Per branch j the pruning is
repeated from j up to the root with P_j replaced by (r_k Q) P_j and by (r_k Q)^2 P_j, which gives
D1_p and D2_p directly; the transition matrices are exp(Q r_k t) by scaling-and-squaring Taylor
series (no eigensystem)."""
from types import SimpleNamespace

import numpy as np

LD = np.longdouble


def gtr_q(rates, freqs, dtype=LD):
    """Q of GTR from its six rates (order AC AG AT CG CT GT) and frequencies, normalised to
    -sum_i pi_i Q_ii = 1.  JC69 is rates = 1, freqs = 1/4."""
    rates, pi = np.asarray(rates, dtype), np.asarray(freqs, dtype)
    Q = np.zeros((4, 4), dtype)
    r = 0
    for i in range(4):
        for j in range(i + 1, 4):
            Q[i, j] = rates[r] * pi[j]
            Q[j, i] = rates[r] * pi[i]
            r += 1
    rows = Q.sum(axis=1)
    Q[np.diag_indices(4)] = -rows
    return Q / np.sum(rows * pi), pi


def tip_vectors(states, dtype=LD):
    """[n][P] state codes -> [n][P][4] tip vectors: one-hot, codes above 3 (gaps) all ones."""
    states = np.asarray(states)
    v = np.ones(states.shape + (4,), dtype)
    known = states <= 3
    v[known] = np.eye(4, dtype=dtype)[states[known]]
    return v


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


def branch_derivatives(parent_ids, lengths, Q, pi, cat_rates, cat_weights, tips, weights, dtype=LD):
    """One unrooted tree: parent ids [2n-3] (root = node 2n-3, a parent's id above its
    children's), lengths [2n-2] (the root's entry 0), Q [4][4], pi [4], category rates and weights
    [K], tip vectors [n][P][4] (gaps, 0/1 masks or real values), pattern weights [P].

    Returns log_likelihood and, in the engine's node-id layout [2n-1] with the last two entries 0,
    g_j = sum w D1/L, S_j = sum w (D1/L)^2, H_j = sum w D2/L - S_j and the scales
    A1_j = sum w |D1/L|, A2_j = sum w |D2/L|; W = sum w and rho = r_max max_i sum_j |Q_ij| (what
    tolerances() needs).  Everything in `dtype`."""
    pid = np.asarray(parent_ids, int)
    root = len(pid)
    n = (root + 3) // 2
    t = np.asarray(lengths, dtype)
    Q, pi = np.asarray(Q, dtype), np.asarray(pi, dtype)
    r, c = np.asarray(cat_rates, dtype), np.asarray(cat_weights, dtype)
    tips, w = np.asarray(tips, dtype), np.asarray(weights, dtype)
    assert t.shape == (root + 1,) and t[root] == 0 and tips.shape[0] == n and tips.shape[2] == 4
    assert np.all(pid > np.arange(root)) and np.all(pid <= root)
    K = len(r)
    kids = [[] for _ in range(root + 1)]
    for v, p in enumerate(pid):
        kids[p].append(v)

    Pm = np.stack([np.stack([expm(Q * (r[k] * t[v])) for k in range(K)]) for v in range(root)])
    rQ = r[:, None, None] * Q  # [K][4][4]

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

    def site(x):  # root vector [K][P][4] -> per-pattern value
        return np.einsum("k,kpi,i->p", c, x, pi)

    def replaced(j, M):
        """Per-pattern likelihood with P_j replaced by M [K][4][4]: pruned again from j up."""
        v, m = j, np.einsum("kij,kpj->kpi", M, L[j])
        while True:
            a = pid[v]
            x = m * np.prod([msg[u] for u in kids[a] if u != v], axis=0)
            if a == root:
                return site(x)
            v, m = a, np.einsum("kij,kpj->kpi", Pm[a], x)

    lik = site(L[root])
    assert np.min(lik) > 0, "a pattern has likelihood 0 (zero-length branches joining different states?)"
    out = SimpleNamespace(log_likelihood=np.sum(w * np.log(lik)), W=np.sum(w),
                          rho=np.max(r) * np.max(np.sum(np.abs(Q), axis=1)))
    for name in ("g", "S", "H", "A1", "A2"):
        setattr(out, name, np.zeros(root + 2, dtype))
    for j in range(root):
        d1 = replaced(j, rQ @ Pm[j]) / lik
        d2 = replaced(j, rQ @ rQ @ Pm[j]) / lik
        out.g[j] = np.sum(w * d1)
        out.S[j] = np.sum(w * d1 * d1)
        out.H[j] = np.sum(w * d2) - out.S[j]
        out.A1[j] = np.sum(w * np.abs(d1))
        out.A2[j] = np.sum(w * np.abs(d2))
    return out


def tolerances(ref, eps):
    """Per-branch bounds for an FP64 evaluator compared with `ref`: eps times the size of the
    terms summed, plus W rho (W rho^2) -- on a saturated branch q.(Q L) cancels from terms of
    size rho, so an FP64 evaluator's absolute error there is ~ 1e-16 W rho whatever the value."""
    eps = LD(eps)
    return SimpleNamespace(g=eps * (ref.A1 + ref.W * ref.rho),
                           S=eps * (ref.S + ref.W * ref.rho ** 2),
                           H=eps * (ref.A2 + ref.S + ref.W * ref.rho ** 2))
