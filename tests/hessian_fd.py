"""Reference values for the branch-length Hessian call (mi_engine_branch_hessian_unrooted):
four-point (Richardson) central differences of the oracle's analytic branch gradient, and the
closed form of a three-taxon JC69 star tree."""
import numpy as np

import oracle_lib as O


def fd_hessian_diagonal(spec, tips, w, pids, bls, params, rescaling=False, rel_h=1e-4, nthreads=8):
    """d^2 logL / d t_j^2 for every branch j < 2n-3 of every tree, [T][2n-1] in the engine's
    node-id order (root and fixed node 0), from the oracle's gradient g_j at t_j +- h, t_j +- 2h
    (h = rel_h t_j).  One oracle call over all perturbed trees."""
    pids, bls, params = np.asarray(pids), np.asarray(bls, float), np.asarray(params, float)
    T, nb = bls.shape
    nbr = nb - 1  # 2n-3 branches; entry 2n-3 is the root's (length 0)
    steps = (1.0, -1.0, 2.0, -2.0)
    rows_p, rows_b, rows_r = [], [], []
    for t in range(T):
        for j in range(nbr):
            h = rel_h * bls[t, j]
            for s in steps:
                b = bls[t].copy()
                b[j] += s * h
                rows_p.append(pids[t])
                rows_b.append(b)
                rows_r.append(params[t])
    g = O.unrooted_gradients(spec, tips, w, np.stack(rows_p), np.stack(rows_b), np.stack(rows_r),
                             rescaling, nthreads)["branch_lengths"]
    g = g.reshape(T, nbr, len(steps), -1)
    out = np.zeros((T, 2 * spec.taxon_count - 1))
    for t in range(T):
        for j in range(nbr):
            gp, gm, gp2, gm2 = (g[t, j, k, j] for k in range(4))
            h = rel_h * bls[t, j]
            out[t, j] = (8.0 * (gp - gm) - (gp2 - gm2)) / (12.0 * h)
    out[:, -2:] = 0.0
    return out


def jc69_star_tree(tips3, w, t):
    """Three-taxon JC69 star tree (root = node 3, branch lengths t[0..2] above tips 0..2),
    written out: log-likelihood, d/dt_j and d^2/dt_j^2 for j = 0, 1, 2 and
    S_j = sum_p w_p (d log L_p / dt_j)^2.  tips3: [3][P] states 0..3 (4 = gap)."""
    tips3 = np.asarray(tips3)
    w = np.asarray(w, float)

    def P(tt):  # P, P', P'' of JC69 (4 x 4)
        e = np.exp(-4.0 * tt / 3.0)
        eye = np.eye(4)
        return (0.25 + e * (eye - 0.25), -4.0 / 3.0 * e * (eye - 0.25),
                16.0 / 9.0 * e * (eye - 0.25))

    def col(M, s):  # column of a tip state (gap: all states)
        return M.sum(axis=1) if s > 3 else M[:, s]

    mats = [P(x) for x in t]
    ll = 0.0
    g, h, sq = np.zeros(3), np.zeros(3), np.zeros(3)
    for p in range(tips3.shape[1]):
        f = [[col(mats[j][d], tips3[j, p]) for d in range(3)] for j in range(3)]
        L = 0.25 * np.sum(f[0][0] * f[1][0] * f[2][0])
        ll += w[p] * np.log(L)
        for j in range(3):
            o = [f[k][0] for k in range(3) if k != j]
            d1 = 0.25 * np.sum(f[j][1] * o[0] * o[1])
            d2 = 0.25 * np.sum(f[j][2] * o[0] * o[1])
            g[j] += w[p] * d1 / L
            h[j] += w[p] * (d2 / L - (d1 / L) ** 2)
            sq[j] += w[p] * (d1 / L) ** 2
    return ll, g, h, sq
