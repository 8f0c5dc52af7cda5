"""An independent reference for the branch-length optimisation call
(mi_engine_optimize_branch_lengths_unrooted): the maximum-likelihood branch lengths of one
unrooted tree under box bounds, computed on the oracle.

Two methods, neither of which uses the engine or its H / S outputs:
  "lbfgsb"  scipy's L-BFGS-B on the oracle's log-likelihood and analytic gradient, finished by
            a few steps of the method below (see _lbfgsb for why);
  "newton"  numpy only: projected diagonal Newton steps whose curvature comes from forward
            differences of the oracle's gradient (one oracle call over the 2n-3 perturbed trees),
            with backtracking on the oracle's log-likelihood.
reference_optimum() takes L-BFGS-B where scipy imports and falls back to the numpy method where
it does not: it never skips."""
import numpy as np

import oracle_lib as O

try:
    from scipy.optimize import minimize as _minimize
    HAVE_SCIPY = True
except Exception:  # (not installed, or installed against another numpy)
    _minimize = None
    HAVE_SCIPY = False

FLOOR = 1e-3  # the length floor of the convergence criterion and of relative length errors


def criterion(t, g, min_length, max_length):
    """max_j |pg_j| max(t_j, 1e-3) over the branches (t, g: [2n-3]); pg: the gradient, 0 where
    t_j sits on a bound and the gradient points outward."""
    t, g = np.asarray(t, float), np.asarray(g, float)
    outward = ((t <= min_length) & (g < 0)) | ((t >= max_length) & (g > 0))
    return float(np.max(np.where(outward, 0.0, np.abs(g)) * np.maximum(t, FLOOR)))


def relative_length_error(a, b):
    """max_j |a_j - b_j| / max(|b_j|, 1e-3)."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), FLOOR)))


class OracleTree:
    """log-likelihood and branch gradient of one tree at rows of branch lengths [m][2n-3]."""

    def __init__(self, spec, tips, w, pids, params, rescaling=False, fixed_entry=0.0, nthreads=8):
        self.spec, self.tips, self.w = spec, tips, w
        self.pids = np.asarray(pids, np.int32).reshape(1, -1)
        self.params = np.asarray(params, float).reshape(1, -1)
        self.rescaling, self.fixed, self.nthreads = rescaling, fixed_entry, nthreads
        self.nb = 2 * spec.taxon_count - 3
        self.evaluations = 0

    def __call__(self, x):
        x = np.atleast_2d(np.asarray(x, float))
        m = x.shape[0]
        bl = np.full((m, self.nb + 1), self.fixed)
        bl[:, :self.nb] = x
        out = O.unrooted_gradients(self.spec, self.tips, self.w, np.repeat(self.pids, m, axis=0), bl,
                                   np.repeat(self.params, m, axis=0), self.rescaling,
                                   min(self.nthreads, m))
        self.evaluations += m
        return out["log_likelihood"].copy(), out["branch_lengths"][:, :self.nb].copy()


class RealTipOracleTree:
    """The same for an alignment whose tip 0 carries real-valued partial vectors v[p][0..3]
    (the oracle takes tip states only).  The likelihood of a pattern is linear in a tip's vector:
    L_p = sum_a v[p][a] L_p(tip 0 in state a), so logL and its gradient follow from the oracle's
    per-pattern values (one-pattern alignments of weight 1) for the four states."""

    def __init__(self, spec_one, tips, w, tip0_partials, pids, params, rescaling=False,
                 fixed_entry=0.0, nthreads=8):
        assert spec_one.pattern_count == 1
        self.spec, self.tips, self.w = spec_one, np.array(tips, np.int32), np.asarray(w, float)
        self.v = np.asarray(tip0_partials, float)
        self.pids = np.asarray(pids, np.int32).reshape(1, -1)
        self.params = np.asarray(params, float).reshape(1, -1)
        self.rescaling, self.fixed, self.nthreads = rescaling, fixed_entry, nthreads
        self.nb = 2 * spec_one.taxon_count - 3
        self.evaluations = 0

    def __call__(self, x):
        x = np.atleast_2d(np.asarray(x, float))
        m = x.shape[0]
        bl = np.full((m, self.nb + 1), self.fixed)
        bl[:, :self.nb] = x
        pid, pr = np.repeat(self.pids, m, axis=0), np.repeat(self.params, m, axis=0)
        ll, g = np.zeros(m), np.zeros((m, self.nb))
        one = np.ones(1)
        for p in range(self.tips.shape[1]):
            col = self.tips[:, p:p + 1].copy()
            L, dL = np.zeros(m), np.zeros((m, self.nb))
            for a in range(4):
                if self.v[p, a] == 0.0:
                    continue
                col[0, 0] = a
                out = O.unrooted_gradients(self.spec, col, one, pid, bl, pr, self.rescaling,
                                           min(self.nthreads, m))
                La = self.v[p, a] * np.exp(out["log_likelihood"])
                L += La
                dL += La[:, None] * out["branch_lengths"][:, :self.nb]
            ll += self.w[p] * np.log(L)
            g += self.w[p] * dL / L[:, None]
        self.evaluations += m
        return ll, g


def _lbfgsb(f, x0, lo, hi):
    """L-BFGS-B accepts steps on the change of logL, so it stops where that change reaches the
    rounding error of logL (about 1e-12 here): on DS1 with the criterion at 1e-6 to 6e-6, the
    optimum's logL reached to 2e-11.  The last digits of the lengths then come from a few of
    the gradient-driven steps below, started at its result (they move no length by more than
    1e-6 relative)."""
    def fun(x):
        ll, g = f(x)
        return -ll[0], -g[0]
    r = _minimize(fun, x0, jac=True, method="L-BFGS-B", bounds=[(lo, hi)] * len(x0),
                  options=dict(maxiter=2000, maxfun=5000, ftol=1e-15, gtol=1e-10, maxcor=30))
    return _newton(f, np.clip(r.x, lo, hi), lo, hi)


def _newton(f, x0, lo, hi, tol=1e-9, max_iterations=400):
    x = np.clip(np.asarray(x0, float), lo, hi)
    nb = len(x)
    ll, g = f(x)
    ll, g = ll[0], g[0]
    alpha = 1.0
    for _ in range(max_iterations):
        if criterion(x, g, lo, hi) <= tol:
            break
        # curvature of branch j from the gradient at x + h_j e_j (backward at the upper bound)
        h = np.maximum(1e-4 * x, 1e-9)
        h = np.where(x + h > hi, -h, h)
        _, gp = f(x[None, :] + np.diag(h))
        c = -(np.diag(gp) - g) / h
        c = np.where(c > 0, c, np.abs(g) / np.maximum(x, FLOOR))
        d = np.where(c > 0, g / np.where(c > 0, c, 1.0), 0.0)
        d = np.clip(d, -0.9 * x, np.maximum(4 * x, 0.1))
        while True:
            xn = np.clip(x + alpha * d, lo, hi)
            lln, gn = f(xn)
            # (near the optimum a step changes logL by less than its rounding error)
            if lln[0] >= ll - 4e-16 * abs(ll) * nb:
                x, ll, g = xn, lln[0], gn[0]
                alpha = min(1.0, 2 * alpha)
                break
            alpha *= 0.5
            if alpha < 1e-8:
                return x
    return x


def reference_optimum(spec, tips, w, pids, start, params, rescaling=False, min_length=1e-8,
                      max_length=10.0, method=None, f=None):
    """Maximum-likelihood branch lengths of ONE tree (pids [2n-3], start [2n-2], params [C])
    within [min_length, max_length], started from `start` clamped into the box.  Returns
    (branch lengths [2n-2] with the caller's fixed-node entry, logL, gradient [2n-3], method),
    logL and gradient the oracle's at the result.  f: the evaluator to use instead of
    OracleTree(spec, tips, w, ...)."""
    start = np.asarray(start, float).reshape(-1)
    if f is None:
        f = OracleTree(spec, tips, w, pids, params, rescaling, fixed_entry=start[-1])
    if method is None:
        method = "lbfgsb" if HAVE_SCIPY else "newton"
    x0 = np.clip(start[:-1], min_length, max_length)
    x = _lbfgsb(f, x0, min_length, max_length) if method == "lbfgsb" else \
        _newton(f, x0, min_length, max_length)
    ll, g = f(x)
    return np.append(x, start[-1]), float(ll[0]), g[0], method
