"""Bootstrap weights drawn by the stated integer rule and the KH, SH and AU tests in plain
Python / numpy (TEST INFRASTRUCTURE ONLY; never imports the library).

The sampler: Philox4x32-10 (sbn_vi_ref.philox4x32_10 is the definition; philox_many is the same
rounds on numpy uint64 arrays, checked against it by tests/test_topology_tests_ref.py), the site of
a draw (x N) >> 64 in Python integers, its pattern by bisect on the exclusive prefix sum.  The
statistics: column means by a sequential loop over the replicates, integer counts, the AU fit in
double with scipy.special.ndtri / ndtr, and once more in 50-digit mpmath."""
import bisect
import math

import numpy as np

import sbn_vi_ref as V

STREAM = 0x72656C6C
M32 = 0xFFFFFFFF
M64 = 2 ** 64 - 1
COLUMNS = ("L", "delta", "bp", "elw", "p_kh", "p_sh", "p_au", "d", "c", "rss", "usable")


def philox_many(c0, c1, c2, c3, key):
    """philox4x32_10 on arrays of counters (uint64 arrays holding 32-bit words): four word arrays."""
    c0, c1, c2, c3 = (np.asarray(x, np.uint64) & np.uint64(M32) for x in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = int(key[0]) & M32, int(key[1]) & M32
    m = np.uint64(M32)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & m, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & m
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def prefix_sum(w):
    """(cum [P+1] of Python integers, N) of integer pattern weights; ValueError where the library refuses."""
    w = np.asarray(w, np.float64).reshape(-1)
    if w.size == 0 or not np.all(np.isfinite(w)) or np.any(w < 0) or np.any(w != np.floor(w)):
        raise ValueError("pattern weights must be non-negative integer site counts")
    cum = [0]
    for x in w:
        cum.append(cum[-1] + int(x))
    if not 1 <= cum[-1] < 2 ** 31:
        raise ValueError("the pattern weights must sum to N with 1 <= N < 2^31")
    return cum, cum[-1]


def draws(seed, rho, n):
    """The n 64-bit draws of replicate number rho, as Python integers."""
    seed, rho = int(seed) & M64, int(rho) & M64
    calls = (n + 1) // 2
    j = np.arange(calls, dtype=np.uint64)
    c = philox_many(j, STREAM, rho & M32, rho >> 32, (seed & M32, seed >> 32))
    x = np.empty(2 * calls, dtype=object)
    x[0::2] = [(int(a) << 32) | int(b) for a, b in zip(c[0], c[1])]
    x[1::2] = [(int(a) << 32) | int(b) for a, b in zip(c[2], c[3])]
    return list(x[:n])


def draws_scalar(seed, rho, n):
    """draws() call by call through sbn_vi_ref.philox4x32_10."""
    seed, rho = int(seed) & M64, int(rho) & M64
    out = []
    for j in range((n + 1) // 2):
        c = V.philox4x32_10([j, STREAM, rho & M32, rho >> 32], [seed & M32, seed >> 32])
        out += [(c[0] << 32) | c[1], (c[2] << 32) | c[3]]
    return out[:n]


def weights_row(seed, rho, n, cum, draw=draws):
    """One replicate: counts [P] of the n draws over the patterns."""
    N, row = cum[-1], [0] * (len(cum) - 1)
    for x in draw(seed, rho, n):
        site = (x * N) >> 64
        row[bisect.bisect_right(cum, site) - 1] += 1  # cum[p] <= site < cum[p+1]
    return row


def bootstrap_weights(w, B, n, seed, first_replicate=0):
    """W [B][P] float64 of mi_engine_bootstrap_weights."""
    cum, _ = prefix_sum(w)
    return np.array([weights_row(seed, first_replicate + b, n, cum) for b in range(B)], dtype=np.float64)


def column_means(c):
    """mean[t] = (sum_b C[b][t]) / B: one accumulator per tree, b ascending."""
    acc = np.zeros(c.shape[1])
    for b in range(c.shape[0]):
        acc = acc + c[b]
    return acc / float(c.shape[0])


def best_two(L):
    """(t1, t2): argmax and the argmax over the others, the lowest index among equals; t2 = -1 for one tree."""
    L = np.asarray(L, np.float64)
    t1 = int(np.argmax(L))
    if L.size == 1:
        return t1, -1
    others = [t for t in range(L.size) if t != t1]
    return t1, int(max(others, key=lambda t: (L[t], -t)))


def kh_sh_counts(c, L, mean):
    """Integer counts (kh [T], sh [T]) from block 0's C [B][T], L [T] and the column means."""
    B, T = c.shape
    t1, t2 = best_two(L)
    z = c - mean[None, :]
    sh = np.sum((z.max(axis=1)[:, None] - z) >= (L[t1] - L)[None, :], axis=0).astype(np.int64)
    if T == 1:
        return np.array([B], np.int64), sh
    ref = np.array([t2 if t == t1 else t1 for t in range(T)])
    kh = np.sum((z[:, ref] - z) >= (L[ref] - L)[None, :], axis=0).astype(np.int64)
    return kh, sh


def au_fit(cnt, sites, reps, N):
    """(p, d, c, rss, usable) of one tree from its counts per block, in double."""
    from scipy.special import ndtr, ndtri
    s11 = s12 = s22 = t1 = t2 = 0.0
    rows = []
    for k in range(len(sites)):
        if not 0 < int(cnt[k]) < int(reps[k]):
            continue
        r = float(sites[k]) / float(N)
        x1 = math.sqrt(r)
        x2 = 1.0 / x1
        pi = float(cnt[k]) / float(reps[k])
        z = -float(ndtri(pi))
        phi = math.exp(-0.5 * (z * z)) * 0.3989422804014326779399461
        om = float(reps[k]) * (phi * phi) / (pi * (1.0 - pi))
        s11 += om * (x1 * x1)
        s12 += om * (x1 * x2)
        s22 += om * (x2 * x2)
        t1 += om * (x1 * z)
        t2 += om * (x2 * z)
        rows.append((x1, x2, z, om))
    if len(rows) < 2:
        return None, math.nan, math.nan, math.nan, len(rows)
    det = s11 * s22 - s12 * s12
    d = (t1 * s22 - t2 * s12) / det
    c = (s11 * t2 - s12 * t1) / det
    rss = 0.0
    for x1, x2, z, om in rows:
        e = z - d * x1 - c * x2
        rss += om * (e * e)
    return float(ndtr(c - d)), d, c, rss, len(rows)


def au_fit_mp(cnt, sites, reps, N, digits=50):
    """au_fit in mpmath at `digits` digits: (p, d, c, rss, usable) as mpf (None for p below two usable scales)."""
    import mpmath as mp
    with mp.workdps(digits):
        s11 = s12 = s22 = t1 = t2 = mp.mpf(0)
        rows = []
        for k in range(len(sites)):
            if not 0 < int(cnt[k]) < int(reps[k]):
                continue
            r = mp.mpf(int(sites[k])) / mp.mpf(int(N))
            x1 = mp.sqrt(r)
            x2 = 1 / x1
            pi = mp.mpf(int(cnt[k])) / mp.mpf(int(reps[k]))
            z = -mp.sqrt(2) * mp.erfinv(2 * pi - 1)
            phi = mp.npdf(z)
            om = mp.mpf(int(reps[k])) * phi * phi / (pi * (1 - pi))
            s11 += om * x1 * x1
            s12 += om * x1 * x2
            s22 += om * x2 * x2
            t1 += om * x1 * z
            t2 += om * x2 * z
            rows.append((x1, x2, z, om))
        if len(rows) < 2:
            return None, None, None, None, len(rows)
        det = s11 * s22 - s12 * s12
        d = (t1 * s22 - t2 * s12) / det
        c = (s11 * t2 - s12 * t1) / det
        rss = sum(om * (z - d * x1 - c * x2) ** 2 for x1, x2, z, om in rows)
        return mp.ncdf(c - d), d, c, rss, len(rows)


def table_from(c0, L, counts, sites, reps, N, elw=None):
    """The [T][11] table from block 0's C, L, the counts [K][T] and the blocks (elw: given, or numpy's)."""
    c0, L, counts = np.asarray(c0, np.float64), np.asarray(L, np.float64), np.asarray(counts)
    B, T = c0.shape
    mean = column_means(c0)
    kh, sh = kh_sh_counts(c0, L, mean)
    t1, _ = best_two(L)
    bp = counts[0] / float(B)
    if elw is None:
        e = np.exp(c0 - c0.max(axis=1, keepdims=True))
        elw = (e / e.sum(axis=1, keepdims=True)).sum(axis=0) / B
    out = np.empty((T, len(COLUMNS)))
    for t in range(T):
        p, d, c, rss, usable = au_fit(counts[:, t], sites, reps, N)
        out[t] = [L[t], L[t1] - L[t], bp[t], elw[t], kh[t] / float(B), sh[t] / float(B),
                  bp[t] if p is None else p, d, c, rss, usable]
    return out, mean, kh, sh


def replicate_log_likelihoods(W, s):
    """C [B][T] = W s^T, a column per call: equal rows of s give equal columns."""
    return np.stack([W @ s[t] for t in range(s.shape[0])], axis=1)


def topology_tests(s, w, sites, reps, seed=0, first_replicate=0):
    """mi_engine_topology_tests restated: (table [T][11], counts [K][T], mean [T], C_0, best_0).
    The products are numpy's (their order of summation is not the library's)."""
    s, w = np.asarray(s, np.float64), np.asarray(w, np.float64).reshape(-1)
    cum, N = prefix_sum(w)
    if int(sites[0]) != N:
        raise ValueError("sites[0] must equal the sum of the pattern weights")
    if len(set(int(x) for x in sites)) != len(sites):
        raise ValueError("the blocks' sites must be pairwise distinct")
    T = s.shape[0]
    L = replicate_log_likelihoods(w[None, :], s)[0]
    counts = np.zeros((len(sites), T), np.int64)
    first, c0, best0 = int(first_replicate), None, None
    for k, (n, B) in enumerate(zip(sites, reps)):
        W = np.array([weights_row(seed, first + b, int(n), cum) for b in range(int(B))], dtype=np.float64)
        first += int(B)
        c = replicate_log_likelihoods(W, s)
        best = np.argmax(c, axis=1)
        counts[k] = np.bincount(best, minlength=T)
        if k == 0:
            c0, best0 = c, best
    table, mean, _, _ = table_from(c0, L, counts, sites, reps, N)
    return table, counts, mean, c0, best0
