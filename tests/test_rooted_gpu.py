"""The rooted path (rate-scaled branch lengths, log-det-Jacobian, height-ratio / root-height and
clock gradients) against the CPU oracle: at every size class of the chain rule in
kernels_finalize.hip, on degenerate trees in every one of its forms, and through every route of
the gradient walk that has a rooted form.

The oracle's own ratio gradient is checked against finite differences on the CPU
(test_oracle_kats.py::test_oracle_ratio_gradient_matches_finite_differences).

Tolerances are the suite's (test_gpu_parity.py): 1e-10 of the largest magnitude of a gradient
vector (_close), 1e-10 relative for log-likelihoods, 1e-9 * max(1, |x|) for the site gradient,
rtol 1e-6 + atol 1e-4 for the finite-difference substitution gradient against the oracle in its
expm1 mode.
"""
import functools

import numpy as np
import pytest

import oracle_lib as O
import tree_utils as TU
from test_gpu_parity import RTOL, WALK_KERNEL, _close, _engine, _params

pytestmark = pytest.mark.gpu

# Where finalize_body_t<LDS, ROOTED> (kernels_finalize.hip) changes form, in taxa n:
#   rooted_recurrences_wave<1>   n - 1 <= 64    ("if (n - 1 <= 64)")                    n <= 65
#   rooted_recurrences_wave<2>   n - 1 <= 128   ("else if (n - 1 <= 128)")              n <= 129
#   rooted_recurrences_wave<4>   n - 1 <= 256   ("else if (n - 1 <= 256)"; 192 = the
#                                               third of its four register blocks)      n <= 257
#   lane-0 loop over LDS         ("else if (lane == 0)")  n >= 258 while the working set of
#                                22 n doubles fits 48 KiB ("a.use_lds = lds <= 48 * 1024"):
#                                22 * 279 * 8 = 49 104 <= 49 152 < 22 * 280 * 8         n <= 279
#   global-memory fallback       finalize_body_t<false, true>: ratio_transform twice
#                                over a.scratch                                          n >= 280
# The same sizes cross the set-up kernel's register-array classes (N = 2n - 1 <= 64 / 128 / 192 /
# 256, then its workgroup form) and the walk's switch from LDS to the arena.
SIZE_CLASSES = (64, 65, 66, 128, 129, 130, 192, 256, 257, 258, 279, 280, 400)
TREE_KINDS = ("random", "random-isochronous", "ladder", "balanced")


def _rel(a, b):
    """Largest difference relative to the largest magnitude of the reference vector b."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _rates(rng, T, N, rcounts):
    rates = rng.uniform(0.01, 0.1, size=(T, N - 1))
    for t, rc in enumerate(rcounts):
        if rc == 1:
            rates[t] = rates[t, 0]
    return rates


def _oracle(c, resc):
    """Everything the rooted calls deliver, from the oracle; asserted finite, so that no case
    can pass by comparing NaN patterns."""
    a = (c["spec"], c["tips"], c["w"], c["pids"], c["bls"], c["pr"], c["rates"])
    out = {"ll_jac": O.rooted_log_likelihoods(*a, c["hs"], c["bds"], True, resc, 4),
           "ll_plain": O.rooted_log_likelihoods(*a, c["hs"], c["bds"], False, resc, 4),
           "grad": O.rooted_gradients(*a, c["rcounts"], c["hs"], c["bds"], c["ras"], resc, 4)}
    if c["subst"] == "GTR":
        O.set_transition_mode(1)
        try:
            out["subst"] = O.rooted_gradients(*a, c["rcounts"], c["hs"], c["bds"], c["ras"], resc,
                                              4)["substitution_model"]
        finally:
            O.set_transition_mode(0)
    for key in ("ll_jac", "ll_plain"):
        assert np.all(np.isfinite(out[key])), (key, c["what"], resc, out[key])
    for key, val in out["grad"].items():
        assert np.all(np.isfinite(val)), (key, c["what"], resc)
    return out


def _case(n, P, T, rng, subst="JC69", site="weibull+4", kinds=None, use_tip_states=1, what=""):
    """Inputs of one rooted case (never changed afterwards); kinds: one of TREE_KINDS per tree."""
    N = 2 * n - 1
    kinds = kinds or ("random",) * T
    tips, w = TU.random_alignment(n, P, rng)
    topo = {"ladder": TU.ladder_topology, "balanced": TU.balanced_topology}
    pids, bls, hs, bds, ras = TU.rooted_batch(
        n, T, rng, [topo[k](n, rooted=True) if k in topo else None for k in kinds],
        [k == "random-isochronous" for k in kinds])
    rcounts = [1 if t % 2 == 0 else N - 1 for t in range(T)]
    spec = O.make_spec(n, P, subst, site, "strict", use_tip_states=use_tip_states)
    blocks = {}
    if subst == "GTR":
        blocks["GTR rates"], blocks["frequencies"] = TU.random_gtr_params(T, rng)
    if site != "constant":
        blocks["Weibull shape"] = rng.uniform(0.3, 2.0, size=(T, 1))
    return dict(n=n, P=P, T=T, N=N, kinds=kinds, tips=tips, w=w, pids=pids, bls=bls, hs=hs, bds=bds,
                ras=ras, rcounts=rcounts, rates=_rates(rng, T, N, rcounts), spec=spec, subst=subst,
                site=site, pr=_params(spec, T, **blocks), what=what or f"n={n} P={P} T={T}")


def _compare(eng, c, resc, oracle):
    """Every output of the rooted calls of engine `eng` on case c against the oracle's.  Returns
    the largest relative error of the ratio vector over the trees; every figure is printed before
    it is asserted."""
    og = oracle["grad"]
    args = (c["pids"], c["bls"], c["pr"], c["rates"])
    ll = eng.rooted_log_likelihoods(*args, c["hs"], c["bds"], resc, True)
    where = f"{c['what']} rescaling={resc} loglik: {eng.last_call_info()[0]}"
    ll0 = eng.rooted_log_likelihoods(*args, c["hs"], c["bds"], resc, False)
    g = eng.rooted_gradients(*args, c["rcounts"], c["hs"], c["bds"], c["ras"], resc)
    where += f" gradient: {eng.last_call_path()} {eng.last_call_info()}"
    worst = 0.0
    for t in range(c["T"]):
        at = f"tree {t} ({c['kinds'][t]}, {c['rcounts'][t]} rates) {where}"
        gt = g[t].gradient
        oc = og["clock_model"][t, :1] if c["rcounts"][t] == 1 else og["clock_model"][t]
        assert gt["ratios_root_height"].shape == (c["n"] - 1,), at
        assert gt["clock_model"].shape == oc.shape, at
        figs = {"ll+jac": abs(ll[t] - oracle["ll_jac"][t]) / abs(oracle["ll_jac"][t]),
                "ll": abs(ll0[t] - oracle["ll_plain"][t]) / abs(oracle["ll_plain"][t]),
                "gradient ll": abs(g[t].log_likelihood - og["log_likelihood"][t]) /
                abs(og["log_likelihood"][t]),
                "ratios": _rel(gt["ratios_root_height"], og["ratios_root_height"][t]),
                "root height": abs(gt["ratios_root_height"][-1] - og["ratios_root_height"][t, -1]) /
                max(np.max(np.abs(og["ratios_root_height"][t])), 1e-300),
                "clock": _rel(gt["clock_model"], oc)}
        if c["site"] != "constant":
            figs["site"] = abs(gt["site_model"][0] - og["site_model"][t]) / \
                max(1.0, abs(og["site_model"][t]))
        print("  ".join(f"{k} {v:.2e}" for k, v in figs.items()), "|", at)
        worst = max(worst, figs["ratios"])
        for key in ("ll+jac", "ll", "gradient ll"):
            assert figs[key] <= RTOL, (key, figs[key], at)
        assert np.all(np.isfinite(gt["ratios_root_height"])), at
        assert _close(gt["ratios_root_height"], og["ratios_root_height"][t]), (figs["ratios"], at)
        assert _close(gt["clock_model"], oc), (figs["clock"], at)
        if c["site"] != "constant":
            assert figs["site"] <= 1e-9, (figs["site"], at)
        if c["subst"] == "GTR":
            assert np.allclose(gt["substitution_model"], oracle["subst"][t], rtol=1e-6, atol=1e-4), \
                (gt["substitution_model"], oracle["subst"][t], at)
    return worst


# ---- 2. every form of the chain rule -----------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _size_class_case(n):
    rng = np.random.default_rng(5000 + n)
    return _case(n, 12, 4, rng, kinds=TREE_KINDS, what=f"size class n={n}")


@pytest.mark.parametrize("n,rescaling", [(n, r) for n in SIZE_CLASSES for r in (False, True)
                                         if r or n <= 280])
def test_ratio_gradient_size_classes(n, rescaling):
    """Taxa counts on both sides of every switch of the rooted chain rule (SIZE_CLASSES, above):
    four trees per size -- random with random tip dates, random isochronous (every epoch term on
    its equal-bounds branch), a ladder (the longest dependent chain: every bottom-up step reads
    the node just written) and a balanced tree -- with a strict clock on trees 0 and 2 and
    per-branch rates on 1 and 3, 12 patterns, JC69 + weibull+4.  Rescaling off and on; at 400 taxa
    on only, where the oracle itself underflows to -inf without it.
    All outputs at the suite's bars, the ratio vector at 1e-10 of its largest entry."""
    c = _size_class_case(n)
    eng = _engine("JC69", "weibull+4", "strict", c["tips"], c["w"])
    _compare(eng, c, rescaling, _oracle(c, rescaling))


# ---- 3. degenerate trees in every form ---------------------------------------------------------

@pytest.mark.parametrize("n", [20, 100, 200, 258, 300])
def test_degenerate_rooted_tree_size_classes(n):
    """test_degenerate_rooted_tree_poisons_only_what_the_reference_poisons (test_gpu_parity.py) at
    one size per form of the chain rule -- wave<1>, <2>, <4>, the lane-0 loop over LDS, the
    global-memory fallback: a height on its bound makes that node's log-time derivative 1 / 0, and
    non-finite entries must appear exactly where the reference's loops put them, all others match.
    A random tree with the first internal node degenerate (node 0 of the recurrences), and a
    ladder.  On a ladder every other internal node is an ancestor of the first, so there the node
    in the middle of the chain is the degenerate one: the lower half stays finite.
    Each call runs twice on one engine and must give the same bits: the forms differ in what they
    leave behind in LDS, which is not cleared between workgroups."""
    rng = np.random.default_rng(1700 + n)
    P, N, resc = 8, 2 * n - 1, n >= 200
    tips, w = TU.random_alignment(n, P, rng)
    pids, bls, hs, bds, ras = TU.rooted_batch(n, 2, rng, [None, TU.ladder_topology(n, rooted=True)])
    bds = bds.copy()
    degenerate = (n, n + (n - 1) // 2)
    for t, v in enumerate(degenerate):
        bds[t, v] = hs[t, v]
    rates = np.full((2, N - 1), 0.05)
    eng = _engine("JC69", "constant", "strict", tips, w)
    spec = O.make_spec(n, P, "JC69", "constant", "strict")
    args = (pids, bls, np.ones((2, 1)), rates, [1, 1], hs, bds, ras, resc)
    with np.errstate(all="ignore"):
        first = eng.rooted_gradients(*args)
        again = eng.rooted_gradients(*args)
        og = O.rooted_gradients(spec, tips, w, *args)
    assert np.all(np.isfinite(og["log_likelihood"]))
    for t, kind in enumerate(("random", "ladder")):
        at = f"n={n} {kind} tree, node {degenerate[t]} degenerate, rescaling={resc}, " \
             f"{eng.last_call_path()} {eng.last_call_info()}"
        g, want = first[t].gradient["ratios_root_height"], og["ratios_root_height"][t]
        fin = np.isfinite(want)
        assert not np.all(fin) and fin.sum() >= 3, at
        assert np.array_equal(np.isfinite(g), fin), (at, g, want)
        print(f"ratios {_rel(g[fin], want[fin]):.2e} over {fin.sum()} finite of {n - 1} | {at}")
        assert _close(g[fin], want[fin]), (_rel(g[fin], want[fin]), at)
        assert abs(first[t].log_likelihood - og["log_likelihood"][t]) <= \
            RTOL * abs(og["log_likelihood"][t]), at
        assert _close(first[t].gradient["clock_model"], og["clock_model"][t, :1]), at
        for key, val in first[t].gradient.items():
            assert val.tobytes() == again[t].gradient[key].tobytes(), (key, at)
        assert first[t].log_likelihood == again[t].log_likelihood, at


# ---- 4. every route of the walk ----------------------------------------------------------------

ROUTES = {
    # name: (n, P, T, substitution, site, switches, engine keywords, kernel)
    "default-batch": (50, 60, 40, "JC69", "weibull+4", {}, {}, WALK_KERNEL),
    "arena-several-launches": (50, 60, 40, "JC69", "weibull+4",
                               {"MI_PHYLO_GRADIENT_STORE": "arena", "MI_PHYLO_PLV_BYTES": "3000000"},
                               {}, WALK_KERNEL),
    "second-generation": (33, 70, 5, "JC69", "weibull+4", {"MI_PHYLO_GRADIENT_WALK": "v2"}, {},
                          ("gradient_walk_kernel",)),
    "hbm": (33, 70, 5, "GTR", "weibull+4", {"MI_PHYLO_GRADIENT_PATH": "hbm"}, {},
            ("gradient_hbm_kernel",)),
    "eight-categories": (20, 70, 3, "JC69", "weibull+8", {}, {}, None),
    "one-category-gtr": (20, 65, 3, "GTR", "constant", {}, {}, None),
    "two-categories-gtr": (20, 65, 3, "GTR", "weibull+2", {}, {}, None),
    "separate-finalize": (14, 70, 6, "JC69", "weibull+4", {"MI_PHYLO_FUSE_FINALIZE": "0"}, {}, None),
    "tip-partials": (14, 70, 3, "JC69", "weibull+4", {}, {"use_tip_states": False}, None),
    "gtr-two-blocks": (100, 20, 2, "GTR", "weibull+4", {}, {}, None),
}


def _outputs(eng, c, resc):
    args = (c["pids"], c["bls"], c["pr"], c["rates"])
    g = eng.rooted_gradients(*args, c["rcounts"], c["hs"], c["bds"], c["ras"], resc)
    out = [eng.rooted_log_likelihoods(*args, c["hs"], c["bds"], resc, True),
           np.array([x.log_likelihood for x in g])]
    for x in g:
        out += [x.gradient[k] for k in sorted(x.gradient)]
    return out


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_rooted_routes_match_oracle(route, monkeypatch):
    """The rooted form of the walk (two children at the root) in the look-up walk with its
    vectors in LDS and in the arena (one launch and several), the second-generation walk, the
    HBM-streamed kernel, the per-group pass of more than four categories, one and two categories,
    tip partials instead of tip states, the separate reduction and finalize launches
    (bit-identical to the fused ones), and the finite-difference substitution gradient with the
    Jacobian added to both of its log-likelihoods at a size where the Jacobian sum strides.
    Switches are read when the engine is created.  Every output against the oracle, rescaling
    off and on, random trees with random tip dates, strict and per-branch clock alternating."""
    n, P, T, subst, site, switches, kw, kernels = ROUTES[route]
    rng = np.random.default_rng(4000 + sorted(ROUTES).index(route))
    c = _case(n, P, T, rng, subst, site, use_tip_states=int(kw.get("use_tip_states", True)),
              what=f"route {route} n={n} P={P} T={T} {subst}+{site}")
    default = _engine(subst, site, "strict", c["tips"], c["w"]) if route == "separate-finalize" else None
    for name, value in switches.items():
        monkeypatch.setenv(name, value)
    eng = _engine(subst, site, "strict", c["tips"], c["w"], **kw)
    for resc in (False, True):
        _compare(eng, c, resc, _oracle(c, resc))
        at = f"{c['what']} rescaling={resc} {eng.last_call_path()} {eng.last_call_info()}"
        if kernels:
            assert eng.last_call_info()[0] in kernels, at
        if route == "arena-several-launches":
            assert "store=arena" in eng.last_call_path() and eng.last_call_launches()[0] > 1, at
        if default is not None:
            for a, b in zip(_outputs(eng, c, resc), _outputs(default, c, resc)):
                assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), at
