"""The branch-length Hessian call per branch, against the analytic long-double reference of
tests/dense_ref.py, at the edges: branch lengths 0, 1e-8 and 10 in one tree, pattern counts on
and around the kernels' tile widths and P = 1, ambiguity masks and real-valued tip vectors,
weights from 1e-3 to 1e6 and 0, a 100-taxon ladder, DS1 at its own branch lengths.

Bounds, per branch j (W = sum of the weights, rho = r_max max_i sum_j |Q_ij|; dense_ref.tolerances):
    log L   1e-10 relative
    g_j     1e-10 (A1_j + W rho)              A1_j = sum_p w_p |D1_p / L_p|
    S_j     1e-10 (S_j + W rho^2)
    H_j     1e-10 (A2_j + S_j + W rho^2)      A2_j = sum_p w_p |D2_p / L_p|
    root and fixed entries exactly 0
1e-10 is the project's parity bound.  The W rho terms: on a saturated branch q.(Q L) cancels to
~ e^(-lambda r t) from terms of size rho, so an FP64 pre-order evaluator's absolute error there is
~ 1e-16 W rho whatever the true value; on ordinary branches the term is of the size of the scale
itself.  tests/test_dense_ref.py holds FP64 evaluators to 1e-12 in the same form on these inputs.

Each case prints max_j error_j / bound_j per quantity, one "ratio ..." line per call; run with
-s (or -rP) to see them.  DESIGN.md 4.8 records the worst per kernel and store."""
import pytest

import hessian_edge_cases as E

pytestmark = pytest.mark.gpu


def _engine(x):
    import libsbn_amd as L
    spec = L.PhyloModelSpecification("GTR", x.site, "strict")
    if x.states is None:
        return L.Engine(spec, None, x.w, device=0, use_tip_states=False, tip_partials=x.vectors)
    return L.Engine(spec, x.states, x.w, device=0)


def _path(eng, c, rescaled):
    p = eng.last_call_path()
    assert p.startswith(c.kernel + " ") and " hess" in p and ("rescaled" in p) == rescaled, p
    assert f" K={c.K}" in p, p
    assert f" store={c.store} " in p, p
    assert eng.last_call_info()[0] == c.kernel


@pytest.mark.parametrize("name", [c.name for c in E.CASES])
def test_every_branch_matches_the_analytic_reference(name, monkeypatch):
    c = E.BY_NAME[name]
    x = E.inputs(name)
    refs = E.references(name)
    for key, value in c.env.items():
        monkeypatch.setenv(key, value)
    eng = _engine(x)
    for rescaling in c.rescaling:
        ll, g, h, s = eng.branch_hessian(x.pids, x.bls, x.pr, rescaling=rescaling, squared_gradient=True)
        _path(eng, c, rescaling)
        r = E.ratios(refs, ll, g, h, s)
        print(f"ratio {name} {c.kernel} store={c.store} rescaled={int(rescaling)} " +
              " ".join(f"{k}={v:.3e}" for k, v in r.items()))
        assert E.within(r), (rescaling, r)
