"""The 20-state engine (kernels_aa.hip) per branch, against the analytic long-double reference of
tests/dense_ref.py, at the edges and in every kernel form: branch lengths 0, 1e-8 and 10 in one
tree, pattern counts on and around the tile groups, schedule-window refills, ring spills, padding
waves, calls split into several launches, gaps and one-state columns, weights from 1e-3 to 1e6
and 0, a rooted tree (tests/aa_edge_cases.py).

Bounds (W = sum of the weights, rho = r_max max_i sum_j |Q_ij|, rho_site = max_k |dr_k/dalpha|
max_i sum_j |Q_ij|; aa_edge_cases.bounds):
    log L            1e-10 relative
    g_j              1e-10 (A1_j + W rho)                     A1_j = sum_p w_p |D1_p / L_p|
    d/d shape        1e-10 (A_site + W rho_site sum_j t_j)
    d/d clock rate   1e-10 sum_j t_j (A1_j + W rho)
    root and fixed entries exactly 0
1e-10 is the project's parity bound; tests/test_dense_ref.py holds the FP64 oracle to a tenth of
these on the same inputs.  Every form must also say in last_call_path() that it ran the kernels,
tiles per wave and ring sizes it names, and every form's outputs are bit-identical to those of
the automatic choice.

Each case prints max_j error_j / bound_j per quantity, one "ratio <case> <form> ..." line per
form; run with -s (or -rP) to see them.  DESIGN.md 4.6 records the worst per form."""
import numpy as np
import pytest

import aa_edge_cases as E

pytestmark = pytest.mark.gpu


def _engine(x, form, monkeypatch, plv_bytes=None):
    import libsbn_amd as L
    for key, value in form.env.items():
        monkeypatch.delenv("MI_PHYLO_" + key, raising=False)
        if value:
            monkeypatch.setenv("MI_PHYLO_" + key, value)
    monkeypatch.delenv("MI_PHYLO_PLV_BYTES", raising=False)
    if plv_bytes is not None:
        monkeypatch.setenv("MI_PHYLO_PLV_BYTES", str(plv_bytes))
    spec = L.PhyloModelSpecification("WAG" if x.case.model == "WAG" else "reversible", x.site, "strict")
    model = None if x.case.model == "WAG" else x.model
    if x.partials is not None:
        return L.Engine(spec, None, x.w, device=0, use_tip_states=False, tip_partials=x.partials,
                        reversible_model=model)
    return L.Engine(spec, x.states, x.w, device=0, reversible_model=model)


def _compute_units():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _ran_as_named(eng, form, c, evals, gradient):
    """A switch that silently falls back fails here."""
    kernel, fields = E.expected(form, c, evals, _compute_units(), gradient)
    assert eng.last_call_path() == kernel + fields, (form.name, eng.last_call_path(), kernel + fields)
    assert eng.last_call_info()[0] == kernel, (form.name, eng.last_call_info())
    if not gradient:
        assert "pre-ring" not in eng.last_call_path()


def _unrooted(x, form, monkeypatch, refs, plv_bytes=None, launches=None):
    """log_likelihoods and gradients of one engine: (outputs, ratios)."""
    c = x.case
    T = len(x.pids)
    eng = _engine(x, form, monkeypatch, plv_bytes)
    try:
        ll = eng.log_likelihoods(x.pids, x.bls, x.pr)
        chunk = T if plv_bytes is None else plv_bytes // E.arena_bytes(c, False)
        _ran_as_named(eng, form, c, min(T, chunk), False)
        if launches == "log_likelihoods":
            assert eng.last_call_launches()[0] == 3
        g = eng.gradients(x.pids, x.bls, x.pr)
        chunk = T if plv_bytes is None else plv_bytes // E.arena_bytes(c, True)
        _ran_as_named(eng, form, c, min(T, chunk), True)
        if launches == "gradients":
            assert eng.last_call_launches()[0] == 3
    finally:
        eng.close()
    out = dict(ll=ll, gll=np.array([v.log_likelihood for v in g]),
               g=np.stack([v.gradient["branch_lengths"] for v in g]))
    if c.K > 1:
        out["site"] = np.array([v.gradient["site_model"][0] for v in g])
    r = E.ratios(refs, x, out["ll"], out["g"], out.get("site"))
    r["logL-of-gradients"] = E.ratios(refs, x, out["gll"])["logL"]
    return out, r


def _rooted(x, form, monkeypatch, refs):
    c = x.case
    eng = _engine(x, form, monkeypatch)
    try:
        ll = eng.rooted_log_likelihoods(x.pids, x.bls, x.pr, x.rates, x.heights, x.bounds)
        _ran_as_named(eng, form, c, 1, False)
        g = eng.rooted_gradients(x.pids, x.bls, x.pr, x.rates, x.rate_counts, x.heights, x.bounds, x.ratios)
        _ran_as_named(eng, form, c, 1, True)
    finally:
        eng.close()
    out = dict(ll=ll, gll=np.array([v.log_likelihood for v in g]),
               site=np.array([v.gradient["site_model"][0] for v in g]),
               clock=np.array([v.gradient["clock_model"][0] for v in g]))
    r = E.ratios(refs, x, out["ll"], site=out["site"], clock=out["clock"])
    r["logL-of-gradients"] = E.ratios(refs, x, out["gll"], jacobian=False)["logL"]
    return out, r


@pytest.mark.parametrize("name", [c.name for c in E.CASES])
def test_every_branch_matches_the_analytic_reference_in_every_form(name, monkeypatch):
    c = E.BY_NAME[name]
    x = E.inputs(name)
    refs = E.references(name)
    runs = [{}]
    if c.launches:  # two and a half evaluations of the gradient arena; of the log-likelihood arena
        runs = [dict(plv_bytes=5 * E.arena_bytes(c, True) // 2, launches="gradients"),
                dict(plv_bytes=5 * E.arena_bytes(c, False) // 2, launches="log_likelihoods")]
    first, failed = None, []
    for form in E.FORMS:
        for run in runs:
            out, r = _rooted(x, form, monkeypatch, refs) if c.rooted else \
                _unrooted(x, form, monkeypatch, refs, **run)
            print(f"ratio {name} {form.name}" + (f" launches-of-{run['launches']}" if run else "") + " " +
                  " ".join(f"{k}={v:.3e}" for k, v in r.items()))
            if not E.within(r):
                failed.append((form.name, run, r))
            if first is None:
                first = out
            for key, got in out.items():  # every form and launch split: the same bits as `auto`
                assert np.array_equal(got, first[key]), (form.name, run, key)
    assert not failed, failed
