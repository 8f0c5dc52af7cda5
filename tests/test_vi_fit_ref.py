"""The reference of the variational fit's optimiser (tests/vi_fit_ref.py) against closed forms,
and the bindings of the new calls.  No GPU."""
import ctypes
import math

import numpy as np
import pytest

import vi_fit_ref as F


def _ulps(a, b):
    return abs(a - b) / np.spacing(abs(b)) if b != 0.0 else (0.0 if a == 0.0 else math.inf)


@pytest.mark.parametrize("g", [3.5, -3.5, 0.25, -1e-3, 0.0, 1e-300, -1e-300, 1e300, -1e300, 1.7e308])
def test_first_adam_step_closed_form(g):
    """From zero moments, delta = step g / (|g| + epsilon) within 2 ulp.  At |g| = 1e300 the square
    g g overflows (the stored v is +inf, as the plain rule gives it, and as the reference's
    grad ** 2 does): the root in delta is taken in a scaled range there, so the step is still
    Adam's, the step size in the direction of g."""
    o = F.Options()
    step = 0.37
    s = F.State(np.array([1.5]), np.zeros((0, 2)), sbn_step_size=step)
    after, row = F.update(s, o, np.array([g]), np.zeros((0, 2)), [0.0], [0.0], [0.0], [0.0])
    delta = after.log_params[0] - 1.5
    want = step * g / (abs(g) + o.adam_epsilon)
    got, _, _ = F.adam(0.0, 0.0, 0.0, np.float64(g), step, o.adam_beta0, o.adam_beta1, o)
    print("g", g, "delta", float(got), "closed form", want, "ulps", _ulps(float(got), want))
    assert _ulps(float(got), want) <= 2
    assert abs(delta - want) <= 4 * np.spacing(1.5) and row[5] == 1.0
    assert after.sbn_moments[1, 0] == (np.inf if abs(g) > 1e200 else (1.0 - o.adam_beta1) * (g * g))


def test_the_scaled_root_is_the_plain_root():
    """Above 2^500 and below the overflow of v / (1 - b1) both forms of the root exist: the same bits, with
    and without an earlier second moment; and an infinite second moment gives a step of zero."""
    o = F.Options()
    rng = np.random.default_rng(2)
    g = np.concatenate([rng.uniform(1.0, 2.0, 200) * 2.0 ** rng.integers(500, 506, 200) * rng.choice([-1, 1], 200)])
    for old_v in (np.zeros(200), rng.uniform(0.5, 1.0, 200) * 2.0 ** rng.integers(900, 1010, 200)):
        old_m = rng.normal(size=200) * 1e150
        got = F.adam(0.0, old_m, old_v, g, 0.01, 0.9 ** 3, 0.999 ** 3, o)
        keep = F.HUGE_GRADIENT
        try:
            F.HUGE_GRADIENT = np.inf   # (the plain rule everywhere)
            want = F.adam(0.0, old_m, old_v, g, 0.01, 0.9 ** 3, 0.999 ** 3, o)
        finally:
            F.HUGE_GRADIENT = keep
        assert np.all(np.isfinite(want[0])) and np.all(want[0] != 0.0)
        for a, b in zip(got, want):
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    delta, _, v = F.adam(0.0, 0.0, np.inf, np.array([1e300, 3.0]), 0.01, 0.9, 0.999, o)
    assert delta.tolist() == [0.0, 0.0] and np.all(np.isinf(v))


def test_running_products():
    o = F.Options()
    s = F.State(np.zeros(1), np.array([[0.0, 1.0]]))
    for t in range(1, 51):
        s, _ = F.update(s, o, np.ones(1), np.zeros((1, 2)), [0.0], [0.0], [0.0], [0.0])
        assert s.successes == t and s.steps == t
        assert abs(s.b0 - o.adam_beta0 ** t) <= 1e-14 * o.adam_beta0 ** t
        assert abs(s.b1 - o.adam_beta1 ** t) <= 1e-14 * o.adam_beta1 ** t


@pytest.mark.parametrize("S", [1, 7, 2000])
def test_beta_schedule(S):
    want = np.maximum(np.arange(1, S + 1) / S, 0.001)
    got = np.array([F.beta(t, S) for t in range(S)])
    assert got.tobytes() == want.astype(np.float64).tobytes()
    assert all(F.beta(t, S) == 1.0 for t in (S, S + 1, 10 * S))
    assert F.beta(0, 0) == 1.0 and F.beta(123, 0) == 1.0


@pytest.mark.parametrize("bad", ["nan_sbn", "inf_q", "-inf_q", "sigma_zero", "sigma_negative"])
def test_a_failed_step_halves_the_step_sizes_and_nothing_else(bad):
    o = F.Options()
    rng = np.random.default_rng(1)
    s = F.State(rng.normal(size=5), np.stack([rng.normal(size=4), rng.uniform(0.1, 1.0, 4)], axis=1),
                rng.uniform(size=(2, 5)), rng.uniform(size=(2, 4, 2)), 0.9 ** 3, 0.999 ** 3, [0.02, 0.04], 0.001, 5, 3, 17)
    g_sbn, g_q = rng.normal(size=5), rng.normal(size=(4, 2))
    if bad == "nan_sbn":
        g_sbn[-1] = np.nan
    elif bad == "inf_q":
        g_q[-1, 0] = np.inf
    elif bad == "-inf_q":
        g_q[-1, 1] = -np.inf
    else:
        # the sigma of variable 2 that the step takes to exactly 0, resp. below: minus the step's delta
        g_q[2, 1] = -50.0
        moved, _, _ = F.adam(0.0, s.q_moments[0, 2, 1], s.q_moments[1, 2, 1], -50.0, 0.04, s.b0 * o.adam_beta0,
                             s.b1 * o.adam_beta1, o)
        assert moved < 0.0
        s.q_params[2, 1] = -moved if bad == "sigma_zero" else -moved * 0.75
    after, row = F.update(s, o, g_sbn, g_q, [1.0, 2.0], [0.0, 0.0], [0.5, 0.5], [0.25, 0.25])
    assert row[5] == 0.0 and after.steps == 6 and after.successes == 3
    assert after.step_size.tolist() == [0.01, 0.02] and row[3:5].tolist() == [0.01, 0.02]
    assert after.sbn_step_size == s.sbn_step_size and after.first_sample == 17
    for name in ("log_params", "q_params", "sbn_moments", "q_moments"):
        assert getattr(after, name).tobytes() == getattr(s, name).tobytes()
    assert (after.b0, after.b1) == (s.b0, s.b1)
    assert row[1] == ((1.0 - 0.5 - 0.25) + (2.0 - 0.5 - 0.25)) / 2


def test_sigma_just_above_zero_is_a_success():
    o = F.Options()
    s = F.State(np.zeros(1), np.array([[0.0, 0.05]]), step_size=[0.04, 0.04])
    after, row = F.update(s, o, np.zeros(1), np.array([[0.0, -1.0]]), [0.0], [0.0], [0.0], [0.0])
    assert row[5] == 1.0 and 0.0 < after.q_params[0, 1] < 0.011
    assert after.log_params[0] == 0.0 and after.q_params[0, 0] == 0.0   # (zero gradient, zero moments: it stays put)


def test_trace_sums():
    f = np.array([-3.0, -1.0, -2.0])
    elbo, bound = F.trace_sums(f, np.zeros(3), np.zeros(3), np.zeros(3))
    assert elbo == -2.0
    assert abs(bound - (math.log(np.sum(np.exp(f))) - math.log(3))) < 1e-15
    assert F.trace_sums([-math.inf] * 2, [0, 0], [0, 0], [0, 0])[1] == -math.inf


def test_bindings():
    """Every new symbol is exported and bound, the options struct has the header's layout and the
    defaults are the reference's."""
    from libsbn_amd import _capi
    import libsbn_amd as L
    lib = _capi.load()
    for name in ("mi_vi_default_options", "mi_engine_vi_create", "mi_vi_destroy", "mi_vi_sizes", "mi_vi_step_device",
                 "mi_vi_fit", "mi_vi_trace", "mi_vi_update", "mi_vi_update_device", "mi_vi_get_state", "mi_vi_set_state",
                 "mi_vi_particles"):
        assert name in _capi.SYMBOLS and hasattr(lib, name)
    assert ctypes.sizeof(_capi.ViOptions) == 6 * 4 + 8 * 8 + 2 * 8 + 4 * 4
    o = _capi.ViOptions()
    assert lib.mi_vi_default_options(ctypes.byref(o)) == 0
    assert (o.particle_count, o.rows, o.estimator, o.anneal_steps, o.max_steps) == (10, 3, 1, 0, 1000)
    assert (o.prior_rate, o.sbn_step_size, o.step_decay) == (10.0, 0.001, 0.99)
    assert (o.adam_beta0, o.adam_beta1, o.adam_epsilon) == (0.9, 0.999, 1e-8)
    assert lib.mi_vi_default_options(None) != 0
    for name in ("vi_create",):
        assert hasattr(L.Engine, name)
    for name in ("step_device", "fit", "update", "update_device", "state", "set_state", "particles", "trace", "estimate", "close"):
        assert hasattr(L.VariationalFit, name)
