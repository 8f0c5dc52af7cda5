"""Reference of the device-resident variational fit (TEST INFRASTRUCTURE ONLY; DESIGN.md 4.24,
include/mi_phylo.h): the optimiser's rule, the beta schedule, the trace row and the failure rule in
plain numpy, written from the header's text, and one step as the composition of an engine's
existing host-form calls with seed, first_sample + t K and beta_t computed here.  Every one of
those calls is held to a reference of its own elsewhere in the suite."""
import copy
import math
from dataclasses import dataclass, field

import numpy as np


@dataclass
class Options:
    particle_count: int = 10
    rows: int = 3
    estimator: str = "vimco"
    anneal_steps: int = 0
    prior_rate: float = 10.0
    step_decay: float = 0.99
    adam_beta0: float = 0.9
    adam_beta1: float = 0.999
    adam_epsilon: float = 1e-8
    seed: int = 0
    checked: int = None   # variables 0 .. checked-1 must keep a positive sigma (None: all)


@dataclass
class State:
    log_params: np.ndarray
    q_params: np.ndarray
    sbn_moments: np.ndarray = None   # [2][P]
    q_moments: np.ndarray = None     # [2][V][2]
    b0: float = 1.0
    b1: float = 1.0
    step_size: np.ndarray = field(default_factory=lambda: np.array([0.001, 0.001]))
    sbn_step_size: float = 0.001
    steps: int = 0
    successes: int = 0
    first_sample: int = 0

    def __post_init__(self):
        self.log_params = np.array(self.log_params, np.float64)
        self.q_params = np.array(self.q_params, np.float64).reshape(-1, 2)
        self.step_size = np.array(self.step_size, np.float64)
        if self.sbn_moments is None:
            self.sbn_moments = np.zeros((2,) + self.log_params.shape)
        if self.q_moments is None:
            self.q_moments = np.zeros((2,) + self.q_params.shape)


def beta(t, anneal_steps):
    """beta of step t (counted from 0)."""
    if anneal_steps == 0:
        return 1.0
    return float(max(min(np.float64(t + 1) / np.float64(anneal_steps), 1.0), 0.001))


HUGE_GRADIENT, GRADIENT_SCALE = 2.0 ** 500, 2.0 ** -600


def adam(param, m, v, g, step, b0, b1, o):
    """One element-wise ascent step with b0, b1 already advanced: (param, m, v) after it.  Where
    |g| > 2^500 the root in delta is taken of the same sum in a range scaled by 2^-600 (g g may
    overflow there; v is stored as the plain rule gives it, +inf included)."""
    with np.errstate(all="ignore"):
        g, c = np.asarray(g, np.float64), GRADIENT_SCALE
        old_v = v
        m = (o.adam_beta0 * m) + ((1.0 - o.adam_beta0) * g)
        v = (o.adam_beta1 * v) + ((1.0 - o.adam_beta1) * (g * g))
        gs = g * c
        vs = (o.adam_beta1 * ((old_v * c) * c)) + ((1.0 - o.adam_beta1) * (gs * gs))
        root = np.where(np.abs(g) > HUGE_GRADIENT, np.sqrt(vs / (1.0 - b1)) / c, np.sqrt(v / (1.0 - b1)))
        delta = (step * (m / (1.0 - b0))) / (root + o.adam_epsilon)
        return param + delta, m, v


def trace_sums(ll, lprior, lqt, lqb):
    """(elbo, bound) of the particles' terms at beta = 1."""
    f = [((float(a) + float(b)) - float(c)) - float(d) for a, b, c, d in zip(ll, lprior, lqt, lqb)]
    K = len(f)
    total = 0.0
    for x in f:
        total = total + x
    top = -math.inf
    for x in f:
        if x > top:
            top = x
    if top == -math.inf:
        return total / K, top
    s = 0.0
    for x in f:
        s = s + (math.exp(x - top) if not math.isnan(x) else math.nan)
    return total / K, (top + (math.log(s) if s > 0 else (-math.inf if s == 0 else math.nan))) - math.log(K)


def update(state, o, g_sbn, g_q, ll, lprior, lqt, lqb):
    """The state after one update and the step's trace row."""
    s = copy.deepcopy(state)
    g_sbn, g_q = np.asarray(g_sbn, np.float64), np.asarray(g_q, np.float64).reshape(s.q_params.shape)
    b0, b1 = s.b0 * o.adam_beta0, s.b1 * o.adam_beta1
    steps = np.broadcast_to(s.step_size, s.q_params.shape)
    ok = bool(np.all(np.isfinite(g_sbn)) and np.all(np.isfinite(g_q)))
    if ok:
        phi, ms, vs = adam(s.log_params, s.sbn_moments[0], s.sbn_moments[1], g_sbn, s.sbn_step_size, b0, b1, o)
        q, mq, vq = adam(s.q_params, s.q_moments[0], s.q_moments[1], g_q, steps, b0, b1, o)
        sigma = q[:o.checked, 1]
        ok = bool(np.all(sigma > 0.0) and np.all(np.isfinite(sigma)))
    if ok:
        s.log_params, s.q_params = phi, q
        s.sbn_moments, s.q_moments = np.stack([ms, vs]), np.stack([mq, vq])
        s.b0, s.b1, s.successes = b0, b1, s.successes + 1
        s.step_size = s.step_size * o.step_decay
    else:
        s.step_size = s.step_size / 2.0
    elbo, bound = trace_sums(ll, lprior, lqt, lqb)
    row = np.array([beta(state.steps, o.anneal_steps), elbo, bound, s.step_size[0], s.step_size[1], 1.0 if ok else 0.0])
    s.steps = state.steps + 1
    return s, row


class Composer:
    """One step from an engine's host-form calls (a libsbn_amd.Engine, or anything with the same
    methods).  The support's tables are computed once."""

    def __init__(self, engine, support_ids, options, model_params=None):
        import libsbn_amd as L
        self.e, self.ids = engine, np.ascontiguousarray(support_ids, np.int32)
        self.model_params = model_params
        self.support = engine.sbn_index(self.ids)
        self.descent = engine.sbn_descent(self.support)
        self.table = engine.psp_table(self.support)
        if options.rows == 1:   # (the split model's variables are the rootsplits alone)
            S = self.table.rootsplit_count
            self.table = L.PspTable(self.table.psp_of_pcsp, S, S)
        self.parameter_count, self.variable_count = self.support.parameter_count, self.table.variable_count
        self.o = copy.copy(options)
        self.o.checked = self.table.rootsplit_count   # (the split variables)

    def particles(self, state):
        """The particles of step state.steps: trees, the index rows, the draw."""
        e, o, T0 = self.e, self.o, len(self.ids)
        base = state.first_sample + state.steps * o.particle_count
        pid, _, _, _ = e.sbn_sample(self.support, self.descent, state.log_params, o.particle_count, o.seed, first_sample=base)
        both = e.sbn_index(np.concatenate([self.ids, pid]), support_tree_count=T0)
        index = e.psp_index(both, self.table, rows=o.rows, trees=slice(T0, None))
        draw = e.branch_model_sample(index, state.q_params, o.seed, first_sample=base, prior_rate=o.prior_rate)
        return pid, both, index, draw

    def gradients(self, state):
        """(SBN gradient, q gradient, logL, log prior, log q topology, log q branch) of the step."""
        e, o, T0 = self.e, self.o, len(self.ids)
        pid, both, index, draw = self.particles(state)
        params = None if self.model_params is None else np.tile(self.model_params, (o.particle_count, 1))
        grads = e.gradients(pid, draw.branch_lengths, params, gradient_blocks=("branch_lengths",))
        ll = np.array([x.log_likelihood for x in grads])
        g = np.stack([x.gradient["branch_lengths"] for x in grads])
        _, lqt = e.sbn_log_prob(both, state.log_params, trees=slice(T0, None))
        g_q, log_f = e.branch_model_gradient(index, state.q_params, draw, g, ll, log_q_topology=lqt,
                                             beta=beta(state.steps, o.anneal_steps), prior_rate=o.prior_rate)
        g_sbn, _, _ = e.sbn_topology_gradient(both, state.log_params, log_f, estimator=o.estimator, trees=slice(T0, None))
        return g_sbn, g_q, ll, draw.log_prior, lqt, draw.log_q

    def step(self, state):
        """(state after the step, trace row)."""
        return update(state, self.o, *self.gradients(state))


def state_of(s):
    """A State from anything with the fields of libsbn_amd.ViState."""
    return State(s.log_params, s.q_params, np.array(s.sbn_moments), np.array(s.q_moments), s.b0, s.b1, s.step_size,
                 s.sbn_step_size, s.steps, s.successes, s.first_sample)
