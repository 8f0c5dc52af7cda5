"""Marginal ancestral-state and rate-category posteriors per pattern
(mi_engine_ancestral_states_unrooted, Engine.ancestral_states) against
tests/ancestral_ref.py (long double, no pre-order pass): entries of at least 1e-6 to 1e-10
relative, the project's standing tolerance, smaller ones to the absolute floor measured in
tests/test_ancestral_ref.py; rows sum to 1 within 8 x 2^-53 (2 K x 2^-53 for more than four
categories); map states wherever the reference's two largest posteriors are 1e-9 apart."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ancestral_cases as AC
import ancestral_ref as A
import oracle_lib as O
import tree_utils as TU

pytestmark = pytest.mark.gpu

KERNEL = "ancestral_hbm_kernel"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("state_posteriors", "log_likelihoods", "map_states", "category_posteriors", "pattern_rates",
          "tip_posteriors")


def _path(eng, trees, rescaled=False):
    p = eng.last_call_path()
    assert p.startswith(KERNEL + " ") and " ancestral" in p and " store=hbm " in p, p
    assert ("rescaled" in p) == rescaled, p
    assert eng.last_call_info() == (KERNEL, trees, trees)  # one evaluation per tree
    return p


def _full(eng, x, **kw):
    return eng.ancestral_states(x.pids, x.bls, x.pr, map_states=True, categories=True, tips=True, **kw)


def _same(a, b):
    for f in FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True), f


# ---- 1. every output against the reference ----

@pytest.mark.parametrize("P", AC.PS)
@pytest.mark.parametrize("K", AC.KS)
@pytest.mark.parametrize("subst", AC.SUBSTS)
def test_parity(subst, K, P):
    for name in AC.SHAPES:
        x = AC.parity(name, subst, K, P)
        eng = AC.engine(x)
        res = _full(eng, x)
        assert f"K={K}" in _path(eng, AC.T)
        assert res.state_posteriors.shape == (AC.T, x.n - 2, P, 4) and res.map_states.dtype == np.int8
        AC.check_all(res, x, AC.parity_reference(name, subst, K, P), f"{name} {subst} K={K} P={P}")
        if K == 1:
            m = [O.model_set(x.spec, x.pr[t]).cat_rates[0] for t in range(AC.T)]
            assert np.all(res.category_posteriors == 1.0)
            assert np.array_equal(res.pattern_rates, np.repeat(np.array(m)[:, None], P, axis=1))


def test_balanced_eight_has_three_internal_root_children():
    pid = TU.balanced_topology(8)
    kids = [v for v in range(13) if pid[v] == 13]
    assert len(kids) == 3 and all(v >= 8 for v in kids), kids


@pytest.mark.parametrize("name", AC.SHAPES)
def test_root_row_from_either_side_of_the_zero_length_edge(name):
    """The caller's root is R of the set-up tree; the set-up root B above it is R seen across a
    zero-length edge.  R's row is written at R's visit from q_R = P(0)^T (pi o S_c0); B's visit
    holds pi o S_c0 o (P(0) L_R), the reference's own form of the root joint (pi times the three
    child messages), and forms the category terms and the first root child's pre-order vector
    from it.  The root row, the first root child's row (or tip row) and the category posteriors
    agree with the reference: the two views are one."""
    x = AC.parity(name, "GTR", 4, 65)
    res = _full(AC.engine(x), x)
    refs = AC.parity_reference(name, "GTR", 4, 65)
    root = 2 * x.n - 3
    for t, ref in enumerate(refs):
        c0 = min(v for v in range(root) if x.pids[t][v] == root)
        A.check(res.state_posteriors[t][-1], ref.state_post[-1], f"{name} root")
        if c0 >= x.n:
            A.check(res.state_posteriors[t][c0 - x.n], ref.state_post[c0 - x.n], f"{name} c0")
        else:
            A.check(res.tip_posteriors[t][c0], ref.tip_post[c0], f"{name} c0 tip")
        A.check(res.category_posteriors[t], ref.cat_post, f"{name} categories")


# ---- 2. tip partials: 0/1 masks that are not one-hot, real-valued vectors ----

@pytest.mark.parametrize("form", ["masks", "real"])
@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("subst", AC.SUBSTS)
def test_tip_partials(subst, K, form):
    for name in ("balanced8", "random12"):
        x = AC.partials(name, subst, K, form)
        eng = AC.engine(x)
        res = _full(eng, x)
        _path(eng, AC.T)
        AC.check_all(res, x, AC.partials_reference(name, subst, K, form), f"{form} {name} {subst} K={K}")


def test_unambiguous_tips_get_their_own_vector():
    x = AC.parity("random12", "GTR", 4, 65)
    res = _full(AC.engine(x), x)
    known = x.states <= 3
    assert np.any(~known)
    for t in range(AC.T):
        assert np.array_equal(res.tip_posteriors[t][known], x.vectors[known])


# ---- 3. rescaling ----

@pytest.mark.parametrize("subst,K", [("JC69", 4), ("GTR", 2)])
def test_rescaling_on_and_off_agree(subst, K):
    for name in ("balanced8", "random12"):
        x = AC.parity(name, subst, K, 129)
        eng = AC.engine(x)
        off = _full(eng, x)
        on = _full(eng, x, rescaling=True)
        _path(eng, AC.T, rescaled=True)
        refs = AC.parity_reference(name, subst, K, 129)
        AC.check_all(on, x, refs, f"rescaled {name} {subst} K={K}")
        for t in range(AC.T):
            for f in ("state_posteriors", "category_posteriors", "pattern_rates", "tip_posteriors"):
                A.check(getattr(on, f)[t], getattr(off, f)[t], f"{f} on against off")
            clear = refs[t].margin > A.MAP_MARGIN
            assert np.array_equal(on.map_states[t][clear], off.map_states[t][clear])


def test_ladder_200_taxa_rescaled():
    x = AC.ladder200()
    eng = AC.engine(x)
    res = eng.ancestral_states(x.pids, x.bls, x.pr, rescaling=True, map_states=True, categories=True)
    _path(eng, 1, rescaled=True)
    res.tip_posteriors = None
    AC.check_all(res, x, AC.reference(x, with_tips=False), "ladder 200", tips=False)


# ---- 4. logL is the HBM gradient call's, bit for bit ----

def _ds1(T, subst="JC69", seed=51):
    tips, w, pids, bls = O.struct_arrays(O.load_struct("ds1_top100"))
    n, P = tips.shape
    spec = O.make_spec(n, P, subst, "weibull+4")
    pr = AC.params(spec, subst, 4, T, np.random.default_rng(seed))[0]
    return tips, w, pids[:T], bls[:T], pr


def _engine(subst, site, tips, w, **kw):
    import libsbn_amd as L
    return L.Engine(L.PhyloModelSpecification(subst, site, "strict"), tips, w, device=0, **kw)


@pytest.mark.parametrize("rescaling", [False, True])
def test_log_likelihood_is_the_hbm_gradient_calls(monkeypatch, rescaling):
    tips, w, pids, bls, pr = _ds1(5, "GTR", 61)
    eng = _engine("GTR", "weibull+4", tips, w)
    ll = eng.ancestral_states(pids, bls, pr, rescaling=rescaling).log_likelihoods
    monkeypatch.setenv("MI_PHYLO_GRADIENT_PATH", "hbm")
    hbm = _engine("GTR", "weibull+4", tips, w)
    ref = hbm.gradients(pids, bls, pr, rescaling=rescaling, gradient_blocks=())
    assert hbm.last_call_info()[0] == "gradient_hbm_kernel"
    assert np.array_equal(ll, np.array([x.log_likelihood for x in ref]))


# ---- 5. closed forms ----

def test_star_tree_root_posterior_closed_form():
    """n = 3, K = 1: state_post at the root is pi_s prod_i P_i[s][x_i] / sum."""
    rng = np.random.default_rng(71)
    n, P, T = 3, 64, 2
    states = rng.integers(0, 4, size=(n, P)).astype(np.int32)
    w = np.ones(P)
    pids = np.array([[3, 3, 3]] * T, np.int32)
    bls = rng.uniform(0.01, 0.5, size=(T, 4))
    spec = O.make_spec(n, P, "GTR", "constant")
    pr, rates, freqs = AC.params(spec, "GTR", 1, T, rng)
    res = _engine("GTR", "constant", states, w).ancestral_states(pids, bls, pr, categories=True)
    assert res.state_posteriors.shape == (T, 1, P, 4)
    for t in range(T):
        Q, pi = A.gtr_q(rates[t], freqs[t])
        Pm = [A.expm(Q * A.LD(bls[t, i])) for i in range(3)]
        want = np.stack([pi * Pm[0][:, states[0, p]] * Pm[1][:, states[1, p]] * Pm[2][:, states[2, p]]
                         for p in range(P)])
        want = want / want.sum(axis=1, keepdims=True)
        A.check(res.state_posteriors[t, 0], want, "star")
    assert np.all(res.category_posteriors == 1.0) and np.all(res.pattern_rates == 1.0)


def test_all_gap_column_and_weight_zero_patterns():
    """GTR with unequal frequencies: at an all-gap column the posterior is pi at every node, the
    map state argmax pi and cat_post = c.  Values are unweighted: patterns of weight 0 are
    reported like the others."""
    x0 = AC.parity("random12", "GTR", 4, 65)
    states, w = x0.states.copy(), x0.w.copy()
    states[:, 7] = 4
    w[[7, 20]] = 0.0
    import libsbn_amd as L
    eng = L.Engine(L.PhyloModelSpecification("GTR", "weibull+4", "strict"), states, w, device=0)
    res = eng.ancestral_states(x0.pids, x0.bls, x0.pr, map_states=True, categories=True, tips=True)
    keep = [p for p in range(65) if p != 7]
    refs = AC.parity_reference("random12", "GTR", 4, 65)
    for t, ref in enumerate(refs):
        pi = x0.freqs[t] / np.sum(x0.freqs[t])
        c = np.array(O.model_set(x0.spec, x0.pr[t]).cat_weights[:4])
        assert np.all(np.abs(res.state_posteriors[t][:, 7] - pi) <= A.REL * pi)
        assert np.all(np.abs(res.tip_posteriors[t][:, 7] - pi) <= A.REL * pi)
        assert np.all(res.map_states[t][:, 7] == np.argmax(pi))
        assert np.all(np.abs(res.category_posteriors[t][7] - c / c.sum()) <= A.REL * c)
        A.check(res.state_posteriors[t][:, keep], ref.state_post[:, keep], "weight 0")
        A.check(res.category_posteriors[t][keep], ref.cat_post[keep], "weight 0")


def test_pattern_of_likelihood_zero_gives_nan_rows():
    x = AC.partials("balanced8", "GTR", 4, "real")
    vec = x.vectors.copy()
    vec[2, 5] = 0.0
    import libsbn_amd as L
    eng = L.Engine(L.PhyloModelSpecification("GTR", "weibull+4", "strict"), None, x.w, device=0,
                   use_tip_states=False, tip_partials=vec)
    res = eng.ancestral_states(x.pids, x.bls, x.pr, map_states=True, categories=True, tips=True)
    ref = _full(AC.engine(x), x)
    others = [p for p in range(x.P) if p != 5]
    assert np.all(np.isnan(res.state_posteriors[:, :, 5])) and np.all(res.map_states[:, :, 5] == 0)
    assert np.all(np.isnan(res.category_posteriors[:, 5])) and np.all(np.isnan(res.pattern_rates[:, 5]))
    assert np.all(np.isnan(res.tip_posteriors[:, :, 5]))
    for f in FIELDS[2:] + FIELDS[:1]:
        a, b = getattr(res, f), getattr(ref, f)
        if f in ("category_posteriors", "pattern_rates"):
            assert np.array_equal(a[:, others], b[:, others]), f
        else:
            assert np.array_equal(a[:, :, others], b[:, :, others]), f


# ---- 6. optional outputs, single tree, the walk in parts ----

def test_null_outputs_leave_the_others_bit_identical():
    x = AC.parity("random12", "GTR", 4, 65)
    eng = AC.engine(x)
    full = _full(eng, x)
    n, P, K, T = x.n, x.P, x.K, AC.T
    pid = np.ascontiguousarray(x.pids, np.int32)
    bl, pr = np.ascontiguousarray(x.bls), np.ascontiguousarray(x.pr)
    shapes = dict(log_likelihoods=((T,), np.float64), map_states=((T, n - 2, P), np.int8),
                  category_posteriors=((T, P, K), np.float64), pattern_rates=((T, P), np.float64),
                  tip_posteriors=((T, n, P, 4), np.float64))
    order = ("log_likelihoods", "state_posteriors", "map_states", "category_posteriors", "pattern_rates",
             "tip_posteriors")
    ptr = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    for mask in range(32):
        out = {"state_posteriors": np.full((T, n - 2, P, 4), -1.0)}
        for bit, (name, (shape, dtype)) in enumerate(shapes.items()):
            out[name] = np.full(shape, -1, dtype) if mask >> bit & 1 else None
        rc = eng._lib.mi_engine_ancestral_states_unrooted(eng._h, T, ptr(pid), ptr(bl), ptr(pr), 0,
                                                          *[ptr(out[name]) for name in order])
        assert rc == 0
        for name in order:
            if out[name] is not None:
                assert np.array_equal(out[name], getattr(full, name)), (mask, name)


def test_single_tree():
    x = AC.parity("random12", "GTR", 4, 65)
    eng = AC.engine(x)
    full = _full(eng, x)
    one = eng.ancestral_states(x.pids[1:2], x.bls[1:2], x.pr[1:2], map_states=True, categories=True, tips=True)
    _path(eng, 1)
    for f in FIELDS:
        assert np.array_equal(getattr(one, f)[0], getattr(full, f)[1]), f


def test_chunked_call_is_bit_identical(monkeypatch):
    x = AC.parity("random12", "GTR", 4, 129)
    rng = np.random.default_rng(92)
    T, n = 5, 12
    pids = np.stack([TU.random_topology(n, rng) for _ in range(T)])
    bls = rng.uniform(0.01, 0.5, size=(T, 2 * n - 2))
    pr = AC.params(x.spec, "GTR", 4, T, rng)[0]
    kw = dict(map_states=True, categories=True, tips=True)
    whole = AC.engine(x)
    ref = whole.ancestral_states(pids, bls, pr, **kw)
    assert whole.last_call_launches()[0] == 1
    per_eval = (n - 1) * 4 * 3 * 64 * 4 * 8  # [node][category][three tiles of 64 patterns][state] doubles
    monkeypatch.setenv("MI_PHYLO_PLV_BYTES", str(2 * per_eval + per_eval // 2))
    parts = AC.engine(x)
    got = parts.ancestral_states(pids, bls, pr, **kw)
    assert parts.last_call_launches()[0] == 3
    _same(ref, got)


# ---- 7. sharded handles ----

def test_sharded_handles():
    tips, w, pids, bls, pr = _ds1(7, "JC69", 101)
    kw = dict(map_states=True, categories=True, tips=True)
    ref = _engine("JC69", "weibull+4", tips, w).ancestral_states(pids, bls, pr, **kw)
    trees = _engine("JC69", "weibull+4", tips, w, shard_devices=[0, 0])
    _same(ref, trees.ancestral_states(pids, bls, pr, **kw))
    pats = _engine("JC69", "weibull+4", tips, w, shard_devices=[0, 0], shard_mode="patterns")
    with pytest.raises(RuntimeError, match="block of columns"):
        pats.ancestral_states(pids, bls, pr)


# ---- 8. the device-pointer call, reserved, from a graph ----

def test_device_call_replayed_from_a_graph():
    torch = pytest.importorskip("torch")
    T = 16
    tips, w, pids, bls, pr = _ds1(T, "JC69", 111)
    n, P = tips.shape
    eng = _engine("JC69", "weibull+4", tips, w)
    ref = eng.ancestral_states(pids, bls, pr, map_states=True, categories=True, tips=True)
    dev = torch.device("cuda", 0)
    d_pid = torch.from_numpy(np.ascontiguousarray(pids, np.int32)).to(dev)
    d_bl = torch.from_numpy(np.ascontiguousarray(bls)).to(dev)
    d_pr = torch.from_numpy(np.ascontiguousarray(pr)).to(dev)
    f64 = dict(dtype=torch.float64, device=dev)
    outs = dict(state_posteriors=torch.zeros((T, n - 2, P, 4), **f64), log_likelihoods=torch.zeros(T, **f64),
                map_states=torch.zeros((T, n - 2, P), dtype=torch.int8, device=dev),
                category_posteriors=torch.zeros((T, P, 4), **f64), pattern_rates=torch.zeros((T, P), **f64),
                tip_posteriors=torch.zeros((T, n, P, 4), **f64))
    gs = torch.cuda.Stream()

    def call(stream, engine=None):
        (engine or fresh).ancestral_states_device(
            stream, T, d_pid.data_ptr(), d_bl.data_ptr(), d_pr.data_ptr(), outs["state_posteriors"].data_ptr(),
            out_ll=outs["log_likelihoods"].data_ptr(), out_map_states=outs["map_states"].data_ptr(),
            out_category_posteriors=outs["category_posteriors"].data_ptr(),
            out_pattern_rates=outs["pattern_rates"].data_ptr(), out_tip_posteriors=outs["tip_posteriors"].data_ptr())

    # (the other engine runs the same call on the stream first: the kernels' code objects are
    # loaded -- into device memory -- at their first launch, which is not the engine's allocation)
    call(gs.cuda_stream, eng)
    torch.cuda.synchronize()
    fresh = _engine("JC69", "weibull+4", tips, w)
    fresh.reserve_ancestral(T)
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info(0)[0]
    with torch.cuda.stream(gs):
        call(gs.cuda_stream)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info(0)[0] == free_before  # (reserved: the call allocated nothing)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=gs):
        call(torch.cuda.current_stream().cuda_stream)
    _path(fresh, T)
    for _ in range(2):
        for o in outs.values():
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for f in FIELDS:
            assert np.array_equal(outs[f].cpu().numpy(), getattr(ref, f)), f
    fresh.check_status()


# ---- 9. refusals ----

def test_twenty_state_engine_refuses():
    import aa_utils
    rng = np.random.default_rng(121)
    tips, w = aa_utils.random_aa_alignment(6, 20, rng)
    pids, bls = TU.random_trees(6, 2, rng)
    eng = _engine("WAG", "constant", tips, w)
    with pytest.raises(RuntimeError, match="4-state only"):
        eng.ancestral_states(pids, bls, None)
    with pytest.raises(RuntimeError, match="4-state only"):
        eng.reserve_ancestral(2)


def test_bad_tree_is_reported_with_its_index():
    x = AC.parity("n5", "JC69", 1, 13)
    bad = x.pids.copy()
    bad[1, 0] = 0
    with pytest.raises(RuntimeError, match=r"post-order id form \(tree 1\)"):
        AC.engine(x).ancestral_states(bad, x.bls, x.pr, map_states=True, categories=True, tips=True)


# ---- 10. the C++ adapter ----

def test_cpp_adapter_gives_the_python_call_bit_for_bit(tmp_path):
    exe = tmp_path / "ancestral_example"
    lib = os.path.join(REPO, "libsbn_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(REPO, "tests/cpp/ancestral_example.cpp"),
                    "-L" + lib, "-lmi_phylo", "-lmi_phylo_host", "-Wl,-rpath," + lib, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe), os.path.join(REPO, "tests/golden/data")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    got, shape = {}, None
    for line in out.stdout.splitlines():
        name, *rest = line.split()
        if name == "shape":
            shape = tuple(int(v) for v in rest)
        else:
            got.setdefault(name, []).append(int(rest[1]) if name == "map" else float.fromhex(rest[1]))
    tips, w, pids, bls = O.struct_arrays(O.load_struct("hello"))
    T, (n, P) = len(pids), tips.shape
    assert shape == (T, n, P)
    eng = _engine("JC69", "weibull+4", tips, w)
    pr = np.zeros((T, eng.param_count))
    pr[:, eng.block_specification()["Weibull shape"][0]] = 0.8
    r = eng.ancestral_states(pids, bls, pr, map_states=True, categories=True, tips=True)
    for name, want in (("ll", r.log_likelihoods), ("state", r.state_posteriors), ("map", r.map_states),
                       ("cat", r.category_posteriors), ("rate", r.pattern_rates), ("tip", r.tip_posteriors)):
        assert np.array_equal(got[name], want.reshape(-1)), name
