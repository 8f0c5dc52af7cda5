"""Phylogenetic placement (mi_engine_placement_unrooted, Engine.placement) against
tests/placement_ref.py (long double; the query inserted into the tree explicitly, no pre-order
pass): edge log-likelihoods, the tables and the trees' log-likelihoods to 1e-10 relative, the
project's standing tolerance; pendant indices and best edges wherever the reference's top two are
further apart than that tolerance implies; likelihood weight ratios within what it implies.  The
sums are formed in one fixed order: everything the interface calls bit-identical is compared
with array_equal."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ancestral_cases as AC
import oracle_lib as O
import placement_cases as PC
import placement_ref as R
import tree_utils as TU

pytestmark = pytest.mark.gpu

KERNEL = "placement_table_hbm_kernel"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("log_likelihoods", "edge_log_likelihoods", "best_edge", "pendant_index", "lwr", "tables")


def _path(eng, trees, rescaled=False):
    p = eng.last_call_path()
    assert p.startswith(KERNEL + " ") and " placement" in p and " store=hbm " in p, p
    assert ("rescaled" in p) == rescaled, p
    assert eng.last_call_info() == (KERNEL, trees, trees)  # one evaluation per tree
    return p


def _full(eng, x, q, col=None, w=None, pendants=None, **kw):
    return eng.placement(x.pids, x.bls, q, x.pendants if pendants is None else pendants, x.pr, column_pattern=col,
                         column_weights=w, pendant_index=True, lwr=True, tables=True, **kw)


def _same(a, b, fields=FIELDS):
    for f in fields:
        assert np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True), f


# ---- 1. every output against the reference ----

@pytest.mark.parametrize("P", PC.PS)
@pytest.mark.parametrize("K", PC.KS)
@pytest.mark.parametrize("subst", PC.SUBSTS)
def test_parity(subst, K, P):
    for name in PC.SHAPES:
        x = PC.parity(name, subst, K, P)
        S = PC.parity_tables(name, subst, K, P)
        eng = AC.engine(x)
        for label, q, col, w in PC.maps(x):
            res = _full(eng, x, q, col, w)
            assert f"K={K}" in _path(eng, PC.T)
            E = 2 * x.n - 3
            assert res.edge_log_likelihoods.shape == (PC.T, PC.Q, E) and res.tables.shape == (PC.T, E, 2, 5, P)
            assert res.best_edge.dtype == np.int32 and res.pendant_index.dtype == np.int8
            left = PC.check_result(res, x, S, q, col, w, f"{name} {subst} K={K} P={P} {label}")
            assert left == 0.0  # (the committed seeds leave nothing out)
            # a copy of taxon 0 belongs on the edge above taxon 0
            assert np.all(res.best_edge[:, 0] == 0)


def test_three_taxa_all_edges_are_root_edges():
    assert list(PC.parity("n3", "GTR", 4, 65).pids[0]) == [3, 3, 3]


# ---- 2. tip partials: 0/1 masks that are not one-hot, real-valued vectors ----

@pytest.mark.parametrize("form", ["masks", "real"])
@pytest.mark.parametrize("name", ["n5", "random12"])
def test_tip_partials(name, form):
    x = PC.partials(name, form)
    S = PC.partials_tables(name, form)
    eng = AC.engine(x)
    for label, q, col, w in PC.maps(x):
        res = _full(eng, x, q, col, w)
        _path(eng, len(x.pids))
        PC.check_result(res, x, S, q, col, w, f"{name} {form} {label}")


# ---- 3. rescaling ----

@pytest.mark.parametrize("name", ["n3", "random12"])
def test_rescaling_on_against_off(name):
    x = PC.parity(name, "GTR", 4, 65)
    eng = AC.engine(x)
    off = _full(eng, x, x.q_site, x.col_site, x.w_site)
    on = _full(eng, x, x.q_site, x.col_site, x.w_site, rescaling=True)
    _path(eng, PC.T, rescaled=True)
    for f in ("log_likelihoods", "edge_log_likelihoods", "tables"):
        a, b = getattr(on, f), getattr(off, f)
        assert np.all(np.abs(a - b) <= R.REL * np.abs(b)), f
    S = PC.parity_tables(name, "GTR", 4, 65)
    PC.check_result(on, x, S, x.q_site, x.col_site, x.w_site, f"{name} rescaled")


def test_ladder_of_200_taxa_under_rescaling():
    """Pattern likelihoods down to 1e-126: the table form of the reference (held to explicit
    insertion in tests/test_placement_ref.py), one pendant length."""
    x = PC.ladder200()
    pend = x.pendants[1:]
    S = [R.formula_tables(x.pids[0], x.bls[0], *AC.model(x, 0), x.vectors, pend)[0]]
    eng = AC.engine(x)
    res = _full(eng, x, x.q_site, x.col_site, x.w_site, pendants=pend, rescaling=True)
    _path(eng, 1, rescaled=True)
    assert np.all(np.isfinite(res.edge_log_likelihoods))
    PC.check_result(res, x, S, x.q_site, x.col_site, x.w_site, "ladder200 rescaled")


# ---- 4. the log-likelihood is the family's, bit for bit ----

@pytest.mark.parametrize("form", ["states", "real"])
@pytest.mark.parametrize("n", [3, 12])
def test_log_likelihood_is_the_hbm_gradient_calls(monkeypatch, n, form):
    import libsbn_amd as L
    rng = np.random.default_rng(5100 + 10 * n + (form == "real"))
    P, K, T = 65, 4, 3
    pids = np.stack([TU.random_topology(n, rng) for _ in range(T)]) if n > 3 else np.array([[3, 3, 3]] * T, np.int32)
    states, w = TU.random_alignment(n, P, rng)
    bls = rng.uniform(0.01, 0.5, size=(T, 2 * n - 2))
    bls[:, -1] = 0.0
    pr = AC.params(O.make_spec(n, P, "GTR", AC.site(K)), "GTR", K, T, rng)[0]
    spec = L.PhyloModelSpecification("GTR", AC.site(K), "strict")
    if form == "states":
        monkeypatch.setenv("MI_PHYLO_GRADIENT_PATH", "hbm")
        eng = L.Engine(spec, states, w, device=0)
    else:
        vectors = R.tip_vectors(states, np.float64)
        vectors[:3] = 1.0 - rng.uniform(0.0, 0.95, size=vectors[:3].shape)
        eng = L.Engine(spec, None, w, device=0, use_tip_states=False, tip_partials=vectors)
    q = rng.integers(0, 5, size=(4, P)).astype(np.int8)
    for rescaling in (False, True):
        grad = eng.gradients(pids, bls, pr, rescaling=rescaling, gradient_blocks=())
        assert eng.last_call_info()[0] == "gradient_hbm_kernel"
        ll = np.array([g.log_likelihood for g in grad])
        res = eng.placement(pids, bls, q, [0.1], pr, rescaling=rescaling, column_pattern=np.arange(P),
                            column_weights=w)
        _path(eng, T, rescaled=rescaling)
        assert np.array_equal(res.log_likelihoods, ll)


# ---- 5. determinism: one fixed order of summation ----

def _det_case():
    x = PC.parity("random12", "GTR", 4, 129)
    rng = np.random.default_rng(6200)
    q = PC.queries(x, rng, 130, x.col_site)
    q[77] = q[5]
    q[129] = q[5]
    return x, q


def test_single_query_calls_and_duplicate_rows():
    x, q = _det_case()
    eng = AC.engine(x)
    whole = _full(eng, x, q, x.col_site, x.w_site)
    for row in (0, 64, 129):
        one = _full(eng, x, q[row:row + 1], x.col_site, x.w_site)
        for f in ("edge_log_likelihoods", "pendant_index", "lwr"):
            assert np.array_equal(getattr(one, f)[:, 0], getattr(whole, f)[:, row]), (f, row)
        assert np.array_equal(one.best_edge[:, 0], whole.best_edge[:, row])
        assert np.array_equal(one.tables, whole.tables)
    for f in ("edge_log_likelihoods", "pendant_index", "lwr"):
        v = getattr(whole, f)
        assert np.array_equal(v[:, 5], v[:, 77]) and np.array_equal(v[:, 5], v[:, 129]), f


def test_table_in_memory_gives_the_bits_of_the_table_in_lds(monkeypatch):
    x, q = _det_case()
    y = PC.parity("n3", "JC69", 1, 13)
    lds = [_full(AC.engine(x), x, q, x.col_site, x.w_site), _full(AC.engine(y), y, y.q_identity)]
    monkeypatch.setenv("MI_PHYLO_PLACE_TABLE", "global")
    _same(lds[0], _full(AC.engine(x), x, q, x.col_site, x.w_site))
    _same(lds[1], _full(AC.engine(y), y, y.q_identity))
    monkeypatch.setenv("MI_PHYLO_PLACE_TABLE", "lds")
    _same(lds[1], _full(AC.engine(y), y, y.q_identity))


def test_call_cut_into_three_launches_is_bit_identical(monkeypatch):
    x, q = _det_case()
    whole = AC.engine(x)
    ref = _full(whole, x, q, x.col_site, x.w_site)
    assert whole.last_call_launches()[0] == 1
    per_table = (2 * x.n - 3) * 2 * 5 * 3 * 64 * 8  # [edge][pendant][code][three tiles of 64 patterns] doubles
    per_eval = (x.n - 1) * 4 * 3 * 64 * 4 * 8       # the vector arena of one tree
    assert per_table > per_eval
    monkeypatch.setenv("MI_PHYLO_PLV_BYTES", str(per_table + per_table // 2))
    parts = AC.engine(x)
    got = _full(parts, x, q, x.col_site, x.w_site)
    assert parts.last_call_launches()[0] == 3
    _same(ref, got)
    monkeypatch.setenv("MI_PHYLO_PLV_BYTES", str(per_table - 8))
    with pytest.raises(RuntimeError, match=f"table of one tree \\({per_table} bytes"):
        _full(AC.engine(x), x, q, x.col_site, x.w_site)


def test_one_pendant_length_is_its_column_of_two():
    x, q = _det_case()
    eng = AC.engine(x)
    two = _full(eng, x, q, x.col_site, x.w_site)
    one = _full(eng, x, q, x.col_site, x.w_site, pendants=x.pendants[1:])
    assert np.array_equal(one.tables[:, :, 0], two.tables[:, :, 1])
    pick = two.pendant_index == 1
    assert np.any(pick) and np.array_equal(one.edge_log_likelihoods[pick], two.edge_log_likelihoods[pick])


# ---- 6. closed form ----

def test_closed_form_star():
    """JC69, one category, the 3-taxon star, one pattern, against the hand formula."""
    import libsbn_amd as L
    t = np.array([[0.11, 0.27, 0.05, 0.0]])
    tips = np.array([[1], [1], [3]], np.int32)
    eng = L.Engine(L.PhyloModelSpecification("JC69", "constant", "strict"), tips, np.ones(1), device=0)
    q = np.arange(5, dtype=np.int8).reshape(5, 1)
    res = eng.placement(np.array([[3, 3, 3]], np.int32), t, q, [0.07], None, tables=True)
    for code in range(5):
        want, s = R.star3_closed_form(t[0], 0.07, (1, 1, 3), code)
        assert abs(res.tables[0, 0, 0, code, 0] - want) <= R.REL * abs(want)
        assert abs(res.edge_log_likelihoods[0, code, 0] - want) <= R.REL * abs(want)
    assert abs(res.log_likelihoods[0] - s) <= R.REL * abs(s)


# ---- 7. optional outputs ----

def test_null_outputs_leave_the_others_bit_identical():
    x = PC.parity("random12", "GTR", 4, 65)
    eng = AC.engine(x)
    q, col, w = x.q_site, x.col_site, np.ascontiguousarray(x.w_site)
    full = _full(eng, x, q, col, w)
    T, Qn, E, G, P = PC.T, len(q), 2 * x.n - 3, 2, x.P
    pid = np.ascontiguousarray(x.pids, np.int32)
    bl, pr, pend = np.ascontiguousarray(x.bls), np.ascontiguousarray(x.pr), np.ascontiguousarray(x.pendants)
    q = np.ascontiguousarray(q, np.int8)
    shapes = dict(log_likelihoods=((T,), np.float64), pendant_index=((T, Qn, E), np.int8),
                  best_edge=((T, Qn), np.int32), lwr=((T, Qn, E), np.float64), tables=((T, E, G, 5, P), np.float64))
    order = ("log_likelihoods", "edge_log_likelihoods", "pendant_index", "best_edge", "lwr", "tables")
    ptr = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    for mask in range(32):
        out = {"edge_log_likelihoods": np.full((T, Qn, E), -1.0)}
        for bit, (name, (shape, dtype)) in enumerate(shapes.items()):
            out[name] = np.full(shape, -1, dtype) if mask >> bit & 1 else None
        rc = eng._lib.mi_engine_placement_unrooted(eng._h, T, ptr(pid), ptr(bl), ptr(pr), 0, Qn, len(col), ptr(q),
                                                   ptr(col), ptr(w), G, ptr(pend), *[ptr(out[name]) for name in order])
        assert rc == 0
        for name in order:
            if out[name] is not None:
                assert np.array_equal(out[name], getattr(full, name)), (mask, name)


# ---- 8. the device-pointer call, reserved, from a graph ----

def test_device_call_replayed_from_a_graph():
    torch = pytest.importorskip("torch")
    x = PC.parity("random12", "GTR", 4, 129)
    T, Qn, E, G, P = PC.T, PC.Q, 2 * x.n - 3, 2, x.P
    eng = AC.engine(x)
    ref = _full(eng, x, x.q_site, x.col_site, x.w_site)
    dev = torch.device("cuda", 0)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)  # noqa: E731
    d_pid, d_bl, d_pr = up(x.pids, np.int32), up(x.bls, np.float64), up(x.pr, np.float64)
    d_q, d_col, d_w, d_pend = up(x.q_site, np.int8), up(x.col_site, np.int32), up(x.w_site, np.float64), \
        up(x.pendants, np.float64)
    f64 = dict(dtype=torch.float64, device=dev)
    outs = dict(log_likelihoods=torch.zeros(T, **f64), edge_log_likelihoods=torch.zeros((T, Qn, E), **f64),
                best_edge=torch.zeros((T, Qn), dtype=torch.int32, device=dev),
                pendant_index=torch.zeros((T, Qn, E), dtype=torch.int8, device=dev),
                lwr=torch.zeros((T, Qn, E), **f64), tables=torch.zeros((T, E, G, 5, P), **f64))
    gs = torch.cuda.Stream()

    def call(stream, engine=None):
        (engine or fresh).placement_device(
            stream, T, d_pid.data_ptr(), d_bl.data_ptr(), d_pr.data_ptr(), Qn, len(x.col_site), d_q.data_ptr(),
            d_col.data_ptr(), d_w.data_ptr(), G, d_pend.data_ptr(), outs["edge_log_likelihoods"].data_ptr(),
            out_ll=outs["log_likelihoods"].data_ptr(), out_pendant_index=outs["pendant_index"].data_ptr(),
            out_best_edge=outs["best_edge"].data_ptr(), out_lwr=outs["lwr"].data_ptr(),
            out_tables=outs["tables"].data_ptr())

    # (the other engine runs the same call on the stream first: the kernels' code objects are
    # loaded -- into device memory -- at their first launch, which is not the engine's allocation)
    call(gs.cuda_stream, eng)
    torch.cuda.synchronize()
    fresh = AC.engine(x)
    fresh.reserve_placement(T, Qn, len(x.col_site), G)
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


def test_device_call_reports_bad_columns_and_pendants_through_the_status_word():
    torch = pytest.importorskip("torch")
    x = PC.parity("n5", "JC69", 1, 13)
    eng = AC.engine(x)
    dev = torch.device("cuda", 0)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)  # noqa: E731
    d_pid, d_bl, d_pr = up(x.pids, np.int32), up(x.bls, np.float64), up(x.pr, np.float64)
    d_q = up(x.q_identity, np.int8)
    out = torch.zeros((PC.T, PC.Q, 7), dtype=torch.float64, device=dev)
    for col, pend, message in ((np.r_[np.arange(12), 13], [0.1], r"column_pattern.*\(column 12\)"),
                               (np.r_[-1, np.arange(1, 13)], [0.1], r"column_pattern.*\(column 0\)"),
                               (np.arange(13), [0.1, np.nan], r"pendant length.*\(pendant 1\)"),
                               (np.arange(13), [-0.5], r"pendant length.*\(pendant 0\)")):
        d_col, d_pend = up(col, np.int32), up(pend, np.float64)
        eng.placement_device(None, PC.T, d_pid.data_ptr(), d_bl.data_ptr(), d_pr.data_ptr(), PC.Q, 13, d_q.data_ptr(),
                             d_col.data_ptr(), None, len(pend), d_pend.data_ptr(), out.data_ptr())
        with pytest.raises(RuntimeError, match=message):
            eng.check_status()
    eng.check_status()


# ---- 9. sharded handles ----

def test_tree_sharded_handle_gives_the_unsharded_rows():
    import torch
    x = PC.parity("random12", "GTR", 4, 65)
    ref = _full(AC.engine(x), x, x.q_site, x.col_site, x.w_site)
    layouts = [[0, 0]] + ([[0, 1]] if torch.cuda.device_count() > 1 else [])
    for devices in layouts:
        _same(ref, _full(AC.engine(x, shard_devices=devices), x, x.q_site, x.col_site, x.w_site))
    pats = AC.engine(x, shard_devices=[0, 0], shard_mode="patterns")
    with pytest.raises(RuntimeError, match="block of columns"):
        _full(pats, x, x.q_site, x.col_site, x.w_site)


# ---- 10. refusals ----

def test_twenty_state_engine_refuses():
    import aa_utils
    import libsbn_amd as L
    rng = np.random.default_rng(121)
    tips, w = aa_utils.random_aa_alignment(6, 20, rng)
    pids, bls = TU.random_trees(6, 2, rng)
    eng = L.Engine(L.PhyloModelSpecification("WAG", "constant", "strict"), tips, w, device=0)
    with pytest.raises(RuntimeError, match="4-state only"):
        eng.placement(pids, bls, np.zeros((2, 20), np.int8), [0.1])
    with pytest.raises(RuntimeError, match="4-state only"):
        eng.reserve_placement(2, 2, 20, 1)


def test_rooted_parent_id_rows_do_not_fit_the_unrooted_form():
    """The call has an unrooted entry point only: a rooted tree's 2n-2 parent ids make no whole
    rows of 2n-3, and a row of 2n-3 ids whose root is no trifurcation is reported by the set-up."""
    x = PC.parity("n5", "JC69", 1, 13)
    eng = AC.engine(x)
    rooted = TU.random_topology(5, np.random.default_rng(3), rooted=True)
    with pytest.raises((RuntimeError, ValueError)):
        eng.placement(rooted, x.bls[:1], x.q_identity, [0.1], x.pr[:1])
    bad = x.pids.copy()
    bad[1, 0] = 0
    with pytest.raises(RuntimeError, match=r"post-order id form \(tree 1\)"):
        eng.placement(bad, x.bls, x.q_identity, [0.1], x.pr)


def test_bad_arguments_are_refused_before_any_device_work():
    x = PC.parity("n5", "JC69", 1, 13)
    eng = AC.engine(x)
    eng.log_likelihoods(x.pids, x.bls, x.pr)
    before = eng.last_call_path()
    q = x.q_identity
    call = lambda pend, queries=q, **kw: eng.placement(x.pids, x.bls, queries, pend, x.pr, **kw)  # noqa: E731
    for pend in ([], [0.1] * 5):
        with pytest.raises(RuntimeError, match=r"pendant_count must be in \[1, 4\]"):
            call(pend)
    for pend, g in (([0.1, -1e-9], 1), ([np.inf], 0), ([0.1, 0.2, np.nan], 2)):
        with pytest.raises(RuntimeError, match=rf"not finite or is negative \(pendant {g}\)"):
            call(pend)
    with pytest.raises(RuntimeError, match="query_count must be positive"):
        call([0.1], np.zeros((0, 13), np.int8))
    with pytest.raises(RuntimeError, match="column_count must be positive"):
        call([0.1], np.zeros((2, 0), np.int8), column_pattern=np.zeros(0, np.int32))
    for bad, c in ((13, 4), (-1, 0)):
        col = np.arange(13, dtype=np.int32)
        col[c] = bad
        with pytest.raises(RuntimeError, match=rf"outside \[0, pattern_count\) \(column {c}\)"):
            call([0.1], column_pattern=col, column_weights=np.ones(13))
    with pytest.raises(RuntimeError, match="reserve|pendant_count"):
        eng.reserve_placement(3, 5, 13, 0)
    assert eng.last_call_path() == before  # nothing ran
    assert np.all(np.isfinite(call([0.0, 0.1]).edge_log_likelihoods))


def test_zero_weight_columns_are_skipped_and_minus_infinity_propagates():
    """Pendant length 0 on a zero-length leaf edge: a query of another state has likelihood 0
    there.  With weight 0 on such columns nothing of it shows; with weight 1 the edge scores -inf."""
    x = PC.parity("n5", "JC69", 1, 13)
    bls = x.bls.copy()
    bls[:, 0] = 0.0
    eng = AC.engine(x)
    known = x.states[0] <= 3
    assert np.any(known)
    row = np.where(known, (x.states[0] + 1) % 4, 4)  # another state than taxon 0's wherever that is known
    q = np.ascontiguousarray(np.broadcast_to(row, (2, 13)), np.int8)
    col = np.arange(13)
    res = eng.placement(x.pids, bls, q, [0.0], x.pr, column_pattern=col, column_weights=np.ones(13), lwr=True)
    assert np.all(res.edge_log_likelihoods[:, :, 0] == -np.inf)
    assert np.all(np.isfinite(res.edge_log_likelihoods[:, :, 1:]))
    assert np.all(res.lwr[:, :, 0] == 0.0) and np.all(res.best_edge != 0)
    res = eng.placement(x.pids, bls, q, [0.0], x.pr, column_pattern=col, column_weights=np.where(known, 0.0, 1.0))
    assert np.all(np.isfinite(res.edge_log_likelihoods))


# ---- 11. the C++ adapter ----

def test_cpp_adapter_gives_the_python_call_bit_for_bit(tmp_path):
    import libsbn_amd as L
    exe = tmp_path / "placement_example"
    lib = os.path.join(REPO, "libsbn_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(REPO, "tests/cpp/placement_example.cpp"),
                    "-L" + lib, "-lmi_phylo", "-lmi_phylo_host", "-Wl,-rpath," + lib, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe), os.path.join(REPO, "tests/golden/data")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    got, shape = {}, None
    for line in out.stdout.splitlines():
        name, *rest = line.split()
        if name == "shape":
            shape = tuple(int(v) for v in rest)
        else:
            got.setdefault(name, []).append(int(rest[1]) if name in ("best", "pend") else float.fromhex(rest[1]))
    tips, w, pids, bls = O.struct_arrays(O.load_struct("hello"))
    T, (n, P) = len(pids), tips.shape
    assert shape == (T, n, P)
    eng = L.Engine(L.PhyloModelSpecification("JC69", "weibull+4", "strict"), tips, w, device=0)
    pr = np.zeros((T, eng.param_count))
    pr[:, eng.block_specification()["Weibull shape"][0]] = 0.8
    q = np.array([[(qi + c) % 5 for c in range(P)] for qi in range(5)], np.int8)
    r = eng.placement(pids, bls, q, [0.05, 0.4], pr, pendant_index=True, lwr=True, tables=True)
    for name, want in (("ll", r.log_likelihoods), ("edge", r.edge_log_likelihoods), ("best", r.best_edge),
                       ("pend", r.pendant_index), ("lwr", r.lwr), ("table", r.tables)):
        assert np.array_equal(got[name], want.reshape(-1)), name
