"""The SPR neighbourhood scan (mi_engine_spr_scan_unrooted, Engine.spr_scan):
delta[t][s][dir][f] = logL(neighbour) - logL(tree t) of every move "cut edge s, re-attach the
loose part on the midpoint of edge f".  The reference is the oracle's log-likelihood of every
neighbour rebuilt and renumbered by tests/spr_ref.py (which does not use the library; for
real-valued tip vectors, which the oracle does not take, spr_ref's own pruning in longdouble):
|logL + delta - reference| <= 1e-10 |reference|, the project's standing tolerance, and logL itself
to the same bound.  Best targets and best moves must equal the reference's -- tests/test_spr_ref.py
shows that no such decision of these inputs rests on a margin the tolerance could overturn --, and
-inf and -1 sit exactly where the definition has no move."""
import ctypes as C

import numpy as np
import pytest

import spr_cases as SC
import spr_ref as R

pytestmark = pytest.mark.gpu

KERNEL = "spr_vectors_hbm_kernel"


def _path(eng, rescaled=False):
    p = eng.last_call_path()
    assert p.startswith(KERNEL + " ") and " spr" in p and " store=hbm " in p, p
    assert ("rescaled" in p) == rescaled, p
    assert eng.last_call_info()[0] == KERNEL
    return p


def _scan(eng, x, radius=0, trees=None, table=True):
    t = slice(None) if trees is None else trees
    return eng.spr_scan(x.pids[t], x.bls[t], x.pr[t], rescaling=x.rescaling, radius=radius, table=table)


def _same(a, b):
    return all(np.array_equal(getattr(a, k), getattr(b, k))
               for k in ("log_likelihoods", "best_target", "best_delta", "best_move", "delta"))


# ---- 1. the small shapes against the reference ----

@pytest.mark.parametrize("c", SC.SMALL, ids=SC.case_id)
def test_small_shapes_match_the_reference(c):
    x = SC.case(*c)
    eng = SC.engine(x)
    res = _scan(eng, x)
    assert f"K={x.K}" in _path(eng, x.rescaling)
    worst = max(SC.check_tree(res, t, x, SC.small_reference(c)[t], label=SC.case_id(c)) for t in range(SC.T))
    print(f"{SC.case_id(c)}: logL + delta {worst:.2e}")
    assert worst <= R.REL
    if x.n == 3:
        assert np.all(res.best_move == -1) and np.all(res.best_target == -1) and np.all(np.isneginf(res.delta))


# ---- 2. the radius ----

@pytest.mark.parametrize("radius", (1, 2, 3))
@pytest.mark.parametrize("c", SC.RADIUS, ids=SC.case_id)
def test_radius_keeps_the_moves_of_the_distance_rule(c, radius):
    x = SC.case(*c)
    res = _scan(SC.engine(x), x, radius=radius)
    worst = max(SC.check_tree(res, t, x, SC.small_reference(c)[t], radius=radius, label=SC.case_id(c))
                for t in range(SC.T))
    assert worst <= R.REL
    whole = sum(len(SC.small_reference(c)[t][1]) for t in range(SC.T))
    assert 0 < int(np.sum(~np.isneginf(res.delta))) < whole


def _refused_without_touching_outputs(eng, n, pids, bls, pr, radius, message):
    """mi_engine_spr_scan_unrooted itself, with outputs filled beforehand: nonzero, a message, and
    every output as it was."""
    from libsbn_amd import _capi
    T, E = len(pids), 2 * n - 3
    ll, target, best = np.full(T, 7.0), np.full((T, E, 2), 7, np.int32), np.full((T, E, 2), 7.0)
    move, delta = np.full((T, 3), 7, np.int32), np.full((T, E, 2, E), 7.0)

    def ptr(a):
        return None if a is None else np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)

    pids, bls = np.ascontiguousarray(pids, np.int32), np.ascontiguousarray(bls, np.float64)
    pr = None if pr is None else np.ascontiguousarray(pr, np.float64)
    rc = eng._lib.mi_engine_spr_scan_unrooted(eng._h, T, ptr(pids), ptr(bls), ptr(pr), 0, radius, ptr(ll), ptr(target),
                                              ptr(best), ptr(move), ptr(delta))
    assert rc != 0
    assert message in _capi.last_error(), _capi.last_error()
    for a in (ll, target, best, move, delta):
        assert np.all(a == 7)


def test_negative_radius_is_refused_and_touches_no_output():
    x = SC.case(*SC.SMALL[2])
    eng = SC.engine(x)
    _refused_without_touching_outputs(eng, x.n, x.pids, x.bls, x.pr, -1, "radius")
    with pytest.raises(RuntimeError, match="radius"):
        eng.spr_scan(x.pids, x.bls, x.pr, radius=-1)


# ---- 3. 70 taxa, rescaling on: the stored exponents at work (test_spr_ref.py shows they are) ----

@pytest.mark.parametrize("name", SC.BIG)
def test_70_taxa_rescaled_radius_3(name):
    x = SC.big(name)
    eng = SC.engine(x)
    res = _scan(eng, x, radius=3)
    _path(eng, rescaled=True)
    ref = SC.big_radius3_reference(name)
    E = 2 * x.n - 3
    want = R.table(x.n, ref[1], ref[2] - ref[0])
    assert np.array_equal(np.isneginf(res.delta[0]), np.isneginf(want))
    worst = SC.check_rows(res, x, ref, [(s, d) for s in range(E) for d in (0, 1) if np.any(~np.isneginf(want[s, d]))],
                          label=name)
    target, _, _, move, _ = R.decisions(want)
    assert np.array_equal(res.best_target[0], target)
    assert tuple(int(v) for v in res.best_move[0]) == move
    print(f"{name} radius 3: {len(ref[1])} moves, logL + delta {worst:.2e}")
    assert worst <= R.REL


@pytest.mark.parametrize("name", SC.BIG)
def test_70_taxa_rescaled_sample_of_all_moves(name):
    """At radius 0: a fixed-seed sample of at least 300 moves, drawn by whole rows (s, dir), and
    the reference's best target of every sampled row."""
    x = SC.big(name)
    res = _scan(SC.engine(x), x)
    ref = SC.big_sample_reference(name)
    assert len(ref[1]) >= 300 and max(m[3] for m in ref[1]) > 3
    worst = SC.check_rows(res, x, ref, sorted({m[:2] for m in ref[1]}), label=name)
    assert int(np.sum(~np.isneginf(res.delta[0]))) == len(R.moves(x.n, x.pids[0]))
    print(f"{name} sample: {len(ref[1])} moves, logL + delta {worst:.2e}")
    assert worst <= R.REL


# ---- 4. the root cases occur in the small shapes (and are therefore checked above) ----

def test_both_root_cases_occur():
    seen = dict(parent_is_root=0, path_through_root=0, rest_moves_below_root=0)
    for c in SC.SMALL:
        x = SC.case(*c)
        root = 2 * x.n - 3
        for t in range(SC.T):
            par, kids, below = R.tree(x.n, x.pids[t])

            def top(v):  # the child of the root that v lies under
                while par[v] != root:
                    v = par[v]
                return v

            for s, d, f, _ in SC.small_reference(c)[t][1]:
                if d == 0 and par[s] == root:
                    seen["parent_is_root"] += 1  # dir = 0 with parent(s) the root
                if d == 0 and par[s] != root and top(s) != top(f):
                    seen["path_through_root"] += 1  # dir = 0 with the target path through the root
                if d == 1 and par[s] == root:
                    seen["rest_moves_below_root"] += 1  # dir = 1 with s a child of the root
    assert all(seen.values()), seen


# ---- 5. a second reference: the engine's own log-likelihood call on mi_spr_neighbour's trees ----

def test_agrees_with_log_likelihoods_of_mi_spr_neighbour_trees():
    from libsbn_amd import spr_neighbour
    c = SC.SMALL[1]
    x = SC.case(*c)
    assert x.n == 8
    eng = SC.engine(x)
    res = _scan(eng, x, trees=slice(0, 1))
    mv = R.moves(x.n, x.pids[0])
    nb = [spr_neighbour(x.n, x.pids[0], x.bls[0], s, d, f) for s, d, f, _ in mv]
    own = eng.log_likelihoods(x.pids[:1], x.bls[:1], x.pr[:1], rescaling=x.rescaling)[0]
    nll = eng.log_likelihoods(np.stack([a for a, _ in nb]), np.stack([b for _, b in nb]),
                              np.repeat(x.pr[:1], len(nb), axis=0), rescaling=x.rescaling)
    got = res.log_likelihoods[0] + np.array([res.delta[0][s, d, f] for s, d, f, _ in mv])
    err = float(np.max(np.abs(got - nll) / np.abs(nll)))
    print(f"{len(mv)} moves of an 8-taxon tree: logL + delta against the log-likelihood call {err:.2e}")
    assert err <= R.REL and abs(res.log_likelihoods[0] - own) <= R.REL * abs(own)


# ---- 6. batching: bit for bit ----

def _five():
    return SC.case("n12", 65, 4, "GTR", "states", True, count=5, seed_offset=500)


def test_alone_and_in_a_batch():
    x = _five()
    eng = SC.engine(x)
    batch = _scan(eng, x)
    for t in (0, 3):
        alone = _scan(eng, x, trees=slice(t, t + 1))
        for k in ("log_likelihoods", "best_target", "best_delta", "best_move", "delta"):
            assert np.array_equal(getattr(alone, k)[0], getattr(batch, k)[t]), (t, k)
    slim = _scan(eng, x, table=False)
    assert slim.delta is None and np.array_equal(slim.best_target, batch.best_target)
    assert np.array_equal(slim.best_delta, batch.best_delta) and np.array_equal(slim.best_move, batch.best_move)


def test_cut_into_launches_by_the_budget(monkeypatch):
    x = _five()
    whole = SC.engine(x)
    ref = _scan(whole, x)
    assert whole.last_call_launches()[0] == 1
    n, K, tiles = x.n, x.K, 2
    E, ppad = 2 * n - 3, tiles * 64
    per_tree = 8 * ((2 * n - 2) * K * ppad * 4 + ppad + tiles * 2 * E * E) + 4 * ((n - 1) + (2 * n - 2) + 1) * ppad
    monkeypatch.setenv("MI_PHYLO_PLV_BYTES", str(2 * per_tree + per_tree // 2))
    parts = SC.engine(x)
    got = _scan(parts, x)
    assert parts.last_call_launches()[0] >= 3
    assert _same(ref, got)
    monkeypatch.setenv("MI_PHYLO_PLV_BYTES", str(per_tree - 1))
    small = SC.engine(x)
    with pytest.raises(RuntimeError, match=rf"{per_tree} bytes.*{per_tree - 1} bytes"):
        _scan(small, x)


def test_tree_sharded_handle_and_pattern_sharded_refusal():
    x = _five()
    ref = _scan(SC.engine(x), x)
    trees = SC.engine(x, shard_devices=[0, 0])
    assert _same(ref, _scan(trees, x))
    _path(trees, rescaled=True)
    pats = SC.engine(x, shard_devices=[0, 0], shard_mode="patterns")
    _refused_without_touching_outputs(pats, x.n, x.pids, x.bls, x.pr, 0, "pattern-sharded")
    with pytest.raises(RuntimeError, match="pattern-sharded"):
        _scan(pats, x)
    with pytest.raises(RuntimeError, match="pattern-sharded"):
        pats.reserve_spr_scan(5)


def test_device_call_after_the_reservation_replayed_from_a_graph():
    torch = pytest.importorskip("torch")
    x = _five()
    T, E = 5, 2 * x.n - 3
    eng = SC.engine(x)
    ref = _scan(eng, x, radius=2)
    dev = torch.device("cuda", 0)
    d_pid = torch.from_numpy(np.ascontiguousarray(x.pids, np.int32)).to(dev)
    d_bl = torch.from_numpy(np.ascontiguousarray(x.bls)).to(dev)
    d_pr = torch.from_numpy(np.ascontiguousarray(x.pr)).to(dev)
    outs = dict(log_likelihoods=torch.zeros(T, dtype=torch.float64, device=dev),
                best_target=torch.zeros((T, E, 2), dtype=torch.int32, device=dev),
                best_delta=torch.zeros((T, E, 2), dtype=torch.float64, device=dev),
                best_move=torch.zeros((T, 3), dtype=torch.int32, device=dev),
                delta=torch.zeros((T, E, 2, E), dtype=torch.float64, device=dev))
    gs = torch.cuda.Stream()

    def call(stream, engine=None):
        (engine or fresh).spr_scan_device(
            stream, T, d_pid.data_ptr(), d_bl.data_ptr(), d_pr.data_ptr(), outs["best_target"].data_ptr(),
            outs["best_delta"].data_ptr(), out_ll=outs["log_likelihoods"].data_ptr(),
            out_best_move=outs["best_move"].data_ptr(), out_delta=outs["delta"].data_ptr(), rescaling=x.rescaling,
            radius=2)

    # (the other engine runs the same call on the stream first: the kernels' code objects are
    # loaded -- into device memory -- at their first launch, which is not the engine's allocation)
    call(gs.cuda_stream, eng)
    torch.cuda.synchronize()
    fresh = SC.engine(x)
    fresh.reserve_spr_scan(T)
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info(0)[0]
    with torch.cuda.stream(gs):
        call(gs.cuda_stream)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info(0)[0] == free_before  # (reserved: the call allocated nothing)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=gs):
        call(torch.cuda.current_stream().cuda_stream)
    _path(fresh, rescaled=True)
    for _ in range(2):
        for o in outs.values():
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for k, o in outs.items():
            assert np.array_equal(o.cpu().numpy(), getattr(ref, k)), k
    fresh.check_status()


# ---- 7. refusals and reports ----

def test_twenty_state_engine_refuses():
    import aa_utils as A
    import libsbn_amd as L
    import tree_utils as TU
    rng = np.random.default_rng(121)
    tips, w = A.random_aa_alignment(6, 20, rng)
    pids, bls = TU.random_trees(6, 2, rng)
    eng = L.Engine(L.PhyloModelSpecification("WAG", "constant", "strict"), tips, w, device=0)
    _refused_without_touching_outputs(eng, 6, pids, bls, eng._params(None, 2), 0, "4-state only")
    with pytest.raises(RuntimeError, match="4-state only"):
        eng.spr_scan(pids, bls, None)
    with pytest.raises(RuntimeError, match="4-state only"):
        eng.reserve_spr_scan(2)


def test_bad_tree_is_reported():
    x = SC.case(*SC.SMALL[4])
    bad = x.pids.copy()
    bad[1, 0] = 0
    with pytest.raises(RuntimeError, match="post-order id form"):
        SC.engine(x).spr_scan(bad, x.bls, x.pr)
