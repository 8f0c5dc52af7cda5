"""Taking NNI moves on the device (mi_engine_nni_apply_unrooted, Engine.nni_apply): per tree the
tree mi_nni_neighbour returns, bit for bit, and for the small sizes tests/nni_ref.py's too."""
import numpy as np
import pytest

import nni_ref as R
import tree_utils as TU

pytestmark = pytest.mark.gpu


def _engine(n):
    """(The alignment plays no part in a move: four patterns of anything.)"""
    import libsbn_amd as L
    tips = np.zeros((n, 4), np.int32)
    return L.Engine(L.PhyloModelSpecification("JC69", "constant", "strict"), tips, np.ones(4), device=0)


def _lengths(n, rng):
    bl = rng.exponential(0.1, size=2 * n - 2)
    bl[-1] = rng.random()  # (the entry of 2n-3 is copied, whatever it is)
    return bl


def _kinds(n, pid, v):
    """What a move across inner edge v exercises: u is the root, c's id is larger than v's."""
    root = 2 * n - 3
    kids = R.children(n, pid)
    u = int(pid[v])
    c = [x for x in kids[u] if x != v][0]
    return u == root, c > v


def _reorders_the_path(n, pid, new_pid, bl, new_bl, v):
    """Does the move change the child order above v?  v's largest leaf id changes with the move,
    and with it v's place among the children of u (subtrees are told apart by their lengths,
    which are all different).  Nothing changes further up: u's subtree keeps its leaves."""
    before = R.children(n, pid)[int(pid[v])].index(v)
    moved_v = int(np.flatnonzero(new_bl[:-1] == bl[v])[0])
    return R.children(n, new_pid)[int(new_pid[moved_v])].index(moved_v) != before


def _check_moves(n, pid, bl, codes, eng=None, reference=False):
    import libsbn_amd as L
    eng = eng or _engine(n)
    codes = np.asarray(codes, np.int32)
    T = len(codes)
    got_pid, got_bl = eng.nni_apply(np.tile(pid, (T, 1)), np.tile(bl, (T, 1)), codes)
    seen = dict(root=0, c_above=0, reorder=0)
    for t, code in enumerate(codes):
        v, i = int(code) >> 1, int(code) & 1
        want_pid, want_bl = L.nni_neighbour(n, pid, bl, v, i)
        assert np.array_equal(got_pid[t], want_pid), (n, v, i)
        assert np.array_equal(got_bl[t], want_bl), (n, v, i)
        if reference:
            ref_pid, ref_bl = R.neighbour(n, pid, bl, v, i)
            assert np.array_equal(got_pid[t], ref_pid) and np.array_equal(got_bl[t], ref_bl), (n, v, i)
        at_root, c_above = _kinds(n, pid, v)
        seen["root"] += at_root
        seen["c_above"] += c_above
        seen["reorder"] += _reorders_the_path(n, pid, want_pid, bl, want_bl, v)
    return seen


def _all_codes(n):
    return [2 * v + i for v in R.inner_edges(n) for i in (0, 1)]


@pytest.mark.parametrize("n", [4, 5, 6, 9])
def test_every_move_of_small_random_trees(n):
    rng = np.random.default_rng(50 + n)
    for _ in range(3):
        _check_moves(n, TU.random_topology(n, rng), _lengths(n, rng), _all_codes(n), reference=True)


def test_every_move_of_27_taxa_covers_every_kind():
    rng = np.random.default_rng(61)
    n = 27
    pid = TU.random_topology(n, rng)
    seen = _check_moves(n, pid, _lengths(n, rng), _all_codes(n), reference=True)
    assert seen["c_above"] > 0 and seen["reorder"] > 0, seen


@pytest.mark.parametrize("n", [33, 34])
def test_every_move_of_ladders_either_side_of_64_nodes(n):
    rng = np.random.default_rng(62)
    assert 2 * n - 2 in (64, 66)
    _check_moves(n, TU.ladder_topology(n), _lengths(n, rng), _all_codes(n), reference=True)


def test_every_move_of_a_balanced_64_taxon_tree_with_three_internal_root_children():
    rng = np.random.default_rng(63)
    n = 64
    pid = TU.balanced_topology(n)
    root = 2 * n - 3
    root_kids = R.children(n, pid)[root]
    assert all(k >= n for k in root_kids)
    seen = _check_moves(n, pid, _lengths(n, rng), _all_codes(n))
    assert seen["root"] == 6, seen  # u is the root for v each of its three children, both moves
    assert seen["c_above"] > 0 and seen["reorder"] > 0, seen


@pytest.mark.parametrize("n", [257, 258, 300])
def test_sampled_moves_of_large_random_trees(n):
    """512 nodes and fewer keep the working arrays in LDS, 514 and more in the global workspace."""
    rng = np.random.default_rng(64 + n)
    pid = TU.random_topology(n, rng)
    codes = rng.choice(_all_codes(n), size=200, replace=False)
    seen = _check_moves(n, pid, _lengths(n, rng), codes)
    assert seen["c_above"] > 0 and seen["reorder"] > 0, seen


def test_codes_and_copies_mixed_in_one_batch():
    import libsbn_amd as L
    rng = np.random.default_rng(65)
    n, T = 9, 12
    pids, _ = TU.random_trees(n, T, rng)
    bls = np.stack([_lengths(n, rng) for _ in range(T)])
    codes = np.array([-1 if t % 3 == 0 else int(rng.choice(_all_codes(n))) for t in range(T)], np.int32)
    got_pid, got_bl = _engine(n).nni_apply(pids, bls, codes)
    for t in range(T):
        want = (pids[t], bls[t]) if codes[t] < 0 else L.nni_neighbour(n, pids[t], bls[t], codes[t] >> 1, codes[t] & 1)
        assert np.array_equal(got_pid[t], want[0]) and np.array_equal(got_bl[t], want[1]), t


@pytest.mark.parametrize("code", [-2, 0, 2 * 9 - 1, 2 * (2 * 9 - 3), 1 << 20])
def test_bad_code_is_reported_and_the_engine_stays_usable(code):
    rng = np.random.default_rng(66)
    n = 9
    pids, bls = TU.random_trees(n, 3, rng)
    eng = _engine(n)
    good = 2 * n
    with pytest.raises(RuntimeError, match=r"NNI move.*\(tree 1\)"):
        eng.nni_apply(pids, bls, [good, code, good])
    # (the error does not stick)
    got_pid, got_bl = eng.nni_apply(pids, bls, [good, -1, good])
    assert np.array_equal(got_pid[1], pids[1]) and np.array_equal(got_bl[1], bls[1])


def test_malformed_tree_is_reported():
    rng = np.random.default_rng(67)
    n = 9
    pids, bls = TU.random_trees(n, 3, rng)
    bad = pids.copy()
    bad[1, 5] = 2  # a tip as a parent
    eng = _engine(n)
    with pytest.raises(RuntimeError, match=r"\(tree 1\)"):
        eng.nni_apply(bad, bls, [2 * n] * 3)
    eng.nni_apply(pids, bls, [2 * n] * 3)


@pytest.mark.parametrize("n", [12, 300])
def test_device_form_equals_the_host_form_and_allocates_nothing(n):
    import torch
    rng = np.random.default_rng(68)
    T = 40
    pids, _ = TU.random_trees(n, T, rng)
    bls = np.stack([_lengths(n, rng) for _ in range(T)])
    codes = rng.choice(_all_codes(n) + [-1], size=T).astype(np.int32)
    other = _engine(n)
    want_pid, want_bl = other.nni_apply(pids, bls, codes)
    dev = torch.device("cuda", 0)
    d_pid = torch.from_numpy(np.ascontiguousarray(pids, np.int32)).to(dev)
    d_bl = torch.from_numpy(np.ascontiguousarray(bls)).to(dev)
    d_mv = torch.from_numpy(codes).to(dev)
    o_pid = torch.zeros((T, 2 * n - 3), dtype=torch.int32, device=dev)
    o_bl = torch.zeros((T, 2 * n - 2), dtype=torch.float64, device=dev)
    stream = torch.cuda.Stream()

    def call(engine):
        engine.nni_apply_device(stream.cuda_stream, T, d_pid.data_ptr(), d_bl.data_ptr(), d_mv.data_ptr(),
                                o_pid.data_ptr(), o_bl.data_ptr())
        torch.cuda.synchronize()

    # (the same call of another engine first: what the runtime sets up on the first use of a
    # stream is not the engine's -- tests/test_branch_opt_gpu.py)
    call(other)
    o_pid.zero_()
    o_bl.zero_()
    eng = _engine(n)
    eng.reserve_nni_search(T)
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info(0)[0]
    call(eng)
    free_after = torch.cuda.mem_get_info(0)[0]
    eng.check_status()
    assert free_after == free_before, (free_before, free_after)
    assert np.array_equal(o_pid.cpu().numpy(), want_pid)
    assert np.array_equal(o_bl.cpu().numpy(), want_bl)
