"""Taking SPR moves on the device (mi_engine_spr_apply_unrooted, Engine.spr_apply): per tree the
tree mi_spr_neighbour returns, bit for bit -- parent ids equal, the lengths' bits equal.  The
lengths are distinct random doubles, so a length on the wrong edge shows."""
import numpy as np
import pytest

import spr_ref as R
import tree_utils as TU

pytestmark = pytest.mark.gpu

COPY = (-1, -1, -1)


def _engine(n):
    """(The alignment plays no part in a move: four patterns of anything.)"""
    import libsbn_amd as L
    tips = np.zeros((n, 4), np.int32)
    return L.Engine(L.PhyloModelSpecification("JC69", "constant", "strict"), tips, np.ones(4), device=0)


def _lengths(n, rng):
    bl = rng.exponential(0.1, size=2 * n - 2) + 1e-3
    bl[-1] = rng.random()  # (the entry of 2n-3 is copied, whatever it is)
    assert len(set(bl.tolist())) == len(bl)
    return bl


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.int64),
                          np.ascontiguousarray(b, np.float64).view(np.int64))


def _reversed_path(n, pid, s, d, f):
    """Nodes whose parent link the move reverses: from par[f] up to the hub's child on that side
    (none for dir = 0 with the hub below the root)."""
    root = 2 * n - 3
    hub = int(pid[s]) if d == 0 else s
    if d == 0 and hub != root:
        return 0
    k, v = 0, int(pid[f])
    while v != hub:
        k, v = k + 1, int(pid[v])
    return k


def _maxleaf(n, pid):
    ml = list(range(n)) + [-1] * (n - 2)
    for v in range(2 * n - 3):  # (ids are a post-order)
        ml[pid[v]] = max(ml[pid[v]], ml[v])
    return ml


def _reorders_elsewhere(n, pid, bl, new_pid, new_bl):
    """Does a node that the surgery did not touch -- both child edges keep their lengths and still
    meet in one parent -- see its children in another order?  (Edges are told apart by their
    lengths, which are all different.)"""
    root = 2 * n - 3
    where = {float(t): v for v, t in enumerate(new_bl[:root])}
    ml, new_ml = _maxleaf(n, pid), _maxleaf(n, new_pid)
    kids = {}
    for v in range(root):
        kids.setdefault(int(pid[v]), []).append(v)
    for w, ks in kids.items():
        if w == root:
            continue
        a, b = ks
        if float(bl[a]) not in where or float(bl[b]) not in where:
            continue
        a2, b2 = where[float(bl[a])], where[float(bl[b])]
        if new_pid[a2] != new_pid[b2]:
            continue
        if (ml[a] < ml[b]) != (new_ml[a2] < new_ml[b2]):
            return True
    return False


def _census(n, pid, bl, s, d, f, dist, want_pid, want_bl, seen):
    root = 2 * n - 3
    hub = int(pid[s]) if d == 0 else s
    if d == 0 and hub == root:
        seen["dir0_hub_root"] += 1
    elif d == 0:
        y = [v for v in range(root) if pid[v] == hub and v != s][0]
        seen["dir0_y_leaf" if y < n else "dir0_y_internal"] += 1
    else:
        seen["dir1"] += 1
    seen["f_root_child"] += int(pid[f]) == root
    seen["near" if dist == 1 else "far"] += 1
    seen["reorder"] += _reorders_elsewhere(n, pid, bl, want_pid, want_bl)
    seen["longest_path"] = max(seen["longest_path"], _reversed_path(n, pid, s, d, f))


def _check_moves(n, pid, bl, triples, seen, eng=None, dists=None, reference=False):
    """The kernel on T copies of (pid, bl), one triple each, against mi_spr_neighbour."""
    import libsbn_amd as L
    eng = eng or _engine(n)
    triples = np.asarray(triples, np.int32).reshape(-1, 3)
    T = len(triples)
    got_pid, got_bl = eng.spr_apply(np.tile(pid, (T, 1)), np.tile(bl, (T, 1)), triples)
    for t, (s, d, f) in enumerate(triples.tolist()):
        want_pid, want_bl = L.spr_neighbour(n, pid, bl, s, d, f)
        assert np.array_equal(got_pid[t], want_pid), (n, s, d, f)
        assert _same_bits(got_bl[t], want_bl), (n, s, d, f)
        if reference:
            ref_pid, ref_bl = R.neighbour(n, pid, bl, s, d, f, known_move=True)
            assert np.array_equal(got_pid[t], ref_pid) and _same_bits(got_bl[t], ref_bl), (n, s, d, f)
        _census(n, pid, bl, s, d, f, dists[t] if dists is not None else 2, want_pid, want_bl, seen)


def _new_census():
    return dict(dir0_hub_root=0, dir0_y_leaf=0, dir0_y_internal=0, dir1=0, f_root_child=0, near=0, far=0,
                reorder=0, longest_path=0)


def _every_move(n, pid, bl, seen, reference=False):
    mv = R.moves(n, pid)
    _check_moves(n, pid, bl, [m[:3] for m in mv], seen, dists=[m[3] for m in mv], reference=reference)
    return len(mv)


def test_every_valid_move_of_small_random_trees():
    """n = 4 (the smallest tree with a move; the hub is often the root), 5, 6 and 9: every triple
    of every tree in one call per tree, and a census of what the batch covers."""
    seen = _new_census()
    for n in (4, 5, 6, 9):
        rng = np.random.default_rng(150 + n)
        for _ in range(3):
            assert _every_move(n, TU.random_topology(n, rng), _lengths(n, rng), seen, reference=True) > 0
    for kind in ("dir0_hub_root", "dir0_y_leaf", "dir0_y_internal", "dir1", "f_root_child", "near", "far", "reorder"):
        assert seen[kind] > 0, seen


@pytest.mark.parametrize("n", [33, 34])
def test_every_move_of_ladders_either_side_of_64_nodes(n):
    rng = np.random.default_rng(162)
    assert 2 * n - 2 in (64, 66)
    seen = _new_census()
    _every_move(n, TU.ladder_topology(n), _lengths(n, rng), seen)
    assert seen["dir1"] > 0 and seen["dir0_hub_root"] > 0 and seen["reorder"] > 0, seen


def _lds_nodes():
    """kSprApplyLdsNodes: the node count up to which the kernel keeps a tree's arrays in LDS."""
    import pathlib
    import re
    header = pathlib.Path(__file__).resolve().parent.parent / "libsbn_amd" / "csrc" / "mi_phylo_kernels.h"
    return int(re.search(r"kSprApplyLdsNodes = (\d+)", header.read_text()).group(1))


def _sampled_moves(n, pid, bl, count, rng):
    """`count` valid triples drawn at random: the host function says which are moves."""
    import libsbn_amd as L
    E = 2 * n - 3
    out = []
    while len(out) < count:
        s, d, f = int(rng.integers(0, E)), int(rng.integers(0, 2)), int(rng.integers(0, E))
        try:
            L.spr_neighbour(n, pid, bl, s, d, f)
        except RuntimeError:
            continue
        out.append((s, d, f))
    return out


def _deep_moves(n, pid):
    """Moves of a ladder whose reversed path is long: the deepest leaf as the target, pruned edges
    s far above it (dir = 1: the clade of s keeps f), and the rest of the tree hung below (dir = 0
    of a root child, the hub the root)."""
    root = 2 * n - 3
    depth = np.zeros(root + 1, int)
    for v in range(root - 1, -1, -1):
        depth[v] = depth[pid[v]] + 1
    f = int(np.argmax(depth[:n]))
    chain, v = [], int(pid[f])
    while v != root:
        chain.append(v)
        v = int(pid[v])
    out = [(s, 1, f) for s in chain[-8:]] + [(s, 1, f) for s in chain[70:74]]
    out += [(v, 0, f) for v in range(root) if pid[v] == root and v != chain[-1]]
    return out


@pytest.mark.parametrize("shape", ["random", "ladder"])
@pytest.mark.parametrize("n", [256, 257, 258, 300])
def test_sampled_moves_of_large_trees(n, shape):
    """512 nodes (n = 257) and fewer keep the working arrays in LDS, 514 and more in the global
    workspace.  The ladder makes the reversed path longer than one block of 64 lanes and the
    pointer-jumping depth about n."""
    assert _lds_nodes() == 2 * 257 - 2
    rng = np.random.default_rng(164 + n)
    pid = TU.random_topology(n, rng) if shape == "random" else TU.ladder_topology(n)
    bl = _lengths(n, rng)
    triples = _sampled_moves(n, pid, bl, 200, rng)
    if shape == "ladder":
        triples += _deep_moves(n, pid)
    seen = _new_census()
    _check_moves(n, pid, bl, triples, seen)
    assert seen["dir1"] > 0 and seen["dir0_y_internal"] > 0 and seen["reorder"] > 0, seen
    if shape == "ladder":
        assert seen["longest_path"] > 64 and seen["dir0_hub_root"] > 0, seen


def test_triples_and_copies_mixed_in_one_batch():
    import libsbn_amd as L
    rng = np.random.default_rng(165)
    n, T = 9, 14
    pids, _ = TU.random_trees(n, T, rng)
    bls = np.stack([_lengths(n, rng) for _ in range(T)])
    triples = []
    for t in range(T):
        mv = R.moves(n, pids[t])
        triples.append(COPY if t % 3 == 0 else mv[int(rng.integers(0, len(mv)))][:3])
    got_pid, got_bl = _engine(n).spr_apply(pids, bls, triples)
    for t, (s, d, f) in enumerate(triples):
        want = (pids[t], bls[t]) if s < 0 else L.spr_neighbour(n, pids[t], bls[t], s, d, f)
        assert np.array_equal(got_pid[t], want[0]) and _same_bits(got_bl[t], want[1]), t


def _bad_triples(n, pid):
    """One triple of every kind mi_spr_neighbour refuses, from the tree itself."""
    root = 2 * n - 3
    par, kids, below = R.tree(n, pid)
    s0 = next(v for v in range(n, root) if par[v] != root and len(below[v]) >= 3)  # an inner edge below the root's children
    inside = next(v for v in range(root) if v != s0 and below[v] <= below[s0])
    outside = next(v for v in range(root) if not (below[v] <= below[s0]) and par[v] != s0 and v != par[s0]
                   and par[v] != par[s0])
    sibling = next(v for v in kids[par[s0]] if v != s0)
    return {
        "f in the moving part (dir 0)": (s0, 0, inside),
        "f in the moving part (dir 1)": (s0, 1, outside),
        "f the sibling half of the merged edge": (s0, 0, sibling),
        "f the upper half of the merged edge": (s0, 0, par[s0]),
        "f a child of s (dir 1)": (s0, 1, kids[s0][0]),
        "f = s (dir 1)": (s0, 1, s0),
        "dir 1 on a leaf": (0, 1, s0),
        "dir 2": (s0, 2, outside),
        "dir -1": (s0, -1, outside),
        "s negative": (-2, 0, outside),
        "s past the edges": (root + 5, 0, outside),
        "f negative": (s0, 0, -3),
        "f past the edges": (s0, 0, 1 << 20),
        "s the root": (root, 0, outside),
        "f the root": (s0, 0, root),
        "a copy with a hole": (-1, 0, -1),
    }


def test_bad_triples_are_reported_and_the_engine_stays_usable():
    import libsbn_amd as L
    rng = np.random.default_rng(166)
    n = 9
    pids, _ = TU.random_trees(n, 3, rng)
    bls = np.stack([_lengths(n, rng) for _ in range(3)])
    eng = _engine(n)
    good = [R.moves(n, pids[t])[0][:3] for t in range(3)]
    for what, bad in _bad_triples(n, pids[1]).items():
        if min(bad) >= 0 and max(bad[0], bad[2]) < 2 * n - 3:
            with pytest.raises(RuntimeError):  # (the host function refuses it too)
                L.spr_neighbour(n, pids[1], bls[1], *bad)
        with pytest.raises(RuntimeError, match=r"SPR move.*\(tree 1\)"):
            eng.spr_apply(pids, bls, [good[0], bad, good[2]])
        # (the error does not stick; a refused tree is copied -- seen through the device form below)
        got_pid, got_bl = eng.spr_apply(pids, bls, [good[0], COPY, good[2]])
        assert np.array_equal(got_pid[1], pids[1]) and _same_bits(got_bl[1], bls[1]), what
        want = L.spr_neighbour(n, pids[2], bls[2], *good[2])
        assert np.array_equal(got_pid[2], want[0]) and _same_bits(got_bl[2], want[1]), what


def test_a_refused_tree_is_copied():
    """The device form hands the outputs over whatever the status word says."""
    import torch
    import libsbn_amd as L
    rng = np.random.default_rng(167)
    n = 9
    pids, _ = TU.random_trees(n, 3, rng)
    bls = np.stack([_lengths(n, rng) for _ in range(3)])
    good = [R.moves(n, pids[t])[0][:3] for t in range(3)]
    bad = list(_bad_triples(n, pids[1]).values())
    eng = _engine(n)
    dev = torch.device("cuda", 0)
    B = len(bad)
    d_pid = torch.from_numpy(np.tile(pids, (B, 1)).astype(np.int32)).to(dev)
    d_bl = torch.from_numpy(np.tile(bls, (B, 1))).to(dev)
    moves = np.array([[good[0], b, good[2]] for b in bad], np.int32).reshape(3 * B, 3)
    d_mv = torch.from_numpy(moves).to(dev)
    o_pid = torch.zeros((3 * B, 2 * n - 3), dtype=torch.int32, device=dev)
    o_bl = torch.zeros((3 * B, 2 * n - 2), dtype=torch.float64, device=dev)
    eng.spr_apply_device(None, 3 * B, d_pid.data_ptr(), d_bl.data_ptr(), d_mv.data_ptr(), o_pid.data_ptr(),
                         o_bl.data_ptr())
    with pytest.raises(RuntimeError, match=r"SPR move.*\(tree \d+\)"):
        eng.check_status()
    got_pid, got_bl = o_pid.cpu().numpy(), o_bl.cpu().numpy()
    for i in range(B):
        assert np.array_equal(got_pid[3 * i + 1], pids[1]) and _same_bits(got_bl[3 * i + 1], bls[1]), bad[i]
        want = L.spr_neighbour(n, pids[2], bls[2], *good[2])
        assert np.array_equal(got_pid[3 * i + 2], want[0]) and _same_bits(got_bl[3 * i + 2], want[1])
    eng.spr_apply(pids, bls, good)  # (the engine still works)


def test_malformed_tree_is_reported():
    rng = np.random.default_rng(168)
    n = 9
    pids, _ = TU.random_trees(n, 3, rng)
    bls = np.stack([_lengths(n, rng) for _ in range(3)])
    good = [R.moves(n, pids[t])[0][:3] for t in range(3)]
    bad = pids.copy()
    bad[1, 5] = 2  # a tip as a parent
    eng = _engine(n)
    with pytest.raises(RuntimeError, match=r"\(tree 1\)"):
        eng.spr_apply(bad, bls, good)
    # a node with three children, another with one: parents above their children, still no tree
    bad = pids.copy()
    other = next(v for v in range(1, n) if pids[1, v] != pids[1, 0])
    bad[1, 0] = pids[1, other]
    with pytest.raises(RuntimeError, match=r"\(tree 1\)"):
        eng.spr_apply(bad, bls, good)
    eng.spr_apply(pids, bls, good)


@pytest.mark.parametrize("n", [12, 300])
def test_device_form_equals_the_host_form_and_allocates_nothing(n):
    import torch
    rng = np.random.default_rng(169)
    T = 40
    pids, _ = TU.random_trees(n, T, rng)
    bls = np.stack([_lengths(n, rng) for _ in range(T)])
    triples = np.array([COPY if t % 7 == 0 else _sampled_moves(n, pids[t], bls[t], 1, rng)[0] for t in range(T)],
                       np.int32)
    other = _engine(n)
    want_pid, want_bl = other.spr_apply(pids, bls, triples)
    dev = torch.device("cuda", 0)
    d_pid = torch.from_numpy(np.ascontiguousarray(pids, np.int32)).to(dev)
    d_bl = torch.from_numpy(np.ascontiguousarray(bls)).to(dev)
    d_mv = torch.from_numpy(triples).to(dev)
    o_pid = torch.zeros((T, 2 * n - 3), dtype=torch.int32, device=dev)
    o_bl = torch.zeros((T, 2 * n - 2), dtype=torch.float64, device=dev)
    stream = torch.cuda.Stream()

    def call(engine):
        engine.spr_apply_device(stream.cuda_stream, T, d_pid.data_ptr(), d_bl.data_ptr(), d_mv.data_ptr(),
                                o_pid.data_ptr(), o_bl.data_ptr())
        torch.cuda.synchronize()

    # (the same call of another engine first: what the runtime sets up on the first use of a
    # stream is not the engine's -- tests/test_branch_opt_gpu.py)
    call(other)
    o_pid.zero_()
    o_bl.zero_()
    eng = _engine(n)
    eng.reserve_spr_search(T)
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info(0)[0]
    call(eng)
    free_after = torch.cuda.mem_get_info(0)[0]
    eng.check_status()
    assert free_after == free_before, (free_before, free_after)
    assert np.array_equal(o_pid.cpu().numpy(), want_pid)
    assert _same_bits(o_bl.cpu().numpy(), want_bl)
