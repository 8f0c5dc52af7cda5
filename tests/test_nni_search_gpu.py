"""The NNI hill-climbing search (mi_engine_nni_search_unrooted, Engine.nni_search): optimise,
scan, move, per tree, on the device.  Against the independent CPU reference of
tests/nni_search_ref.py on its committed cases (whose decisions tests/test_nni_search_ref.py
shows to be clear of the optimiser's tolerance), and against a Python loop over the engine's own
public calls."""
import os
import subprocess

import numpy as np
import pytest

import branch_opt_ref as R
import nni_ref as NR
import nni_search_ref as S
import oracle_lib as O
import tree_utils as TU

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("parent_ids", "branch_lengths", "log_likelihood", "best_delta", "move_count", "move_log", "move_gain",
          "status", "branch_opt_status")
THREE_MOVES = S.CASES[-1]  # its last tree takes three moves (tests/test_nni_search_ref.py prints them)


def _engine(subst, site, tips, w, **kw):
    import libsbn_amd as L
    return L.Engine(L.PhyloModelSpecification(subst, site, "strict"), tips, w, device=0, **kw)


def _case_engine(case, **kw):
    spec, tips, w, pids, start, pr = case.build()
    return _engine(case.subst, case.site, tips, w, **kw)


def _log(res, t):
    return res.move_log[t, :res.move_count[t]].tolist()


def _python_loop(eng, pids, start, pr, rescaling=False, max_moves=100, min_gain=S.MIN_GAIN):
    """optimize_branch_lengths -> nni_scan -> nni_neighbour, always on all T trees (so that the
    route is the search's): (move logs, parent ids, lengths, logL, best delta, status)."""
    import libsbn_amd as L
    n = eng.taxon_count
    T = len(pids)
    pid, bl = np.array(pids, np.int32), np.array(start, float)
    logs = [[] for _ in range(T)]
    searching = np.ones(T, bool)
    out_pid, out_bl = pid.copy(), bl.copy()
    out_ll, out_delta, out_status = np.zeros(T), np.zeros(T), np.zeros(T, np.int32)
    while searching.any():
        opt = eng.optimize_branch_lengths(pid, bl, pr, rescaling=rescaling)
        _, delta, best = eng.nni_scan(pid, opt.branch_lengths, pr, rescaling=rescaling)
        bl = opt.branch_lengths.copy()  # (a tree that has stopped is carried along at its optimum)
        for t in np.flatnonzero(searching):
            gain = delta[t].reshape(-1)[best[t]] if best[t] >= 0 else 0.0
            if gain > min_gain and len(logs[t]) < max_moves:
                logs[t].append(int(best[t]))
                pid[t], bl[t] = L.nni_neighbour(n, pid[t], opt.branch_lengths[t], best[t] >> 1, best[t] & 1)
                continue
            searching[t] = False
            out_pid[t], out_bl[t], out_ll[t], out_delta[t] = pid[t], opt.branch_lengths[t], opt.log_likelihood[t], gain
            out_status[t] = S.MOVE_LIMIT if gain > min_gain else S.LOCAL_OPTIMUM
    return logs, out_pid, out_bl, out_ll, out_delta, out_status


def _same_numbers(a_ll, a_bl, b_ll, b_bl):
    """What tests/test_branch_opt_gpu.py allows between packed and unpacked runs."""
    assert np.all(np.abs(a_ll - b_ll) <= 1e-9 * np.abs(b_ll)), (a_ll, b_ll)
    for x, y in zip(a_bl, b_bl):
        assert R.relative_length_error(x[:-1], y[:-1]) <= 1e-5
        assert x[-1] == y[-1]


def _matches_python_loop(eng, res, pids, start, pr, **kw):
    logs, pid, bl, ll, delta, status = _python_loop(eng, pids, start, pr, **kw)
    for t in range(len(pids)):
        assert _log(res, t) == logs[t], (t, _log(res, t), logs[t])
        assert np.all(res.move_log[t, res.move_count[t]:] == -1) and np.all(res.move_gain[t, res.move_count[t]:] == 0)
        assert np.all(res.move_gain[t, :res.move_count[t]] > kw.get("min_gain", S.MIN_GAIN))
    assert np.array_equal(res.parent_ids, pid)
    assert np.array_equal(res.status, status)
    _same_numbers(res.log_likelihood, res.branch_lengths, ll, bl)
    return logs


def _path(eng):
    p = eng.last_call_path()
    assert " hess" in p and " nni-search rounds=" in p and " moves=" in p and " batches=" in p, p
    assert " opt iters=" not in p, p
    return p


# ---- 1. against the CPU reference ----

@pytest.mark.parametrize("case", S.CASES, ids=repr)
def test_matches_the_cpu_reference(case):
    spec, tips, w, pids, start, pr = case.build()
    eng = _case_engine(case)
    res = eng.nni_search(pids, start, pr)
    path = _path(eng)
    refs = case.reference()
    print(path)
    for t, ref in enumerate(refs):
        err = R.relative_length_error(res.branch_lengths[t, :-1], ref.branch_lengths[:-1])
        print(f"{case} tree {t}: moves {_log(res, t)} reference {ref.moves} logL {res.log_likelihood[t]!r} "
              f"- reference {res.log_likelihood[t] - ref.log_likelihood:.2e} lengths {err:.2e}")
        assert _log(res, t) == ref.moves and res.move_count[t] == len(ref.moves)
        assert NR.splits(case.n, res.parent_ids[t]) == NR.splits(case.n, ref.parent_ids)
        assert res.status[t] == ref.status
        assert abs(res.log_likelihood[t] - ref.log_likelihood) <= 1e-7
        assert err <= 1e-5
    assert f"moves={sum(len(r.moves) for r in refs)} " in path, path
    print("optimiser status", res.branch_opt_status.tolist())


# ---- 2. against a Python loop over the engine's own calls ----

@pytest.mark.parametrize("case", [S.CASES[2], S.CASES[4], S.CASES[5]], ids=repr)
def test_matches_a_python_loop_over_the_public_calls(case):
    spec, tips, w, pids, start, pr = case.build()
    eng = _case_engine(case)
    res = eng.nni_search(pids, start, pr)
    _matches_python_loop(eng, res, pids, start, pr)


# ---- 3. max_moves = 0: optimise and scan only ----

def test_no_moves_allowed_is_the_optimiser_and_the_scan():
    case = THREE_MOVES
    spec, tips, w, pids, start, pr = case.build()
    eng = _case_engine(case)
    res = eng.nni_search(pids, start, pr, max_moves=0)
    assert " rounds=1 moves=0 " in _path(eng)
    opt = eng.optimize_branch_lengths(pids, start, pr)
    _, delta, _ = eng.nni_scan(pids, opt.branch_lengths, pr)
    top = delta[:, case.n:2 * case.n - 3].reshape(len(pids), -1).max(axis=1)
    assert np.array_equal(res.branch_lengths, opt.branch_lengths)
    assert np.array_equal(res.log_likelihood, opt.log_likelihood)
    assert np.array_equal(res.branch_opt_status, opt.status)
    assert np.array_equal(res.best_delta, top)
    assert np.array_equal(res.parent_ids, pids)
    assert np.array_equal(res.status == S.MOVE_LIMIT, top > S.MIN_GAIN) and np.all(res.status <= 1)
    assert res.status[-1] == S.MOVE_LIMIT  # (the tree that would take three moves)
    assert np.all(res.move_count == 0) and res.move_log.shape == (len(pids), 0)


# ---- 4. the move limit ----

def test_one_move_of_three():
    case = THREE_MOVES
    spec, tips, w, pids, start, pr = case.build()
    t = len(pids) - 1
    assert len(case.reference()[t].moves) >= 3
    eng = _case_engine(case)
    res = eng.nni_search(pids, start, pr, max_moves=1)
    opt = eng.optimize_branch_lengths(pids, start, pr)
    assert res.status[t] == S.MOVE_LIMIT and res.move_count[t] == 1
    assert _log(res, t) == case.reference()[t].moves[:1] and res.move_log.shape == (len(pids), 1)
    ll = res.log_likelihood[t]
    assert ll >= opt.log_likelihood[t] + S.MIN_GAIN - 2.0 ** -40 * abs(ll)
    assert res.move_gain[t, 0] > S.MIN_GAIN


# ---- 5. restart ----

def test_restart_from_a_result_changes_nothing():
    case = THREE_MOVES
    spec, tips, w, pids, start, pr = case.build()
    eng = _case_engine(case)
    first = eng.nni_search(pids, start, pr)
    again = eng.nni_search(first.parent_ids, first.branch_lengths, pr)
    assert np.all(again.move_count == 0) and np.all(again.status == S.LOCAL_OPTIMUM)
    assert np.array_equal(again.parent_ids, first.parent_ids)
    assert np.array_equal(again.branch_lengths, first.branch_lengths)


# ---- 6. packing of the trees that are still searching ----

def test_packing_changes_the_cost_not_the_results():
    case = THREE_MOVES
    spec, tips, w, _, _, _ = case.build()
    n, T = case.n, 64
    rng = np.random.default_rng(71)
    true_pid = TU.random_topology(n, np.random.default_rng(case.seed))  # (the tree the case's alignment evolved down)
    start = np.full((T, 2 * n - 2), 0.1)
    start[:, -1] = 0.0
    pool = np.stack([S.random_nni_walk(n, true_pid, start[0], 5, rng)[0] for _ in range(T)])
    pr = np.repeat(case.build()[5][:1], T, axis=0)
    eng = _case_engine(case)
    first = eng.nni_search(pool, start, pr)
    movers = np.flatnonzero(first.move_count >= 1)
    assert len(movers) >= 16, first.move_count
    fresh = np.arange(2, 64, 4)  # 16 trees that will move, spread over a batch of results
    pids, bls = first.parent_ids.copy(), first.branch_lengths.copy()
    pids[fresh], bls[fresh] = pool[movers[:16]], start[movers[:16]]
    packed = eng.nni_search(pids, bls, pr)
    path, evals = _path(eng), eng.last_call_info()[1]
    assert "batches=64x1,16x" in path, path
    plain = eng.nni_search(pids, bls, pr, pack_active=False)
    plain_path, plain_evals = _path(eng), eng.last_call_info()[1]
    print(path, "|", plain_path, "| evaluations", evals, plain_evals)
    assert "batches=64x" in plain_path and "16x" not in plain_path and plain_path.endswith(" pack=off")
    others = np.setdiff1d(np.arange(T), fresh)
    assert np.all(packed.move_count[others] == 0) and np.all(packed.move_count[fresh] >= 1)
    assert np.array_equal(packed.move_log, plain.move_log) and np.array_equal(packed.move_count, plain.move_count)
    assert np.array_equal(packed.parent_ids, plain.parent_ids) and np.array_equal(packed.status, plain.status)
    _same_numbers(packed.log_likelihood, packed.branch_lengths, plain.log_likelihood, plain.branch_lengths)
    assert evals < plain_evals


# ---- 7. other paths, each against the Python loop ----

def test_rescaling():
    case = S.CASES[3]
    spec, tips, w, pids, start, pr = case.build()
    eng = _case_engine(case)
    res = eng.nni_search(pids, start, pr, rescaling=True)
    assert " rescaled " in _path(eng)
    _matches_python_loop(eng, res, pids, start, pr, rescaling=True)


def test_real_valued_tip_partials():
    case = S.CASES[3]
    spec, tips, w, pids, start, pr = case.build()
    rng = np.random.default_rng(72)
    n, P = tips.shape
    parts = np.zeros((n, P, 4))
    parts[np.arange(n)[:, None], np.arange(P)[None, :], tips] = 1.0
    parts[0] = np.where(parts[0] > 0, 1.0, rng.uniform(0.05, 0.4, size=parts[0].shape))
    eng = _engine(case.subst, case.site, None, w, use_tip_states=False, tip_partials=parts)
    res = eng.nni_search(pids, start, pr)
    assert _path(eng).startswith("gradient_hbm_hess_kernel ")
    _matches_python_loop(eng, res, pids, start, pr)


def test_six_categories_run_the_hbm_hessian_kernel():
    case = S.Case("n8-jc-k6", 8, 200, "JC69", "weibull+6", 107, (1, 2, 4))
    spec, tips, w, pids, start, pr = case.build()
    eng = _case_engine(case)
    res = eng.nni_search(pids, start, pr)
    path = _path(eng)
    assert path.startswith("gradient_hbm_hess_kernel ") and " K=6" in path, path
    _matches_python_loop(eng, res, pids, start, pr)


def test_arena_store_36_taxa(monkeypatch):
    case = S.Case("n36-jc-k4", 36, 1812, "JC69", "weibull+4", 110, (3, 6))
    spec, tips, w, pids, start, pr = case.build()
    monkeypatch.setenv("MI_PHYLO_GRADIENT_STORE", "arena")
    eng = _case_engine(case)
    res = eng.nni_search(pids, start, pr)
    assert " store=arena " in _path(eng)
    logs = _matches_python_loop(eng, res, pids, start, pr)
    print("moves", logs)


def test_step_kernel_workspace_branch_after_a_pack():
    """258 taxa: 2n-2 = 514 nodes do not fit the step kernel's LDS arrays (512), so a move is taken
    in the global workspace -- and, after a pack, in the piece of the tree's PACKED position.
    min_gain is set between the best deltas of the trees at their first optimum so that two of
    five move: round 0 of the search runs the route and the numbers of the max_moves = 0 call,
    and a tree's numbers do not depend on which others search."""
    n, T = 258, 5
    rng = np.random.default_rng(75)
    pids, bls = TU.random_trees(n, T, rng)
    tips, w = TU.random_alignment(n, 64, rng)
    eng = _engine("JC69", "constant", tips, w)
    top = eng.nni_search(pids, bls, None, max_moves=0).best_delta
    rank = np.argsort(-top)
    min_gain = 0.5 * (top[rank[1]] + top[rank[2]])
    print("best deltas", top.tolist(), "min_gain", min_gain)
    assert top[rank[1]] > min_gain > top[rank[2]]
    order = rank[[2, 0, 3, 1, 4]]  # the two that will move at indices 1 and 3: packed positions 0 and 1
    pids, bls = pids[order], bls[order]
    res = eng.nni_search(pids, bls, None, max_moves=2, min_gain=min_gain)
    path = _path(eng)
    assert "batches=5x1,2x" in path, path
    assert np.array_equal(res.move_count >= 1, [False, True, False, True, False]), res.move_count
    _matches_python_loop(eng, res, pids, bls, None, max_moves=2, min_gain=min_gain)


# ---- 8. handles and refusals ----

def test_tree_sharded_handle_gives_the_single_engines_results():
    case = THREE_MOVES
    spec, tips, w, pids, start, pr = case.build()
    pids, start, pr = np.tile(pids, (3, 1)), np.tile(start, (3, 1)), np.tile(pr, (3, 1))
    ref = _case_engine(case).nni_search(pids, start, pr)
    trees = _case_engine(case, shard_devices=[0, 0])
    got = trees.nni_search(pids, start, pr)
    _path(trees)
    for name in FIELDS:
        assert np.array_equal(getattr(ref, name), getattr(got, name)), name


def test_refusals():
    import aa_utils as A
    case = S.CASES[2]
    spec, tips, w, pids, start, pr = case.build()
    pats = _case_engine(case, shard_devices=[0, 0], shard_mode="patterns")
    with pytest.raises(RuntimeError, match="pattern-sharded"):
        pats.nni_search(pids, start, pr)
    with pytest.raises(RuntimeError, match="pattern-sharded"):
        pats.reserve_nni_search(3)
    eng = _case_engine(case)
    for bad in (-1, 10001):
        with pytest.raises(RuntimeError, match="max_moves"):
            eng.nni_search(pids, start, pr, max_moves=bad)
    for bad in (-1e-3, float("nan")):
        with pytest.raises(RuntimeError, match="min_gain"):
            eng.nni_search(pids, start, pr, min_gain=bad)
    with pytest.raises(RuntimeError, match="max_iterations"):
        eng.nni_search(pids, start, pr, branch_opt=dict(max_iterations=1001))
    broken = pids.copy()
    broken[1, 5] = 2  # a tip as a parent: not the reference's id form
    with pytest.raises(RuntimeError, match=r"\(tree 1\)"):
        eng.nni_search(broken, start, pr)
    # (the engine is still usable, and the error does not stick)
    assert np.all(eng.nni_search(pids, start, pr).status == S.LOCAL_OPTIMUM)
    rng = np.random.default_rng(73)
    atips, aw = A.random_aa_alignment(6, 20, rng)
    apids, abls = TU.random_trees(6, 2, rng)
    aa = _engine("WAG", "constant", atips, aw)
    with pytest.raises(RuntimeError, match="4-state only"):
        aa.nni_search(apids, abls, None)
    with pytest.raises(RuntimeError, match="4-state only"):
        aa.reserve_nni_search(2)


def test_three_taxa_stop_after_one_optimisation():
    rng = np.random.default_rng(74)
    pids, bls = TU.random_trees(3, 2, rng)
    tips, w = TU.random_alignment(3, 50, rng)
    eng = _engine("JC69", "constant", tips, w)
    res = eng.nni_search(pids, bls, None)
    assert " rounds=1 moves=0 " in _path(eng)
    opt = eng.optimize_branch_lengths(pids, bls, None)
    assert np.all(res.move_count == 0) and np.all(res.status == S.LOCAL_OPTIMUM) and np.all(res.best_delta == 0)
    assert np.array_equal(res.branch_lengths, opt.branch_lengths) and np.array_equal(res.parent_ids, pids)


# ---- 9. the reserved device-pointer call ----

def test_reserved_device_call_allocates_nothing_and_matches_the_host_call():
    import torch
    case = THREE_MOVES
    spec, tips, w, pids, start, pr = case.build()
    reps = 8
    pids, start, pr = np.tile(pids, (reps, 1)), np.tile(start, (reps, 1)), np.tile(pr, (reps, 1))
    T, n, M = len(pids), case.n, 6
    other = _case_engine(case)
    ref = other.nni_search(pids, start, pr, max_moves=M)
    assert f"batches={T}x1,{T // 3}x" in _path(other)  # (one tree in three moves: the call also packs)
    dev = torch.device("cuda", 0)
    d_pid = torch.from_numpy(np.ascontiguousarray(pids, np.int32)).to(dev)
    d_bl = torch.from_numpy(np.ascontiguousarray(start)).to(dev)
    d_pr = torch.from_numpy(np.ascontiguousarray(pr)).to(dev) if pr.shape[1] else torch.zeros(1, dtype=torch.float64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    f64 = dict(dtype=torch.float64, device=dev)
    outs = dict(parent_ids=torch.zeros((T, 2 * n - 3), **i32), branch_lengths=torch.zeros((T, 2 * n - 2), **f64),
                log_likelihood=torch.zeros(T, **f64), best_delta=torch.zeros(T, **f64),
                move_count=torch.zeros(T, **i32), move_log=torch.zeros((T, M), **i32),
                move_gain=torch.zeros((T, M), **f64), status=torch.full((T,), 7, **i32),
                branch_opt_status=torch.full((T,), 7, **i32))
    stream = torch.cuda.Stream()

    def call(engine):
        o = {k: v.data_ptr() for k, v in outs.items()}
        engine.nni_search_device(stream.cuda_stream, T, d_pid.data_ptr(), d_bl.data_ptr(), d_pr.data_ptr(),
                                 o["parent_ids"], o["branch_lengths"], o["log_likelihood"], o["move_count"],
                                 o["status"], out_best_delta=o["best_delta"], out_move_log=o["move_log"],
                                 out_move_gain=o["move_gain"], out_branch_opt_status=o["branch_opt_status"],
                                 max_moves=M)
        torch.cuda.synchronize()

    # (the same call of ANOTHER engine first, on the same stream: tests/test_branch_opt_gpu.py)
    call(other)
    for v in outs.values():
        v.fill_(7)
    eng = _case_engine(case)
    eng.reserve_nni_search(T)
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info(0)[0]
    call(eng)
    free_after = torch.cuda.mem_get_info(0)[0]
    _path(eng)
    eng.check_status()
    assert free_after == free_before, (free_before, free_after)
    for name in FIELDS:
        assert np.array_equal(outs[name].cpu().numpy(), getattr(ref, name)), name
    host = eng.nni_search(pids, start, pr, max_moves=M)
    for name in FIELDS:
        assert np.array_equal(getattr(host, name), getattr(ref, name)), name


# ---- 10. the C++ adapter ----

def test_cpp_adapter_gives_the_python_result(tmp_path):
    import libsbn_amd as L
    exe = tmp_path / "nni_search_example"
    lib = os.path.join(REPO, "libsbn_amd")
    data = os.path.join(REPO, "tests/golden/data")
    subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(REPO, "tests/cpp/nni_search_example.cpp"),
                    "-L" + lib, "-lmi_phylo", "-lmi_phylo_host", "-Wl,-rpath," + lib, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe), data], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.endswith("done\n"), out.stdout + out.stderr
    inst = L.unrooted_instance("ds1")
    inst.read_nexus_file(os.path.join(data, "DS1.subsampled_10.t"))
    inst.read_fasta_file(os.path.join(data, "DS1.fasta"))
    inst.prepare_for_phylo_likelihood(L.PhyloModelSpecification("JC69", "constant", "strict"), 1)
    pids, bls = inst._trees()
    eng = inst.get_engine()
    res = eng.nni_search(pids, bls, inst.get_phylo_model_params(), max_moves=5)
    first = np.where(res.move_count > 0, res.move_log[:, 0], -1)
    moved, _ = eng.nni_apply(pids, bls, first)
    lines = out.stdout.splitlines()
    assert len(lines) == 2 * len(pids) + 1
    for t in range(len(pids)):
        want = (f"tree {t} status {res.status[t]} opt {res.branch_opt_status[t]} ll {float(res.log_likelihood[t]).hex()} "
                f"delta {float(res.best_delta[t]).hex()} moves" + "".join(f" {m}" for m in _log(res, t)) +
                " parents" + "".join(f" {p}" for p in res.parent_ids[t]))
        got = lines[t].split()
        # (C's %a and Python's hex() write the same number differently: compare the values)
        exp = want.split()
        for i in (got.index("ll") + 1, got.index("delta") + 1):
            got[i], exp[i] = float.fromhex(got[i]), float.fromhex(exp[i])
        assert got == exp, (t, lines[t], want)
        assert lines[len(pids) + t] == f"applied {t} move {first[t]} parents" + "".join(f" {p}" for p in moved[t])
    print("moves per tree:", res.move_count.tolist())
