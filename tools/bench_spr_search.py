#!/usr/bin/env python3
"""Cost of the SPR hill-climbing search next to what a caller had before it.

Shapes: DS1 (27 taxa x 934 patterns) and 100 taxa x 500 patterns, each x a batch of trees (the
SPR scan's workspace is 7.3 MB per DS1 tree: small batches), JC69 + weibull+4; every tree starts
`--away` random SPR moves from its topology, all branches at 0.1; radius 3 and radius 0.  Legs,
each in a child process of its own, alternating within a round after a warm-up:
  search  one spr_search_device call of T trees on this build: milliseconds between device
          events around the call, and the wall clock of the same call
  loop    the Python loop a caller had to write (optimize_branch_lengths -> spr_scan ->
          spr_neighbour per tree, on all T trees every round) with the yardstick library: wall
          clock (its device work runs on the engine's own stream between host steps)
  parts   with the yardstick library, the standalone optimize_branch_lengths_device and
          spr_scan_device calls over the search's per-round batches (the trees still searching,
          at the lengths they carried): device events, summed over the rounds
  apply   spr_apply_device alone on T trees taking their first move (this build): device events
  grad    (DS1, with --yardstick) the default gradient call on DS1 x 1000 on this build and on
          the yardstick library, as tools/bench_nni_scan.py measures it
Median of `--rounds` rounds with the spread (min, max).  The yardstick library is another build
(e.g. the parent commit's: it has every call the loop and the parts need); without --yardstick
it is this build.

    python tools/bench_spr_search.py [--rounds 7] [--shapes ds1,100x500] [--trees 64,8]
                                     [--radii 3,0] [--away 3] [--max-moves 10]
                                     [--yardstick other/libmi_phylo.so]"""
import argparse
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench_nni_scan as B  # noqa: E402
import libsbn_amd as L  # noqa: E402
from bench_nni_search import Leg as _NniLeg, event_ms, on_device  # noqa: E402

MIN_GAIN = 1e-3


def random_move(n, pid, bl, rng):
    """A random SPR move of one tree: triples are drawn until mi_spr_neighbour takes one."""
    E = 2 * n - 3
    while True:
        s, d, f = int(rng.integers(0, E)), int(rng.integers(0, 2)), int(rng.integers(0, E))
        try:
            return L.spr_neighbour(n, pid, bl, s, d, f)
        except RuntimeError:
            continue


def start_trees(shape, T, away):
    tips, w, pids, _ = B.workload(shape, T)
    n = tips.shape[0]
    rng = np.random.default_rng(59)
    bl = np.full(2 * n - 2, 0.1)
    bl[-1] = 0.0
    pids = np.array(pids, np.int32)
    for t in range(T):
        for _ in range(away):
            pids[t], _ = random_move(n, pids[t], bl, rng)
    return tips, w, pids, np.tile(bl, (T, 1)), np.tile([0.7, 1.0], (T, 1))


def python_loop(eng, pids, start, pr, radius, max_moves, record=None):
    """The caller's loop over the public calls; record: a list that gets, per round, the
    searching trees' (parent ids, start lengths, optimised lengths, params)."""
    n, T = eng.taxon_count, len(pids)
    pid, bl = pids.copy(), start.copy()
    searching = np.ones(T, bool)
    taken = np.zeros(T, int)
    while searching.any():
        opt = eng.optimize_branch_lengths(pid, bl, pr)
        scan = eng.spr_scan(pid, opt.branch_lengths, pr, radius=radius)
        if record is not None:
            on = np.flatnonzero(searching)
            record.append((pid[on].copy(), bl[on].copy(), opt.branch_lengths[on].copy(), pr[on].copy()))
        bl = opt.branch_lengths.copy()
        for t in np.flatnonzero(searching):
            s, d, f = (int(x) for x in scan.best_move[t])
            if s >= 0 and scan.best_delta[t, s, d] > MIN_GAIN and taken[t] < max_moves:
                pid[t], bl[t] = L.spr_neighbour(n, pid[t], opt.branch_lengths[t], s, d, f)
                taken[t] += 1
            else:
                searching[t] = False
    return int(taken.sum())


def worker(leg, shape, T, away, radius, max_moves):
    import ctypes
    from libsbn_amd import _capi
    probe = ctypes.CDLL(_capi.LIB_PATH)
    for name in [k for k in _capi.SYMBOLS if not hasattr(probe, k)]:
        del _capi.SYMBOLS[name]  # (an older build does not export the calls added since)
    tips, w, pids, start, pr = start_trees(shape, T, away)
    n = tips.shape[0]
    N = 2 * n - 1
    dev = torch.device("cuda", 0)
    f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
    eng = B.engine(tips, w)
    side = torch.cuda.Stream()
    info = ""
    if leg == "search":
        d_pid, d_bl, d_pr = on_device(pids, start, pr)
        o_pid, o_bl, o_ll = torch.empty((T, N - 2), **i32), torch.empty((T, N - 1), **f64), torch.empty(T, **f64)
        o_cnt, o_st = torch.empty(T, **i32), torch.empty(T, **i32)
        eng.reserve_spr_search(T)

        def run():
            t0 = time.perf_counter()
            ms = event_ms(side, lambda: eng.spr_search_device(
                side.cuda_stream, T, d_pid.data_ptr(), d_bl.data_ptr(), d_pr.data_ptr(), o_pid.data_ptr(),
                o_bl.data_ptr(), o_ll.data_ptr(), o_cnt.data_ptr(), o_st.data_ptr(), max_moves=max_moves,
                radius=radius))
            return f"{ms} {(time.perf_counter() - t0) * 1e3}"
        run()
        info = f"{eng.last_call_path()} evaluations={eng.last_call_info()[1]} moved trees={int((o_cnt > 0).sum())}"
    elif leg == "loop":
        def run():
            t0 = time.perf_counter()
            python_loop(eng, pids, start, pr, radius, max_moves)
            return f"{(time.perf_counter() - t0) * 1e3}"
        info = f"moves={python_loop(eng, pids, start, pr, radius, max_moves)}"
    elif leg == "parts":
        rounds = []
        python_loop(eng, pids, start, pr, radius, max_moves, rounds)
        batches = []
        for r_pid, r_start, r_opt, r_pr in rounds:
            c = len(r_pid)
            batches.append((c, on_device(r_pid, r_start, r_opt, r_pr),
                            (torch.empty((c, N - 1), **f64), torch.empty(c, **f64), torch.empty(c, **i32),
                             torch.empty((c, N - 2, 2), **i32), torch.empty((c, N - 2, 2), **f64),
                             torch.empty((c, 3), **i32))))
        eng.reserve_branch_opt(T)
        eng.reserve_spr_scan(T)

        def run():
            opt_ms = scan_ms = 0.0
            for c, (p, s, o, q), (o_bl, o_ll, o_st, o_target, o_delta, o_move) in batches:
                opt_ms += event_ms(side, lambda: eng.optimize_branch_lengths_device(
                    side.cuda_stream, c, p.data_ptr(), s.data_ptr(), q.data_ptr(), o_bl.data_ptr(), o_ll.data_ptr(),
                    o_st.data_ptr()))
                scan_ms += event_ms(side, lambda: eng.spr_scan_device(
                    side.cuda_stream, c, p.data_ptr(), o.data_ptr(), q.data_ptr(), o_target.data_ptr(),
                    o_delta.data_ptr(), out_best_move=o_move.data_ptr(), radius=radius))
            return f"{opt_ms} {scan_ms}"
        info = "batches=" + ",".join(str(c) for c, _, _ in batches)
    elif leg == "apply":
        opt = eng.optimize_branch_lengths(pids, start, pr)
        scan = eng.spr_scan(pids, opt.branch_lengths, pr, radius=radius)
        d_pid, d_bl, d_mv = on_device(pids, opt.branch_lengths, scan.best_move.astype(np.int32))
        o_pid, o_bl = torch.empty((T, N - 2), **i32), torch.empty((T, N - 1), **f64)
        eng.reserve_spr_search(T)

        def once():
            for _ in range(10):
                eng.spr_apply_device(side.cuda_stream, T, d_pid.data_ptr(), d_bl.data_ptr(), d_mv.data_ptr(),
                                     o_pid.data_ptr(), o_bl.data_ptr())

        def run():
            return f"{event_ms(side, once) / 10}"
    run()
    torch.cuda.synchronize()
    eng.check_status()
    print("ready " + info, flush=True)
    for line in sys.stdin:
        if line.strip() != "go":
            break
        print(run(), flush=True)


class Leg(_NniLeg):
    def __init__(self, leg, shape, T, away, radius, max_moves, library=None):
        env = dict(os.environ)
        if library:
            env["MI_PHYLO_LIBRARY"] = os.path.abspath(library)
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", leg, "--shapes", shape,
                                   "--trees", str(T), "--away", str(away), "--radii", str(radius),
                                   "--max-moves", str(max_moves)],
                                  stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=env)
        first = self.p.stdout.readline().strip()
        if not first.startswith("ready"):
            raise RuntimeError(f"the {leg} process did not start")
        self.info = first[6:]


def measure(shape, T, away, radius, max_moves, rounds, yardstick, with_grad):
    args = (shape, T, away, radius, max_moves)
    legs = {"search": Leg("search", *args), "loop": Leg("loop", *args, yardstick),
            "parts": Leg("parts", *args, yardstick), "apply": Leg("apply", *args)}
    grads = [B.Yardstick(None, 10, 1000), B.Yardstick(yardstick, 10, 1000)] if with_grad else []
    columns = {"search": ("search (events)", "search (wall)"), "loop": ("loop (wall)",),
               "parts": ("parts: optimiser", "parts: scan"), "apply": ("apply",)}
    times = {c: [] for cs in columns.values() for c in cs}
    times.update({"grad": [], "grad-yardstick": []})
    try:
        for r in range(rounds):
            for leg, cs in columns.items():
                for c, v in zip(cs, legs[leg].go()):
                    times[c].append(v)
            # (the two builds take turns at going first: whichever follows the short apply leg
            # finds the device idle and reads a few per cent slower)
            for k in ((0, 1) if r % 2 == 0 else (1, 0)) if grads else ():
                times["grad" if k == 0 else "grad-yardstick"].append(grads[k].grad())
    finally:
        for x in list(legs.values()) + grads:
            x.close()
    name = f"{shape} x {T} r={radius}"
    for leg in legs:
        print(f"{name:20s} {leg}: {legs[leg].info}")
    med = {k: float(np.median(v)) for k, v in times.items() if v}
    for k, v in med.items():
        print(f"{name:20s} {k:18s} {v:10.3f} ms  (min {min(times[k]):.3f}, max {max(times[k]):.3f})")
    parts = med["parts: optimiser"] + med["parts: scan"]
    print(f"{name:20s} search / parts = {med['search (events)'] / parts:.3f}   loop / search (wall) = "
          f"{med['loop (wall)'] / med['search (wall)']:.2f}   apply / search = {med['apply'] / med['search (events)']:.5f}")
    if "grad-yardstick" in med:
        print(f"{name:20s} grad (DS1 x 1000) here / yardstick = {med['grad'] / med['grad-yardstick']:.3f}")
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--shapes", default=",".join(B.SHAPES))
    ap.add_argument("--trees", default="64,8", help="batch size per shape")
    ap.add_argument("--radii", default="3,0")
    ap.add_argument("--away", type=int, default=3, help="random SPR moves between a topology and its start")
    ap.add_argument("--max-moves", type=int, default=10)
    ap.add_argument("--yardstick", default=None, help="another build of the library for loop, parts and grad")
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        worker(a.worker, a.shapes, int(a.trees), a.away, int(a.radii), a.max_moves)
        return
    shapes, trees = a.shapes.split(","), [int(x) for x in a.trees.split(",")]
    first = True
    for shape, T in zip(shapes, trees):
        for radius in (int(x) for x in a.radii.split(",")):
            measure(shape, T, a.away, radius, a.max_moves, a.rounds, a.yardstick,
                    with_grad=first and shape == "ds1" and a.yardstick is not None)
            first = False


if __name__ == "__main__":
    main()
