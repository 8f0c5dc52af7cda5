#!/usr/bin/env python3
"""Cost of the NNI hill-climbing search next to what a caller had before it.

Shapes: DS1 (27 taxa x 934 patterns) x 1000 trees and 100 taxa x 500 patterns x 1000 random
trees, JC69 + weibull+4; every tree starts `--away` random NNI moves from its topology, all
branches at 0.1.  Legs, each in a child process of its own, alternating within a round after a
warm-up:
  search  one nni_search_device call of T trees on this build: milliseconds between device
          events around the call, and the wall clock of the same call
  loop    the Python loop a caller had to write (optimize_branch_lengths -> nni_scan ->
          nni_neighbour per tree, on all T trees every round) with the yardstick library: wall
          clock (its device work runs on the engine's own stream between host steps)
  parts   with the yardstick library, the standalone optimize_branch_lengths_device and
          nni_scan_device calls over the search's per-round batches (the trees still searching,
          at the lengths they carried): device events, summed over the rounds
  apply   nni_apply_device alone on T trees taking their first move (this build): device events
  grad    (DS1, with --yardstick) the default gradient call on this build and on the yardstick
          library, as tools/bench_nni_scan.py measures it
Median of `--rounds` rounds with the spread (min, max).  The yardstick library is another build
(e.g. the parent commit's: it has every call the loop and the parts need); without --yardstick
it is this build.

    python tools/bench_nni_search.py [--rounds 7] [--shapes ds1,100x500] [--trees 1000]
                                     [--away 3] [--yardstick other/libmi_phylo.so]"""
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

MIN_GAIN = 1e-3


def start_trees(shape, T, away):
    tips, w, pids, _ = B.workload(shape, T)
    n = tips.shape[0]
    rng = np.random.default_rng(53)
    bl = np.full(2 * n - 2, 0.1)
    bl[-1] = 0.0
    pids = np.array(pids, np.int32)
    for t in range(T):
        for _ in range(away):
            pids[t], _ = L.nni_neighbour(n, pids[t], bl, int(rng.integers(n, 2 * n - 3)), int(rng.integers(0, 2)))
    return tips, w, pids, np.tile(bl, (T, 1)), np.tile([0.7, 1.0], (T, 1))


def on_device(*arrays):
    dev = torch.device("cuda", 0)
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def event_ms(stream, call):
    with torch.cuda.stream(stream):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
    return a.elapsed_time(b)


def python_loop(eng, pids, start, pr, record=None):
    """The caller's loop over the public calls; record: a list that gets, per round, the
    searching trees' (parent ids, start lengths, optimised lengths, params)."""
    n, T = eng.taxon_count, len(pids)
    pid, bl = pids.copy(), start.copy()
    searching = np.ones(T, bool)
    moves = 0
    while searching.any():
        opt = eng.optimize_branch_lengths(pid, bl, pr)
        _, delta, best = eng.nni_scan(pid, opt.branch_lengths, pr)
        if record is not None:
            on = np.flatnonzero(searching)
            record.append((pid[on].copy(), bl[on].copy(), opt.branch_lengths[on].copy(), pr[on].copy()))
        bl = opt.branch_lengths.copy()
        for t in np.flatnonzero(searching):
            if best[t] >= 0 and delta[t].reshape(-1)[best[t]] > MIN_GAIN:
                pid[t], bl[t] = L.nni_neighbour(n, pid[t], opt.branch_lengths[t], best[t] >> 1, best[t] & 1)
                moves += 1
            else:
                searching[t] = False
    return moves


def worker(leg, shape, T, away):
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
        M = 100
        o_pid, o_bl, o_ll = torch.empty((T, N - 2), **i32), torch.empty((T, N - 1), **f64), torch.empty(T, **f64)
        o_cnt, o_st = torch.empty(T, **i32), torch.empty(T, **i32)
        eng.reserve_nni_search(T)

        def run():
            t0 = time.perf_counter()
            ms = event_ms(side, lambda: eng.nni_search_device(
                side.cuda_stream, T, d_pid.data_ptr(), d_bl.data_ptr(), d_pr.data_ptr(), o_pid.data_ptr(),
                o_bl.data_ptr(), o_ll.data_ptr(), o_cnt.data_ptr(), o_st.data_ptr(), max_moves=M))
            return f"{ms} {(time.perf_counter() - t0) * 1e3}"
        run()
        info = f"{eng.last_call_path()} evaluations={eng.last_call_info()[1]} moved trees={int((o_cnt > 0).sum())}"
    elif leg == "loop":
        def run():
            t0 = time.perf_counter()
            python_loop(eng, pids, start, pr)
            return f"{(time.perf_counter() - t0) * 1e3}"
        info = f"moves={python_loop(eng, pids, start, pr)}"
    elif leg == "parts":
        rounds = []
        python_loop(eng, pids, start, pr, rounds)
        batches = []
        for r_pid, r_start, r_opt, r_pr in rounds:
            c = len(r_pid)
            batches.append((c, on_device(r_pid, r_start, r_opt, r_pr),
                            (torch.empty((c, N - 1), **f64), torch.empty(c, **f64), torch.empty(c, **i32),
                             torch.empty((c, N, 2), **f64))))
        eng.reserve_branch_opt(T)
        eng.reserve_nni_scan(T)

        def run():
            opt_ms = scan_ms = 0.0
            for c, (p, s, o, q), (o_bl, o_ll, o_st, o_delta) in batches:
                opt_ms += event_ms(side, lambda: eng.optimize_branch_lengths_device(
                    side.cuda_stream, c, p.data_ptr(), s.data_ptr(), q.data_ptr(), o_bl.data_ptr(), o_ll.data_ptr(),
                    o_st.data_ptr()))
                scan_ms += event_ms(side, lambda: eng.nni_scan_device(
                    side.cuda_stream, c, p.data_ptr(), o.data_ptr(), q.data_ptr(), o_delta.data_ptr()))
            return f"{opt_ms} {scan_ms}"
        info = "batches=" + ",".join(str(c) for c, _, _ in batches)
    elif leg == "apply":
        opt = eng.optimize_branch_lengths(pids, start, pr)
        _, _, best = eng.nni_scan(pids, opt.branch_lengths, pr)
        d_pid, d_bl, d_mv = on_device(pids, opt.branch_lengths, best.astype(np.int32))
        o_pid, o_bl = torch.empty((T, N - 2), **i32), torch.empty((T, N - 1), **f64)
        eng.reserve_nni_search(T)

        def once():
            for _ in range(10):
                eng.nni_apply_device(side.cuda_stream, T, d_pid.data_ptr(), d_bl.data_ptr(), d_mv.data_ptr(),
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


class Leg:
    def __init__(self, leg, shape, T, away, library=None):
        env = dict(os.environ)
        if library:
            env["MI_PHYLO_LIBRARY"] = os.path.abspath(library)
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", leg, "--shapes", shape,
                                   "--trees", str(T), "--away", str(away)],
                                  stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=env)
        first = self.p.stdout.readline().strip()
        if not first.startswith("ready"):
            raise RuntimeError(f"the {leg} process did not start")
        self.info = first[6:]

    def go(self):
        self.p.stdin.write("go\n")
        self.p.stdin.flush()
        out = self.p.stdout.readline().split()
        if not out:
            raise RuntimeError("a leg's process ended")
        return [float(x) for x in out]

    def close(self):
        try:
            self.p.stdin.write("quit\n")
            self.p.stdin.flush()
        except OSError:
            pass
        self.p.wait(timeout=120)


def measure(shape, T, away, rounds, yardstick):
    legs = {"search": Leg("search", shape, T, away), "loop": Leg("loop", shape, T, away, yardstick),
            "parts": Leg("parts", shape, T, away, yardstick), "apply": Leg("apply", shape, T, away)}
    grads = [B.Yardstick(None, 10, T), B.Yardstick(yardstick, 10, T)] if shape == "ds1" and yardstick else []
    columns = {"search": ("search (events)", "search (wall)"), "loop": ("loop (wall)",),
               "parts": ("parts: optimiser", "parts: scan"), "apply": ("apply",)}
    times = {c: [] for cs in columns.values() for c in cs}
    times.update({"grad": [], "grad-yardstick": []})
    try:
        for _ in range(rounds):
            for leg, cs in columns.items():
                for c, v in zip(cs, legs[leg].go()):
                    times[c].append(v)
            if grads:
                times["grad"].append(grads[0].grad())
                times["grad-yardstick"].append(grads[1].grad())
    finally:
        for x in list(legs.values()) + grads:
            x.close()
    name = f"{shape} x {T}"
    for leg in legs:
        print(f"{name:16s} {leg}: {legs[leg].info}")
    med = {k: float(np.median(v)) for k, v in times.items() if v}
    for k, v in med.items():
        print(f"{name:16s} {k:18s} {v:10.3f} ms  (min {min(times[k]):.3f}, max {max(times[k]):.3f})")
    parts = med["parts: optimiser"] + med["parts: scan"]
    print(f"{name:16s} search / parts = {med['search (events)'] / parts:.3f}   loop / search (wall) = "
          f"{med['loop (wall)'] / med['search (wall)']:.2f}")
    if "grad-yardstick" in med:
        print(f"{name:16s} grad here / yardstick = {med['grad'] / med['grad-yardstick']:.3f}")
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--trees", type=int, default=1000)
    ap.add_argument("--away", type=int, default=3, help="random NNI moves between a topology and its start")
    ap.add_argument("--shapes", default=",".join(B.SHAPES))
    ap.add_argument("--yardstick", default=None, help="another build of the library for loop, parts and grad")
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        worker(a.worker, a.shapes, a.trees, a.away)
        return
    for shape in a.shapes.split(","):
        measure(shape, a.trees, a.away, a.rounds, a.yardstick)


if __name__ == "__main__":
    main()
