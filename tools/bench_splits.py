#!/usr/bin/env python3
"""Cost of the split-table calls: the split index of a batch of trees (with its
statistics) and the Robinson-Foulds / branch-score matrix from it.

Shapes: DS1's (27 taxa) and 100 taxa; T = 1 and 1000 trees.  Inputs: uniform random-join trees
(almost no nontrivial split is shared: the table is as large as it gets), and the output of a
short SPR search (two moves, radius 3) from neighbour-joining trees of bootstrap replicates (most
splits shared: what a bootstrap analysis hands over).  Every leg runs in a child process of its
own.  Per leg, milliseconds between device events around ONE call on a stream of its own, median
of `--rounds` rounds after a warm-up, the calls alternating within a round:
  index   split_index_device   (statistics included)
  rf      rf_distances_device  (branch score included)
Nothing is asserted about the times: no other implementation of this work exists in the library
(the tests' Python sets are the only other one).

    python tools/bench_splits.py [--rounds 5] [--shapes ds1,100x500] [--trees 1,1000] [--inputs random,searched]"""
import argparse
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

ROW = np.array([0.12, 0.28, 0.1, 0.14, 0.26, 0.1, 0.3, 0.2, 0.24, 0.26, 0.7])  # GTR rates, frequencies, shape


def workload(shape):
    import bench
    if shape == "ds1":
        tips, w, _, _ = bench.ds1_workload(1)
        return tips, w
    n, P = (int(x) for x in shape.split("x"))
    rng = np.random.default_rng(47)
    pid = bench.random_unrooted_topology(n, rng)
    bl = rng.exponential(0.05, size=2 * n - 2)
    return bench.evolved_alignment(pid, bl, P, rng), np.ones(P)


def trees_of(eng, kind, n, T, w):
    import bench
    import libsbn_amd as L
    rng = np.random.default_rng(11)
    if kind == "random":
        pids = np.stack([bench.random_unrooted_topology(n, rng) for _ in range(T)]).astype(np.int32)
        bls = rng.exponential(0.05, size=(T, 2 * n - 2))
        bls[:, -1] = 0.0
        return pids, bls
    start = eng.starting_trees(L.rell_weights(w, T, 1) if T > 1 else None, ROW)
    found = eng.spr_search(start.parent_ids, start.branch_lengths, np.tile(ROW, (T, 1)), max_moves=2, radius=3)
    return found.parent_ids, found.branch_lengths


def leg(shape, kind, T, rounds):
    import torch
    import libsbn_amd as L
    tips, w = workload(shape)
    n, P = tips.shape
    dev = torch.device("cuda", 0)
    eng = L.Engine(L.PhyloModelSpecification("GTR", "weibull+4", "none"), tips, w, device=0)
    pids, bls = trees_of(eng, kind, n, T, w)
    E, cap, W = 2 * n - 3, T * (2 * n - 3), (n + 31) // 32
    d_pid, d_bl = torch.from_numpy(np.array(pids)).to(dev), torch.from_numpy(np.array(bls)).to(dev)
    i32, f64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float64, device=dev)
    index, count = torch.empty((T, E + 2), **i32), torch.zeros(1, **i32)
    bits, first, trees = torch.empty((cap, W), **i32), torch.empty(cap, **i32), torch.empty(cap, **i32)
    stats = torch.empty((cap, 3), **f64)
    rf, bs = torch.empty((T, T), **i32), torch.empty((T, T), **f64)
    side = torch.cuda.Stream()
    s = side.cuda_stream
    calls = {
        "index": lambda: eng.split_index_device(s, T, n, d_pid.data_ptr(), cap, index.data_ptr(), count.data_ptr(),
                                                bits.data_ptr(), first.data_ptr(), trees.data_ptr(),
                                                stats.data_ptr(), d_bl.data_ptr()),
        "rf": lambda: eng.rf_distances_device(s, T, n, index.data_ptr(), rf.data_ptr(), bs.data_ptr(),
                                              d_bl.data_ptr()),
    }
    eng.reserve_splits(T, n)
    paths = {}
    for _ in range(2):
        for name, call in calls.items():
            call()
            paths[name] = eng.last_call_path()
    torch.cuda.synchronize()
    eng.check_status()
    times = {k: [] for k in calls}
    for _ in range(rounds):
        for name, call in calls.items():
            with torch.cuda.stream(side):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                call()
                b.record()
                b.synchronize()
            times[name].append(a.elapsed_time(b))
    tag = f"{shape} ({n} taxa) {kind} T={T}"
    S = int(count.cpu()[0])
    off = rf.cpu().numpy()[~np.eye(T, dtype=bool)]
    print(f"{tag:34s} [{paths['index']}] S = {S} of {cap} occurrences; mean RF "
          f"{(off.mean() if T > 1 else 0.0):.1f} of {2 * (n - 3)}")
    for k, v in times.items():
        print(f"{tag:34s} {k:6s} {np.median(v):9.3f} ms  (min {min(v):.3f}, max {max(v):.3f})")
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="ds1,100x500")
    ap.add_argument("--trees", default="1,1000")
    ap.add_argument("--inputs", default="random,searched")
    ap.add_argument("--leg", nargs=3, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        leg(a.leg[0], a.leg[1], int(a.leg[2]), a.rounds)
        return
    for shape in a.shapes.split(","):
        for kind in a.inputs.split(","):
            for T in a.trees.split(","):
                subprocess.run([sys.executable, os.path.abspath(__file__), "--rounds", str(a.rounds), "--leg", shape,
                                kind, T], check=True)


if __name__ == "__main__":
    main()
