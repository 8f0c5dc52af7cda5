#!/usr/bin/env python3
"""Cost of the starting-tree calls: pairwise maximum-likelihood distances,
neighbour joining, and the two in one call.

Inputs: DS1 (27 taxa x its site patterns) and 100 taxa x 500 patterns evolved along a random
tree, under GTR + weibull+4; B = 1 (the engine's own pattern weights) and B = 1000 rows of
bootstrap weights (rell_weights).  Every leg (input, B) runs in a child process of its own.
Per leg, milliseconds between device events around ONE call on a stream of its own, median of
`--rounds` rounds after a warm-up, the three calls alternating within a round:
  dist    pairwise_distances_device   model set-up, counts (matrix cores), distances
  nj      neighbour_joining_device    on those distances
  start   starting_trees_device       both
Printed with them: the call's path, the solver's statuses, and the matrix-core fraction of the
WHOLE `dist` call -- 2 x 256 x (tile blocks on or above the diagonal) x P x B flops against
the FP64 matrix peak measured on this machine (README) -- a lower bound of the counts
kernel's own, which the call's other two kernels share the time of.

    python tools/bench_start_trees.py [--rounds 9] [--shapes ds1,100x500] [--replicates 1,1000]"""
import argparse
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

PEAK_TFLOPS = 71.0  # FP64 matrix peak as measured (tools/fp64_peak_probe.hip; README)
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


def leg(shape, B, rounds):
    import torch
    import libsbn_amd as L
    tips, w = workload(shape)
    n, P = tips.shape
    dev = torch.device("cuda", 0)
    eng = L.Engine(L.PhyloModelSpecification("GTR", "weibull+4", "none"), tips, w, device=0)
    d_w = torch.from_numpy(L.rell_weights(w, B, 1)).to(dev) if B > 1 else None
    d_row = torch.from_numpy(ROW).to(dev)
    pairs = n * (n - 1) // 2
    f64 = dict(dtype=torch.float64, device=dev)
    dist, bl = torch.empty((B, n, n), **f64), torch.empty((B, 2 * n - 2), **f64)
    pid = torch.empty((B, 2 * n - 3), dtype=torch.int32, device=dev)
    status = torch.empty((B, pairs), dtype=torch.int8, device=dev)
    side = torch.cuda.Stream()
    s, wp = side.cuda_stream, (d_w.data_ptr() if B > 1 else None)
    calls = {
        "dist": lambda: eng.pairwise_distances_device(s, B, wp, d_row.data_ptr(), dist.data_ptr(),
                                                      out_pair_status=status.data_ptr()),
        "nj": lambda: eng.neighbour_joining_device(s, B, n, dist.data_ptr(), pid.data_ptr(), bl.data_ptr()),
        "start": lambda: eng.starting_trees_device(s, B, wp, d_row.data_ptr(), pid.data_ptr(), bl.data_ptr(),
                                                   dist.data_ptr()),
    }
    eng.reserve_start_trees(B)
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
    tag = f"{shape} ({n} x {P}) B={B}"
    print(f"{tag:28s} [{paths['start']}]")
    print(f"{tag:28s} pair status: {np.bincount(status.cpu().numpy().reshape(-1), minlength=5).tolist()} "
          "(converged, lower, upper, no data, limit)")
    for k, v in times.items():
        print(f"{tag:28s} {k:6s} {np.median(v):9.3f} ms  (min {min(v):.3f}, max {max(v):.3f})")
    nt = (n + 3) // 4
    flops = 2.0 * 256 * (nt * (nt + 1) // 2) * P * B
    frac = flops / (np.median(times["dist"]) * 1e-3) / (PEAK_TFLOPS * 1e12)
    print(f"{tag:28s} matrix-core fraction of the dist call: {100 * frac:.2f} % of {PEAK_TFLOPS:.0f} TFLOP/s; "
          f"nj / start = {100 * np.median(times['nj']) / np.median(times['start']):.1f} %")
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--shapes", default="ds1,100x500")
    ap.add_argument("--replicates", default="1,1000")
    ap.add_argument("--leg", nargs=2, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        leg(a.leg[0], int(a.leg[1]), a.rounds)
        return
    for shape in a.shapes.split(","):
        for B in a.replicates.split(","):
            subprocess.run([sys.executable, os.path.abspath(__file__), "--rounds", str(a.rounds), "--leg", shape, B],
                           check=True)


if __name__ == "__main__":
    main()
