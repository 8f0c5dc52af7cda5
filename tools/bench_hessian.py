#!/usr/bin/env python3
"""Cost of the branch-length Hessian call next to the plain gradient call.

Per shape, milliseconds per call (device events around `--reps` back-to-back *_device calls,
median of `--rounds` rounds; the legs alternate within a round, after a warm-up):
  plain     gradients, default path
  plain-v2  gradients under MI_PHYLO_GRADIENT_WALK=v2 (the second-generation walk)
  hess      branch_hessian (log-likelihood, gradient, Hessian diagonal, squared-gradient sum)
Shapes: DS1 x 1000 trees (JC69 + weibull+4) and 36 taxa x 1812 patterns x 1000 trees (the
shape whose gradient calls keep their stored vectors in the arena).

    python tools/bench_hessian.py [--trees 1000] [--reps 10] [--rounds 7]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import libsbn_amd as L  # noqa: E402


def ds3_shape(T):
    rng = np.random.default_rng(46)
    n, P = 36, 1812
    top = np.stack([bench.random_unrooted_topology(n, rng) for _ in range(50)])
    pids = np.ascontiguousarray(np.tile(top, (T // 50 + 1, 1))[:T]).astype(np.int32)
    bls = rng.exponential(0.1, size=(T, 2 * n - 2))
    bls[:, -1] = 0
    tips = bench.evolved_alignment(pids[0], bls[0], P, rng)
    return tips, np.ones(P), pids, bls


def engine(tips, w, walk=None):
    old = os.environ.get("MI_PHYLO_GRADIENT_WALK")
    if walk:
        os.environ["MI_PHYLO_GRADIENT_WALK"] = walk
    try:
        return L.Engine(L.PhyloModelSpecification("JC69", "weibull+4", "strict"), tips, w, device=0)
    finally:
        if walk and old is None:
            os.environ.pop("MI_PHYLO_GRADIENT_WALK")
        elif walk:
            os.environ["MI_PHYLO_GRADIENT_WALK"] = old


def measure(name, tips, w, pids, bls, reps, rounds):
    dev = torch.device("cuda", 0)
    T, n = pids.shape[0], tips.shape[0]
    N = 2 * n - 1
    params = np.tile([0.7, 1.0], (T, 1))
    d_pid, d_bl, d_pr = (torch.from_numpy(np.ascontiguousarray(a)).to(dev)
                         for a in (pids.astype(np.int32), bls, params))
    ll = torch.empty(T, dtype=torch.float64, device=dev)
    g, h, s = (torch.empty((T, N), dtype=torch.float64, device=dev) for _ in range(3))
    site = torch.empty(T, dtype=torch.float64, device=dev)
    side = torch.cuda.Stream()  # (a stream of its own: 0 would mean the engine's own stream)
    stream = side.cuda_stream
    plain, v2 = engine(tips, w), engine(tips, w, "v2")
    for e in (plain, v2):
        e.reserve(T, True)
    plain.reserve_hessian(T)
    args = (d_pid.data_ptr(), d_bl.data_ptr(), d_pr.data_ptr())
    legs = {
        "plain": (plain, lambda: plain.gradients_device(stream, T, *args, ll.data_ptr(), g.data_ptr(),
                                                        site.data_ptr(), None)),
        "plain-v2": (v2, lambda: v2.gradients_device(stream, T, *args, ll.data_ptr(), g.data_ptr(),
                                                     site.data_ptr(), None)),
        "hess": (plain, lambda: plain.branch_hessian_device(stream, T, *args, h.data_ptr(), ll.data_ptr(),
                                                            g.data_ptr(), s.data_ptr())),
    }
    paths = {}
    torch.cuda.set_stream(side)
    for key, (e, call) in legs.items():
        for _ in range(3):
            call()
        paths[key] = e.last_call_path()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(rounds):
        for key, (e, call) in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                call()
            b.record()
            b.synchronize()
            times[key].append(a.elapsed_time(b) / reps)
    torch.cuda.set_stream(torch.cuda.default_stream())
    plain.check_status()
    v2.check_status()
    med = {k: float(np.median(v)) for k, v in times.items()}
    for k in legs:
        spread = (min(times[k]), max(times[k]))
        print(f"{name:28s} {k:9s} {med[k]:8.3f} ms per call  (min {spread[0]:.3f}, max {spread[1]:.3f})  "
              f"[{paths[k]}]")
    print(f"{name:28s} hess / plain-v2 = {med['hess'] / med['plain-v2']:.2f}, "
          f"hess / plain = {med['hess'] / med['plain']:.2f}")
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trees", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    T = a.trees
    tips, w, pids, bls = bench.ds1_workload(T)
    measure(f"DS1 x {T} JC69+G4", tips, w, pids, bls, a.reps, a.rounds)
    tips, w, pids, bls = ds3_shape(T)
    measure(f"36 x 1812 x {T} JC69+G4", tips, w, pids, bls, a.reps, a.rounds)


if __name__ == "__main__":
    main()
