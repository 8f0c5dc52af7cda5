#!/usr/bin/env python3
"""Cost of the per-pattern log-likelihoods and of the RELL re-summation.

Shape: DS1 (27 taxa x 934 patterns) x `--trees` trees, JC69 + weibull+4.  Legs, alternating
within a round after a warm-up:
  loglik    log_likelihoods_device of T trees
  pattern   pattern_log_likelihoods_device of the same trees on the same engine: the only added
            work is T P 8 bytes of stores
  rell B    rell_device (the matrix-core product, the row pass and the column pass) for B = each
            of --replicates, on replicate weights resident on the device
  matmul B  torch.matmul of the same device tensors (W s^T): an outside yardstick
  fused B   Engine.rell_bootstrap from host arrays (upload, both calls, download)
  numpy B   the alternative without it: pattern_log_likelihoods to the host, then W @ s.T, the
            argmax and the ELW sums in numpy on --threads host threads
Milliseconds between device events around `--reps` back-to-back calls (host legs: wall clock of
one call), median of `--rounds` rounds with the spread (min, max).  `copy` is a device-to-device
copy of 1 GiB: the HBM rate the excess of `pattern` over `loglik` is judged by.

    python tools/bench_rell.py [--rounds 7] [--reps 10] [--trees 1000] [--replicates 1000,10000]
                               [--fp64-peak 71] [--threads 16]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import libsbn_amd as L  # noqa: E402


def timed(stream, call, reps):
    with torch.cuda.stream(stream):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            call()
        b.record()
        b.synchronize()
    return a.elapsed_time(b) / reps


def wall(call):
    t = time.perf_counter()
    call()
    return (time.perf_counter() - t) * 1e3


def numpy_rell(eng, pids, bls, params, W):
    ll, s = eng.pattern_log_likelihoods(pids, bls, params)
    c = W @ s.T
    best = np.argmax(c, axis=1)
    e = np.exp(c - c.max(axis=1, keepdims=True))
    return np.bincount(best, minlength=len(pids)) / len(W), (e / e.sum(axis=1, keepdims=True)).mean(axis=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--trees", type=int, default=1000)
    ap.add_argument("--replicates", default="1000,10000")
    ap.add_argument("--fp64-peak", type=float, default=71.0, help="TFLOP/s measured by tools/fp64_peak_probe.hip")
    ap.add_argument("--threads", type=int, default=16, help="host threads of the numpy leg")
    a = ap.parse_args()
    torch.set_num_threads(a.threads)
    T = a.trees
    tips, w, pids, bls = bench.ds1_workload(T)
    P = tips.shape[1]
    dev = torch.device("cuda", 0)
    f64 = dict(dtype=torch.float64, device=dev)
    side = torch.cuda.Stream()
    eng = L.Engine(L.PhyloModelSpecification("JC69", "weibull+4", "strict"), tips, w, device=0)
    params = np.tile([0.7, 1.0], (T, 1))
    d_pid, d_bl, d_pr = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (pids.astype(np.int32), bls, params))
    d_ll, d_s = torch.empty(T, **f64), torch.empty((T, P), **f64)
    eng.reserve(T, False)
    st = side.cuda_stream

    def loglik():
        eng.log_likelihoods_device(st, T, d_pid.data_ptr(), d_bl.data_ptr(), d_pr.data_ptr(), d_ll.data_ptr())

    def pattern():
        eng.pattern_log_likelihoods_device(st, T, d_pid.data_ptr(), d_bl.data_ptr(), d_pr.data_ptr(), d_s.data_ptr(),
                                           out_ll=d_ll.data_ptr())

    big = torch.empty(1 << 27, **f64)  # 1 GiB
    half = big.numel() // 2

    def copy():
        with torch.cuda.stream(side):
            big[:half].copy_(big[half:])

    for _ in range(3):
        loglik()
        pattern()
        copy()
    torch.cuda.synchronize()
    eng.check_status(st)
    pattern_path = eng.last_call_path()
    times = {"loglik": [], "pattern": [], "copy": []}
    for _ in range(a.rounds):
        times["loglik"].append(timed(side, loglik, a.reps))
        times["pattern"].append(timed(side, pattern, a.reps))
        times["copy"].append(timed(side, copy, 3))
    med = {k: float(np.median(v)) for k, v in times.items()}
    hbm = 2 * half * 8 / (med["copy"] * 1e-3) / 1e12  # read + write, TB/s
    name = f"ds1 x {T}"
    print(f"{name} [{pattern_path}]")
    for k in ("loglik", "pattern"):
        print(f"{name} {k:10s} {med[k]:9.4f} ms  (min {min(times[k]):.4f}, max {max(times[k]):.4f})")
    stores = T * P * 8
    spread = max(max(times[k]) - min(times[k]) for k in ("loglik", "pattern"))
    print(f"{name} copy rate {hbm:.2f} TB/s; pattern - loglik = {med['pattern'] - med['loglik']:.4f} ms; "
          f"{stores / 1e6:.2f} MB of stores at that rate = {stores / (hbm * 1e12) * 1e3:.4f} ms; spread {spread:.4f} ms")
    sys.stdout.flush()

    for B in (int(x) for x in a.replicates.split(",")):
        W = L.rell_weights(w, B, 1)
        d_w = torch.from_numpy(W).to(dev)
        d_c = torch.empty((B, T), **f64)
        d_best = torch.empty(B, dtype=torch.int32, device=dev)
        d_bp, d_elw = torch.empty(T, **f64), torch.empty(T, **f64)
        eng.reserve_rell(B, T, P)

        def rell():
            eng.rell_device(st, B, T, P, d_s.data_ptr(), d_w.data_ptr(), d_bp.data_ptr(),
                            out_replicate_ll=d_c.data_ptr(), out_best=d_best.data_ptr(), out_elw=d_elw.data_ptr())

        def matmul():
            with torch.cuda.stream(side):
                torch.matmul(d_w, d_s.T, out=d_c)

        def fused():
            return eng.rell_bootstrap(pids, bls, W, params)

        for _ in range(2):
            rell()
            matmul()
        torch.cuda.synchronize()
        eng.check_status(st)
        r = fused()
        nbp, nelw = numpy_rell(eng, pids, bls, params, W)
        agree = (np.array_equal(r.bootstrap_proportion, nbp), float(np.abs(r.expected_likelihood_weight - nelw).max()))
        tb = {k: [] for k in ("rell", "matmul", "fused", "numpy")}
        for _ in range(a.rounds):
            tb["rell"].append(timed(side, rell, a.reps))
            tb["matmul"].append(timed(side, matmul, a.reps))
            tb["fused"].append(wall(fused))
            tb["numpy"].append(wall(lambda: numpy_rell(eng, pids, bls, params, W)))
        mb = {k: float(np.median(v)) for k, v in tb.items()}
        flop = 2.0 * B * T * P
        traffic = 8.0 * (B * P + T * P + B * T)
        for k in tb:
            print(f"{name} B={B:<6d} {k:8s} {mb[k]:10.4f} ms  (min {min(tb[k]):.4f}, max {max(tb[k]):.4f})")
        for k in ("rell", "matmul"):
            print(f"{name} B={B:<6d} {k:8s} {flop / (mb[k] * 1e-3) / 1e12:6.2f} TFLOP/s = "
                  f"{flop / (mb[k] * 1e-3) / 1e12 / a.fp64_peak:.3f} of the FP64 matrix peak; "
                  f"{traffic / (mb[k] * 1e-3) / 1e12 / hbm:.3f} of the copy rate")
        print(f"{name} B={B:<6d} matmul / rell = {mb['matmul'] / mb['rell']:.2f}   numpy / fused = "
              f"{mb['numpy'] / mb['fused']:.2f}   (bp equal: {agree[0]}, elw differs by {agree[1]:.1e})")
        sys.stdout.flush()


if __name__ == "__main__":
    main()
