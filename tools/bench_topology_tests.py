#!/usr/bin/env python3
"""Cost of drawing bootstrap weights on the device and of the KH / SH / AU tests.

Shape: DS1 (27 taxa x 934 patterns) x `--trees` trees, JC69 + weibull+4, `--replicates`
replicates per block, the ten default scales.  Legs, alternating within a round after a warm-up:
  sampler   bootstrap_weights_device: B rows of N sites, the matrix left on the device
  host      the way without it: rell_weights on the host (numpy's multinomial) and the upload of
            its [B][P] matrix
  call      Engine.topology_tests from host arrays: upload, per-pattern log-likelihoods, the ten
            blocks, the table, one download (wall clock)
  device    topology_tests_device on per-pattern log-likelihoods resident on the device
  samplers  the ten blocks' samplers alone (bootstrap_weights_device at the ten site counts)
  products  the ten blocks' rell_device calls alone, on one block's weights
The statistics' share of `device` is what `samplers` and `products` leave.  Milliseconds between
device events around `--reps` back-to-back calls (host legs: wall clock of one call), median of
`--rounds` rounds with the spread (min, max).  No time is asserted.

    python tools/bench_topology_tests.py [--rounds 7] [--reps 5] [--trees 100] [--replicates 10000]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import libsbn_amd as L  # noqa: E402

SCALES = (1.0, 0.5, 0.6, 0.7, 0.8, 0.9, 1.1, 1.2, 1.3, 1.4)


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
    torch.cuda.synchronize()
    t = time.perf_counter()
    call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trees", type=int, default=100)
    ap.add_argument("--replicates", type=int, default=10000)
    a = ap.parse_args()
    T, B = a.trees, a.replicates
    tips, w, pids, bls = bench.ds1_workload(T)
    P, N = tips.shape[1], int(w.sum())
    sites = [int(np.floor(x * N + 0.5)) for x in SCALES]
    reps = [B] * len(SCALES)
    dev = torch.device("cuda", 0)
    f64 = dict(dtype=torch.float64, device=dev)
    side = torch.cuda.Stream()
    st = side.cuda_stream
    eng = L.Engine(L.PhyloModelSpecification("JC69", "weibull+4", "strict"), tips, w, device=0)
    params = np.tile([0.7, 1.0], (T, 1))
    ll, s = eng.pattern_log_likelihoods(pids, bls, params)
    d_s, d_w = torch.from_numpy(s).to(dev), torch.from_numpy(np.ascontiguousarray(w, np.float64)).to(dev)
    d_W, d_c = torch.empty((B, P), **f64), torch.empty((B, T), **f64)
    d_table, d_bp = torch.empty((T, 11), **f64), torch.empty(T, **f64)
    d_counts = torch.empty((len(SCALES), T), dtype=torch.int32, device=dev)
    eng.reserve_bootstrap_weights(B, P)
    eng.reserve_topology_tests(T, P, B)
    eng.reserve_rell(B, T, P)

    def sampler(n=N):
        eng.bootstrap_weights_device(st, P, d_w.data_ptr(), B, n, 1, 0, d_W.data_ptr())

    def host():
        with torch.cuda.stream(side):
            torch.from_numpy(L.rell_weights(w, B, 1)).to(dev)

    def call():
        return eng.topology_tests(pids, bls, params, replicates=B, seed=1)

    def device():
        eng.topology_tests_device(st, T, P, d_s.data_ptr(), d_w.data_ptr(), sites, reps, 1, 0, d_table.data_ptr(),
                                  d_counts.data_ptr())

    def samplers():
        for n in sites:
            sampler(n)

    def products():
        for _ in sites:
            eng.rell_device(st, B, T, P, d_s.data_ptr(), d_W.data_ptr(), d_bp.data_ptr(), out_replicate_ll=d_c.data_ptr())

    for _ in range(2):
        sampler()
        device()
        products()
    host()
    r = call()
    torch.cuda.synchronize()
    eng.check_status(st)
    assert np.array_equal(d_table.cpu().numpy(), r.table, equal_nan=True)  # (the two forms: the same bits)
    legs = {"sampler": lambda: timed(side, sampler, a.reps), "host": lambda: wall(host), "call": lambda: wall(call),
            "device": lambda: timed(side, device, a.reps), "samplers": lambda: timed(side, samplers, a.reps),
            "products": lambda: timed(side, products, a.reps)}
    times = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, leg in legs.items():
            times[k].append(leg())
    med = {k: float(np.median(v)) for k, v in times.items()}
    name = f"ds1 x {T}, B = {B}, N = {N}, P = {P}"
    for k in legs:
        print(f"{name} {k:9s} {med[k]:10.4f} ms  (min {min(times[k]):.4f}, max {max(times[k]):.4f})")
    print(f"{name} host / sampler = {med['host'] / med['sampler']:.1f}; draws per second of the sampler: "
          f"{B * N / (med['sampler'] * 1e-3):.3e}; bytes written per second: {8.0 * B * P / (med['sampler'] * 1e-3):.3e}")
    rest = med["device"] - med["samplers"] - med["products"]
    print(f"{name} shares of the device form: sampler {med['samplers'] / med['device']:.3f}, product and its passes "
          f"{med['products'] / med['device']:.3f}, statistics and the rest {rest / med['device']:.3f}; "
          f"device / call = {med['device'] / med['call']:.3f}")
    best = int(np.argmin(r.delta))
    print(f"{name} best tree {best}: p_AU in [{r.p_au.min():.4f}, {r.p_au.max():.4f}], "
          f"trees with two or more usable scales: {int((r.usable_scales >= 2).sum())}")


if __name__ == "__main__":
    main()
