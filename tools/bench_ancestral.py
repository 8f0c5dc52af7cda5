#!/usr/bin/env python3
"""Cost of the ancestral-state call next to its yardsticks.

Shapes: DS1 (27 taxa x 934 patterns) x 1000 trees and 100 taxa x 500 patterns x 1000 random
trees, JC69 + weibull+4 (tools/bench_nni_scan.py's workloads).  Legs, alternating within a round
after a warm-up, all on the device form of their call:
  all     ancestral_states_device, every output asked for
  state   ancestral_states_device, state_posteriors only
  scan    nni_scan_device on the same engine
  hbm     the gradient call of T trees under MI_PHYLO_GRADIENT_PATH=hbm: the kernel family's
          yardstick (the expectation: `state` costs about this walk without its two Q products,
          plus the stores, T (n-2) P 32 bytes)
  copy    a 1 GiB device-to-device copy: the rate the stores are judged against
  host    (--host) downloading nothing and running tests/ancestral_ref.py's algorithm in float64
          numpy for 8 trees on up to 16 processes, in a child process that never opens the GPU,
          scaled to the batch
Milliseconds between device events around `--reps` back-to-back calls, median of `--rounds`
rounds with the spread (min, max).

    python tools/bench_ancestral.py [--rounds 7] [--reps 5] [--shapes ds1,100x500] [--trees 1000] [--host]"""
import argparse
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import numpy as np  # noqa: E402

SHAPES = ("ds1", "100x500")
SHAPE_PARAMS = (0.7, 1.0)  # Weibull shape, clock rate: bench_nni_scan's model row
HOST_TREES = 8


def _host_tree(job):
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import ancestral_ref as A
    pid, bl, vec, rates, weights = job
    Q, pi = A.gtr_q(np.ones(6), np.full(4, 0.25), np.float64)
    A.ancestral(pid, bl, Q, pi, rates, weights, vec, dtype=np.float64, with_tips=True)
    return 0


def host_leg(shape, T):
    """Seconds for HOST_TREES trees with the reference's algorithm in float64, scaled to T."""
    from concurrent.futures import ProcessPoolExecutor
    import multiprocessing
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import ancestral_ref as A
    import bench_nni_scan as S
    import oracle_lib as O
    tips, w, pids, bls = S.workload(shape, T)
    rates, weights, _ = O.weibull_rates(4, SHAPE_PARAMS[0])
    vec = A.tip_vectors(tips, np.float64)
    jobs = [(pids[t], bls[t], vec, rates, weights) for t in range(HOST_TREES)]
    with ProcessPoolExecutor(max_workers=min(16, HOST_TREES),
                             mp_context=multiprocessing.get_context("spawn")) as pool:
        list(pool.map(_host_tree, jobs[:1]))  # (workers started, modules imported)
        t0 = time.perf_counter()
        list(pool.map(_host_tree, jobs))
        dt = time.perf_counter() - t0
    print(dt * T / HOST_TREES * 1e3, flush=True)


def measure(shape, T, rounds, reps, host):
    import torch
    import bench_nni_scan as S
    tips, w, pids, bls = S.workload(shape, T)
    n, P = tips.shape
    N, K = 2 * n - 1, 4
    dev = torch.device("cuda", 0)
    f64 = dict(dtype=torch.float64, device=dev)
    side = torch.cuda.Stream()
    eng = S.engine(tips, w)
    params = np.tile(SHAPE_PARAMS, (T, 1))
    d_pid, d_bl, d_pr = (torch.from_numpy(np.ascontiguousarray(a)).to(dev)
                         for a in (pids.astype(np.int32), bls, params))
    state, ll = torch.empty((T, n - 2, P, 4), **f64), torch.empty(T, **f64)
    mp = torch.empty((T, n - 2, P), dtype=torch.int8, device=dev)
    cat, rate, tip = torch.empty((T, P, K), **f64), torch.empty((T, P), **f64), torch.empty((T, n, P, 4), **f64)
    delta, best = torch.empty((T, N, 2), **f64), torch.empty(T, dtype=torch.int32, device=dev)
    eng.reserve_ancestral(T)
    eng.reserve_nni_scan(T)
    ins = (d_pid.data_ptr(), d_bl.data_ptr(), d_pr.data_ptr())

    def call_all():
        eng.ancestral_states_device(side.cuda_stream, T, *ins, state.data_ptr(), out_ll=ll.data_ptr(),
                                    out_map_states=mp.data_ptr(), out_category_posteriors=cat.data_ptr(),
                                    out_pattern_rates=rate.data_ptr(), out_tip_posteriors=tip.data_ptr())

    def call_state():
        eng.ancestral_states_device(side.cuda_stream, T, *ins, state.data_ptr())

    def scan():
        eng.nni_scan_device(side.cuda_stream, T, *ins, delta.data_ptr(), out_ll=ll.data_ptr(), out_best=best.data_ptr())

    src = torch.empty(1 << 27, **f64)  # 1 GiB
    dst = torch.empty_like(src)

    def copy():
        with torch.cuda.stream(side):
            dst.copy_(src, non_blocking=True)

    hbm = S.GradBatch(tips, w, pids, bls, hbm=True)
    for _ in range(2):
        call_all()
        call_state()
        scan()
        hbm.call()
        copy()
    torch.cuda.synchronize()
    path = eng.last_call_path()
    for e in (eng, hbm.eng):
        e.check_status()
    legs = dict(all=(side, call_all), state=(side, call_state), scan=(side, scan), hbm=(hbm.side, hbm.call),
                copy=(side, copy))
    times = {k: [] for k in legs}
    for _ in range(rounds):
        for k, (stream, call) in legs.items():
            times[k].append(S.timed(stream, call, reps))
    med = {k: float(np.median(v)) for k, v in times.items()}
    name = f"{shape} x {T}"
    state_bytes = T * (n - 2) * P * 32
    all_bytes = state_bytes + T * (n - 2) * P + T * P * 8 * (K + 1) + T * n * P * 32
    print(f"{name:16s} [{path}] | hbm: [{hbm.eng.last_call_path()}]")
    for k in legs:
        print(f"{name:16s} {k:6s} {med[k]:10.3f} ms  (min {min(times[k]):.3f}, max {max(times[k]):.3f})")
    gib = 2 ** 30
    print(f"{name:16s} state / hbm = {med['state'] / med['hbm']:.2f}   state / scan = {med['state'] / med['scan']:.2f}   "
          f"all / state = {med['all'] / med['state']:.2f}")
    print(f"{name:16s} stores: state {state_bytes / 1e6:.0f} MB, all {all_bytes / 1e6:.0f} MB; the copy moves 1 GiB in "
          f"{med['copy']:.3f} ms ({gib / med['copy'] / 1e6:.0f} GB/s written): the state rows alone would take "
          f"{state_bytes / gib * med['copy']:.3f} ms at that rate, all outputs {all_bytes / gib * med['copy']:.3f} ms")
    if host:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--host-leg", shape, "--trees", str(T)],
                             capture_output=True, text=True, check=True)
        ms = float(out.stdout.strip().splitlines()[-1])
        print(f"{name:16s} host   {ms:10.1f} ms  ({HOST_TREES} trees in float64 numpy on {min(16, HOST_TREES)} processes, "
              f"scaled; no download) = {ms / med['all']:.0f} x all")
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trees", type=int, default=1000)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--host", action="store_true", help="also time the host alternative")
    ap.add_argument("--host-leg", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.host_leg:
        host_leg(a.host_leg, a.trees)
        return
    for shape in a.shapes.split(","):
        measure(shape, a.trees, a.rounds, a.reps, a.host)


if __name__ == "__main__":
    main()
