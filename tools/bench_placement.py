#!/usr/bin/env python3
"""Cost of the placement call next to its yardsticks.

Shapes: DS1 (27 taxa x 934 patterns) and 100 taxa x 500 patterns, one tree, JC69 + weibull+4
(tools/bench_nni_scan.py's workloads), Q = 10 000 random queries over the identity column map,
G = 1 and G = 4 pendant lengths.  Legs, alternating within a round after a warm-up, all on the
device form of their call and on the same engine:
  place   placement_device, edge log-likelihoods, best edges and weight ratios
  table   placement_device of ONE query: set-up, matrices and the table walk (its scoring launch
          is one workgroup per edge) -- the table part
  (score  = place - table, derived: the scoring part and the finalize launch)
  state   ancestral_states_device with state_posteriors only: the nearest walk of the family
  copy    a 1 GiB device-to-device copy
  host    (--host) the alternative without the scoring kernel: download the table once and do the
          gather-sum in float64 numpy on up to 16 processes, in a child process that never opens
          the GPU; HOST_QUERIES queries, scaled to Q
Milliseconds between device events around `--reps` back-to-back calls, median of `--rounds`
rounds with the spread (min, max).  Nothing here asserts a time.

    python tools/bench_placement.py [--rounds 7] [--reps 5] [--shapes ds1,100x500] [--queries 10000] [--host]"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import numpy as np  # noqa: E402

SHAPES = ("ds1", "100x500")
SHAPE_PARAMS = (0.7, 1.0)  # Weibull shape, clock rate: bench_nni_scan's model row
PENDANTS = (0.05, 0.01, 0.2, 0.8)
HOST_QUERIES = 512


def _host_block(job):
    path, queries, weights = job
    S = np.load(path, mmap_mode="r")  # [E][G][5][P]
    cols = np.arange(S.shape[3])
    out = np.empty((len(queries),) + S.shape[:2])
    for i, x in enumerate(queries):
        out[i] = np.sum(weights * S[:, :, np.minimum(x, 4), cols], axis=-1)
    return out.max(axis=2).argmax(axis=1)


def host_leg(path, Q):
    """Seconds for HOST_QUERIES queries against the downloaded table in float64 numpy, scaled to Q."""
    from concurrent.futures import ProcessPoolExecutor
    import multiprocessing
    S = np.load(path, mmap_mode="r")
    rng = np.random.default_rng(1)
    x = rng.integers(0, 5, size=(HOST_QUERIES, S.shape[3]))
    w = np.ones(S.shape[3])
    jobs = [(path, x[i::16], w) for i in range(16)]
    with ProcessPoolExecutor(max_workers=16, mp_context=multiprocessing.get_context("spawn")) as pool:
        list(pool.map(_host_block, jobs[:1]))  # (workers started, modules imported)
        t0 = time.perf_counter()
        list(pool.map(_host_block, jobs))
        dt = time.perf_counter() - t0
    print(dt * Q / HOST_QUERIES * 1e3, flush=True)


def measure(shape, Q, G, rounds, reps, host):
    import torch
    import bench_nni_scan as S
    tips, w, pids, bls = S.workload(shape, 1)
    n, P = tips.shape
    E = 2 * n - 3
    dev = torch.device("cuda", 0)
    f64 = dict(dtype=torch.float64, device=dev)
    side = torch.cuda.Stream()
    eng = S.engine(tips, w)
    params = np.tile(SHAPE_PARAMS, (1, 1))
    rng = np.random.default_rng(7)
    queries = rng.integers(0, 4, size=(Q, P)).astype(np.int8)
    queries[rng.random((Q, P)) < 0.05] = 4
    pend = np.array(PENDANTS[:G])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_pid, d_bl, d_pr = up(pids.astype(np.int32)), up(bls), up(params)
    d_q, d_col, d_w, d_pend = up(queries), up(np.arange(P, dtype=np.int32)), up(np.asarray(w, np.float64)), up(pend)
    edge, lwr = torch.empty((1, Q, E), **f64), torch.empty((1, Q, E), **f64)
    best = torch.empty((1, Q), dtype=torch.int32, device=dev)
    state = torch.empty((1, n - 2, P, 4), **f64)
    eng.reserve_placement(1, Q, P, G)
    eng.reserve_ancestral(1)
    ins = (d_pid.data_ptr(), d_bl.data_ptr(), d_pr.data_ptr())

    def place(count=Q):
        eng.placement_device(side.cuda_stream, 1, *ins, count, P, d_q.data_ptr(), d_col.data_ptr(), d_w.data_ptr(), G,
                             d_pend.data_ptr(), edge.data_ptr(), out_best_edge=best.data_ptr(), out_lwr=lwr.data_ptr())

    def table():
        place(1)

    def call_state():
        eng.ancestral_states_device(side.cuda_stream, 1, *ins, state.data_ptr())

    src = torch.empty(1 << 27, **f64)  # 1 GiB
    dst = torch.empty_like(src)

    def copy():
        with torch.cuda.stream(side):
            dst.copy_(src, non_blocking=True)

    for _ in range(2):
        place()
        table()
        call_state()
        copy()
    torch.cuda.synchronize()
    place()
    torch.cuda.synchronize()
    path = eng.last_call_path()
    eng.check_status()
    legs = dict(place=place, table=table, state=call_state, copy=copy)
    times = {k: [] for k in legs}
    for _ in range(rounds):
        for k, call in legs.items():
            times[k].append(S.timed(side, call, reps))
    med = {k: float(np.median(v)) for k, v in times.items()}
    name = f"{shape} Q={Q} G={G}"
    print(f"{name:24s} [{path}]")
    for k in legs:
        print(f"{name:24s} {k:6s} {med[k]:10.3f} ms  (min {min(times[k]):.3f}, max {max(times[k]):.3f})")
    score = med["place"] - med["table"]
    lookups = Q * E * P * G
    print(f"{name:24s} score  {score:10.3f} ms  (place - table, derived): {lookups:.3g} look-ups, "
          f"{lookups / max(score, 1e-9) / 1e9:.2f} T look-ups/s; table {E * G * 5 * P * 8 / 1e6:.2f} MB; "
          f"table / state = {med['table'] / med['state']:.2f}")
    if host:
        res = eng.placement(pids, bls, queries[:1], pend, params, column_pattern=np.arange(P), column_weights=w,
                            tables=True)
        with tempfile.TemporaryDirectory() as tmp:
            file = os.path.join(tmp, "table.npy")
            np.save(file, res.tables[0])
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--host-leg", file, "--queries", str(Q)],
                                 capture_output=True, text=True, check=True)
        ms = float(out.stdout.strip().splitlines()[-1])
        print(f"{name:24s} host   {ms:10.1f} ms  ({HOST_QUERIES} queries in float64 numpy on 16 processes, scaled; "
              f"the table's download not counted) = {ms / max(score, 1e-9):.0f} x score")
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--queries", type=int, default=10000)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--pendants", default="1,4")
    ap.add_argument("--host", action="store_true", help="also time the host alternative")
    ap.add_argument("--host-leg", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.host_leg:
        host_leg(a.host_leg, a.queries)
        return
    for shape in a.shapes.split(","):
        for G in (int(g) for g in a.pendants.split(",")):
            measure(shape, a.queries, G, a.rounds, a.reps, a.host)


if __name__ == "__main__":
    main()
