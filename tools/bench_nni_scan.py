#!/usr/bin/env python3
"""Cost of the NNI neighbourhood scan next to what it replaces.

Shapes: DS1 (27 taxa x 934 patterns) x 1000 trees and 100 taxa x 500 patterns x 1000 random
trees, JC69 + weibull+4.  Legs, alternating within a round after a warm-up:
  scan    one nni_scan_device call of T trees
  brute   log_likelihoods_device on all 2 (n-3) T neighbour trees, already resident on the device
          (building them with mi_nni_neighbour and uploading them is NOT in the time), in calls
          of at most --brute-chunk trees
  hbm     the gradient call of T trees under MI_PHYLO_GRADIENT_PATH=hbm: the kernel family's
          yardstick
  grad    (DS1 only, with --yardstick) the default gradient call on this build and on another
          build of the library (e.g. the parent commit's), each in a child process of its own
          that runs nothing else
Milliseconds between device events around `--reps` back-to-back calls (one call for `brute`),
median of `--rounds` rounds, with the spread (min, max).  Printed per shape: brute / scan and
scan / hbm.

    python tools/bench_nni_scan.py [--rounds 7] [--reps 10] [--shapes ds1,100x500]
                                   [--trees 1000] [--yardstick other/libmi_phylo.so]"""
import argparse
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import libsbn_amd as L  # noqa: E402

SHAPES = ("ds1", "100x500")


def workload(shape, T):
    if shape == "ds1":
        return bench.ds1_workload(T)
    n, P = (int(x) for x in shape.split("x"))
    rng = np.random.default_rng(47)
    top = np.stack([bench.random_unrooted_topology(n, rng) for _ in range(50)])
    pids = np.ascontiguousarray(np.tile(top, (T // 50 + 1, 1))[:T]).astype(np.int32)
    bls = rng.exponential(0.1, size=(T, 2 * n - 2))
    bls[:, -1] = 0
    return bench.evolved_alignment(pids[0], bls[0], P, rng), np.ones(P), pids, bls


def engine(tips, w, hbm=False):
    old = os.environ.get("MI_PHYLO_GRADIENT_PATH")
    if hbm:
        os.environ["MI_PHYLO_GRADIENT_PATH"] = "hbm"
    try:
        return L.Engine(L.PhyloModelSpecification("JC69", "weibull+4", "strict"), tips, w, device=0)
    finally:
        if hbm and old is None:
            os.environ.pop("MI_PHYLO_GRADIENT_PATH")
        elif hbm:
            os.environ["MI_PHYLO_GRADIENT_PATH"] = old


def timed(stream, call, reps):
    with torch.cuda.stream(stream):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            call()
        b.record()
        b.synchronize()
    return a.elapsed_time(b) / reps


class GradBatch:
    """The gradient call of T trees on one engine (this build's default, its HBM path, or
    another build's default in the child process)."""

    def __init__(self, tips, w, pids, bls, hbm=False):
        T, N = len(pids), 2 * tips.shape[0] - 1
        dev = torch.device("cuda", 0)
        self.T = T
        self.keep = [torch.from_numpy(np.ascontiguousarray(a)).to(dev)
                     for a in (pids.astype(np.int32), bls, np.tile([0.7, 1.0], (T, 1)))]
        f64 = dict(dtype=torch.float64, device=dev)
        self.ll, self.g, self.site = torch.empty(T, **f64), torch.empty((T, N), **f64), torch.empty(T, **f64)
        self.eng = engine(tips, w, hbm)
        self.eng.reserve(T, True)
        self.side = torch.cuda.Stream()

    def call(self):
        self.eng.gradients_device(self.side.cuda_stream, self.T, *(x.data_ptr() for x in self.keep),
                                  self.ll.data_ptr(), self.g.data_ptr(), self.site.data_ptr(), None)


def worker(reps, T):
    """A child process (--yardstick): the default gradient call on DS1 with the library
    MI_PHYLO_LIBRARY names."""
    import ctypes
    from libsbn_amd import _capi
    probe = ctypes.CDLL(_capi.LIB_PATH)
    for name in [k for k in _capi.SYMBOLS if not hasattr(probe, k)]:
        del _capi.SYMBOLS[name]  # (an older build does not export the calls added since)
    b = GradBatch(*workload("ds1", T))
    for _ in range(3):
        b.call()
    torch.cuda.synchronize()
    print("ready", flush=True)
    for line in sys.stdin:
        if line.strip() != "grad":
            break
        print(timed(b.side, b.call, reps), flush=True)


class Yardstick:
    def __init__(self, library, reps, T):
        env = dict(os.environ)
        if library:
            env["MI_PHYLO_LIBRARY"] = os.path.abspath(library)
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--reps", str(reps),
                                   "--trees", str(T)],
                                  stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=env)
        if self.p.stdout.readline().strip() != "ready":
            raise RuntimeError("the yardstick process did not start")

    def grad(self):
        self.p.stdin.write("grad\n")
        self.p.stdin.flush()
        out = self.p.stdout.readline().strip()
        if not out:
            raise RuntimeError("the yardstick process ended")
        return float(out)

    def close(self):
        try:
            self.p.stdin.write("quit\n")
            self.p.stdin.flush()
        except OSError:
            pass
        self.p.wait(timeout=60)


def measure(shape, T, rounds, reps, chunk, yards):
    tips, w, pids, bls = workload(shape, T)
    n = tips.shape[0]
    N = 2 * n - 1
    dev = torch.device("cuda", 0)
    f64 = dict(dtype=torch.float64, device=dev)
    side = torch.cuda.Stream()
    # scan
    scan_eng = engine(tips, w)
    params = np.tile([0.7, 1.0], (T, 1))
    d_pid, d_bl, d_pr = (torch.from_numpy(np.ascontiguousarray(a)).to(dev)
                         for a in (pids.astype(np.int32), bls, params))
    ll, delta = torch.empty(T, **f64), torch.empty((T, N, 2), **f64)
    best = torch.empty(T, dtype=torch.int32, device=dev)
    scan_eng.reserve_nni_scan(T)

    def scan():
        scan_eng.nni_scan_device(side.cuda_stream, T, d_pid.data_ptr(), d_bl.data_ptr(), d_pr.data_ptr(),
                                 delta.data_ptr(), out_ll=ll.data_ptr(), out_best=best.data_ptr())

    # brute force: every neighbour tree, built on the host and uploaded once
    moves = [(v, i) for v in range(n, 2 * n - 3) for i in (0, 1)]
    E = T * len(moves)
    nb_pid, nb_bl = np.empty((E, 2 * n - 3), np.int32), np.empty((E, 2 * n - 2))
    for t in range(T):
        for k, (v, i) in enumerate(moves):
            nb_pid[t * len(moves) + k], nb_bl[t * len(moves) + k] = L.nni_neighbour(n, pids[t], bls[t], v, i)
    b_pid, b_bl = torch.from_numpy(nb_pid).to(dev), torch.from_numpy(nb_bl).to(dev)
    b_pr = torch.from_numpy(np.tile([0.7, 1.0], (E, 1))).to(dev)
    b_ll = torch.empty(E, **f64)
    brute_eng = engine(tips, w)
    chunk = min(chunk, E)
    brute_eng.reserve(chunk, False)

    def brute():
        for lo in range(0, E, chunk):
            c = min(chunk, E - lo)
            brute_eng.log_likelihoods_device(side.cuda_stream, c, b_pid[lo:].data_ptr(), b_bl[lo:].data_ptr(),
                                             b_pr[lo:].data_ptr(), b_ll[lo:].data_ptr())

    hbm = GradBatch(tips, w, pids, bls, hbm=True)
    for _ in range(3):
        scan()
        hbm.call()
    brute()
    torch.cuda.synchronize()
    for e in (scan_eng, brute_eng, hbm.eng):
        e.check_status()
    # (the two ways agree: the scan's delta against the brute-force difference)
    want = (b_ll.cpu().numpy().reshape(T, len(moves)) - ll.cpu().numpy()[:, None])
    got = delta.cpu().numpy()[:, n:2 * n - 3, :].reshape(T, len(moves))
    agree = np.max(np.abs(got - want) / np.abs(ll.cpu().numpy())[:, None])
    times = {k: [] for k in ("scan", "brute", "hbm", "grad", "grad-yardstick")}
    for _ in range(rounds):
        times["scan"].append(timed(side, scan, reps))
        times["brute"].append(timed(side, brute, 1))
        times["hbm"].append(timed(hbm.side, hbm.call, reps))
        if shape == "ds1" and yards:
            times["grad"].append(yards[0].grad())
            times["grad-yardstick"].append(yards[1].grad())
    med = {k: float(np.median(v)) for k, v in times.items() if v}
    name = f"{shape} x {T}"
    print(f"{name:16s} [{scan_eng.last_call_path()}] | brute: {E} trees [{brute_eng.last_call_path()}] | "
          f"hbm: [{hbm.eng.last_call_path()}]")
    print(f"{name:16s} scan delta against brute-force differences: {agree:.2e} of |logL|")
    for k, v in med.items():
        print(f"{name:16s} {k:14s} {v:10.3f} ms  (min {min(times[k]):.3f}, max {max(times[k]):.3f})")
    print(f"{name:16s} brute / scan = {med['brute'] / med['scan']:.2f}   scan / hbm = {med['scan'] / med['hbm']:.2f}")
    if "grad-yardstick" in med:
        print(f"{name:16s} grad here / yardstick = {med['grad'] / med['grad-yardstick']:.3f}")
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--trees", type=int, default=1000)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--brute-chunk", type=int, default=32768, help="trees per brute-force call")
    ap.add_argument("--yardstick", default=None, help="another build of the library for the DS1 gradient leg")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        worker(a.reps, a.trees)
        return
    yards = [Yardstick(None, a.reps, a.trees), Yardstick(a.yardstick, a.reps, a.trees)] if a.yardstick else []
    try:
        for shape in a.shapes.split(","):
            measure(shape, a.trees, a.rounds, a.reps, a.brute_chunk, yards)
    finally:
        for y in yards:
            y.close()


if __name__ == "__main__":
    main()
