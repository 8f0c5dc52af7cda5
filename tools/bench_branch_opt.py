#!/usr/bin/env python3
"""Cost of the branch-length optimisation call next to the Hessian passes it
is made of.

Batches of 1000 and 125 trees on DS1 and on 36 taxa x 1812 patterns (JC69 + weibull+4), every
branch started at 0.1.  Per batch:
  opt       one optimize_branch_lengths_device call, active-set packing on (the default)
  opt-off   the same with pack_active = 0: every pass runs on all T trees
  hess      one standalone branch_hessian_device call of T trees -- the yardstick
  grad      (DS1 x 1000 only) the default gradient call
Milliseconds between device events around a call (for `hess` and `grad` around `--reps`
back-to-back calls), median of `--rounds` rounds; the legs alternate within a round, after a
warm-up.  `hess` and `grad` run in a child process, which loads the library `--yardstick` names
through MI_PHYLO_LIBRARY (another build, e.g. the parent commit's; default: this build), and
`grad` is also measured here on this build.  Printed per batch: evaluations per tree (median,
max), the Hessian launches and the trees in each, and
  opt-off / (passes x hess)   the cost of the loop itself: step kernel, check points
  opt / opt-off               what packing saves

    python tools/bench_branch_opt.py [--rounds 7] [--reps 10] [--yardstick other/libmi_phylo.so]
                                     [--max-iterations 100] [--shapes ds1,36x1812]"""
import argparse
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import bench_hessian  # noqa: E402
import libsbn_amd as L  # noqa: E402

SHAPES = ("ds1", "36x1812")


def workload(shape, T):
    if shape == "ds1":
        tips, w, pids, _ = bench.ds1_workload(T)
    else:
        tips, w, pids, _ = bench_hessian.ds3_shape(T)
    start = np.full((T, 2 * tips.shape[0] - 2), 0.1)
    start[:, -1] = 0.0
    return tips, w, pids, start


class Batch:
    """Device copies of one batch and the timed calls on it."""

    def __init__(self, shape, T):
        tips, w, pids, start = workload(shape, T)
        self.T, n = T, tips.shape[0]
        N = 2 * n - 1
        dev = torch.device("cuda", 0)
        params = np.tile([0.7, 1.0], (T, 1))
        self.d_pid, self.d_bl, self.d_pr = (torch.from_numpy(np.ascontiguousarray(a)).to(dev)
                                            for a in (pids.astype(np.int32), start, params))
        f64 = dict(dtype=torch.float64, device=dev)
        self.o_bl, self.ll = torch.empty((T, N - 1), **f64), torch.empty(T, **f64)
        self.g, self.h, self.s = (torch.empty((T, N), **f64) for _ in range(3))
        self.site = torch.empty(T, **f64)
        self.iters = torch.empty(T, dtype=torch.int32, device=dev)
        self.status = torch.empty(T, dtype=torch.int32, device=dev)
        self.eng = L.Engine(L.PhyloModelSpecification("JC69", "weibull+4", "strict"), tips, w, device=0)
        self.side = torch.cuda.Stream()
        self.args = (self.d_pid.data_ptr(), self.d_bl.data_ptr(), self.d_pr.data_ptr())

    max_iterations = 100

    def opt(self, pack):
        self.eng.optimize_branch_lengths_device(
            self.side.cuda_stream, self.T, *self.args, self.o_bl.data_ptr(), self.ll.data_ptr(),
            self.status.data_ptr(), out_branch=self.g.data_ptr(), out_hess=self.h.data_ptr(),
            out_iterations=self.iters.data_ptr(), pack_active=pack, max_iterations=self.max_iterations)

    def hess(self):
        self.eng.branch_hessian_device(self.side.cuda_stream, self.T, *self.args, self.h.data_ptr(),
                                       self.ll.data_ptr(), self.g.data_ptr(), self.s.data_ptr())

    def grad(self):
        self.eng.gradients_device(self.side.cuda_stream, self.T, *self.args, self.ll.data_ptr(),
                                  self.g.data_ptr(), self.site.data_ptr(), None)

    def timed(self, call, reps=1):
        with torch.cuda.stream(self.side):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                call()
            b.record()
            b.synchronize()
        return a.elapsed_time(b) / reps


def worker(reps):
    """The child process: builds the batches it is told to, times `hess` / `grad` on request.
    Lines in: "batch <shape> <T>", "hess", "grad", "quit"; a line out per request."""
    # (an older build does not export the calls added since: bind what it has)
    import ctypes
    from libsbn_amd import _capi
    import torch  # noqa: F401  (before the library, as _capi.load does)
    probe = ctypes.CDLL(_capi.LIB_PATH)
    for name in [k for k in _capi.SYMBOLS if not hasattr(probe, k)]:
        del _capi.SYMBOLS[name]
    batch = None
    for line in sys.stdin:
        cmd = line.split()
        if not cmd or cmd[0] == "quit":
            break
        if cmd[0] == "batch":
            batch = Batch(cmd[1], int(cmd[2]))
            batch.eng.reserve(batch.T, True)
            batch.eng.reserve_hessian(batch.T)
            for _ in range(3):
                batch.hess()
                batch.grad()
            torch.cuda.synchronize()
            print("ready", flush=True)
        else:
            call = batch.hess if cmd[0] == "hess" else batch.grad
            print(batch.timed(call, reps), flush=True)


class Yardstick:
    def __init__(self, library, reps):
        env = dict(os.environ)
        if library:
            env["MI_PHYLO_LIBRARY"] = os.path.abspath(library)
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--reps", str(reps)],
                                  stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=env)

    def ask(self, line):
        self.p.stdin.write(line + "\n")
        self.p.stdin.flush()
        out = self.p.stdout.readline().strip()
        if not out:
            raise RuntimeError("the yardstick process ended")
        return out

    def close(self):
        try:
            self.p.stdin.write("quit\n")
            self.p.stdin.flush()
        except OSError:
            pass
        self.p.wait(timeout=60)


def measure(shape, T, yard, rounds, reps, with_grad):
    b = Batch(shape, T)
    b.eng.reserve_branch_opt(T)
    b.eng.reserve(T, True)
    yard.ask(f"batch {shape} {T}")
    info = {}
    for pack in (True, False):
        b.opt(pack)
        torch.cuda.synchronize()
        b.eng.check_status()
        info[pack] = (b.eng.last_call_path(), b.eng.last_call_info()[1], b.iters.cpu().numpy().copy(),
                      b.status.cpu().numpy().copy())
    for _ in range(3):
        b.grad()
    torch.cuda.synchronize()
    times = {k: [] for k in ("opt", "opt-off", "hess", "grad", "grad-here")}
    for _ in range(rounds):
        times["opt"].append(b.timed(lambda: b.opt(True)))
        times["opt-off"].append(b.timed(lambda: b.opt(False)))
        times["hess"].append(float(yard.ask("hess")))
        if with_grad:
            times["grad-here"].append(b.timed(b.grad, reps))
            times["grad"].append(float(yard.ask("grad")))
    med = {k: float(np.median(v)) for k, v in times.items() if v}
    name = f"{shape} x {T}"
    path, evals, iters, status = info[True]
    path_off, evals_off, iters_off, _ = info[False]
    passes = int(path.split(" opt iters=")[1].split()[0])
    passes_off = int(path_off.split(" opt iters=")[1].split()[0])
    print(f"{name:16s} [{path}]")
    print(f"{name:16s} status: {np.bincount(status, minlength=3).tolist()} (converged, limit, stalled); "
          f"evaluations per tree: median {int(np.median(iters))}, max {int(iters.max())}; "
          f"tree evaluations {evals} packed, {evals_off} unpacked; passes {passes} / {passes_off}")
    for k, v in med.items():
        print(f"{name:16s} {k:9s} {v:9.3f} ms  (min {min(times[k]):.3f}, max {max(times[k]):.3f})")
    print(f"{name:16s} opt-off / (passes x hess) = {med['opt-off'] / (passes_off * med['hess']):.3f}   "
          f"opt / opt-off = {med['opt'] / med['opt-off']:.3f}")
    if with_grad:
        print(f"{name:16s} grad here / yardstick = {med['grad-here'] / med['grad']:.3f}")
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--max-iterations", type=int, default=100)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--yardstick", default=None, help="library the hess / grad yardstick loads")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        worker(a.reps)
        return
    Batch.max_iterations = a.max_iterations
    yard = Yardstick(a.yardstick, a.reps)
    try:
        for shape in a.shapes.split(","):
            for T in (1000, 125):
                measure(shape, T, yard, a.rounds, a.reps, shape == "ds1" and T == 1000)
    finally:
        yard.close()


if __name__ == "__main__":
    main()
