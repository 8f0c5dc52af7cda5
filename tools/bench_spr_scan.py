#!/usr/bin/env python3
"""Cost of the SPR neighbourhood scan next to what it replaces.

Shapes: DS1 (27 taxa x 934 patterns) and 100 taxa x 500 patterns, JC69 + weibull+4, T trees each
(T small enough that the scan's workspace fits one launch).  Legs, each in a child process of its
own that runs nothing else, alternating within a round after a warm-up:
  scan0   one spr_scan_device call of T trees, radius 0 (every move), whole table written
  scan3   the same at radius 3
  brute   log_likelihoods_device on every neighbour tree of radius 0, already resident on the
          device (building them with mi_spr_neighbour and uploading them is NOT in the time), in
          calls of at most --brute-chunk trees
  hbm     the gradient call of T trees under MI_PHYLO_GRADIENT_PATH=hbm: the kernel family's
          yardstick
Milliseconds between device events around `--reps` back-to-back calls (one pass for `brute`),
median of `--rounds` rounds with minimum and maximum.  Printed per shape: brute / scan0,
scan0 / hbm, scan3 / hbm, and the agreement of the scan's delta with the brute-force differences.

    python tools/bench_spr_scan.py [--rounds 5] [--reps 5] [--shapes ds1:16,100x500:2]"""
import argparse
import os
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

LEGS = ("scan0", "scan3", "brute", "hbm")


def workload(shape, T):
    import bench
    if shape == "ds1":
        tips, w, pids, bls = bench.ds1_workload(T)
        return tips, w, pids[:T], bls[:T]
    n, P = (int(x) for x in shape.split("x"))
    rng = np.random.default_rng(47)
    pids = np.stack([bench.random_unrooted_topology(n, rng) for _ in range(T)]).astype(np.int32)
    bls = rng.exponential(0.1, size=(T, 2 * n - 2))
    bls[:, -1] = 0
    return bench.evolved_alignment(pids[0], bls[0], P, rng), np.ones(P), pids, bls


def all_moves(n, pid):
    """Every (s, dir, f) of one tree, from the definition (include/mi_phylo.h)."""
    root = 2 * n - 3
    par = [int(p) for p in pid] + [-1]
    kids = {v: [] for v in range(n, root + 1)}
    for v in range(root):
        kids[par[v]].append(v)

    def clade(s):
        out, stack = [], [s]
        while stack:
            v = stack.pop()
            out.append(v)
            stack.extend(kids.get(v, ()))
        return set(out)

    out = []
    for s in range(root):
        inside = clade(s)
        u = par[s]
        merged = {x for x in kids[u] if x != s} | ({u} if u != root else set())
        out += [(s, 0, f) for f in range(root) if f not in inside and f not in merged]
        if s >= n:
            out += [(s, 1, f) for f in sorted(inside - {s} - set(kids[s]))]
    return out


def worker(leg, shape, T, reps, chunk, scratch):
    import torch

    import libsbn_amd as L
    tips, w, pids, bls = workload(shape, T)
    n = tips.shape[0]
    E = 2 * n - 3
    if leg == "hbm":
        os.environ["MI_PHYLO_GRADIENT_PATH"] = "hbm"
    eng = L.Engine(L.PhyloModelSpecification("JC69", "weibull+4", "strict"), tips, w, device=0)
    dev = torch.device("cuda", 0)
    f64 = dict(dtype=torch.float64, device=dev)
    side = torch.cuda.Stream()

    def on_device(*arrays):
        return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]

    d_pid, d_bl, d_pr = on_device(pids.astype(np.int32), bls, np.tile([0.7, 1.0], (T, 1)))
    passes = reps
    if leg in ("scan0", "scan3"):
        ll, best = torch.empty(T, **f64), torch.empty((T, E, 2), **f64)
        target = torch.empty((T, E, 2), dtype=torch.int32, device=dev)
        move = torch.empty((T, 3), dtype=torch.int32, device=dev)
        delta = torch.empty((T, E, 2, E), **f64)
        eng.reserve_spr_scan(T)

        def call():
            eng.spr_scan_device(side.cuda_stream, T, d_pid.data_ptr(), d_bl.data_ptr(), d_pr.data_ptr(),
                                target.data_ptr(), best.data_ptr(), out_ll=ll.data_ptr(),
                                out_best_move=move.data_ptr(), out_delta=delta.data_ptr(),
                                radius=0 if leg == "scan0" else 3)
    elif leg == "brute":
        moves = [all_moves(n, pids[t]) for t in range(T)]
        total = sum(len(m) for m in moves)
        nb_pid, nb_bl = np.empty((total, 2 * n - 3), np.int32), np.empty((total, 2 * n - 2))
        i = 0
        for t in range(T):
            for s, d, f in moves[t]:
                nb_pid[i], nb_bl[i] = L.spr_neighbour(n, pids[t], bls[t], s, d, f)
                i += 1
        b_pid, b_bl, b_pr = on_device(nb_pid, nb_bl, np.tile([0.7, 1.0], (total, 1)))
        b_ll = torch.empty(total, **f64)
        own = torch.empty(T, **f64)
        chunk = min(chunk, total)
        eng.reserve(max(chunk, T), False)
        passes = 1

        def call():
            for lo in range(0, total, chunk):
                c = min(chunk, total - lo)
                eng.log_likelihoods_device(side.cuda_stream, c, b_pid[lo:].data_ptr(), b_bl[lo:].data_ptr(),
                                           b_pr[lo:].data_ptr(), b_ll[lo:].data_ptr())
    else:
        N = 2 * n - 1
        ll, g, site = torch.empty(T, **f64), torch.empty((T, N), **f64), torch.empty(T, **f64)
        eng.reserve(T, True)

        def call():
            eng.gradients_device(side.cuda_stream, T, d_pid.data_ptr(), d_bl.data_ptr(), d_pr.data_ptr(),
                                 ll.data_ptr(), g.data_ptr(), site.data_ptr(), None)

    for _ in range(2):
        with torch.cuda.stream(side):
            call()
    torch.cuda.synchronize()
    eng.check_status()
    # what the parent compares: the scan's table, the brute-force differences in the same layout
    if leg == "scan0":
        np.save(os.path.join(scratch, f"{shape}_scan.npy"), delta.cpu().numpy())
    if leg == "brute":
        with torch.cuda.stream(side):
            eng.log_likelihoods_device(side.cuda_stream, T, d_pid.data_ptr(), d_bl.data_ptr(), d_pr.data_ptr(),
                                       own.data_ptr())
        torch.cuda.synchronize()
        tab = np.full((T, E, 2, E), -np.inf)
        got, base, i = b_ll.cpu().numpy(), own.cpu().numpy(), 0
        for t in range(T):
            for s, d, f in moves[t]:
                tab[t, s, d, f] = got[i] - base[t]
                i += 1
        np.save(os.path.join(scratch, f"{shape}_brute.npy"), tab)
        np.save(os.path.join(scratch, f"{shape}_ll.npy"), base)
    print(f"ready {eng.last_call_path()}", flush=True)
    for line in sys.stdin:
        if line.strip() != "run":
            break
        with torch.cuda.stream(side):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(passes):
                call()
            b.record()
            b.synchronize()
        print(a.elapsed_time(b) / passes, flush=True)


class Leg:
    def __init__(self, leg, shape, T, a, scratch):
        self.p = subprocess.Popen(
            [sys.executable, os.path.abspath(__file__), "--worker", leg, "--shapes", f"{shape}:{T}", "--reps",
             str(a.reps), "--brute-chunk", str(a.brute_chunk), "--scratch", scratch],
            stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        first = self.p.stdout.readline().strip()
        if not first.startswith("ready"):
            raise RuntimeError(f"the {leg} process did not start")
        self.path = first[6:]

    def run(self):
        self.p.stdin.write("run\n")
        self.p.stdin.flush()
        out = self.p.stdout.readline().strip()
        if not out:
            raise RuntimeError("a leg's process ended")
        return float(out)

    def close(self):
        try:
            self.p.stdin.write("quit\n")
            self.p.stdin.flush()
        except OSError:
            pass
        self.p.wait(timeout=60)


def measure(shape, T, a, scratch):
    legs = {}
    try:
        for k in LEGS:
            legs[k] = Leg(k, shape, T, a, scratch)
        times = {k: [] for k in LEGS}
        for _ in range(a.rounds):
            for k in LEGS:
                times[k].append(legs[k].run())
    finally:
        for leg in legs.values():
            leg.close()
    scan, brute = np.load(os.path.join(scratch, f"{shape}_scan.npy")), np.load(os.path.join(scratch, f"{shape}_brute.npy"))
    ll = np.load(os.path.join(scratch, f"{shape}_ll.npy"))
    there = ~np.isneginf(brute)
    assert np.array_equal(there, ~np.isneginf(scan)), "the scan and the enumeration disagree on what a move is"
    scale = np.broadcast_to(np.abs(ll)[:, None, None, None], scan.shape)
    agree = float(np.max(np.abs(scan[there] - brute[there]) / scale[there]))
    name = f"{shape} x {T}"
    med = {k: float(np.median(v)) for k, v in times.items()}
    print(f"{name:14s} {int(there.sum())} moves | scan [{legs['scan0'].path}] | brute [{legs['brute'].path}] | "
          f"hbm [{legs['hbm'].path}]")
    print(f"{name:14s} scan delta against brute-force differences: {agree:.2e} of |logL|")
    for k in LEGS:
        print(f"{name:14s} {k:6s} {med[k]:10.3f} ms  (min {min(times[k]):.3f}, max {max(times[k]):.3f})")
    print(f"{name:14s} brute / scan0 = {med['brute'] / med['scan0']:.2f}   scan0 / hbm = {med['scan0'] / med['hbm']:.1f}   "
          f"scan3 / hbm = {med['scan3'] / med['hbm']:.1f}")
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="ds1:16,100x500:2", help="shape:trees, comma-separated")
    ap.add_argument("--brute-chunk", type=int, default=32768, help="trees per brute-force call")
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--scratch", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    shapes = [(s.split(":")[0], int(s.split(":")[1])) for s in a.shapes.split(",")]
    if a.worker:
        worker(a.worker, shapes[0][0], shapes[0][1], a.reps, a.brute_chunk, a.scratch)
        return
    with tempfile.TemporaryDirectory() as scratch:
        for shape, T in shapes:
            measure(shape, T, a, scratch)


if __name__ == "__main__":
    main()
