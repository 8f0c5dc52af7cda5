#!/usr/bin/env python3
"""Cost of the branch-length side of one variational step, by
tools/bench_sbn_vi.py's method: the PSP rows of K sampled trees, one draw of their branch lengths
with log q and the prior, and the gradient with respect to the (mu, sigma) tables with log_f.

Batches `<support>x<K>`: K samples from the support of the 100 golden DS1 topologies (ds1x1,
ds1x1000) and from the support of 1000 uniform random-join trees of 100 taxa (100x1000).  Every
batch runs in a child process of its own.  Per leg, milliseconds between device events around ONE
call on a stream of its own, median of `--rounds` rounds after a warm-up, the calls in the order of
a step within a round:
  psp_index              psp_index_device              (rows = 3, the samples behind the support)
  branch_model_sample    branch_model_sample_device
  branch_model_gradient  branch_model_gradient_device  (terms, keys, radix sort, runs)
The branch gradients and log-likelihoods the gradient call reads are made up: the likelihood call
is bench.py's to measure.  With --headline the 1000-tree gradient step of bench.py's headline is
measured on the same box and printed beside the sum of the three legs of ds1x1000.  Nothing is
asserted about the times: no other implementation of this work exists in the library.

    python tools/bench_branch_model.py [--rounds 5] [--batches ds1x1,ds1x1000,100x1000] [--headline]"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import numpy as np  # noqa: E402

from bench_sbn_vi import support_trees  # noqa: E402


def leg(batch, rounds):
    import torch
    import libsbn_amd as L
    shape, K = batch.split("x")
    K = int(K)
    pids = support_trees(shape)
    T0, E = pids.shape
    n = (E + 3) // 2
    dev = torch.device("cuda", 0)
    tips = np.random.default_rng(5).integers(0, 4, size=(4, 7)).astype(np.int32)
    eng = L.Engine(L.PhyloModelSpecification("JC69", "constant", "strict"), tips, np.ones(7), device=0)
    sup = eng.sbn_index(pids)
    S, C = sup.rootsplit_count, sup.pcsp_count
    table = eng.psp_table(sup)
    V = table.variable_count
    drawn = eng.sbn_sample(sup, eng.sbn_descent(sup), eng.sbn_train(sup, "sa")[0], K, 20261021)[0]
    both = eng.sbn_index(np.concatenate([pids, drawn]), support_tree_count=T0)
    i32, f64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float64, device=dev)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    root, slot, psp = up(both.root_index[T0:]), up(both.slot_index[T0:]), up(table.psp_of_pcsp)
    q = np.zeros((V, 2))
    q[:S] = (-2.0, 0.5)
    rng = np.random.default_rng(3)
    q, g, ll = up(q), up(rng.normal(0.0, 20.0, (K, E + 2))), up(rng.normal(-7000.0, 3.0, K))
    index = torch.empty((K, 3, E), **i32)
    bl, eps, lq, lp = torch.empty((K, E + 1), **f64), torch.empty((K, E), **f64), torch.empty(K, **f64), torch.empty(K, **f64)
    grad, log_f = torch.empty((V, 2), **f64), torch.empty(K, **f64)
    side = torch.cuda.Stream()
    s = side.cuda_stream
    calls = {
        "psp_index": lambda: eng.psp_index_device(s, K, n, root.data_ptr(), slot.data_ptr(), S, C, psp.data_ptr(), V, 3,
                                                  index.data_ptr()),
        "branch_model_sample": lambda: eng.branch_model_sample_device(
            s, K, n, 3, index.data_ptr(), V, q.data_ptr(), 20261021, 0, 10.0, bl.data_ptr(), eps.data_ptr(),
            lq.data_ptr(), lp.data_ptr()),
        "branch_model_gradient": lambda: eng.branch_model_gradient_device(
            s, K, n, 3, index.data_ptr(), V, q.data_ptr(), bl.data_ptr(), eps.data_ptr(), lq.data_ptr(), lp.data_ptr(),
            g.data_ptr(), ll.data_ptr(), 1.0, 10.0, grad.data_ptr(), log_f.data_ptr()),
    }
    eng.reserve_branch_model(K, n, 3)
    path = ""
    for _ in range(2):
        for name, call in calls.items():
            call()
            path = eng.last_call_path()
    torch.cuda.synchronize()
    eng.check_status()
    assert bool(torch.all(index[:, 0] < S)) and bool(torch.all(torch.isfinite(grad))) and bool(torch.all(torch.isfinite(log_f)))
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
    tag = f"{batch} ({n} taxa, T0={T0}, K={K})"
    print(f"{tag:34s} [{path}] S = {S}, V = {V}, entries = {K * 3 * E}")
    for k, v in times.items():
        print(f"{tag:34s} {k:22s} {np.median(v):9.3f} ms  (min {min(v):.3f}, max {max(v):.3f})")
    print("BENCH_BRANCH_MODEL", json.dumps({"batch": batch, **{k: float(np.median(v)) for k, v in times.items()}}))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", default="ds1x1,ds1x1000,100x1000")
    ap.add_argument("--headline", action="store_true")
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        leg(a.leg, a.rounds)
        return
    step_ms = None
    for batch in a.batches.split(","):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--rounds", str(a.rounds), "--leg", batch],
                             check=True, capture_output=True, text=True).stdout
        for line in out.splitlines():
            if line.startswith("BENCH_BRANCH_MODEL"):
                if batch == "ds1x1000":
                    r = json.loads(line.split(" ", 1)[1])
                    step_ms = r["psp_index"] + r["branch_model_sample"] + r["branch_model_gradient"]
            else:
                print(line, flush=True)
    if a.headline:
        out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "10", "--warmup",
                              "3", "--headline-only"], check=True, capture_output=True, text=True).stdout
        result = json.loads([line for line in out.splitlines() if line.startswith("{")][-1])
        step = result.get("ms_per_step")
        print(f"gradient step, 1000 DS1 trees (bench.py headline): {step} ms" +
              (f"; branch-length side of a step (psp_index + branch_model_sample + branch_model_gradient) "
               f"{step_ms:.3f} ms, ratio {step_ms / step:.3f}" if step_ms and step else ""))


if __name__ == "__main__":
    main()
