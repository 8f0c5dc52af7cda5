#!/usr/bin/env python3
"""Cost of the SBN side of one variational step, by tools/bench_sbn.py's method:
the descent table of a support (once per support), K topologies drawn from it (the CDF included),
the index of support + samples, log_prob of the samples and the topology gradient (VIMCO).

Batches `<support>x<K>`: K samples from the support of the 100 golden DS1 topologies (ds1x1,
ds1x1000) and from the support of 1000 uniform random-join trees of 100 taxa (100x1000: almost
nothing shared, the support is as large as it gets).  Every batch runs in a child process of its
own.  Per leg, milliseconds between device events around ONE call on a stream of its own, median of
`--rounds` rounds after a warm-up, the calls in the order of a step within a round:
  descent            sbn_descent_device
  sample             sbn_sample_device            (parameter check, CDF kernel and draws)
  index              sbn_index_device             (support trees + samples, support_tree_count = T0)
  log_prob           sbn_log_prob_device          (the samples; no expected counts)
  topology_gradient  sbn_topology_gradient_device (VIMCO; its own walk included)
With --headline the 1000-tree gradient step of bench.py's headline is measured on the same box and
printed beside the sum of the four per-step legs of ds1x1000.  Nothing is asserted about the times:
no other implementation of this work exists in the library.

    python tools/bench_sbn_vi.py [--rounds 5] [--batches ds1x1,ds1x1000,100x1000] [--headline]"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402


def support_trees(shape):
    import bench
    if shape == "ds1":
        with open(os.path.join(REPO, "tests", "golden", "ds1_top100.struct.json")) as f:
            return np.array([t["parent_ids"] for t in json.load(f)["trees"]], np.int32)
    rng = np.random.default_rng(11)
    return np.stack([bench.random_unrooted_topology(int(shape), rng) for _ in range(1000)]).astype(np.int32)


def leg(batch, rounds):
    import torch
    import libsbn_amd as L
    shape, K = batch.split("x")
    K = int(K)
    pids = support_trees(shape)
    T0, E = pids.shape
    n, T = (E + 3) // 2, T0 + K
    dev = torch.device("cuda", 0)
    tips = np.random.default_rng(5).integers(0, 4, size=(4, 7)).astype(np.int32)
    eng = L.Engine(L.PhyloModelSpecification("JC69", "constant", "strict"), tips, np.ones(7), device=0)
    sup = eng.sbn_index(pids)
    S, C, parents, P = sup.rootsplit_count, sup.pcsp_count, sup.parent_count, sup.parameter_count
    W = (n + 31) // 32
    i32, f64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float64, device=dev)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    s_pid, s_root, s_slot, s_parent, s_range = (up(x) for x in (
        sup.parent_ids, sup.root_index, sup.slot_index, sup.pcsp_parent, sup.parent_range))
    theta = up(eng.sbn_train(sup, "sa")[0])
    log_f = up(np.random.default_rng(3).normal(-7000.0, 3.0, K))
    desc = torch.empty((P, 2), **i32)
    all_pid = torch.empty((T, E), **i32)
    all_pid[:T0] = s_pid
    edge, params, lp = torch.empty(K, **i32), torch.empty((K, n - 1), **i32), torch.empty(K, **f64)
    root, slot, counts = torch.empty((T, E), **i32), torch.empty((T, 2 * E, 3), **i32), torch.zeros(3, **i32)
    bits, clades = torch.empty((S, W), **i32), torch.empty((C, 3), **i32)
    prange, parent = torch.empty((C, 2), **i32), torch.empty(C, **i32)
    rooting, lq = torch.empty((K, E), **f64), torch.empty(K, **f64)
    grad, factors, glq = torch.empty(P, **f64), torch.empty(K, **f64), torch.empty(K, **f64)
    side = torch.cuda.Stream()
    s = side.cuda_stream
    mine = all_pid[T0:]
    calls = {
        "descent": lambda: eng.sbn_descent_device(s, T0, n, s_pid.data_ptr(), s_root.data_ptr(), s_slot.data_ptr(),
                                                  S, C, s_parent.data_ptr(), desc.data_ptr()),
        "sample": lambda: eng.sbn_sample_device(s, K, n, S, C, parents, s_range.data_ptr(), desc.data_ptr(),
                                                theta.data_ptr(), 20261020, 0, mine.data_ptr(), edge.data_ptr(),
                                                params.data_ptr(), lp.data_ptr()),
        "index": lambda: eng.sbn_index_device(s, T, n, all_pid.data_ptr(), T0, S, C, root.data_ptr(), slot.data_ptr(),
                                              counts.data_ptr(), bits.data_ptr(), clades.data_ptr(),
                                              prange.data_ptr(), parent.data_ptr()),
        "log_prob": lambda: eng.sbn_log_prob_device(s, K, n, mine.data_ptr(), root[T0:].data_ptr(),
                                                    slot[T0:].data_ptr(), S, C, parents, s_range.data_ptr(),
                                                    theta.data_ptr(), True, rooting.data_ptr(), lq.data_ptr()),
        "topology_gradient": lambda: eng.sbn_topology_gradient_device(
            s, K, n, mine.data_ptr(), root[T0:].data_ptr(), slot[T0:].data_ptr(), S, C, parents, s_range.data_ptr(),
            theta.data_ptr(), True, log_f.data_ptr(), "vimco" if K > 1 else "plain", grad.data_ptr(),
            factors.data_ptr(), glq.data_ptr()),
    }
    eng.reserve_sbn(T, n)
    path = ""
    for _ in range(2):
        for name, call in calls.items():
            call()
            path = eng.last_call_path()
    torch.cuda.synchronize()
    eng.check_status()
    assert counts.cpu().tolist() == [S, C, parents]
    assert bool(torch.all(root[T0:] < S)) and bool(torch.all(torch.isfinite(grad)))
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
    print(f"{tag:34s} [{path}] S = {S}, C = {C} in {parents} blocks")
    for k, v in times.items():
        print(f"{tag:34s} {k:18s} {np.median(v):9.3f} ms  (min {min(v):.3f}, max {max(v):.3f})")
    print("BENCH_SBN_VI", json.dumps({"batch": batch, **{k: float(np.median(v)) for k, v in times.items()}}))
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
            if line.startswith("BENCH_SBN_VI"):
                if batch == "ds1x1000":
                    r = json.loads(line.split(" ", 1)[1])
                    step_ms = r["sample"] + r["index"] + r["log_prob"] + r["topology_gradient"]
            else:
                print(line, flush=True)
    if a.headline:
        out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "10", "--warmup",
                              "3", "--headline-only"], check=True, capture_output=True, text=True).stdout
        result = json.loads([line for line in out.splitlines() if line.startswith("{")][-1])
        step = result.get("ms_per_step")
        print(f"gradient step, 1000 DS1 trees (bench.py headline): {step} ms" +
              (f"; SBN side of a step (sample + index + log_prob + topology_gradient) {step_ms:.3f} ms, "
               f"ratio {step_ms / step:.3f}" if step_ms and step else ""))


if __name__ == "__main__":
    main()
