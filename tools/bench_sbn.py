#!/usr/bin/env python3
"""Cost of the subsplit-Bayesian-network calls: the support and slots of a batch
(index), the probabilities of all rootings with the expected usages (log_prob: the per-step call
of variational inference and the E-step), and one EM iteration of training.

Batches: one DS1 tree, 1000 DS1 trees (the 100 golden topologies ten times over: most PCSPs
shared) and 1000 uniform random-join trees of 100 taxa (almost nothing shared: the support is as
large as it gets).  Every leg runs in a child process of its own.  Per leg, milliseconds between
device events around ONE call on a stream of its own, median of `--rounds` rounds after a warm-up,
the calls alternating within a round:
  index     sbn_index_device
  log_prob  sbn_log_prob_device  (unnormalised parameters, expected counts included)
  em        sbn_train_device     (the counts and ONE EM iteration; it synchronises)
With --headline the 1000-tree gradient step of bench.py's headline is measured on the same box and
printed beside the 1000-tree DS1 log_prob: the ratio says whether log q hides under the
likelihood.  Nothing is asserted about the times: no other implementation of this work exists in
the library.

    python tools/bench_sbn.py [--rounds 5] [--batches ds1x1,ds1x1000,100x1000] [--headline]"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402


def trees_of(batch):
    import bench
    shape, T = batch.split("x")
    T = int(T)
    if shape == "ds1":
        with open(os.path.join(REPO, "tests", "golden", "ds1_top100.struct.json")) as f:
            tops = np.array([t["parent_ids"] for t in json.load(f)["trees"]], np.int32)
        return tops[np.arange(T) % len(tops)]
    rng = np.random.default_rng(11)
    return np.stack([bench.random_unrooted_topology(int(shape), rng) for _ in range(T)]).astype(np.int32)


def leg(batch, rounds):
    import torch
    import libsbn_amd as L
    pids = trees_of(batch)
    T, E = pids.shape
    n = (E + 3) // 2
    dev = torch.device("cuda", 0)
    tips = np.random.default_rng(5).integers(0, 4, size=(4, 7)).astype(np.int32)
    eng = L.Engine(L.PhyloModelSpecification("JC69", "constant", "strict"), tips, np.ones(7), device=0)
    sup = eng.sbn_index(pids)
    S, C, parents, P = sup.rootsplit_count, sup.pcsp_count, sup.parent_count, sup.parameter_count
    rcap, pcap, W = T * E, T * E * 6, (n + 31) // 32
    i32, f64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float64, device=dev)
    d_pid = torch.from_numpy(np.ascontiguousarray(pids)).to(dev)
    root, slot, counts = torch.empty((T, E), **i32), torch.empty((T, 2 * E, 3), **i32), torch.zeros(3, **i32)
    bits, clades = torch.empty((rcap, W), **i32), torch.empty((pcap, 3), **i32)
    prange, parent = torch.empty((pcap, 2), **i32), torch.empty(pcap, **i32)
    theta = torch.from_numpy(np.random.default_rng(3).normal(0.0, 1.0, P)).to(dev)
    lp, lq, usage = torch.empty((T, E), **f64), torch.empty(T, **f64), torch.empty(P, **f64)
    trained, history, iters = torch.empty(P, **f64), torch.zeros(1, **f64), torch.zeros(1, **i32)
    side = torch.cuda.Stream()
    s = side.cuda_stream
    calls = {
        "index": lambda: eng.sbn_index_device(s, T, n, d_pid.data_ptr(), T, rcap, pcap, root.data_ptr(),
                                              slot.data_ptr(), counts.data_ptr(), bits.data_ptr(),
                                              clades.data_ptr(), prange.data_ptr(), parent.data_ptr()),
        "log_prob": lambda: eng.sbn_log_prob_device(s, T, n, d_pid.data_ptr(), root.data_ptr(), slot.data_ptr(), S, C,
                                                    parents, prange.data_ptr(), theta.data_ptr(), False,
                                                    lp.data_ptr(), lq.data_ptr(), usage.data_ptr()),
        "em": lambda: eng.sbn_train_device(s, T, n, d_pid.data_ptr(), root.data_ptr(), slot.data_ptr(), S, C, parents,
                                           prange.data_ptr(), "em", 0.0, 1, 0.0, trained.data_ptr(),
                                           history.data_ptr(), iters.data_ptr()),
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
    tag = f"{batch} ({n} taxa, T={T})"
    print(f"{tag:28s} [{path}] S = {S}, C = {C} in {parents} blocks; {T * E * 7} entries")
    for k, v in times.items():
        print(f"{tag:28s} {k:9s} {np.median(v):9.3f} ms  (min {min(v):.3f}, max {max(v):.3f})")
    print("BENCH_SBN", json.dumps({"batch": batch, **{k: float(np.median(v)) for k, v in times.items()}}))
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
    log_prob_ms = None
    for batch in a.batches.split(","):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--rounds", str(a.rounds), "--leg", batch],
                             check=True, capture_output=True, text=True).stdout
        for line in out.splitlines():
            if line.startswith("BENCH_SBN"):
                if batch == "ds1x1000":
                    log_prob_ms = json.loads(line.split(" ", 1)[1])["log_prob"]
            else:
                print(line, flush=True)
    if a.headline:
        out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "10", "--warmup",
                              "3", "--headline-only"], check=True, capture_output=True, text=True).stdout
        result = json.loads([line for line in out.splitlines() if line.startswith("{")][-1])
        step = result.get("ms_per_step")
        print(f"gradient step, 1000 DS1 trees (bench.py headline): {step} ms" +
              (f"; log_prob / step = {log_prob_ms / step:.3f}" if log_prob_ms and step else ""))


if __name__ == "__main__":
    main()
