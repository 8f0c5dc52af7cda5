#!/usr/bin/env python3
"""Cost of the tree side of generalized pruning for 1000 trees, on the two DAGs of
tools/bench_gp.py:
  ds1      the 100 golden DS1 topologies, each rooted on the edge above taxon 0 (27 taxa)
  36x1812  36 taxa, 40 topologies a few NNI moves away from one random tree
Every leg runs in a child process of its own.  Per leg, milliseconds between device events around
ONE enqueued call sequence on a stream of its own, the median of `--rounds` rounds after a warm-up,
with the minimum and the maximum:
  index      tree_index_device + tree_log_prob_device of 1000 sampled trees
  sample     sample_trees_device (the CDF and 1000 draws, with the GP lengths)
  enumerate  enumerate_trees_device of the DAG's first 1000 trees (with the GP lengths)
--store global measures the same legs with every tree's node words in the reservation's workspace
instead of LDS (MI_PHYLO_GP_TREES_STORE, set for the child processes): the A/B behind the lane map.
Nothing is asserted about the times: no other implementation of this work exists in the library.

    python tools/bench_gp_trees.py [--rounds 5] [--trees 1000] [--store lds|global]"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np  # noqa: E402

LEGS = ("index", "sample", "enumerate")


def trees_of(name):
    import gp_ref as R
    if name == "ds1":
        with open(os.path.join(REPO, "tests", "golden", "ds1_top100.struct.json")) as f:
            return np.stack([R.root_above_leaf0(t["parent_ids"]) for t in json.load(f)["trees"]])
    return R.nni_batch(36, 40, 3, np.random.default_rng(36))


def leg(name, which, rounds, K):
    import torch
    import libsbn_amd as L
    pids = trees_of(name)
    n = pids.shape[1] // 2 + 1
    tips = np.random.default_rng(5).integers(0, 4, size=(n, 7)).astype(np.int32)
    eng = L.Engine(L.PhyloModelSpecification("JC69", "constant", "strict"), tips, np.ones(7), device=0)
    gp = eng.gp_create_dag(pids)
    total = gp.topology_count()
    count = int(min(K, total))
    gp.reserve_trees(K)
    dev = torch.device("cuda", 0)
    i32, f64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float64, device=dev)
    par, ent, nodes = torch.empty((K, 2 * n - 2), **i32), torch.empty((K, 2 * n - 1), **i32), torch.empty((K, 2 * n - 1), **i32)
    log_q, lengths = torch.empty(K, **f64), torch.empty((K, 2 * n - 1), **f64)
    side = torch.cuda.Stream()
    s = side.cuda_stream
    gp.sample_trees_device(s, K, 7, 0, par.data_ptr(), ent.data_ptr(), log_q.data_ptr(), lengths.data_ptr())

    def index():
        gp.tree_index_device(s, K, par.data_ptr(), ent.data_ptr(), nodes.data_ptr())
        gp.tree_log_prob_device(s, K, ent.data_ptr(), log_q.data_ptr())

    calls = {"index": index,
             "sample": lambda: gp.sample_trees_device(s, K, 7, 0, par.data_ptr(), ent.data_ptr(), log_q.data_ptr(),
                                                      lengths.data_ptr()),
             "enumerate": lambda: gp.enumerate_trees_device(s, 0, count, par.data_ptr(), ent.data_ptr(), log_q.data_ptr(),
                                                            lengths.data_ptr())}
    call = calls[which]
    for _ in range(2):
        call()
    path = eng.last_call_path()
    torch.cuda.synchronize()
    eng.check_status()
    times = []
    for _ in range(rounds):
        with torch.cuda.stream(side):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            b.synchronize()
        times.append(a.elapsed_time(b))
    trees = count if which == "enumerate" else K
    tag = f"{name} ({n} taxa, G={gp.entry_count}, {total} topologies)"
    print(f"{tag:48s} {which:9s} {trees:5d} trees {np.median(times):9.3f} ms  (min {min(times):.3f}, max {max(times):.3f})  [{path}]")
    sys.stdout.flush()
    gp.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trees", type=int, default=1000)
    ap.add_argument("--store", choices=("lds", "global"), default=None)
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.store:
        os.environ["MI_PHYLO_GP_TREES_STORE"] = a.store
    if a.leg:
        name, which = a.leg.split(":")
        leg(name, which, a.rounds, a.trees)
        return
    for name in ("ds1", "36x1812"):
        for which in LEGS:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--rounds", str(a.rounds), "--trees", str(a.trees),
                                  "--leg", f"{name}:{which}"], check=True, capture_output=True, text=True).stdout
            print(out, end="", flush=True)


if __name__ == "__main__":
    main()
