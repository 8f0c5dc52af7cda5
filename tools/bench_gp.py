#!/usr/bin/env python3
"""Time of generalized pruning on two DAGs:
  ds1      the 100 golden DS1 topologies, each rooted on the edge above taxon 0 (27 taxa, 934 patterns)
  36x1812  36 taxa, 1812 random patterns, 40 topologies a few NNI moves away from one random tree
Per DAG, device events around `--repeats` enqueued calls on a side stream, the median of 7 rounds
after a warm-up, in milliseconds per call, of
  populate+likelihoods   populate_device, likelihoods_device
  optimiser evaluation   populate_device, branch_derivatives_device (what one evaluation of
                         optimize_branch_lengths runs before its step kernel)
and the algorithmic bytes of the two sweeps against the 8 TB/s HBM roofline: per
pattern a stored vector is 4 doubles and an exponent, 36 bytes, a tip code 1 byte;
  rootward  per entry the child's p, per internal node three vectors written
  leafward  per entry the parent's r, per node p once; per internal node two phat read, two r written
Nothing is asserted about the times.

    python tools/bench_gp.py [--repeats 20]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np  # noqa: E402

HBM_BYTES_PER_S = 8e12


def sweep_bytes(s):
    """algorithmic bytes of (rootward, leafward) over all patterns"""
    n, P = s.taxon_count, s.pattern_count
    child = s.entries[s.rootsplit_count:, 2]
    internal = s.node_count - n
    to_internal, to_leaf = int(np.sum(child >= n)), int(np.sum(child < n))
    rootward = P * (36 * to_internal + to_leaf + 3 * 36 * internal)
    leafward = P * (36 * (to_internal + to_leaf) + 36 * internal + n + 4 * 36 * internal)
    return rootward, leafward


def case(name):
    import gp_ref as R
    if name == "ds1":
        with open(os.path.join(REPO, "tests", "golden", "ds1_top100.struct.json")) as f:
            st = json.load(f)
        pids = np.stack([R.root_above_leaf0(t["parent_ids"]) for t in st["trees"]])
        return pids, np.array(st["patterns"], np.int32), np.array(st["weights"], np.float64)
    rng = np.random.default_rng(36)
    pids = R.nni_batch(36, 40, 3, rng)
    tips = rng.integers(0, 4, (36, 1812)).astype(np.int32)
    return pids, tips, np.ones(1812)


def run(name, repeats):
    import torch
    import libsbn_amd as L
    pids, tips, w = case(name)
    eng = L.Engine(L.PhyloModelSpecification("JC69", "constant", "strict"), tips, w, device=0)
    gp = eng.gp_create(pids, params=np.ones(eng.param_count))
    s = gp.structure()
    G = s.entry_count
    dev = torch.device("cuda", 0)
    per, marg = torch.zeros(G, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.float64, device=dev)
    pair, g, h, sq = (torch.zeros(k * G, dtype=torch.float64, device=dev) for k in (2, 1, 1, 1))
    side = torch.cuda.Stream()

    def likelihoods(stream):
        gp.populate_device(stream)
        gp.likelihoods_device(stream, per.data_ptr(), marg.data_ptr())

    def evaluation(stream):
        gp.populate_device(stream)
        gp.branch_derivatives_device(stream, pair.data_ptr(), g.data_ptr(), h.data_ptr(), sq.data_ptr())

    def between_events(enqueue):
        with torch.cuda.stream(side):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(repeats):
                enqueue(side.cuda_stream)
            b.record()
            b.synchronize()
        return a.elapsed_time(b) / repeats

    out = {"dag": name, "taxa": s.taxon_count, "patterns": s.pattern_count, "nodes": s.node_count, "entries": G,
           "levels": gp.level_count, "topologies": s.topology_count, "path": None}
    for key, enqueue in (("populate_likelihoods_ms", likelihoods), ("optimiser_evaluation_ms", evaluation)):
        between_events(enqueue)
        out[key] = float(np.median([between_events(enqueue) for _ in range(7)]))
    out["path"] = eng.last_call_path()
    assert np.isfinite(float(marg.cpu()[0])) and bool(torch.all(torch.isfinite(g)))
    rootward, leafward = sweep_bytes(s)
    out["sweep_bytes"] = [rootward, leafward]
    out["hbm_frac"] = (rootward + leafward) / (out["populate_likelihoods_ms"] * 1e-3) / HBM_BYTES_PER_S
    gp.close()
    print("BENCH_GP", json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    a = ap.parse_args()
    for name in ("ds1", "36x1812"):
        run(name, a.repeats)


if __name__ == "__main__":
    main()
