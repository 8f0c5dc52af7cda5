#!/usr/bin/env python3
"""Time of the quartet hybrid marginals on the DS1 DAG of tools/bench_gp.py: the
100 golden DS1 topologies, each rooted on the edge above taxon 0 (27 taxa, 934 patterns).
Reports the formed entries, the summands S, the widest request, and -- device events around
`--repeats` enqueued calls on a side stream, the median of 7 rounds after a warm-up, milliseconds
per call, bench_gp.py's protocol -- of
  hybrid_marginals        hybrid_marginals_device alone (node probabilities, evolve pass, summands,
                          finalize), over the vectors of one populate
  populate+likelihoods    populate_device, likelihoods_device of the same DAG, in the same run
and hybrid_marginals once more with every request's pairs in ONE workgroup per pattern tile
(MI_PHYLO_GP_HYBRID_Z=1), the bits compared.  Nothing is asserted about the times.

    python tools/bench_gp_hybrid.py [--repeats 20]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import numpy as np  # noqa: E402


def main():
    import torch
    import libsbn_amd as L
    from bench_gp import case
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    repeats = ap.parse_args().repeats
    pids, tips, w = case("ds1")
    eng = L.Engine(L.PhyloModelSpecification("JC69", "constant", "strict"), tips, w, device=0)
    gp = eng.gp_create(pids, params=np.ones(eng.param_count))
    s, req = gp.structure(), gp.hybrid_requests()
    G, S = s.entry_count, len(req.summands)
    dev = torch.device("cuda", 0)
    per, marg = torch.zeros(G, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.float64, device=dev)
    hyb, each = torch.zeros(G, dtype=torch.float64, device=dev), torch.zeros(max(S, 1), dtype=torch.float64, device=dev)
    side = torch.cuda.Stream()
    host = gp.hybrid_marginals(summands=True)   # (reserves, populates)

    def likelihoods(stream):
        gp.populate_device(stream)
        gp.likelihoods_device(stream, per.data_ptr(), marg.data_ptr())

    def hybrid(stream):
        gp.hybrid_marginals_device(stream, hyb.data_ptr(), each.data_ptr())

    def between_events(enqueue):
        with torch.cuda.stream(side):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(repeats):
                enqueue(side.cuda_stream)
            b.record()
            b.synchronize()
        return a.elapsed_time(b) / repeats

    out = {"dag": "ds1", "taxa": s.taxon_count, "patterns": s.pattern_count, "nodes": s.node_count, "entries": G,
           "formed": int(np.sum(req.formed)), "summands": S, "widest_request": int(np.max(req.summand_count))}
    for key, enqueue in (("populate_likelihoods_ms", likelihoods), ("hybrid_marginals_ms", hybrid)):
        between_events(enqueue)
        out[key] = float(np.median([between_events(enqueue) for _ in range(7)]))
    out["path"] = eng.last_call_path()
    assert hyb.cpu().numpy().tobytes() == host.hybrid.tobytes() and each.cpu().numpy()[:S].tobytes() == host.summands.tobytes()
    assert np.all(np.isfinite(host.hybrid[req.formed])) and np.all(host.hybrid[~req.formed] == -np.inf)
    gp.close()
    # the same with the z-split off: another engine (switches are read at engine creation)
    os.environ["MI_PHYLO_GP_HYBRID_Z"] = "1"
    eng1 = L.Engine(L.PhyloModelSpecification("JC69", "constant", "strict"), tips, w, device=0)
    gp = eng1.gp_create(pids, params=np.ones(eng1.param_count))
    one = gp.hybrid_marginals(summands=True)
    assert one.hybrid.tobytes() == host.hybrid.tobytes() and one.summands.tobytes() == host.summands.tobytes()
    between_events(hybrid)
    out["hybrid_marginals_z1_ms"] = float(np.median([between_events(hybrid) for _ in range(7)]))
    out["path_z1"] = eng1.last_call_path()
    gp.close()
    print("BENCH_GP_HYBRID", json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
