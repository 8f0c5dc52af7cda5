#!/usr/bin/env python3
"""Time per step of a device-resident variational fit, by
tools/bench_branch_model.py's method: DS1 (the golden alignment, the support of its 100 golden
topologies, q by mode matching, the SBN at zero), K particles per step, every batch in a child
process of its own, the median of `--rounds` rounds after a warm-up with minimum and maximum.

Per batch, milliseconds per step of
  fit               VariationalFit.fit(steps): wall clock around the call (it enqueues the steps on
                    the engine's stream, checks the status once and downloads the trace rows)
  replay            step_device captured once in a graph on one stream, `steps` replays between two
                    device events
  yardstick         what the library could do before the fit existed: the same chain enqueued
                    through the by-value *_device calls (the same particles and the same beta every
                    time, no update, no trace), `steps` times between two device events
  yardstick_replay  ... captured once and replayed
Nothing is asserted about the times.

    python tools/bench_vi_fit.py [--rounds 5] [--steps 20] [--batches 64,1000]"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402


def leg(K, rounds, steps):
    import torch
    import libsbn_amd as L
    with open(os.path.join(REPO, "tests", "golden", "ds1_top100.struct.json")) as f:
        st = json.load(f)
    pids = np.array([t["parent_ids"] for t in st["trees"]], np.int32)
    bls = np.array([t["branch_lengths"] for t in st["trees"]], np.float64)
    T0, E = pids.shape
    n = (E + 3) // 2
    eng = L.Engine(L.PhyloModelSpecification("JC69", "constant", "strict"), np.array(st["patterns"], np.int32),
                   np.array(st["weights"], np.float64), device=0)
    sup = eng.sbn_index(pids)
    S, C, parents, P = sup.rootsplit_count, sup.pcsp_count, sup.parent_count, sup.parameter_count
    desc, table = eng.sbn_descent(sup), eng.psp_table(sup)
    V = table.variable_count
    split = eng.split_index(pids, branch_lengths=bls)
    q = L.lognormal_mode_match(split.stats[:, 1] / split.stats[:, 0], table)
    phi = np.zeros(P)
    total = (rounds + 1) * steps + 1
    params = np.ones(eng.param_count)

    def new_fit():
        return eng.vi_create(pids, phi, q, particle_count=K, anneal_steps=total, max_steps=total, seed=20261021,
                             model_params=params)

    side = torch.cuda.Stream()
    dev = torch.device("cuda", 0)

    def between_events(run):
        with torch.cuda.stream(side):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run()
            b.record()
            b.synchronize()
        return a.elapsed_time(b) / steps

    times = {}
    # fit
    fit = new_fit()
    fit.fit(steps)
    path = eng.last_call_path()
    times["fit"] = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        trace = fit.fit(steps)
        times["fit"].append((time.perf_counter() - t0) * 1e3 / steps)
    assert np.all(np.isfinite(trace)) and np.all(trace[:, 5] == 1.0)
    fit.close()
    # a caller-captured step
    fit = new_fit()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        fit.step_device(torch.cuda.current_stream().cuda_stream)
    between_events(lambda: [graph.replay() for _ in range(steps)])
    times["replay"] = [between_events(lambda: [graph.replay() for _ in range(steps)]) for _ in range(rounds)]
    eng.check_status(side.cuda_stream)
    assert fit.state().successes == (rounds + 1) * steps
    fit.close()
    # the yardstick: by-value arguments, no update
    i32, f64 = torch.int32, torch.float64
    up = lambda x: torch.tensor(np.ascontiguousarray(x), device=dev)  # noqa: E731
    d_range, d_desc, d_psp, d_phi, d_q = up(sup.parent_range), up(desc), up(table.psp_of_pcsp), up(phi), up(q)
    d_params = up(np.ones((K, max(eng.param_count, 1))))
    all_pid = torch.zeros((T0 + K, E), dtype=i32, device=dev)
    all_pid[:T0] = up(pids)
    z = lambda shape, dtype=f64: torch.zeros(shape, dtype=dtype, device=dev)  # noqa: E731
    o_edge, o_params, o_lp = z(K, i32), z((K, n - 1), i32), z(K)
    o_root, o_slot, o_counts = z((T0 + K, E), i32), z((T0 + K, 2 * E, 3), i32), z(3, i32)
    o_bits, o_clades, o_prange, o_parent = z((S, 1), i32), z((C, 3), i32), z((C, 2), i32), z(C, i32)
    o_index, o_bl, o_eps, o_lqb, o_lprior = z((K, 3, E), i32), z((K, E + 1)), z((K, E)), z(K), z(K)
    o_ll, o_g, o_rooting, o_lqt = z(K), z((K, E + 2)), z((K, E)), z(K)
    o_qgrad, o_f, o_grad, o_factors, o_glq = z((V, 2)), z(K), z(P), z(K), z(K)
    samples, root, slot = all_pid[T0:].data_ptr(), o_root[T0:].data_ptr(), o_slot[T0:].data_ptr()

    def chain(s):
        eng.sbn_sample_device(s, K, n, S, C, parents, d_range.data_ptr(), d_desc.data_ptr(), d_phi.data_ptr(), 20261021, 0,
                              samples, o_edge.data_ptr(), o_params.data_ptr(), o_lp.data_ptr())
        eng.sbn_index_device(s, T0 + K, n, all_pid.data_ptr(), T0, S, C, o_root.data_ptr(), o_slot.data_ptr(),
                             o_counts.data_ptr(), o_bits.data_ptr(), o_clades.data_ptr(), o_prange.data_ptr(),
                             o_parent.data_ptr())
        eng.psp_index_device(s, K, n, root, slot, S, C, d_psp.data_ptr(), V, 3, o_index.data_ptr())
        eng.branch_model_sample_device(s, K, n, 3, o_index.data_ptr(), V, d_q.data_ptr(), 20261021, 0, 10.0,
                                       o_bl.data_ptr(), o_eps.data_ptr(), o_lqb.data_ptr(), o_lprior.data_ptr())
        eng.gradients_device(s, K, samples, o_bl.data_ptr(), d_params.data_ptr(), o_ll.data_ptr(), o_g.data_ptr())
        eng.sbn_log_prob_device(s, K, n, samples, root, slot, S, C, parents, d_range.data_ptr(), d_phi.data_ptr(), False,
                                o_rooting.data_ptr(), o_lqt.data_ptr())
        eng.branch_model_gradient_device(s, K, n, 3, o_index.data_ptr(), V, d_q.data_ptr(), o_bl.data_ptr(),
                                         o_eps.data_ptr(), o_lqb.data_ptr(), o_lprior.data_ptr(), o_g.data_ptr(),
                                         o_ll.data_ptr(), 1.0, 10.0, o_qgrad.data_ptr(), o_f.data_ptr(),
                                         log_q_topology=o_lqt.data_ptr())
        eng.sbn_topology_gradient_device(s, K, n, samples, root, slot, S, C, parents, d_range.data_ptr(),
                                         d_phi.data_ptr(), False, o_f.data_ptr(), "vimco", o_grad.data_ptr(),
                                         o_factors.data_ptr(), o_glq.data_ptr())

    torch.cuda.synchronize()
    between_events(lambda: [chain(side.cuda_stream) for _ in range(steps)])
    times["yardstick"] = [between_events(lambda: [chain(side.cuda_stream) for _ in range(steps)]) for _ in range(rounds)]
    eng.check_status(side.cuda_stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        chain(torch.cuda.current_stream().cuda_stream)
    between_events(lambda: [graph.replay() for _ in range(steps)])
    times["yardstick_replay"] = [between_events(lambda: [graph.replay() for _ in range(steps)]) for _ in range(rounds)]
    eng.check_status(side.cuda_stream)
    assert bool(torch.all(torch.isfinite(o_grad))) and bool(torch.all(torch.isfinite(o_qgrad)))

    tag = f"ds1 K={K} (T0={T0}, P={P}, V={V})"
    print(f"{tag:34s} [{path}]")
    for k, v in times.items():
        print(f"{tag:34s} {k:17s} {np.median(v):9.3f} ms per step  (min {min(v):.3f}, max {max(v):.3f})")
    print("BENCH_VI_FIT", json.dumps({"K": K, **{k: float(np.median(v)) for k, v in times.items()}}))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batches", default="64,1000")
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        leg(int(a.leg), a.rounds, a.steps)
        return
    for batch in a.batches.split(","):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--rounds", str(a.rounds), "--steps", str(a.steps),
                              "--leg", batch], check=True, capture_output=True, text=True).stdout
        for line in out.splitlines():
            print(line, flush=True)


if __name__ == "__main__":
    main()
