#!/usr/bin/env python3
"""Time per step of a variational fit over the rooted trees of a subsplit DAG, by
tools/bench_vi_fit.py's method: DS1 (the golden alignment, its 100 golden topologies rooted as the
GP tests root them, the DAG they span, the default start), K particles per step, every batch in a
child process of its own, the median of `--rounds` rounds after a warm-up with minimum and maximum.

Per batch, milliseconds per step of
  fit         RootedVariationalFit.fit(steps): wall clock around the call
  replay      step_device captured once in a graph on one stream, `steps` replays between two
              device events
and two yardsticks, in a child process that loads `--yardstick-library` (another build of the
library, for instance the parent commit's; default: this one):
  unrooted_fit, unrooted_replay   the unrooted VariationalFit at the same K on the
              support of the same topologies, by the same two methods
  gradient    the bare gradient call of K de-rooted trees, enqueued `steps` times between two events
Nothing is asserted about the times.

    python tools/bench_gp_vi.py [--rounds 5] [--steps 20] [--batches 64,1000] [--yardstick-library PATH]"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np  # noqa: E402


def _ds1():
    with open(os.path.join(REPO, "tests", "golden", "ds1_top100.struct.json")) as f:
        return json.load(f)


def _events(torch, side, steps, run):
    with torch.cuda.stream(side):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        b.synchronize()
    return a.elapsed_time(b) / steps


def _fit_and_replay(torch, eng, new_fit, rounds, steps, names, times):
    side = torch.cuda.Stream()
    fit = new_fit()
    fit.fit(steps)
    path = eng.last_call_path()
    times[names[0]] = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        trace = fit.fit(steps)
        times[names[0]].append((time.perf_counter() - t0) * 1e3 / steps)
    assert np.all(np.isfinite(trace)) and np.all(trace[:, 5] == 1.0)
    fit.close()
    fit = new_fit()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        fit.step_device(torch.cuda.current_stream().cuda_stream)
    replay = lambda: [graph.replay() for _ in range(steps)]  # noqa: E731
    _events(torch, side, steps, replay)
    times[names[1]] = [_events(torch, side, steps, replay) for _ in range(rounds)]
    eng.check_status(side.cuda_stream)
    assert fit.state().successes == (rounds + 1) * steps
    fit.close()
    return path


def rooted_leg(K, rounds, steps):
    import torch
    import gp_ref as R
    import libsbn_amd as L
    st = _ds1()
    pids = np.stack([R.root_above_leaf0(t["parent_ids"]) for t in st["trees"]])
    eng = L.Engine(L.PhyloModelSpecification("JC69", "constant", "strict"), np.array(st["patterns"], np.int32),
                   np.array(st["weights"], np.float64), device=0)
    gp = eng.gp_create_dag(pids)
    total = (rounds + 1) * steps + 1
    params = np.ones(eng.param_count)
    times = {}
    path = _fit_and_replay(torch, eng, lambda: gp.vi_create(model_params=params, particle_count=K, anneal_steps=total,
                                                            max_steps=total, seed=20261021), rounds, steps,
                           ("fit", "replay"), times)
    report(f"ds1 rooted K={K} (G={gp.entry_count}, R={gp.rootsplit_count})", path, K, times)


def yardstick_leg(K, rounds, steps):
    import ctypes
    import torch
    from libsbn_amd import _capi
    if os.environ.get("MI_PHYLO_LIBRARY"):   # (an earlier build lacks the calls this one added: bind what it has)
        torch.cuda.init()
        old = ctypes.CDLL(os.environ["MI_PHYLO_LIBRARY"])
        for name in [x for x in _capi.SYMBOLS if not hasattr(old, x)]:
            del _capi.SYMBOLS[name]
    import libsbn_amd as L
    st = _ds1()
    pids = np.array([t["parent_ids"] for t in st["trees"]], np.int32)
    bls = np.array([t["branch_lengths"] for t in st["trees"]], np.float64)
    eng = L.Engine(L.PhyloModelSpecification("JC69", "constant", "strict"), np.array(st["patterns"], np.int32),
                   np.array(st["weights"], np.float64), device=0)
    sup = eng.sbn_index(pids)
    table = eng.psp_table(sup)
    split = eng.split_index(pids, branch_lengths=bls)
    q = L.lognormal_mode_match(split.stats[:, 1] / split.stats[:, 0], table)
    phi = np.zeros(sup.parameter_count)
    total = (rounds + 1) * steps + 1
    params = np.ones(eng.param_count)
    times = {}
    path = _fit_and_replay(torch, eng, lambda: eng.vi_create(pids, phi, q, particle_count=K, anneal_steps=total,
                                                             max_steps=total, seed=20261021, model_params=params),
                           rounds, steps, ("unrooted_fit", "unrooted_replay"), times)
    # the bare gradient call of K trees
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream()
    up = lambda x: torch.tensor(np.ascontiguousarray(x), device=dev)  # noqa: E731
    take = np.arange(K) % len(pids)
    d_pid, d_bl, d_params = up(pids[take]), up(bls[take]), up(np.ones((K, max(eng.param_count, 1))))
    o_ll = torch.zeros(K, dtype=torch.float64, device=dev)
    o_g = torch.zeros((K, pids.shape[1] + 2), dtype=torch.float64, device=dev)
    eng.reserve(K, True)
    torch.cuda.synchronize()
    call = lambda: [eng.gradients_device(side.cuda_stream, K, d_pid.data_ptr(), d_bl.data_ptr(), d_params.data_ptr(),  # noqa: E731
                                         o_ll.data_ptr(), o_g.data_ptr()) for _ in range(steps)]
    _events(torch, side, steps, call)
    times["gradient"] = [_events(torch, side, steps, call) for _ in range(rounds)]
    eng.check_status(side.cuda_stream)
    assert bool(torch.all(torch.isfinite(o_ll)))
    report(f"ds1 yardsticks K={K} [{os.environ.get('MI_PHYLO_LIBRARY', 'this build')}]", path, K, times)


def report(tag, path, K, times):
    print(f"{tag} [{path}]")
    for k, v in times.items():
        print(f"  {k:17s} {np.median(v):9.3f} ms per step  (min {min(v):.3f}, max {max(v):.3f})")
    print("BENCH_GP_VI", json.dumps({"K": K, **{k: float(np.median(v)) for k, v in times.items()}}))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batches", default="64,1000")
    ap.add_argument("--yardstick-library", default=None)
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        kind, K = a.leg.split(":")
        (rooted_leg if kind == "rooted" else yardstick_leg)(int(K), a.rounds, a.steps)
        return
    for batch in a.batches.split(","):
        for kind in ("rooted", "yardstick"):
            env = dict(os.environ)
            if kind == "yardstick" and a.yardstick_library:
                env["MI_PHYLO_LIBRARY"] = os.path.abspath(a.yardstick_library)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--rounds", str(a.rounds), "--steps", str(a.steps),
                                  "--leg", f"{kind}:{batch}"], check=True, capture_output=True, text=True, env=env).stdout
            for line in out.splitlines():
                print(line, flush=True)


if __name__ == "__main__":
    main()
