#!/usr/bin/env python3
"""A/B timing of builds of libmi_phylo.so on the headline step, interleaved in ONE process
chain on ONE box (kernel times differ by 2-3 % from box to box and run to run: only
back-to-back alternation tells a 2 % change from noise).

  python tools/ab_kernels.py [--rounds 3] [--bench-args "..."] name=path.so[,ENV=value...] ...

Each variant is a library path (or "default") plus optional environment settings; every round
runs bench.py once per variant, each run under its own time limit; the table gives min / median
of the dominant kernel's launch time and of the step.  The first run that fails or outlasts its
limit ends the whole comparison with a non-zero exit status: nothing more is started on the GPU
after a failure."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--bench-args", default="--steps 20 --warmup 3 --headline-only --full")
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds per bench.py run")
    ap.add_argument("variants", nargs="+")
    args = ap.parse_args()
    variants = []
    for v in args.variants:
        name, _, rest = v.partition("=")
        parts = rest.split(",") if rest else ["default"]
        env = {}
        if parts[0] != "default":
            env["MI_PHYLO_LIBRARY"] = os.path.abspath(parts[0])
        for kv in parts[1:]:
            k, _, val = kv.partition("=")
            env[k] = val
        variants.append((name, env))
    res = {name: {"kernel": [], "step": []} for name, _ in variants}
    for _ in range(args.rounds):
        for name, env in variants:
            try:
                r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + args.bench_args.split(),
                                   env=dict(os.environ, **env), capture_output=True, text=True,
                                   timeout=args.timeout)
            except subprocess.TimeoutExpired:
                print(name, f"TIMED OUT after {args.timeout:.0f} s: stopping")
                sys.exit(124)
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            if r.returncode != 0 or not lines:
                print(name, f"FAILED (exit status {r.returncode}): stopping", r.stdout[-500:], r.stderr[-1500:])
                sys.exit(r.returncode if r.returncode > 0 else 1)
            d = json.loads(lines[-1])
            res[name]["kernel"].append(d["step_ms_device"]["kernel_median"])
            res[name]["step"].append(d["step_ms_device"]["median"])
            res[name]["name"] = d["roofline"]["kernel"]
    for name, _ in variants:
        k, s = res[name]["kernel"], res[name]["step"]
        if k:
            print(f"{name:24s} {res[name].get('name', ''):24s} kernel min {min(k):.4f} median {np.median(k):.4f} ms | "
                  f"step min {min(s):.4f} median {np.median(s):.4f} ms   ({len(k)} runs)")
            # (each round's step median: their largest minus smallest is the day's noise)
            print(f"{'':24s} kernel by round: " + " ".join(f"{x:.4f}" for x in k) + f"   spread {max(k) - min(k):.4f} ms")
            print(f"{'':24s} step by round: " + " ".join(f"{x:.4f}" for x in s) + f"   spread {max(s) - min(s):.4f} ms")


if __name__ == "__main__":
    main()
