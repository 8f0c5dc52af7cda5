"""Every route an engine call can take, replayed against a recording.

`tests/golden/call_paths.json` was recorded from the library of the commit BEFORE the host
side's route decisions were gathered into one call plan (mi_phylo_call.cpp): for every case
below it holds the generator's seed and shape, a SHA-256 of the input arrays, what
mi_engine_last_call_path / _info / _launches said after the call, and a SHA-256 of the float64
bytes of every output, in a fixed order.  The kernels sum with integer atomics and in fixed
orders only, so a call's outputs are reproducible bit for bit (recorded twice, compared,
before the fixture was written).  The test replays every case on the current build and asks
for equal strings, counts and hashes: the same route, the same launches, the same bits.

Routes no default shape reaches are reached with the engine's switches (README, "Switches");
the shapes are those of test_gpu_parity.py and test_fused_setup_gpu.py.

Recording (from a build of the commit to compare with, loaded through the loader variable):
  MI_PHYLO_LIBRARY=/path/to/libmi_phylo.so python tests/test_call_paths_gpu.py [out.json]
"""
import contextlib
import hashlib
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import tree_utils as TU  # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "call_paths.json")

SMALL = dict(n=14, P=70, T=40)     # LDS store, the one-launch call applies
LARGE = dict(n=50, P=60, T=300)    # the arena variants (test_fused_setup_gpu.py)
MANY = dict(n=5, P=10, T=33000)    # more evaluations than one launch covers
GTR = dict(n=14, P=70, T=6)
ARENA = {"MI_PHYLO_GRADIENT_STORE": "arena", "MI_PHYLO_WALK_TILE_REGS": "3"}


def _case(name, kind, subst="JC69", site="weibull+4", shape=SMALL, seed=1, env=None, rescaling=False,
          blocks=None):
    return dict(name=name, kind=kind, subst=subst, site=site, seed=seed, env=env or {},
                rescaling=rescaling, blocks=blocks, **shape)


CASES = [
    # ---- unrooted gradient calls: set-up forms, stores, walk generations ----
    _case("grad_one_launch", "gradient"),
    _case("grad_one_launch_rescaled", "gradient", rescaling=True),
    _case("grad_setup_with_records", "gradient",
          env={"MI_PHYLO_FUSED_MAX_TREES": "8", "MI_PHYLO_SETUP_RECORDS": "1"}),
    _case("grad_four_launches", "gradient", env={"MI_PHYLO_FUSED_SETUP": "0"}),
    _case("grad_separate_reduction", "gradient", env={"MI_PHYLO_FUSE_FINALIZE": "0"}),
    _case("grad_k1", "gradient", site="constant"),
    _case("grad_k1_second_generation", "gradient", site="constant",
          env={"MI_PHYLO_WALK3_K1": "0", "MI_PHYLO_FUSED_SETUP": "0"}),
    _case("grad_k2", "gradient", site="weibull+2"),
    _case("grad_k3_rescaled", "gradient", site="weibull+3", rescaling=True),
    _case("grad_k8", "gradient", site="weibull+8"),
    _case("grad_k8_rescaled", "gradient", site="weibull+8", rescaling=True),
    _case("grad_second_generation", "gradient", env={"MI_PHYLO_GRADIENT_WALK": "v2"}),
    _case("grad_hbm", "gradient", env={"MI_PHYLO_GRADIENT_PATH": "hbm"}),
    _case("grad_hbm_rescaled", "gradient", env={"MI_PHYLO_GRADIENT_PATH": "hbm"}, rescaling=True),
    _case("grad_large_default", "gradient", shape=LARGE),
    _case("grad_large_few_trees", "gradient", shape=dict(LARGE, T=4)),
    _case("grad_arena_wide", "gradient", shape=LARGE,
          env={"MI_PHYLO_GRADIENT_STORE": "arena", "MI_PHYLO_WALK_TILE_REGS": "4"}),
    _case("grad_arena", "gradient", shape=LARGE, env=ARENA),
    _case("grad_arena_rescaled", "gradient", shape=LARGE, env=ARENA, rescaling=True),
    _case("grad_arena_second_generation", "gradient", shape=LARGE,
          env=dict(ARENA, MI_PHYLO_WALK3_ARENA="0")),
    _case("grad_arena_in_parts", "gradient", shape=LARGE, env=dict(ARENA, MI_PHYLO_PLV_BYTES="3000000")),
    _case("grad_large_lds", "gradient", shape=LARGE,
          env={"MI_PHYLO_GRADIENT_STORE": "lds", "MI_PHYLO_WALK_TILE_REGS": "3"}),
    _case("grad_many_trees", "gradient", shape=MANY),
    # ---- GTR: finite differences, site pass, optional outputs, analytic gradient ----
    _case("gtr_full", "gradient", subst="GTR", shape=GTR),
    _case("gtr_full_rescaled", "gradient", subst="GTR", shape=GTR, rescaling=True),
    _case("gtr_branch_only", "gradient", subst="GTR", shape=GTR, blocks=["branch_lengths"]),
    _case("gtr_subst_only", "gradient", subst="GTR", shape=GTR, blocks=["substitution_model"]),
    _case("gtr_site_only", "gradient", subst="GTR", shape=GTR, blocks=["site_model"]),
    _case("gtr_analytic", "gradient", subst="GTR", shape=GTR, env={"MI_PHYLO_SUBST_GRADIENT": "analytic"}),
    _case("gtr_k1", "gradient", subst="GTR", site="constant", shape=GTR),
    _case("gtr_hbm", "gradient", subst="GTR", shape=GTR, env={"MI_PHYLO_GRADIENT_PATH": "hbm"}),
    _case("gtr_second_generation", "gradient", subst="GTR", shape=GTR, env={"MI_PHYLO_GRADIENT_WALK": "v2"}),
    # ---- log-likelihood calls, both kernels ----
    _case("loglik_default", "loglik"),
    _case("loglik_rescaled", "loglik", rescaling=True),
    _case("loglik_valu", "loglik", env={"MI_PHYLO_LOGLIK_PATH": "valu"}),
    _case("loglik_mfma", "loglik", env={"MI_PHYLO_LOGLIK_PATH": "mfma"}),
    _case("loglik_k8", "loglik", site="weibull+8"),
    _case("loglik_gtr", "loglik", subst="GTR", shape=GTR),
    _case("loglik_many_trees", "loglik", shape=MANY),
    # ---- rooted calls ----
    _case("rooted_gradient", "rooted_gradient"),
    _case("rooted_gradient_gtr", "rooted_gradient", subst="GTR", shape=GTR),
    _case("rooted_loglik", "rooted_loglik"),
    # ---- the branch-length Hessian call: walk and HBM kernels, LDS and arena stores ----
    _case("hess_walk_lds", "hessian"),
    _case("hess_walk_lds_rescaled", "hessian", rescaling=True),
    _case("hess_walk_arena", "hessian", shape=LARGE, env={"MI_PHYLO_GRADIENT_STORE": "arena"}),
    _case("hess_walk_arena_in_parts", "hessian", shape=LARGE,
          env={"MI_PHYLO_GRADIENT_STORE": "arena", "MI_PHYLO_PLV_BYTES": "3000000"}),
    _case("hess_hbm", "hessian", env={"MI_PHYLO_GRADIENT_PATH": "hbm"}),
    _case("hess_k8", "hessian", site="weibull+8"),
    _case("hess_gtr", "hessian", subst="GTR", shape=GTR),
    # ---- branch-length optimisation that packs its active trees; 20 states ----
    _case("branch_opt_packs", "branch_opt", shape=dict(n=14, P=70, T=24)),
    _case("aa_gradient", "aa_gradient", subst="WAG", shape=dict(n=9, P=40, T=2)),
    _case("aa_loglik", "aa_loglik", subst="WAG", shape=dict(n=9, P=40, T=2)),
]


def _inputs(c):
    """The arrays of a case, from its seed and shape alone: (engine arrays, call arrays)."""
    rng = np.random.default_rng(c["seed"])
    n, P, T, kind = c["n"], c["P"], c["T"], c["kind"]
    a = {}
    if kind.startswith("aa_"):
        import aa_utils as A
        a["tips"], a["weights"] = A.random_aa_alignment(n, P, rng)
    else:
        a["tips"], a["weights"] = TU.random_alignment(n, P, rng, gap_fraction=0.05)
    if kind.startswith("rooted"):
        import oracle_lib as O
        trees = [TU.clocklike_rooted_tree(n, rng) for _ in range(T)]
        a["parent_ids"] = np.stack([t[0] for t in trees])
        a["branch_lengths"] = np.stack([t[1] for t in trees])
        state = [O.time_tree_init(n, t[0], t[1], t[2]) for t in trees]
        a["heights"] = np.stack([s[0] for s in state])
        a["bounds"] = np.stack([s[1] for s in state])
        a["ratios"] = np.stack([s[2] for s in state])
        a["rates"] = np.full((T, 2 * n - 2), 0.7)
        a["rate_counts"] = np.ones(T, np.int32)
    else:
        a["parent_ids"], a["branch_lengths"] = TU.random_trees(n, T, rng, mean_bl=0.07)
    if kind == "branch_opt":
        # tip states evolved down the first tree (the data carry a signal about its branches), and
        # every other tree starts far from its optimum: the trees stop at different passes
        states = np.zeros((2 * n - 2, P), np.int32)
        states[-1] = rng.integers(0, 4, size=P)
        for v in range(2 * n - 4, -1, -1):
            states[v] = np.where(rng.random(P) < 0.08, rng.integers(0, 4, size=P), states[a["parent_ids"][0][v]])
        a["tips"] = states[:n].copy()
        a["branch_lengths"] = np.full((T, 2 * n - 2), 0.1)
        a["branch_lengths"][1::2] = 1.5
        a["branch_lengths"][:, -1] = 0.0
    a["gtr_rates"], a["gtr_freqs"] = TU.random_gtr_params(T, rng)
    a["shape"] = rng.uniform(0.4, 1.5, size=(T, 1))
    return a


def _params(eng, c, a):
    pr = np.zeros((c["T"], eng.param_count))
    for name, (start, length) in eng.block_specification().items():
        if name == "GTR rates":
            pr[:, start:start + length] = a["gtr_rates"]
        elif name == "frequencies":
            pr[:, start:start + length] = a["gtr_freqs"]
        elif name == "Weibull shape":
            pr[:, start:start + length] = a["shape"]
        elif name == "clock rate":
            pr[:, start:start + length] = 1.0
    return pr


def _sha(arrays):
    h = hashlib.sha256()
    for x in arrays:
        x = np.ascontiguousarray(x)
        h.update(str((x.dtype.str, x.shape)).encode())
        h.update(x.tobytes())
    return h.hexdigest()


def _f64(x):
    return hashlib.sha256(np.ascontiguousarray(np.asarray(x), dtype=np.float64).tobytes()).hexdigest()


def _gradient_outputs(grads):
    out = [("log_likelihood", np.array([g.log_likelihood for g in grads]))]
    for key in sorted(grads[0].gradient):
        out.append((key, np.stack([np.atleast_1d(g.gradient[key]) for g in grads])))
    return out


@contextlib.contextmanager
def _switches(env):
    """The engine reads its switches once, at creation: set for that moment only."""
    mine = {k: os.environ.get(k) for k in os.environ if k.startswith("MI_PHYLO_") and k != "MI_PHYLO_LIBRARY"
            and k != "MI_PHYLO_NO_TORCH_PRELOAD"}
    for k in mine:
        del os.environ[k]
    os.environ.update(env)
    try:
        yield
    finally:
        for k in env:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in mine.items() if v is not None})


def run_case(c):
    """Runs one case on the loaded library: what the fixture records of it."""
    import libsbn_amd as L
    a = _inputs(c)
    with _switches(c["env"]):
        eng = L.Engine(L.PhyloModelSpecification(c["subst"], c["site"], "strict"), a["tips"], a["weights"],
                       device=0)
    try:
        pr = _params(eng, c, a)
        pids, bls, resc, kind = a["parent_ids"], a["branch_lengths"], c["rescaling"], c["kind"]
        if kind in ("gradient", "aa_gradient"):
            outs = _gradient_outputs(eng.gradients(pids, bls, pr, resc, gradient_blocks=c["blocks"]))
        elif kind in ("loglik", "aa_loglik"):
            outs = [("log_likelihood", eng.log_likelihoods(pids, bls, pr, resc))]
        elif kind == "rooted_gradient":
            outs = _gradient_outputs(eng.rooted_gradients(pids, bls, pr, a["rates"], a["rate_counts"],
                                                          a["heights"], a["bounds"], a["ratios"], resc))
        elif kind == "rooted_loglik":
            outs = [("log_likelihood", eng.rooted_log_likelihoods(pids, bls, pr, a["rates"], a["heights"],
                                                                  a["bounds"], resc, with_jacobian=True))]
        elif kind == "hessian":
            ll, g, h, s = eng.branch_hessian(pids, bls, pr, resc, squared_gradient=True)
            outs = [("log_likelihood", ll), ("gradient", g), ("hessian", h), ("squared_gradient", s)]
        elif kind == "branch_opt":
            r = eng.optimize_branch_lengths(pids, bls, pr, resc, check_interval=1)
            outs = [("branch_lengths", r.branch_lengths), ("log_likelihood", r.log_likelihood),
                    ("gradient", r.gradient), ("hessian", r.hessian), ("iterations", r.iterations),
                    ("status", r.status)]
        else:
            raise ValueError(kind)
        rec = dict(c)
        rec["input_sha256"] = _sha([a[k] for k in sorted(a)] + [pr])
        rec["last_call_path"] = eng.last_call_path()
        rec["last_call_info"] = list(eng.last_call_info())
        rec["last_call_launches"] = eng.last_call_launches()[0]
        rec["outputs"] = [[name, _f64(x)] for name, x in outs]
        return rec
    finally:
        eng.close()


def _fixture():
    with open(FIXTURE) as fh:
        return {c["name"]: c for c in json.load(fh)["cases"]}


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_case_takes_the_recorded_route_and_gives_the_recorded_bits(name):
    want = _fixture()[name]
    case = next(c for c in CASES if c["name"] == name)
    # (the case is replayed from what the fixture says of it: seed, shape and switches)
    assert {k: want[k] for k in case} == case, "the fixture was recorded for another definition of this case"
    got = run_case(case)
    assert got["input_sha256"] == want["input_sha256"], \
        "the input GENERATOR changed (numpy / tree_utils / oracle time-tree set-up), not the engine: " \
        "the recorded outputs do not apply to these inputs"
    print(name, "|", got["last_call_path"], "|", got["last_call_info"], got["last_call_launches"])
    assert got["last_call_path"] == want["last_call_path"]
    assert got["last_call_info"] == want["last_call_info"]
    assert got["last_call_launches"] == want["last_call_launches"]
    assert got["outputs"] == want["outputs"]


def check_coverage(cases):
    """The routes the recording must reach (each by at least one case)."""
    assert len(cases) == len(CASES) and sorted(c["name"] for c in cases) == sorted(c["name"] for c in CASES)
    paths = [c["last_call_path"] for c in cases]

    def reached(*tokens):
        return [p for p in paths if all((" " + t + " ") in (" " + p + " ") for t in tokens)]

    for token in ("store=hbm", "store=lds", "store=arena", "setup=in-walk", "setup=with-records",
                  "setup=own-launch", "tile=wide", "fd=16", "site-pass", "light", "analytic", "rescaled",
                  "rooted", "hess", "K=1", "K=2", "K=4"):
        assert reached(token), token
    kernels = {p.split(" ")[0] for p in reached("hess")}
    assert len(kernels) == 2, kernels  # the walk's Hessian form and the HBM kernel's
    walk = [k for k in kernels if "walk" in k][0]
    assert reached("hess", "store=hbm") and reached("hess", "store=lds") and reached("hess", "store=arena")
    assert all(p.startswith(walk) for p in reached("hess", "store=lds") + reached("hess", "store=arena"))
    assert any(int(p.split(" K=")[1].split(" ")[0]) > 4 for p in paths)
    loglik = {c["last_call_info"][0] for c in cases if c["kind"] == "loglik"}
    assert len(loglik) == 2, loglik
    assert any(c["last_call_launches"] > 1 and c["kind"] == "gradient" for c in cases)
    assert any(c["last_call_launches"] > 1 and c["kind"] == "loglik" for c in cases)
    opt = [c for c in cases if c["kind"] == "branch_opt"]
    # (a call that packed ran batches of more than one size, and did not have packing turned off)
    assert opt and all("," in c["last_call_path"].split(" batches=")[1].split(" ")[0] and
                       "pack=off" not in c["last_call_path"] for c in opt)
    assert any(c["kind"] == "aa_gradient" and "states=20" in c["last_call_path"] for c in cases)


def test_the_recording_covers_the_routes():
    check_coverage(list(_fixture().values()))
    assert os.path.getsize(FIXTURE) < 64 * 1024


def _record(out):
    first = [run_case(c) for c in CASES]
    second = [run_case(c) for c in CASES]
    for x, y in zip(first, second):
        assert x == y, ("not reproducible", x, y)
    check_coverage(first)
    for c in first:
        print(c["name"], "|", c["last_call_path"], "|", c["last_call_info"], c["last_call_launches"])
    from libsbn_amd import _capi
    with open(out, "w") as fh:
        json.dump({"cases": first}, fh, indent=0)
        fh.write("\n")
    print("recorded", len(first), "cases from", _capi.LIB_PATH, "->", out)


if __name__ == "__main__":
    try:
        import torch  # noqa: F401  (first, as conftest.py: one HIP runtime for both)
    except ImportError:
        pass
    _record(sys.argv[1] if len(sys.argv) > 1 else FIXTURE)
