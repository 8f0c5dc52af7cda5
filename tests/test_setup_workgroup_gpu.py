"""Set-up and operand records of a large gradient call in one launch, a workgroup per tree
(`setup_wg_kernel`, libsbn_amd/csrc/kernels_walk3.hip): beyond the one-launch
call's batch size the tree set-up launch and the record launch are replaced by one kernel whose
four waves build the tree and the model instance side by side and then write a quarter of the
tree's (node, category) records each, staged through LDS in passes.  The device functions are
those of the two launches, so every output must be BIT-IDENTICAL to an engine created with
`MI_PHYLO_SETUP_RECORDS=0`, and the path string must name the route on both sides.

The route is the default where a tree has more than 64 rows of records ((N - 1) K > 64); small
batches reach it through `MI_PHYLO_FUSED_MAX_TREES=8`.  Shapes on the kernel's edges (rows per
wave = a quarter of the rows, rounded up; rows per pass = what 40 KB of LDS allow):
  10 taxa x 4 categories   72 rows, 18 per wave, one pass
  17 x 4                  128 rows, 32 per wave: two full passes of 16
  32 x 4                  248 rows (63 nodes, the largest tree the route takes): three passes
  32 x 2, 22 x 3          two and three categories (31 and 32 rows per wave, two passes)
  27 x 4 at 520 trees     the first size above the one-launch call, no switch set
each with 13 and 16 trees (a last group of fewer than eight trees, and none), rescaling off and on.
"""
import numpy as np
import pytest

import oracle_lib as O
import tree_utils as TU
from test_gpu_parity import _params

pytestmark = pytest.mark.gpu

WALK = "gradient_walk_lut_kernel"
NEW, OLD, QUARTERS = "setup=workgroup-records", "setup=own-launch", "setup=with-records"
SWITCHES = ("MI_PHYLO_SETUP_RECORDS", "MI_PHYLO_FUSED_MAX_TREES", "MI_PHYLO_FUSED_SETUP", "MI_PHYLO_FUSE_FINALIZE")


def _engine(monkeypatch, subst, site, tips, w, **env):
    """An engine created under exactly these switches (they are read at creation)."""
    import libsbn_amd as L
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    eng = L.Engine(L.PhyloModelSpecification(subst, site, "strict"), tips, w)
    for name in env:
        monkeypatch.delenv(name)
    return eng


def _pair(monkeypatch, subst, site, tips, w, small=True):
    """(engine with the switch unset, engine with MI_PHYLO_SETUP_RECORDS=0)"""
    env = {"MI_PHYLO_FUSED_MAX_TREES": "8"} if small else {}
    return (_engine(monkeypatch, subst, site, tips, w, **env),
            _engine(monkeypatch, subst, site, tips, w, MI_PHYLO_SETUP_RECORDS="0", **env))


def _flat(grads):
    out = [np.array([g.log_likelihood for g in grads])]
    for k in sorted(grads[0].gradient):
        out.append(np.stack([np.atleast_1d(g.gradient[k]) for g in grads]).ravel())
    return np.concatenate(out)


def _inputs(n, P, T, site, seed, subst="JC69"):
    rng = np.random.default_rng(seed)
    tips, w = TU.random_alignment(n, P, rng, gap_fraction=0.05)
    pids, bls = TU.random_trees(n, T, rng, mean_bl=0.07)
    spec = O.make_spec(n, P, subst, site, "strict")
    blocks = {"Weibull shape": rng.uniform(0.4, 1.5, size=(T, 1))}
    if subst == "GTR":
        blocks["GTR rates"], blocks["frequencies"] = TU.random_gtr_params(T, rng)
    return tips, w, pids, bls, _params(spec, T, **blocks)


def _same(new, ref, call, token=NEW):
    a = call(new)
    assert new.last_call_info()[0] == WALK and token in new.last_call_path(), new.last_call_path()
    b = call(ref)
    assert ref.last_call_info()[0] == WALK and OLD in ref.last_call_path(), ref.last_call_path()
    a, b = _flat(a), _flat(b)
    assert np.isfinite(a).all() and np.array_equal(a, b)
    return a


@pytest.mark.parametrize("n,K", [(10, 4), (17, 4), (32, 4), (32, 2), (22, 3)])
def test_shapes_on_the_edges_equal_the_two_launches(monkeypatch, n, K):
    tips, w, pids, bls, pr = _inputs(n, 41, 16, f"weibull+{K}", seed=100 * n + K)
    new, ref = _pair(monkeypatch, "JC69", f"weibull+{K}", tips, w)
    for T in (13, 16):
        for rescaling in (False, True):
            _same(new, ref, lambda e: e.gradients(pids[:T], bls[:T], pr[:T], rescaling))
    new.close(); ref.close()


def test_first_size_above_the_one_launch_call_with_no_switch_set(monkeypatch):
    T = 520
    tips, w, pids, bls, pr = _inputs(27, 40, T, "weibull+4", seed=27)
    new, ref = _pair(monkeypatch, "JC69", "weibull+4", tips, w, small=False)
    for rescaling in (False, True):
        _same(new, ref, lambda e: e.gradients(pids, bls, pr, rescaling))
    new.close(); ref.close()


def test_rooted_strict_clock_call(monkeypatch):
    n, P, T = 14, 40, 13
    rng = np.random.default_rng(14)
    tips, w = TU.random_alignment(n, P, rng)
    trees = [TU.clocklike_rooted_tree(n, rng) for _ in range(T)]
    pids = np.stack([t[0] for t in trees]); bls = np.stack([t[1] for t in trees])
    state = [O.time_tree_init(n, t[0], t[1], t[2]) for t in trees]
    h = np.stack([s[0] for s in state]); bd = np.stack([s[1] for s in state]); ra = np.stack([s[2] for s in state])
    rates = np.full((T, 2 * n - 2), 0.7)
    spec = O.make_spec(n, P, "JC69", "weibull+4", "strict")
    pr = _params(spec, T, **{"Weibull shape": rng.uniform(0.4, 1.5, size=(T, 1))})
    new, ref = _pair(monkeypatch, "JC69", "weibull+4", tips, w)
    _same(new, ref, lambda e: e.rooted_gradients(pids, bls, pr, rates, np.ones(T, np.int32), h, bd, ra))
    assert "rooted" in new.last_call_path()
    new.close(); ref.close()


def test_gtr_call_for_the_branch_length_gradient_only(monkeypatch):
    """(the light path: one evaluation and one model instance per tree, the eigensystem by one
    lane of the model wave)"""
    tips, w, pids, bls, pr = _inputs(14, 40, 13, "weibull+4", seed=5, subst="GTR")
    new, ref = _pair(monkeypatch, "GTR", "weibull+4", tips, w)
    _same(new, ref, lambda e: e.gradients(pids, bls, pr, gradient_blocks=("branch_lengths",)))
    assert "light" in new.last_call_path()
    new.close(); ref.close()


def test_a_bad_tree_is_named_and_the_engine_stays_usable(monkeypatch):
    tips, w, pids, bls, pr = _inputs(14, 40, 13, "weibull+4", seed=6)
    new, ref = _pair(monkeypatch, "JC69", "weibull+4", tips, w)
    good = _same(new, ref, lambda e: e.gradients(pids, bls, pr))
    bad = pids.copy()
    bad[6, 5] = 2  # a tip as a parent, in a middle tree
    msgs = []
    for eng in (new, ref):
        with pytest.raises(RuntimeError) as err:
            eng.gradients(bad, bls, pr)
        msgs.append(str(err.value))
    assert "(tree 6)" in msgs[0] and msgs[0] == msgs[1]
    assert NEW in new.last_call_path()
    assert np.array_equal(_flat(new.gradients(pids, bls, pr)), good)
    new.close(); ref.close()


@pytest.mark.parametrize("n", [9, 5])
def test_trees_of_at_most_64_rows_keep_the_two_launches(monkeypatch, n):
    """9 taxa x 4 categories: 64 rows, 5 x 4: 32 -- nothing set: the two launches; the new value
    of the switch takes the workgroup kernel there too (16 and 8 rows per wave), same bits."""
    T = 520
    tips, w, pids, bls, pr = _inputs(n, 9, T, "weibull+4", seed=n)
    dflt = _engine(monkeypatch, "JC69", "weibull+4", tips, w)
    forced = _engine(monkeypatch, "JC69", "weibull+4", tips, w, MI_PHYLO_SETUP_RECORDS="wg")
    quarters = _engine(monkeypatch, "JC69", "weibull+4", tips, w, MI_PHYLO_SETUP_RECORDS="1")
    _same(forced, dflt, lambda e: e.gradients(pids, bls, pr))
    _same(quarters, dflt, lambda e: e.gradients(pids, bls, pr), token=QUARTERS)
    for e in (dflt, forced, quarters):
        e.close()


def test_ds1_1000_trees_take_the_route_by_default(monkeypatch):
    """The headline shape: DS1 (27 taxa, 208 rows of records per tree) x 1000 trees, nothing set."""
    st = O.load_struct("ds1_top100")
    tips, w, pids, _ = O.struct_arrays(st)
    T = 1000
    pids = np.ascontiguousarray(np.tile(pids, ((T + len(pids) - 1) // len(pids), 1))[:T])
    rng = np.random.default_rng(1000)
    bls = rng.exponential(0.1, size=(T, pids.shape[1] + 1))
    bls[:, -1] = 0
    spec = O.make_spec(27, tips.shape[1], "JC69", "weibull+4", "strict")
    pr = _params(spec, T, **{"Weibull shape": rng.uniform(0.3, 2.0, size=(T, 1))})
    new, ref = _pair(monkeypatch, "JC69", "weibull+4", tips, w, small=False)
    _same(new, ref, lambda e: e.gradients(pids, bls, pr))
    new.close(); ref.close()
