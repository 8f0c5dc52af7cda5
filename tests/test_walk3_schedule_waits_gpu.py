"""The look-up walk's schedule words (kernels_walk3.hip, walk_lut_body): every visit loads slot
numbers and the shape of a visit two or three ahead from the tree's macro list -- the post-order
walk at a visit's top, the pre-order walk at its end --, the indices clamped at both ends of the
list, and hands the shapes on through a ring of registers; the last pre-order visit requests no
operands.  None of that may change a number: every output of
`gradients` is compared BIT FOR BIT with the same engine under MI_PHYLO_GRADIENT_WALK=v2 (the
rule of test_gpu_parity.py::test_walk_kernels_agree) and with the CPU oracle at 1e-10.

The shapes sit where rings and clamps go wrong: few macros.  With M macros the walk has
M1 = M - 1 visits besides the root's, and M1 = 0, 1, 2, 3 take the prologue's clamps, the loops'
early ends and the odd / even hand-over of the two operand sets in every combination; the
27-taxon trees give one even and one odd larger value.  The macro counts are computed here on the
CPU by the set-up's rule (mi_phylo_setup_device.h, small_tree_build: children by largest leaf id,
the unrooted root split in two, an internal node is UNSTORED iff each child is a tip or a stored
node, a macro is a stored node or the root) and asserted, so that other trees or another rule
cannot hollow the cases out.  (By that rule M1 = 3 needs eight taxa -- every stored node below
the root has an unstored child of its own -- so an 8-taxon batch stands beside the 4 to 7 taxa.)
"""
import contextlib
import os

import numpy as np
import pytest

import oracle_lib as O
import tree_utils as TU
from test_gpu_parity import _params

gpu = pytest.mark.gpu

FUSED = "gradient_walk_lut_fused_kernel"
PLAIN = "gradient_walk_lut_kernel"
V2 = "gradient_walk_kernel"
_SWITCHES = ("MI_PHYLO_GRADIENT_WALK", "MI_PHYLO_FUSED_SETUP", "MI_PHYLO_GRADIENT_STORE",
             "MI_PHYLO_WALK_TILE_REGS", "MI_PHYLO_WALK3_K1", "MI_PHYLO_WALK3_ARENA",
             "MI_PHYLO_SUBST_GRADIENT", "MI_PHYLO_GRADIENT_PATH")


@contextlib.contextmanager
def _switches(**kw):
    """(an engine reads its switches once, when it is created)"""
    old = {k: os.environ.pop(k, None) for k in _SWITCHES}
    try:
        os.environ.update({"MI_PHYLO_" + k: v for k, v in kw.items()})
        yield
    finally:
        for k in _SWITCHES:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


def macro_count(n, parent_ids):
    """Macros of an unrooted tree as the device set-up forms them (module docstring)."""
    N = 2 * n - 1
    root_in = N - 2
    kids = {}
    for v, p in enumerate(parent_ids):
        kids.setdefault(int(p), []).append(v)
    maxleaf = {v: v for v in range(n)}
    child = {}
    for v in range(n, root_in + 1):
        maxleaf[v] = max(maxleaf[c] for c in kids[v])
        child[v] = sorted(kids[v], key=lambda c: maxleaf[c])
    k0, k1, k2 = child[root_in]
    child[root_in] = [k1, k2]
    child[N - 1] = [k0, root_in]
    stored = {}
    for v in range(n, N - 1):
        stored[v] = not all(c < n or stored[c] for c in child[v])
    return 1 + sum(stored.values())


def _topologies(n):
    """Three unrooted topologies on n taxa and their M1 (checked by the tests)."""
    if n == 4:    # ((0,1),2,3) as _polish numbers it: one macro; the balanced one: two
        return [TU.ladder_topology(4), TU.balanced_topology(4), TU.ladder_topology(4)], [0, 1, 0]
    rng = np.random.default_rng(100 + n)
    want = {5: [1, 1, 1], 6: [1, 2, 2], 7: [2, 1, 2], 8: [3, 2, 3], 27: [12, 11, 9], 36: [16, 11, 13]}[n]
    named = [TU.ladder_topology(n), TU.balanced_topology(n)]
    out = []
    for m1 in want:
        pick = next((p for p in named if macro_count(n, p) - 1 == m1), None)
        for _ in range(2000):
            if pick is not None:
                break
            p = TU.random_topology(n, rng)
            if macro_count(n, p) - 1 == m1:
                pick = p
        assert pick is not None, (n, m1)
        out.append(pick)
    return out, want


def test_macro_counts_of_the_cases():
    """(runs no kernel: the trees of this file have the macro counts its cases are named for)"""
    seen = set()
    for n in (4, 5, 6, 7, 8, 27, 36):
        pids, want = _topologies(n)
        got = [macro_count(n, p) - 1 for p in pids]
        assert got == want, (n, got, want)
        if n != 36:
            seen.update(got)
    assert {0, 1, 2, 3} <= seen
    assert any(m > 3 and m % 2 for m in seen) and any(m > 3 and m % 2 == 0 for m in seen)
    # the rule itself, on trees small enough to do by hand: a cherry below the split root is the
    # only macro; two cherries and the root's half make two
    assert macro_count(4, TU.ladder_topology(4)) == 1
    assert macro_count(4, TU.balanced_topology(4)) == 2


@gpu
def test_macro_counts_are_the_device_set_up_s(tmp_path):
    """macro_count() above restates the rule; this ties it to the device: the engine's tree set-up
    launcher (tests/cpp/tree_setup_compare.hip dumps what it produced) gives the same macro count
    for every tree of this file."""
    import subprocess
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(repo, "libsbn_amd")
    exe = tmp_path / "tree_setup_compare"
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-Wno-unused-result",
                    os.path.join(repo, "tests/cpp/tree_setup_compare.hip"),
                    "-L" + lib, "-lmi_phylo", "-Wl,-rpath," + lib, "-o", str(exe)], check=True)
    env = {k: v for k, v in os.environ.items() if k not in ("MI_PHYLO_TREE_SETUP", "MI_PHYLO_MACRO_SLOTS")}
    for n in (4, 5, 6, 7, 8, 27, 36):
        pids, want = _topologies(n)
        trees, out = tmp_path / f"trees_{n}.bin", tmp_path / f"dump_{n}.bin"
        np.stack(pids).astype(np.int32).tofile(trees)
        r = subprocess.run([str(exe), str(n), str(len(pids)), str(trees), str(out), "0"], env=env,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        dump = np.fromfile(out, dtype=np.int32)
        assert dump[0] == 0, (n, dump[:2])
        assert list(dump[2:2 + len(pids)] - 1) == want, (n, dump[2:2 + len(pids)], want)


def _flat(grads):
    out = [np.array([g.log_likelihood for g in grads])]
    for k in sorted(grads[0].gradient):
        out.append(np.stack([np.atleast_1d(g.gradient[k]) for g in grads]).ravel())
    return np.concatenate(out)


def _case(n, P, site, seed):
    rng = np.random.default_rng(seed)
    tips, w = TU.random_alignment(n, P, rng)
    pids, want = _topologies(n)
    assert [macro_count(n, p) - 1 for p in pids] == want
    pids = np.stack(pids)
    bls = rng.exponential(0.08, size=(len(pids), 2 * n - 2))
    bls[:, -1] = 0.0
    spec = O.make_spec(n, P, "JC69", site, "strict")
    blocks = {} if site == "constant" else {"Weibull shape": rng.uniform(0.4, 1.5, size=(len(pids), 1))}
    return tips, w, pids, bls, spec, _params(spec, len(pids), **blocks)


def _engine(site, tips, w, **switches):
    import libsbn_amd as L
    with _switches(**switches):
        return L.Engine(L.PhyloModelSpecification("JC69", site, "strict"), tips, w)


def _check_oracle(grads, spec, tips, w, pids, bls, pr, rescaling):
    og = O.unrooted_gradients(spec, tips, w, pids, bls, pr, rescaling, 2)
    ll = np.array([g.log_likelihood for g in grads])
    assert np.allclose(ll, og["log_likelihood"], rtol=1e-10, atol=0)
    gb = np.stack([g.gradient["branch_lengths"] for g in grads])
    assert np.allclose(gb, og["branch_lengths"], rtol=0, atol=1e-10 * np.max(np.abs(gb)))


@gpu
@pytest.mark.parametrize("site", ["constant", "weibull+2", "weibull+4"])
@pytest.mark.parametrize("n", [4, 5, 6, 7, 8, 27])
def test_few_macros_bit_identical_to_second_generation(n, site):
    """T = 3 trees through the one-launch call, through the four launches and through the second
    generation's walk: one partial tile, a full one, a full one and a column; rescaled or not."""
    for P in (5, 12, 13):
        tips, w, pids, bls, spec, pr = _case(n, P, site, seed=1000 * n + P)
        fused = _engine(site, tips, w)
        plain = _engine(site, tips, w, FUSED_SETUP="0")
        second = _engine(site, tips, w, GRADIENT_WALK="v2")
        for rescaling in (False, True):
            ga = fused.gradients(pids, bls, pr, rescaling)
            a = _flat(ga)
            assert fused.last_call_info()[0] == FUSED, fused.last_call_info()
            b = _flat(plain.gradients(pids, bls, pr, rescaling))
            assert plain.last_call_info()[0] == PLAIN, plain.last_call_info()
            c = _flat(second.gradients(pids, bls, pr, rescaling))
            assert second.last_call_info()[0] == V2, second.last_call_info()
            assert np.isfinite(c).all()
            assert np.array_equal(a, c), (n, P, site, rescaling, np.max(np.abs(a - c)))
            assert np.array_equal(b, c), (n, P, site, rescaling, np.max(np.abs(b - c)))
            _check_oracle(ga, spec, tips, w, pids, bls, pr, rescaling)
        fused.close(); plain.close(); second.close()


@gpu
@pytest.mark.parametrize("rescaling", [False, True])
def test_arena_both_tile_widths(rescaling):
    """36 taxa x 13 patterns, two trees, stored vectors through the arena: the default tile width
    bit-identical to the second generation's arena walk; the wide tiles bit-identical to the same
    width with every vector in LDS (sums over patterns are formed over other tiles than at the
    default width: last bits) and within 1e-11 of the second generation.  (So at the wide width
    the only bit-exact reference is this same walk with another store -- code under test on both
    sides; the second generation has no wide tiles.  What stands against an independent
    reference there is the 1e-11 bound and the oracle; the default width is bit-exact against
    the second generation.)"""
    n, P, site = 36, 13, "weibull+4"
    tips, w, pids, bls, spec, pr = _case(n, P, site, seed=36013)
    pids, bls, pr = pids[:2], bls[:2], pr[:2]
    second = _engine(site, tips, w, GRADIENT_WALK="v2", GRADIENT_STORE="arena")
    c = _flat(second.gradients(pids, bls, pr, rescaling))
    assert second.last_call_info()[0] == V2
    narrow = _engine(site, tips, w, GRADIENT_STORE="arena", WALK_TILE_REGS="3", FUSED_SETUP="0")
    g3 = narrow.gradients(pids, bls, pr, rescaling)
    a3 = _flat(g3)
    assert narrow.last_call_info()[0] == PLAIN
    assert np.array_equal(a3, c), np.max(np.abs(a3 - c))
    wide = _engine(site, tips, w, GRADIENT_STORE="arena", WALK_TILE_REGS="4", FUSED_SETUP="0")
    g4 = wide.gradients(pids, bls, pr, rescaling)
    a4 = _flat(g4)
    assert wide.last_call_info()[0] == PLAIN
    wide_lds = _engine(site, tips, w, GRADIENT_STORE="lds", WALK_TILE_REGS="4", FUSED_SETUP="0")
    l4 = _flat(wide_lds.gradients(pids, bls, pr, rescaling))
    assert np.array_equal(a4, l4), np.max(np.abs(a4 - l4))
    assert np.allclose(a4, c, rtol=1e-11, atol=1e-12 * np.max(np.abs(c))), np.max(np.abs(a4 - c))
    _check_oracle(g3, spec, tips, w, pids, bls, pr, rescaling)
    _check_oracle(g4, spec, tips, w, pids, bls, pr, rescaling)
    for e in (second, narrow, wide, wide_lds):
        e.close()
