"""The host forms of the DAG's tree calls, of the pieces of a rooted variational step and of de-rooting as
calls of the host-call layer, on the five-taxon golden DAG: a refused sample is delivered
with its error, the engine's staging blocks regrow and are used again, optional arrays change nothing
else, a host form reports its own errors only, and a failed training leaves q alone.  The C ABI is called
through ctypes where the Python wrappers always pass an array or raise before they return one."""
import re

import numpy as np
import pytest

import gp_ref as GR
import gp_trees_ref as TR
import tree_utils as TU

pytestmark = pytest.mark.gpu
_CASE = {}


def _p(a):
    from libsbn_amd.engine import _ptr
    return _ptr(a)


def _five():
    if not _CASE:
        pids, bls, tips, w, _ = GR.load_case("five_taxon_rooted.nwk", "five_taxon.fasta")
        _CASE.update(pids=pids, bls=bls, tips=tips, w=w, d=GR.build_dag(pids))
    return _CASE


def _fresh():
    """a new engine and a DAG-only object on it: their staging blocks have served nothing yet"""
    import libsbn_amd as L
    c = _five()
    eng = L.Engine(L.PhyloModelSpecification("JC69", "constant", "strict"), c["tips"], c["w"], device=0)
    return eng, eng.gp_create_dag(c["pids"], c["bls"])


def _on_fresh(call):
    eng, gp = _fresh()
    out = call(eng, gp)
    gp.close()
    eng.close()
    return out


def _bytes(x):
    if isinstance(x, np.ndarray):
        return x.tobytes()
    if isinstance(x, (tuple, list)):
        return [_bytes(y) for y in x]
    return [None if v is None else v.tobytes() for v in vars(x).values()]


def _sample(gp, K, bl=True, cdf=True, seed=4, fill=None):
    """mi_gp_sample_trees through ctypes: (rc, parent_ids, entries, log_q, branch_lengths or None, cdf or None)"""
    N = 2 * gp.taxon_count - 1
    pid, ent, lq = np.zeros((K, N - 1), np.int32), np.zeros((K, N), np.int32), np.zeros(K)
    lengths, c = (np.zeros((K, N)) if bl else None), (np.zeros(gp.entry_count) if cdf else None)
    if fill is not None:
        for a, value in zip((pid, ent, lq, lengths), fill):
            a[...] = value
    rc = gp._lib.mi_gp_sample_trees(gp._h, K, seed, 0, _p(pid), _p(ent), _p(lq), _p(lengths), _p(c))
    return rc, pid, ent, lq, lengths, c


def test_a_refused_sample_is_delivered_with_its_error():
    """include/mi_phylo.h: a sample that meets a block of zeros has integer outputs -1, log q and lengths NaN"""
    from libsbn_amd import _capi
    eng, gp = _fresh()
    d = _five()["d"]
    gp.set_sbn_parameters(np.where(np.arange(d.G) < d.R, 0.0, gp.get_sbn_parameters()))
    # (markers that no sample has: an id of a million, a positive log q, a negative length)
    rc, pid, ent, lq, lengths, _ = _sample(gp, 3, cdf=False, fill=(10 ** 6, 10 ** 6, 5.0, -5.0))
    assert rc != 0 and re.search(r"all 0 \(sample [012], the rootsplits\)", _capi.last_error())
    assert np.all(pid == -1) and np.all(ent == -1) and np.all(np.isnan(lq)) and np.all(np.isnan(lengths))
    eng.check_status()   # (reported once)
    gp.close()
    eng.close()


def test_the_staging_blocks_regrow_and_are_used_again():
    c = _five()
    small, three = c["pids"][:2], np.asarray([TU.ladder_topology(3, rooted=True)], np.int32)
    many = _on_fresh(lambda eng, gp: gp.sample_trees(65, seed=4, cdf=True))
    calls = [lambda eng, gp: gp.tree_index(small),
             lambda eng, gp: gp.sample_trees(65, seed=4, cdf=True),   # (beyond one wave: both blocks regrow)
             lambda eng, gp: gp.tree_index(small),
             lambda eng, gp: eng.deroot_trees_mapped(three, np.array([[0.1, 0.2, 0.3, 0.4, 0.0]])),
             lambda eng, gp: eng.deroot_trees_mapped(three),
             lambda eng, gp: eng.deroot_trees_mapped(many.parent_ids, many.branch_lengths),
             lambda eng, gp: eng.deroot_trees_mapped(many.parent_ids)]
    eng, gp = _fresh()
    for i, call in enumerate(calls):
        assert _bytes(call(eng, gp)) == _bytes(_on_fresh(call)), i
    gp.close()
    eng.close()


def test_optional_arrays_change_nothing_else():
    """every optional array absent and present: the required outputs have the same bytes (branch_sample's
    epsilon: tests/test_gp_vi_gpu.py hands the draws back)"""
    c = _five()
    d, pids = c["d"], c["pids"]
    eng, gp = _fresh()
    lib, h, G, T = gp._lib, gp._h, d.G, len(pids)
    N = 2 * d.n - 1
    # tree_index: out_nodes
    ent, ent2, nodes = np.zeros((T, N), np.int32), np.zeros((T, N), np.int32), np.zeros((T, N), np.int32)
    assert lib.mi_gp_tree_index(h, T, _p(pids), _p(ent), _p(nodes)) == 0
    assert lib.mi_gp_tree_index(h, T, _p(pids), _p(ent2), None) == 0
    assert ent.tobytes() == ent2.tobytes() == TR.index_batch(d, pids)[0].tobytes()
    # sample_trees: out_branch_lengths, out_cdf
    full, bare = _sample(gp, 7), _sample(gp, 7, bl=False, cdf=False)
    assert full[0] == 0 and bare[0] == 0 and _bytes(full[1:4]) == _bytes(bare[1:4])
    trees, lengths = full[2], full[4]
    # de-rooting: out_branch_lengths, out_new_id (the lengths given both times)
    outs = []
    for wanted in (True, False):
        pid, edge = np.zeros((7, N - 2), np.int32), np.zeros(7, np.int32)
        bl, new_id = (np.zeros((7, N - 1)), np.zeros((7, N), np.int32)) if wanted else (None, None)
        assert lib.mi_engine_deroot_trees_mapped(eng._h, 7, d.n, _p(full[1]), _p(lengths), _p(pid), _p(bl), _p(edge), _p(new_id)) == 0
        outs.append((pid, edge))
    assert _bytes(outs[0]) == _bytes(outs[1])
    un = eng.deroot_trees_mapped(full[1], lengths)
    # branch_gradient: log_q_topology (absent: 0 each), tree_weights (absent: 1 each)
    rng = np.random.default_rng(8)
    qp = np.stack([rng.normal(-2.5, 0.3, G), rng.uniform(0.1, 0.4, G)], axis=1)
    draw = gp.branch_sample(trees, qp, 3)
    g, ll = rng.normal(0.0, 30.0, (7, N)), rng.normal(-80.0, 5.0, 7)
    absent = gp.branch_gradient(trees, qp, draw, un.new_id, g, ll)
    present = gp.branch_gradient(trees, qp, draw, un.new_id, g, ll, log_q_topology=np.zeros(7), tree_weights=np.ones(7))
    assert _bytes(absent) == _bytes(present)
    # topology_gradient: out_factors
    phi, grad = rng.normal(0.0, 1.0, G), np.zeros(G)
    assert lib.mi_gp_topology_gradient(h, 7, _p(trees), _p(phi), _p(absent[1]), 1, _p(grad), None) == 0
    assert grad.tobytes() == gp.topology_gradient(trees, phi, absent[1])[0].tobytes()
    # train_simple_average: tree_weights (absent: 1 each), out_q
    q = gp.train_simple_average(trees, np.ones(7))
    assert gp.train_simple_average(trees).tobytes() == q.tobytes()
    gp.set_sbn_parameters(GR.uniform_prior(d))
    assert lib.mi_gp_train_simple_average(h, 7, _p(trees), None, None) == 0
    assert gp.get_sbn_parameters().tobytes() == q.tobytes()
    gp.close()
    eng.close()


def test_a_host_form_reports_its_own_errors_only():
    """the status word is sticky for the device forms; a host form starts from a cleared one"""
    import torch
    c = _five()
    d, pids = c["d"], c["pids"]
    eng, gp = _fresh()
    gp.reserve_trees(len(pids))
    bad = pids[:1].copy()
    bad[0, 0] = bad[0, 2] if bad[0, 0] != bad[0, 2] else bad[0, 3]
    dev = torch.tensor(bad, device="cuda:0")
    out = torch.zeros(2 * d.n - 1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    gp.tree_index_device(None, 1, dev.data_ptr(), out.data_ptr())   # (its error is left unread)
    got = gp.tree_index(pids)
    ent_ref, nodes_ref = TR.index_batch(d, pids)
    assert got.entries.tobytes() == ent_ref.tobytes() and got.nodes.tobytes() == nodes_ref.tobytes()
    eng.check_status()
    assert np.all(out.cpu().numpy() == d.G)   # (the device form did run)
    gp.close()
    eng.close()


def test_a_failed_training_leaves_q_as_it_was():
    d = _five()["d"]
    eng, gp = _fresh()
    trees = gp.sample_trees(5, seed=2).entries
    gp.set_sbn_parameters(GR.random_q(d, np.random.default_rng(3)))
    before = gp.get_sbn_parameters()
    trees[3, 1] = d.G
    with pytest.raises(RuntimeError, match=r"outside the DAG.*\(tree 3\)"):
        gp.train_simple_average(trees)
    assert gp.get_sbn_parameters().tobytes() == before.tobytes()
    gp.close()
    eng.close()
