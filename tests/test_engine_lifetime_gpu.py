"""An engine gives back every byte of device memory it took: mi_device_bytes_held, the library's
own count of what its buffers hold in this process (not the device-wide free memory, which other
users of a shared GPU change under a test), is back where it was after close() -- for an engine
that ran a call of every family that owns a workspace, a 20-state engine, a sharded handle, an
engine made from device-resident tips, and creations that fail after they have allocated."""
import gc

import numpy as np
import pytest

import aa_utils as A
import tree_utils as TU

pytestmark = pytest.mark.gpu


def _held():
    from libsbn_amd import _capi
    gc.collect()  # (engines other tests left to the collector go now, not inside a test below)
    return _capi.load().mi_device_bytes_held()


def _closes_clean(make, use):
    held = _held()
    eng = make()
    use(eng)
    assert _held() > held  # the counter moves at all
    eng.close()
    assert _held() == held


def test_every_call_family_gives_its_workspace_back():
    import libsbn_amd as L
    rng = np.random.default_rng(11)
    n, P, T = 5, 8, 2
    N = 2 * n - 1
    tips, w = TU.random_alignment(n, P, rng)
    pids, bls = TU.random_trees(n, T, rng)
    spec = L.PhyloModelSpecification("GTR", "weibull+4", "strict")

    def use(eng):
        pr = np.ones((T, eng.param_count))
        pr[:, :6], pr[:, 6:10] = TU.random_gtr_params(T, rng)
        few = {"max_iterations": 2}
        eng.log_likelihoods(pids, bls, pr)
        eng.gradients(pids, bls, pr)
        eng.gradients_reduced(pids, bls, pr, np.tile(np.arange(N, dtype=np.int32), (T, 1)), N)
        eng.branch_hessian(pids, bls, pr)
        eng.nni_scan(pids, bls, pr)
        eng.spr_scan(pids, bls, pr)
        eng.ancestral_states(pids, bls, pr)
        eng.placement(pids, bls, np.zeros((1, P), np.int8), [0.1], pr)
        eng.optimize_branch_lengths(pids, bls, pr, **few)
        eng.nni_search(pids, bls, pr, max_moves=1, branch_opt=few)
        eng.spr_search(pids, bls, pr, max_moves=1, branch_opt=few)
        _, s = eng.pattern_log_likelihoods(pids, bls, pr)
        replicates = L.rell_weights(w, 3, 5)
        eng.rell(s, replicates)
        eng.rell_bootstrap(pids, bls, replicates, pr)
        eng.starting_trees(params=pr[0])
        table = eng.split_index(pids, bls)
        eng.rf_distances(table.split_index, bls)
        support = eng.sbn_index(pids)
        eng.sbn_log_prob(support, np.zeros(support.parameter_count))

    _closes_clean(lambda: L.Engine(spec, tips, w), use)


def test_other_engines_give_everything_back():
    import torch
    import libsbn_amd as L
    rng = np.random.default_rng(12)
    # 20 states, one gradient call
    tips, w = A.random_aa_alignment(12, 40, rng)
    pids, bls = TU.random_trees(12, 2, rng)
    s20 = L.PhyloModelSpecification("WAG", "weibull+4", "strict")
    _closes_clean(lambda: L.Engine(s20, tips, w), lambda e: e.gradients(pids, bls, A.params_for("weibull+4", 2, rng)))
    # a tree-sharded handle of two logical shards on one device; device-resident tips
    tips4, w4 = TU.random_alignment(5, 8, rng)
    p4, b4 = TU.random_trees(5, 2, rng)
    jc = L.PhyloModelSpecification("JC69", "weibull+4", "strict")
    pr = np.ones((2, 2))
    _closes_clean(lambda: L.Engine(jc, tips4, w4, shard_devices=[0, 0]), lambda e: e.gradients(p4, b4, pr))
    d_t, d_w = torch.from_numpy(tips4).to("cuda:0"), torch.from_numpy(w4).to("cuda:0")
    _closes_clean(lambda: L.Engine(jc, None, None, device_tips=(d_t.data_ptr(), d_w.data_ptr(), 5, 8)),
                  lambda e: e.log_likelihoods(p4, b4, pr))
    # creations that fail after they have allocated: nothing of the half-made engine stays
    held = _held()
    partials = np.zeros((12, 40, 20))
    partials[..., 0] = 1.0
    partials[3, 7, :] = 0.5
    with pytest.raises(RuntimeError, match="one-hot"):
        L.Engine(s20, None, w, use_tip_states=False, tip_partials=partials)
    host = np.ascontiguousarray(tips4)
    with pytest.raises(RuntimeError, match="device memory"):
        L.Engine(jc, None, None, device_tips=(host.ctypes.data, d_w.data_ptr(), 5, 8))
    assert _held() == held
