"""CPU checks of the reference values the GPU tests of the branch-length Hessian call use
(tests/hessian_fd.py): the three-taxon closed form against the oracle, and the oracle's
finite-difference Hessian against the closed form."""
import numpy as np

import hessian_fd as H
import oracle_lib as O


def _star(P=40, seed=0):
    rng = np.random.default_rng(seed)
    tips = rng.integers(0, 5, size=(3, P)).astype(np.int32)
    w = rng.integers(1, 4, size=P).astype(float)
    pids = np.array([[3, 3, 3]], np.int32)
    bls = np.array([[0.07, 0.21, 0.33, 0.0]])
    return tips, w, pids, bls


def test_star_tree_closed_form_matches_oracle():
    tips, w, pids, bls = _star()
    ll, g, h, sq = H.jc69_star_tree(tips, w, bls[0, :3])
    spec = O.make_spec(3, tips.shape[1], "JC69", "constant")
    pr = np.zeros((1, O.param_count(spec)))
    og = O.unrooted_gradients(spec, tips, w, pids, bls, pr, False, 1)
    assert abs(og["log_likelihood"][0] - ll) <= 1e-12 * abs(ll)
    assert np.allclose(og["branch_lengths"][0, :3], g, rtol=1e-11, atol=0)
    assert np.all(og["branch_lengths"][0, 3:] == 0)
    assert np.all(sq > 0) and np.all(h < sq)


def test_oracle_finite_differences_match_closed_form():
    tips, w, pids, bls = _star(seed=1)
    _, _, h, _ = H.jc69_star_tree(tips, w, bls[0, :3])
    spec = O.make_spec(3, tips.shape[1], "JC69", "constant")
    pr = np.zeros((1, O.param_count(spec)))
    fd = H.fd_hessian_diagonal(spec, tips, w, pids, bls, pr)
    assert fd.shape == (1, 5)
    assert np.max(np.abs(fd[0, :3] - h)) <= 1e-6 * np.max(np.abs(h))
    assert np.all(fd[0, 3:] == 0)
