"""The restatement of pgd_shuffle_index and pgd_adam_gated (tests/minibatch_ref.py) and the learner's minibatch switches, without a GPU:

* the array hash is tests/policy_ref.py's scalar pgd_rng;
* the permutation is a bijection at every count tried, two epochs differ, no walk has a cap;
* uniformity: the (position, value) chi-square over 4000 epochs at c = 16, 37, 100 for three seeds lies within 4 standard deviations of
  its degrees of freedom (6 rounds: measured within 1.3);
* what shuffling is for: with 64 envs, T = 8 and 4 minibatches the strided plan gives minibatch 0 exactly 16 envs, the shuffled one more
  than half of them;
* the float64 gated Adam: skip and apply, the counters;
* PPOLearner / PPOLagLearner refuse ill-formed switches before they touch a device, and the library exports both entry points.
"""
import numpy as np
import pytest

from tests import minibatch_ref as mr
from tests import policy_ref as pr
from tests import ppo_ref as rf

BIJECTION_COUNTS = (1, 2, 3, 4, 5, 16, 17, 1025, 4099, 300001)
UNIFORM_COUNTS = (16, 37, 100)
UNIFORM_SEEDS = (11, 12, 13)
SIGMA_CAP = 4.0


def test_the_array_hash_is_the_scalar_one():
    rng = np.random.default_rng(0)
    args = rng.integers(0, 1 << 32, size=(50, 4), dtype=np.uint64)
    args[0] = (0, 0, 0, 0)
    args[1] = (0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff)
    got = mr.pgd_rng(args[:, 0], args[:, 1], args[:, 2], args[:, 3])
    for row, g in zip(args, got):
        assert int(g) == pr.pgd_rng(*[int(x) for x in row])


@pytest.mark.parametrize("c", BIJECTION_COUNTS)
def test_bijection(c):
    for seed, epoch in ((0, 0), (11, 3), (0xffffffff, 0xfffffffe)):
        p, steps = mr.walk(np.arange(c), c, seed, epoch)
        assert p.min() == 0 and p.max() == c - 1 and np.array_equal(np.sort(p), np.arange(c)), (c, seed, epoch)
        assert steps < 64, "a walk of %d steps at c = %d: the domain is below 2 c (4 for c <= 2)" % (steps, c)
    bl, br = mr.widths(c)
    assert (1 << (bl + br)) >= c and ((1 << (bl + br)) < 2 * c or c <= 2) and br - bl in (0, 1)


def test_widths_and_the_epoch_rule():
    assert mr.widths(1) == (1, 1) and mr.widths(4) == (1, 1) and mr.widths(5) == (1, 2) and mr.widths(16) == (2, 2) and mr.widths(17) == (2, 3)
    assert np.array_equal(mr.permutation(37, 5, 3, 4), mr.permutation(37, 5, 7))
    assert np.array_equal(mr.permutation(37, 5, 3, -1), mr.permutation(37, 5, 2))  # (uint32)*d_epoch: the sum wraps
    assert np.array_equal(mr.permutations(37, 5, 9)[7], mr.permutation(37, 5, 7))
    assert mr.permutation(0, 5, 0).size == 0


@pytest.mark.parametrize("c", [16, 17, 1025, 4099])
def test_two_epochs_and_two_seeds_differ(c):
    a, b, d = mr.permutation(c, 11, 0), mr.permutation(c, 11, 1), mr.permutation(c, 12, 0)
    assert not np.array_equal(a, b) and not np.array_equal(a, d)
    assert not np.array_equal(a, np.arange(c))


@pytest.mark.parametrize("c", UNIFORM_COUNTS)
def test_uniformity_of_position_and_value(c):
    for seed in UNIFORM_SEEDS:
        z = mr.chi_square_sigmas(c, seed, epochs=4000)
        print("c = %d, seed %d: chi-square %.2f sigma from its dof" % (c, seed, z))
        assert abs(z) < SIGMA_CAP, (c, seed, z)


def test_shuffle_index_restated():
    index = np.arange(100, 120, dtype=np.int32)[::-1].copy()
    out = mr.shuffle_index(index, 7, 20, 3, 0, out=np.full(20, -9, dtype=np.int32))
    assert (out[7:] == -9).all() and sorted(out[:7]) == sorted(index[:7])
    assert np.array_equal(mr.shuffle_index(None, 50, 20, 3, 0), mr.permutation(20, 3, 0))   # the count clamps
    assert np.array_equal(mr.shuffle_index(None, -3, 20, 3, 0, out=np.full(20, -9)), np.full(20, -9))


def test_a_shuffled_minibatch_mixes_the_envs():
    """RolloutCollector's list position is t * N + env.  Strided over the list as it lies, minibatch 0 of 4 holds the 16 envs with
    env % 4 == 0; over a permutation of it, more than half of the 64."""
    from pgdrive_amd import learner
    N, T, n_mb = 64, 8, 4
    start, stride, rows = learner.minibatch_plan(T * N, n_mb)[0]
    pos = np.array(learner.live_positions(start, stride, rows, T * N))
    assert len(set(pos % N)) == 16
    for epoch in range(4):
        rows_of_mb = mr.permutation(T * N, 0, epoch)[pos]
        envs = len(set(rows_of_mb % N))
        print("epoch %d: minibatch 0 of the shuffled plan holds %d of %d envs" % (epoch, envs, N))
        assert envs > N // 2
    # the four minibatches still partition the list
    p = mr.permutation(T * N, 0, 0)
    seen = np.concatenate([p[learner.live_positions(s, st, r, T * N)] for s, st, r in learner.minibatch_plan(T * N, n_mb)])
    assert np.array_equal(np.sort(seen), np.arange(T * N))


def test_gated_adam_restated():
    rng = np.random.default_rng(1)
    p, g = rng.normal(size=9), rng.normal(size=9)
    m, v = np.zeros(9), np.zeros(9)
    hyper = dict(betas=(0.9, 0.999), eps=1e-5, max_grad_norm=0.5)
    want = rf.adam_f64(p, g, m, v, 1, 3e-4, **hyper)
    p1, m1, v1, t, gate, cg = mr.adam_gated_f64(p, g, m, v, 0, 3e-4, (0, 0, 0, 0), kl=0.01, kl_limit=0.015, count_gate=50, **hyper)
    assert t == 1 and gate == [0, 1, 0, 0] and cg == 50 and all(np.array_equal(a, b) for a, b in zip((p1, m1, v1), want))
    for kw in (dict(kl=0.016, kl_limit=0.015), dict(kl=float("nan"), kl_limit=0.015)):
        p2, m2, v2, t2, gate2, cg = mr.adam_gated_f64(p1, g, m1, v1, t, 3e-4, gate, count_gate=50, **kw, **hyper)
        assert t2 == 1 and gate2 == [1, 1, 1, 1] and cg == 0 and p2 is p1 and m2 is m1 and v2 is v1
    _, _, _, t3, gate3, cg = mr.adam_gated_f64(p1, g, m1, v1, t, 3e-4, (1, 1, 1, 1), kl=0.0, kl_limit=0.015, **hyper)   # shut stays shut
    assert t3 == 1 and gate3 == [1, 1, 2, 1] and cg is None
    half = mr.adam_gated_f64(p, g, m, v, 0, 3e-4, (0, 0, 0, 0), lr_scale=0.5, **hyper)
    assert np.array_equal(half[0], rf.adam_f64(p, g, m, v, 1, float(np.float32(3e-4) * np.float32(0.5)), **hyper)[0])


@pytest.mark.parametrize("bad", [dict(shuffle="yes"), dict(shuffle=2), dict(shuffle_seed=-1), dict(shuffle_seed=1 << 32), dict(shuffle_seed=1.5),
                                 dict(target_kl=0.0), dict(target_kl=-0.01), dict(target_kl=float("nan")), dict(target_kl=float("inf")),
                                 dict(lr_scale=0.5), dict(lr_scale=None)])
def test_learners_refuse_ill_formed_switches_before_they_touch_a_device(bad):
    from pgdrive_amd import _abi
    from pgdrive_amd.learner import PPOLagLearner, PPOLearner, minibatch_options
    with pytest.raises(ValueError, match=list(bad)[0]):
        PPOLearner(None, **bad)
    with pytest.raises(ValueError, match="PPOLagLearner"):
        PPOLagLearner(None, 1.0, **bad)
    assert minibatch_options("x", False, 0, None, False) == (False, 0, None, False)
    assert minibatch_options("x", True, 7, 0.01, True) == (True, 7, 1.5 * 0.01, True)
    assert _abi.ADAM_GATE == mr.GATE


def test_the_library_exports_both_entry_points():
    import ctypes as C
    from pgdrive_amd import build, engine
    build.build()
    L = engine.load_library()
    assert "pgd_shuffle_index" in engine.EXPORTS and "pgd_adam_gated" in engine.EXPORTS
    # refusals that need no device: a null handle
    out = (C.c_int32 * 4)()
    assert L.pgd_shuffle_index(None, None, None, 4, 0, 0, None, C.cast(out, C.c_void_p)) == 1
    assert L.pgd_adam_gated(None, None, None, None, None, 1, None, 3e-4, 0.9, 0.999, 1e-5, 0.5, None, None, 0.0, None, None) == 1
