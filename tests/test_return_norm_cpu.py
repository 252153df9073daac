"""Reward scaling by the running return without a GPU: the float64 checker of pgd_return_norm (tests/return_norm_ref.py) against a
step-by-step restatement of VecNormalize's rule and against numpy; its flag form (NaN, seats that change hands); the frozen mode; the
header and the refusals that need no device; and the host logic of the three collectors on a recording engine -- with the switch off
exactly today's calls and batch keys, with it on one return_norm call in front of the same GAE call."""
import os
import re

import numpy as np
import pytest

from tests import actor_critic_ref as ar
from tests import marl_rollout_ref as mr
from tests import return_norm_ref as rn
from tests.recording_engine import CALLS, PRIME, T, TODAY, TODAY_MARL, TODAY_SAFE, collector as _collector

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


# ---------------------------------------------------------------------------------------------------------------------
# the checker
# ---------------------------------------------------------------------------------------------------------------------
def test_the_batch_checker_is_vecnormalize_with_the_final_scale():
    """One call over [T, N] == RunningMeanStd updated step by step over the envs, every step scaled by the final variance: Chan's merge is
    associative up to rounding (1e-12), and the float32 scaled rewards agree to 1 ulp (the scale may round the other way)."""
    rng = np.random.default_rng(0)
    for T, N, gamma in ((1, 1, 0.99), (7, 5, 0.99), (33, 64, 0.9), (128, 16, 0.99)):
        reward = rng.normal(size=(T, N)) * 3.0 + 0.5
        done = (rng.uniform(size=(T, N)) < 0.1).astype(np.uint8)
        got = rn.return_norm_f64(reward, done, gamma, np.zeros(N), rn.RECORD_INIT, eps=1e-8, clip=10.0)
        want, (count, mean, var) = rn.vecnormalize_stepwise(reward, done, gamma, 1e-8, 10.0)
        assert got["record"][0] == count == 1e-4 + T * N
        sd = np.sqrt(var)
        assert abs(got["record"][1] - mean) <= 1e-12 * sd and _rel(got["record"][2] / count, var) < 1e-12
        assert _rel(got["record"][3], 1.0 / np.sqrt(var + 1e-8)) < 1e-12
        assert (np.abs(got["scaled"] - want) <= np.spacing(np.maximum(np.abs(got["scaled"]), np.abs(want)))).all()
        assert np.abs(got["scaled"]).max() <= 10.0


@pytest.mark.parametrize("T", rn.EXACT_T)
def test_chans_merge_over_any_split_is_numpy_on_the_concatenation(T):
    rng = np.random.default_rng(T)
    worst = 0.0
    for rows in rn.EXACT_ROWS:
        x = rng.normal(size=T * rows) * 50.0 + 200.0   # (returns in the hundreds)
        for parts in (1, 2, 3, 64, T * rows):
            cuts = np.sort(rng.integers(0, x.size + 1, size=parts - 1))   # (empty parts included)
            count, mean, m2 = 0.0, 0.0, 0.0
            for chunk in np.split(x, cuts):
                count, mean, m2 = rn.chan(count, mean, m2, *rn.moments(chunk))
            assert count == x.size
            sd = x.std()
            err = max(abs(mean - x.mean()) / max(sd, 1e-300), _rel(m2 / count, x.var()) if x.size > 1 else abs(m2))
            worst = max(worst, err)
            assert err < rn.TOL_STATS, (T, rows, parts, err)
    print("Chan's merge against numpy, T = %d: %.1e (bound %.0e)" % (T, worst, rn.TOL_STATS))


def test_the_exact_inputs_are_exact_in_float32():
    """gamma = 0.5, integer rewards, an integer carry: the float32 recursion gives the float64 one's values at every shape of the GPU
    test, so the device's carry must equal the checker's bit for bit."""
    for T in rn.EXACT_T:
        for rows in rn.EXACT_ROWS:
            for dones in ("some", "all", "none"):
                reward, done = rn.exact_case(T, rows, dones)
                carry = np.random.default_rng(rows).integers(-4, 5, size=rows).astype(np.float64)
                R64, s64, c64 = rn.running_returns(reward, done, rn.EXACT_GAMMA, carry)
                R32, s32, c32 = rn.running_returns(reward, done, rn.EXACT_GAMMA, carry, fp32=True)
                assert np.array_equal(R64, R32) and np.array_equal(c64, c32.astype(np.float64)) and s64.all() and s32.all()
                assert np.array_equal(R64.astype(np.float32).astype(np.float64), R64)


def test_a_nan_at_a_row_that_did_not_act_reaches_nothing():
    rng = np.random.default_rng(1)
    T, rows = 16, 37
    flags, done = rn.seat_history(rng, T, rows)
    reward = rng.normal(size=(T, rows)).astype(np.float32)
    clean = rn.return_norm_f64(np.where(rn.acted(flags), reward, 0.0), done, 0.99, np.zeros(rows), rn.RECORD_INIT, flags=flags)
    reward[~rn.acted(flags)] = np.nan
    assert np.isnan(reward).sum() > 50
    got = rn.return_norm_f64(reward, done, 0.99, np.zeros(rows), rn.RECORD_INIT, flags=flags)
    for key in ("carry", "record", "scaled", "samples"):
        assert np.isfinite(got[key]).all() and np.array_equal(got[key], clean[key]), key
    assert (got["scaled"][~rn.acted(flags)] == 0).all() and got["record"][0] == 1e-4 + rn.acted(flags).sum()


def test_a_seat_that_changes_hands_starts_from_zero():
    """One seat: an agent acts twice, the seat is empty for a step, the next agent acts; then an env-wide restart (PGD_F_RESET without
    done) cuts an agent, and a done ends one."""
    A, N_, X = rn.F_REPORT, rn.F_REPORT | (1 << 18), rn.F_REPORT | rn.F_RESET
    flags = np.array([A, A, 0, N_, X, A, A], dtype=np.int32)[:, None]
    done = np.array([0, 0, 0, 0, 0, 1, 0], dtype=np.uint8)[:, None]
    reward = np.array([1, 2, 100, 4, 8, 16, 32], dtype=np.float32)[:, None]
    R, sampled, carry = rn.running_returns(reward, done, 0.5, np.array([6.0]), flags)
    assert sampled[:, 0].tolist() == [True, True, False, True, True, True, True]
    # 0.5 * 6 + 1;  0.5 * 4 + 2;  (empty: no sample, R = 0);  4;  0.5 * 4 + 8, cut by the restart;  16, done;  32
    assert R[:, 0].tolist() == [4.0, 4.0, 0.0, 4.0, 10.0, 16.0, 32.0] and carry.tolist() == [32.0]
    got = rn.return_norm_f64(reward, done, 0.5, np.array([6.0]), rn.RECORD_INIT, flags=flags, clip=0.0)
    assert got["record"][0] == 1e-4 + 6 and got["scaled"][2, 0] == 0.0 and (got["scaled"][[0, 1, 3, 4, 5, 6], 0] != 0).all()


def test_the_frozen_mode_writes_nothing_but_scaled():
    rng = np.random.default_rng(2)
    T, rows = 9, 11
    reward, done = rng.normal(size=(T, rows)).astype(np.float32), (rng.uniform(size=(T, rows)) < 0.2).astype(np.uint8)
    carry, record = rng.normal(size=rows), np.array([37.0001, 1.5, 400.0, 0.25])
    got = rn.return_norm_f64(reward, done, 0.99, carry, record, freeze=True, clip=0.5)
    assert np.array_equal(got["carry"], carry) and np.array_equal(got["record"], record)
    assert np.array_equal(got["scaled"], np.clip(reward * np.float32(0.25), -0.5, 0.5))
    moved = rn.return_norm_f64(reward, done, 0.99, carry, record, clip=0.5)
    assert moved["record"][0] == 37.0001 + T * rows and not np.array_equal(moved["carry"], carry)


def test_a_call_without_a_sample_keeps_count_mean_and_m2():
    T, rows = 4, 6
    flags, done = np.zeros((T, rows), np.int32), np.zeros((T, rows), np.uint8)
    record = np.array([12.5, -3.0, 77.0, 123.0])
    got = rn.return_norm_f64(np.full((T, rows), np.nan, np.float32), done, 0.99, np.ones(rows), record, flags=flags, eps=1e-8)
    assert np.array_equal(got["record"][:3], record[:3]) and got["record"][3] == 1.0 / np.sqrt(77.0 / 12.5 + 1e-8)
    assert (got["carry"] == 0).all() and (got["scaled"] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# the header, the exports, what is refused without a device
# ---------------------------------------------------------------------------------------------------------------------
def test_the_header_states_the_rule_and_declares_the_entry_points():
    from pgdrive_amd import _abi, engine
    text = open(os.path.join(ROOT, "include", "pgdrive_hip.h")).read()
    for line in ("delta = bmean - mean;  tot = count + n;  mean += delta n / tot;  m2 += bm2 + delta^2 count n / tot;  count = tot",
                 "scale = 1 / sqrt(m2 / count + eps)", "scaled[t][r] = clamp(reward[t][r] * (float)scale, -clip, clip)", "UPDATED scale"):
        assert line in text, line
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+pgd_return_norm\s*\(", src) and re.search(r"\bsize_t\s+pgd_return_norm_work_bytes\s*\(", src)
    assert "pgd_return_norm" in engine.EXPORTS and "pgd_return_norm_work_bytes" in engine.EXPORTS
    assert re.search(r"#define\s+PGD_RN_FREEZE\s+1u", text) and _abi.RN_FREEZE == 1
    assert _abi.RETURN_NORM_RECORD == ("count", "mean", "m2", "scale") and _abi.RETURN_NORM_INIT == rn.RECORD_INIT
    for doc, what in (("DESIGN.md", "\n## 25. "), ("README.md", "normalise_rewards")):
        assert what in open(os.path.join(ROOT, doc)).read(), doc


def test_the_scratch_size_and_the_null_arguments_without_a_gpu():
    import ctypes as C
    from pgdrive_amd import engine
    L = engine.load_library()
    assert [L.pgd_return_norm_work_bytes(r) for r in (-1, 0, 1, 64, 65, 4096)] == [0, 0, 24, 24, 48, 64 * 24]
    assert L.pgd_return_norm(None, None, None, None, 1, 1, 0.99, 1e-8, 10.0, 0, None, None, None, None, C.c_size_t(0)) == 1


# ---------------------------------------------------------------------------------------------------------------------
# host logic: the collectors on a recording engine
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["single", "safe", "marl"])
def test_switch_off_the_collectors_make_todays_calls_and_todays_batch(kind):
    import inspect
    eng, col = _collector(kind)
    batch = col.collect()
    net, per_step, gae, behind = CALLS[kind]
    prime = [c % net if "%" in c else c for c in PRIME]
    if kind == "marl":
        prime = ["sync"] + prime + ["rollout_index"]
    assert eng.calls == prime + ["actor_critic_tick"] + per_step * T + ["actor_critic_tick"] + gae + behind
    assert set(batch) == dict(single=TODAY, safe=TODAY_SAFE, marl=TODAY_MARL)[kind]
    assert eng.gae_reward is col.rewards and not col.normalise_rewards and not hasattr(col, "scaled_rewards")
    assert col.state_dict() == {}
    col.load_state_dict({})
    with pytest.raises(ValueError, match="normalise_rewards=False"):
        col.load_state_dict(dict(return_norm=np.zeros(4)))
    p = inspect.signature(type(col).__init__).parameters
    assert (p["normalise_rewards"].default, p["clip_reward"].default, p["reward_eps"].default) == (False, 10.0, 1e-8)


@pytest.mark.parametrize("kind", ["single", "safe", "marl"])
def test_switch_on_one_call_in_front_of_the_same_gae_call(kind):
    """The calls, the batch's two new keys, GAE fed the scaled rewards, `rewards` raw; three rollouts equal the checker carried by hand;
    a checkpoint round trip; the frozen mode."""
    import torch
    eng, col = _collector(kind, normalise_rewards=True, clip_reward=5.0, reward_eps=1e-6)
    net, per_step, gae, behind = CALLS[kind]
    script = eng.script
    shape = script[0].shape[1:]
    carry, record = np.zeros(shape), np.array(rn.RECORD_INIT)
    for k in range(3):
        del eng.calls[:]
        batch = col.collect()
        want = ["actor_critic_tick"] + per_step * T + ["actor_critic_tick", "return_norm(freeze=False)"] + gae + behind
        assert eng.calls[-len(want):] == want and "return_norm(freeze=False)" not in eng.calls[:-len(want)]
        assert set(batch) == dict(single=TODAY, safe=TODAY_SAFE, marl=TODAY_MARL)[kind] | {"scaled_rewards", "return_norm"}
        assert eng.gae_reward is col.scaled_rewards is batch["scaled_rewards"] and batch["return_norm"] is col.return_norm
        sl = slice(k * T, (k + 1) * T)
        assert np.array_equal(batch["rewards"].numpy(), script[0][sl]), "rewards are no longer raw"
        ref = rn.return_norm_f64(script[0][sl], script[1][sl], 0.5, carry, record, flags=script[2][sl] if kind == "marl" else None, eps=1e-6, clip=5.0)
        carry, record = ref["carry"], ref["record"]
        assert np.array_equal(batch["scaled_rewards"].numpy(), ref["scaled"]) and np.array_equal(batch["return_norm"].numpy(), record)
        assert np.abs(batch["scaled_rewards"].numpy()).max() <= 5.0 and record[3] < 0.05   # (returns in the hundreds)
        if kind == "marl":
            a64, _, _ = mr.gae_masked_f64(ref["scaled"], batch["values"].numpy(), script[1][sl], script[2][sl].view(np.uint32), 0.5, 0.5)
        else:
            a64, _ = ar.gae_f64(ref["scaled"], batch["values"].numpy(), script[1][sl], 0.5, 0.5)
        assert np.array_equal(batch["advantages"].numpy(), a64.astype(np.float32))
    if kind == "safe":   # the cost side reads the flags, not the rewards: unchanged
        off_eng, off = _collector(kind)
        for k in range(3):
            b_off = off.collect()
        for key in ("costs", "cost_advantages", "cost_returns", "ep_cost_sum", "ep_cost_count"):
            assert torch.equal(b_off[key], batch[key]), key
    # a checkpoint: the state into a fresh collector, which continues as the first does
    state = col.state_dict()
    assert set(state) == {"return_norm_carry", "return_norm"} and state["return_norm"].dtype == np.float64
    assert np.array_equal(state["return_norm_carry"].reshape(shape), carry.astype(np.float32)) and np.array_equal(state["return_norm"], record)
    eng2, col2 = _collector(kind, normalise_rewards=True, clip_reward=5.0, reward_eps=1e-6)
    col2.load_state_dict(state)
    assert torch.equal(col2._rn_carry, col._rn_carry) and torch.equal(col2.return_norm, col.return_norm)
    with pytest.raises(ValueError, match="rows"):
        col2.load_state_dict(dict(return_norm_carry=np.zeros(3), return_norm=record))
    # evaluation: nothing moves
    col.freeze_return_norm(True)
    before = col._rn_carry.clone(), col.return_norm.clone()
    batch = col.collect()
    assert "return_norm(freeze=True)" in eng.calls and torch.equal(col._rn_carry, before[0]) and torch.equal(col.return_norm, before[1])
    r0 = script[0][3 * T % len(script[0]):][:T]
    f0 = script[2][3 * T % len(script[0]):][:T] if kind == "marl" else None
    assert np.array_equal(batch["scaled_rewards"].numpy(), rn.scaled_rewards(r0, record[3], 5.0, f0))
    col.freeze_return_norm(False)
    col.collect()
    assert not torch.equal(col.return_norm, before[1])
