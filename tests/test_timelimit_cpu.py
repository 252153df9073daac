"""GAE that bootstraps through a time limit, without a GPU: the float64 checker against its own definition, the property the feature exists
for, the predicate against the step's done rule, the measured tolerance of the device's two GAE forms, and the collectors' host logic on
a recording engine (tests/timelimit_ref.py; the device side is tests/test_timelimit_gpu.py)."""
import itertools
import re
import os
import types

import numpy as np
import pytest

from tests import actor_critic_ref as ar
from tests import safe_ppo_ref as sr
from tests import timelimit_ref as tl
from tests.recording_engine import D, N, T, W6, RecordingEngine, truncation_script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------
# the checker
# ---------------------------------------------------------------------------------------------------------------------
def test_the_recursion_is_the_cut_by_definition():
    """Every episode segment through the plain gae_f64 with its own bootstrap (term_value at a truncated end, 0 at a terminal one,
    value[T] at the rollout's end) == the recursive form, to 1e-12; the cost form the same way on safe_ppo_ref's costs, with its books
    untouched."""
    n = 0
    for c in tl.bootstrap_cases():
        if c["rows"] > 65:
            continue
        for mode in tl.TRUNC_MODES:
            r, v, d, trunc, tv = tl.build_bootstrap(mode=mode, **c)
            assert not (trunc & (d == 0)).any() and (tv[~trunc] == 0).all()
            fl, _, _, cv, tcv, run = tl.build_cost_bootstrap(mode=mode, **c)
            for lam in ar.GAE_LAM + (1.0, ):
                a, ret = tl.gae_bootstrap_f64(r, v, d, tv, ar.GAE_GAMMA, lam)
                a2, ret2 = tl.gae_bootstrap_by_segments_f64(r, v, d, tv, trunc, ar.GAE_GAMMA, lam)
                assert np.abs(a - a2).max() < 1e-12 * max(1.0, np.abs(a2).max()) and np.abs(ret - ret2).max() < 1e-11, (c, mode, lam)
                ref = tl.cost_gae_bootstrap_f64(fl, d, cv, tcv, tl.COSTS, ar.GAE_GAMMA, lam, run)
                plain = sr.cost_gae_f64(fl, d, cv, tl.COSTS, ar.GAE_GAMMA, lam, run)
                a3, ret3 = tl.gae_bootstrap_by_segments_f64(ref["cost"], cv, d, tcv, trunc, ar.GAE_GAMMA, lam)
                assert np.abs(ref["cadv"] - a3).max() < 1e-12 * max(1.0, np.abs(a3).max()) and np.abs(ref["cret"] - ret3).max() < 1e-11
                for key in ("cost", "run", "ep_sum", "ep_count"):
                    assert np.array_equal(ref[key], plain[key]), key
                if mode == "none":  # no truncation: pgd_gae's recursion
                    a0, ret0 = ar.gae_f64(r, v, d, ar.GAE_GAMMA, lam)
                    assert np.array_equal(a, a0) and np.array_equal(ret, ret0)
                    assert np.array_equal(ref["cadv"], plain["cadv"])
                n += 1
    assert n >= 3 * 4 * 5 * 3 * 3


def test_value_behind_a_done_is_selected_away():
    """NaN in value[t + 1] behind every done: the recursion's output is the clean one wherever the row's own value[t] is finite."""
    r, v, d, trunc, tv = tl.build_bootstrap(33, 65, "bernoulli", "bernoulli")
    a, ret = tl.gae_bootstrap_f64(r, v, d, tv, ar.GAE_GAMMA, 0.95)
    vn = v.copy()
    vn[1:][d != 0] = np.nan
    with np.errstate(invalid="ignore"):
        a2, ret2 = tl.gae_bootstrap_f64(r, vn, d, tv, ar.GAE_GAMMA, 0.95)
    own = np.isfinite(vn[:-1])
    assert (~own).any() and np.array_equal(a[own], a2[own]) and np.array_equal(ret[own], ret2[own])


def _constant_history(rng, T, rows, r, gamma, p_trunc=0.1):
    value = np.full((T + 1, rows), r / (1.0 - float(np.float32(gamma))))
    trunc = rng.uniform(size=(T, rows)) < p_trunc
    return np.full((T, rows), r), value, trunc.astype(np.uint8), np.where(trunc, value[:-1], 0.0)


def test_a_time_limit_is_invisible_to_a_correct_critic():
    """Constant reward r and value = term_value = r / (1 - gamma) everywhere, truncations at arbitrary steps: |adv| < 1e-9 at every
    step in float64 -- the critic is right and the clock changes nothing.  The plain gae_f64 on the same data hands every truncated step
    adv = r - value, a large negative advantage for surviving to the limit."""
    rng = np.random.default_rng(0)
    for r, gamma, lam in ((1.0, 0.99, 0.95), (0.37, 0.99, 0.0), (-2.5, 0.9, 1.0), (0.05, 0.999, 0.95)):
        reward, value, done, tv = _constant_history(rng, 200, 17, r, gamma)
        assert done.sum() > 100
        adv, ret = tl.gae_bootstrap_f64(reward, value, done, tv, gamma, lam)
        assert np.abs(adv).max() < 1e-9 * max(1.0, abs(value[0, 0])), (r, gamma, lam, np.abs(adv).max())
        plain, _ = ar.gae_f64(reward, value, done, gamma, lam)
        at = done != 0
        assert np.abs(plain[at] - (r - value[:-1][at])).max() < 1e-9 * abs(value[0, 0])
        assert np.abs(plain[at]).min() > 0.5 * abs(value[0, 0])


# ---------------------------------------------------------------------------------------------------------------------
# the predicate
# ---------------------------------------------------------------------------------------------------------------------
def test_the_predicate_is_the_steps_done_rule_and_the_horizon_line():
    """All 2^7 combinations of the six cause bits and done, safe_rl_env 0 and 1: pgdrive_amd.rollout.truncated (numpy arrays and python
    ints) == the literal restatement; other flag bits do not matter."""
    from pgdrive_amd import _abi
    from pgdrive_amd.rollout import truncated
    assert tl.CAUSE_BITS == (_abi.F_ARRIVE, _abi.F_OUT_OF_ROAD, _abi.F_CRASH_VEHICLE, _abi.F_CRASH_OBJECT, _abi.F_CRASH_BUILDING, _abi.F_MAX_STEP)
    combos = list(itertools.product((0, 1), repeat=7))
    assert len(combos) == 128
    flags = np.array([sum(b * bit for b, bit in zip(c[:6], tl.CAUSE_BITS)) for c in combos], dtype=np.int32)
    done = np.array([c[6] for c in combos], dtype=np.uint8)
    other = _abi.F_ON_YELLOW | _abi.F_OFF_LANE | _abi.F_RESET | _abi.F_OBJECT_HIT
    for safe in (0, 1):
        want = np.array([tl.truncated_ref(int(f), int(d), safe) for f, d in zip(flags, done)])
        assert np.array_equal(truncated(flags, done, safe), want)
        assert np.array_equal(truncated(flags | other, done, safe), want)
        for f, d, w in zip(flags, done, want):
            assert bool(truncated(int(f), int(d), safe)) == bool(w)
        # what it says: only the clock, unless -- safe -- a crash rides along, which is a cost there
        for f, d, w in zip(flags, done, want):
            clock_only = d and f == _abi.F_MAX_STEP
            assert not clock_only or w
            assert not w or (d and f & _abi.F_MAX_STEP)
    n0 = int(np.sum([tl.truncated_ref(int(f), int(d), 0) for f, d in zip(flags, done)]))
    n1 = int(np.sum([tl.truncated_ref(int(f), int(d), 1) for f, d in zip(flags, done)]))
    assert n0 == 1 and n1 == 1 + 3 * 8   # safe: any of the 3 non-empty crash combinations x the 8 combinations of the other causes


def test_the_header_states_the_rule_and_declares_the_entry_points():
    from pgdrive_amd import engine
    text = open(os.path.join(ROOT, "include", "pgdrive_hip.h")).read()
    assert "truncated(t) = d && (f & PGD_F_MAX_STEP) && !natural(t)" in text
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for fn in ("pgd_mlp_terminal_value", "pgd_gae_bootstrap", "pgd_cost_gae_bootstrap"):
        assert re.search(r"\bint\s+%s\s*\(" % fn, src), fn
        assert fn in engine.EXPORTS


def test_null_arguments_are_refused_without_a_gpu():
    from pgdrive_amd import engine
    L = engine.load_library()
    assert L.pgd_mlp_terminal_value(None, -1, None, 0, 0, None, None, None, None, None, None) == 1
    assert L.pgd_gae_bootstrap(None, None, None, None, None, 1, 1, 0.99, 0.95, None, None) == 1
    assert L.pgd_cost_gae_bootstrap(None, None, None, None, None, 1, 1, None, 0.99, 0.95, None, None, None, None, None, None) == 1


# ---------------------------------------------------------------------------------------------------------------------
# the tolerance of the device's two GAE forms
# ---------------------------------------------------------------------------------------------------------------------
def test_tol_gae_bootstrap_is_the_emulations_error_over_the_gpu_histories_doubled():
    worst = tl.emulation_error()
    print("float32 bootstrap GAE against float64: %.3e (recorded %.2e, TOL_GAE_BOOTSTRAP %.2e)" % (
        worst, tl.TOL_GAE_BOOTSTRAP_MEASURED, tl.TOL_GAE_BOOTSTRAP))
    assert tl.TOL_GAE_BOOTSTRAP == 2.0 * tl.TOL_GAE_BOOTSTRAP_MEASURED
    assert 0.8 * tl.TOL_GAE_BOOTSTRAP_MEASURED < worst <= tl.TOL_GAE_BOOTSTRAP_MEASURED


def test_the_emulation_without_truncations_is_k_gaes():
    """term_value = 0 and finite inputs: the select forms give pgd_gae's float values (fma(gamma, 0, r) == fma(0, v, r))."""
    for c in tl.bootstrap_cases():
        if c["rows"] > 65:
            continue
        r, v, d, _, tv = tl.build_bootstrap(mode="none", **c)
        for lam in ar.GAE_LAM:
            a, ret = tl.gae_bootstrap_f32(r, v, d, tv, ar.GAE_GAMMA, lam)
            a0, ret0 = ar.gae_f32(r, v, d, ar.GAE_GAMMA, lam)
            assert np.array_equal(a, a0) and np.array_equal(ret, ret0), c


# ---------------------------------------------------------------------------------------------------------------------
# host logic: the collectors on a recording engine
# ---------------------------------------------------------------------------------------------------------------------
# numbers that are exact in float32, which the collector's buffers are: r + gamma V - V == 0 with V = r / (1 - gamma) = 4
R, GAMMA, LAM, V = 1.0, 0.75, 0.5, 4.0


def _script():
    trunc = np.random.default_rng(3).uniform(size=(3 * T, N)) < 0.3
    trunc[T - 1, 0] = trunc[0, 1] = True   # across the carry, and in a rollout's first step
    return trunc


def _engine(trunc, step_info=None):
    """The recording engine on a script of the constant reward R and the truncations `trunc`; the networks say V, the cost critic V / 2."""
    return RecordingEngine(N, 1, D, truncation_script(R, trunc), value=V, cost_value=0.5 * V, step_info=step_info)


def test_switch_off_the_collectors_make_todays_calls():
    from pgdrive_amd.rollout import RolloutCollector, SafeRolloutCollector
    eng = _engine(_script())
    col = RolloutCollector(eng, W6, W6, T, gamma=GAMMA, lam=LAM)
    batch = col.collect()
    prime = ["actor_critic_tick", "mlp_actor_critic", "actor_critic_tick"]
    assert eng.calls == prime + ["actor_critic_tick"] + ["step", "mlp_actor_critic"] * T + ["actor_critic_tick", "gae"]
    assert eng.step_info is None and "term_values" not in batch and not col.bootstrap_truncations
    eng = _engine(_script())
    col = SafeRolloutCollector(eng, W6, W6, W6, T, gamma=GAMMA, lam=LAM)
    batch = col.collect()
    prime = ["actor_critic_tick", "mlp_actor_critic_cost", "actor_critic_tick"]
    assert eng.calls == prime + ["actor_critic_tick"] + ["step", "mlp_actor_critic_cost"] * T + ["actor_critic_tick", "gae", "cost_gae"]
    assert eng.step_info is None and "term_values" not in batch and "term_cost_values" not in batch


def test_switch_on_one_launch_per_step_and_the_property_through_the_collector():
    """The calls with the switch on; and the property the feature exists for, through collect(): rewards R, a critic that says V = R /
    (1 - gamma) everywhere, scripted truncations -- the advantages are exactly 0 with the switch on, and R - V at every truncated step
    with it off."""
    import torch
    from pgdrive_amd.rollout import RolloutCollector, SafeRolloutCollector
    script = _script()
    on, off = _engine(script), _engine(script)
    c_on = RolloutCollector(on, W6, W6, T, gamma=GAMMA, lam=LAM, bootstrap_truncations=True)
    c_off = RolloutCollector(off, W6, W6, T, gamma=GAMMA, lam=LAM)
    assert on.calls == ["enable_step_info(final_obs=True)"] and on.step_info["final_observation"].shape == (N, D)
    for k in range(3):
        del on.calls[:]
        b_on, b_off = c_on.collect(), c_off.collect()
        want = ["actor_critic_tick"] + ["step", "mlp_terminal_value", "mlp_actor_critic"] * T + ["actor_critic_tick", "gae_bootstrap"]
        assert on.calls == (["actor_critic_tick", "mlp_actor_critic", "actor_critic_tick"] if k == 0 else []) + want
        tr = torch.from_numpy(script[k * T:(k + 1) * T])
        assert tr.any() and torch.equal(b_on["dones"] != 0, tr) and torch.equal(b_off["dones"] != 0, tr)
        assert b_on["term_values"].shape == (T, N) and torch.equal(b_on["term_values"], tr.float() * V)
        assert torch.equal(b_on["advantages"], torch.zeros(T, N)) and torch.equal(b_on["returns"], torch.full((T, N), V))
        assert torch.equal(b_off["advantages"][tr], torch.full((int(tr.sum()), ), R - V))
    # an engine whose step info is on already is used as it is
    eng = _engine(script, step_info={"final_observation": torch.zeros(N, D)})
    RolloutCollector(eng, W6, W6, T, bootstrap_truncations=True)
    assert eng.calls == []
    # the safe collector: the cost critic in the same launch, the cost side's bootstrap form
    eng = _engine(script)
    col = SafeRolloutCollector(eng, W6, W6, W6, T, gamma=GAMMA, lam=LAM, cost_gamma=GAMMA, cost_lam=LAM, bootstrap_truncations=True)
    batch = col.collect()
    assert eng.calls == ["enable_step_info(final_obs=True)", "actor_critic_tick", "mlp_actor_critic_cost", "actor_critic_tick", "actor_critic_tick"] + \
        ["step", "mlp_terminal_value", "mlp_actor_critic_cost"] * T + ["actor_critic_tick", "gae_bootstrap", "cost_gae_bootstrap"]
    tr = torch.from_numpy(script[:T])
    assert torch.equal(batch["term_values"], tr.float() * V) and torch.equal(batch["term_cost_values"], tr.float() * 0.5 * V)
    assert torch.equal(batch["advantages"], torch.zeros(T, N))
    assert torch.equal(batch["ep_cost_count"], tr.sum(dim=0).to(torch.int32))   # a truncated episode still finishes for the books


def test_an_engine_without_final_observation_is_refused():
    import torch
    from pgdrive_amd.rollout import RolloutCollector, SafeRolloutCollector
    info = {"final_observation": None, "cost": torch.zeros(N)}
    for make in (lambda e: RolloutCollector(e, W6, W6, T, bootstrap_truncations=True),
                 lambda e: SafeRolloutCollector(e, W6, W6, W6, T, bootstrap_truncations=True)):
        eng = _engine(_script(), step_info=dict(info))
        with pytest.raises(ValueError, match="final_observation"):
            make(eng)
        assert eng.calls == []
    RolloutCollector(_engine(_script(), step_info=dict(info)), W6, W6, T)   # (the switch off: no objection)


def test_the_multi_agent_collector_has_no_such_switch():
    import inspect
    from pgdrive_amd.rollout import MultiAgentRolloutCollector, RolloutCollector, SafeRolloutCollector
    with pytest.raises(TypeError, match="bootstrap_truncations"):
        MultiAgentRolloutCollector(types.SimpleNamespace(A=4), W6, W6, T=4, bootstrap_truncations=True)
    for cls in (RolloutCollector, SafeRolloutCollector):
        assert inspect.signature(cls.__init__).parameters["bootstrap_truncations"].default is False
