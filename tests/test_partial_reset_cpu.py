"""Partial resets on the fp64 oracle (tests/test_partial_reset_gpu.py holds the engine to the same statements): a restart by id list
between two steps of an `auto_reset=0` run equals the restart the step does itself under `auto_reset=1`, and a call with an id list
writes the rows of the listed envs and no others."""
import numpy as np
import pytest

from pgdrive_amd import _abi
from tests import parity, util

EI = _abi.EI
RESTARTS_FLOOR = dict(single=100, marl8=30)  # conditions of the test (these shapes and seeds give 253 and 53)


def twin_oracles(descs, kind, n_envs=48):
    """(A, B, actions(t), scenarios): two oracles of one configuration, A restarting finished envs inside the step with a re-drawn
    scenario, B never restarting one by itself."""
    from oracle import orc
    rng = np.random.default_rng(17)
    if kind == "single":
        mb, sb = util.make_banks(descs, n_maps=8, num_traffic=16)
        kw = dict(num_agents=1, num_traffic=16, num_lasers=72, horizon=60, seed=7)
        cfgs = [_abi.make_config(n_envs, auto_reset=ar, resample_scenario=ar, **kw) for ar in (1, 0)]
        actions = parity.driving_with_bursts(rng, n_envs)
    else:
        d, mb, sb = util.make_marl_banks(num_agents=8, capacity=8, kind="roundabout")
        cfgs = [util.marl_config(n_envs, sb, horizon=60, delay_done=10, seed=7, auto_reset=ar, resample_scenario=ar) for ar in (1, 0)]
        actions = lambda t: util.marl_actions(rng, n_envs, sb.A)  # noqa: E731
    return orc.Oracle(cfgs[0], mb, sb), orc.Oracle(cfgs[1], mb, sb), actions, len(sb.scenarios)


@pytest.mark.parametrize("kind", ["single", "marl8"])
def test_manual_restart_equals_the_automatic_one(descs, kind):
    """A: auto_reset=1, resample_scenario=1.  B: auto_reset=0; after every step the envs whose flags carry F_RESET in A are restarted by
    id, with the scenario A's EI_SCEN names, into the buffer B's step returned.  At every step: reward, done and the flags (without
    F_RESET, and without F_NEW in the restarted envs) identical; after B's restart the float and the integer state identical, the env
    counters identical except EI_EPISODES (only the restart inside a step counts an episode); the rows of the restarted envs, B's
    reset against A's step, identical; single-agent the rows of every other env too.
    The id list bounds what the call writes: in the buffer handed to reset, and in a second one filled with a sentinel, only the rows
    of the listed envs change -- the terminal rows of agents that reported in the last step of an UNLISTED env (they are ST_DYING now,
    a stand-alone observation gives them a zero row) are still there."""
    a, b, actions, n_scen = twin_oracles(descs, kind)
    n = a.N
    ids0 = np.arange(n) % n_scen
    assert np.array_equal(a.reset(ids0), b.reset(ids0))
    restarts = calls = kept_terminal = 0
    for t in range(200):
        act = actions(t)
        ao, ar, ad, af = a.step(act)
        bo, br, bd, bf = b.step(act)
        assert np.array_equal(ar, br) and np.array_equal(ad, bd), "reward / done differ at step %d" % t
        listed = ((af & _abi.F_RESET) != 0).any(axis=1)
        mask = np.full(af.shape, _abi.F_RESET, dtype=np.uint32) | np.where(listed[:, None], np.uint32(_abi.F_NEW), np.uint32(0))
        assert np.array_equal(af & ~mask, bf & ~mask), "flags differ at step %d" % t
        assert not (bf & _abi.F_RESET).any()
        ids = np.nonzero(listed)[0].astype(np.int32)
        if len(ids):
            scen = a.get_state()[2][EI["SCEN"], ids]
            before = bo.copy()
            sentinel = np.full_like(bo, -7.0)
            b.reset(scen, env_ids=ids, out=sentinel)  # (a restart is a function of the scenario: doing it twice changes nothing)
            assert b.reset(scen, env_ids=ids, out=bo) is bo
            assert np.array_equal(bo[~listed], before[~listed]), "rows of unlisted envs rewritten at step %d" % t
            assert (sentinel[~listed] == -7.0).all() and np.array_equal(sentinel[listed], bo[listed])
            # what a stand-alone observation of all envs would have zeroed: rows of seats that are not active any more
            status = b.get_state()[1][_abi.SI["STATUS"]][:, :a.A]
            kept_terminal += int((bo.any(axis=2) & (status != _abi.ST_ACTIVE) & ~listed[:, None]).sum())
            restarts += len(ids)
            calls += 1
            assert np.array_equal(bo[listed], ao[listed]), "rows of restarted envs differ at step %d" % t
        if kind == "single":
            assert np.array_equal(bo, ao), "rows differ at step %d" % t
        (fa, ia, ea), (fb, ib, eb) = a.get_state(), b.get_state()
        assert np.array_equal(fa.view(np.int64), fb.view(np.int64)) and np.array_equal(ia, ib), "state differs at step %d" % t
        rest = [k for name, k in EI.items() if name != "EPISODES"]
        assert np.array_equal(ea[rest], eb[rest]), "env counters differ at step %d" % t
    ea, eb = a.get_state()[2], b.get_state()[2]
    print("partial reset on the oracle:", kind, "restarts", restarts, "in", calls, "calls; terminal rows of unlisted envs kept", kept_terminal)
    assert int(ea[EI["EPISODES"]].sum()) == restarts and int(eb[EI["EPISODES"]].sum()) == 0
    assert restarts >= RESTARTS_FLOOR[kind]
    assert kind == "single" or kept_terminal > 0
