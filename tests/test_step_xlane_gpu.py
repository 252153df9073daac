"""The step's results, bit for bit, against fingerprints recorded before the LDS reads of the IDM path were batched.

The IDM broad phase and the front/back search read the snapshot of an env's vehicles from LDS.  How those reads are issued (one slot at a
time behind the previous slot's verdict, or a batch ahead of the tests that use them) moves no value: every output bit of a step has to
stay what it was.  tests/golden/step_xlane_v0.json holds, for each case below, one fingerprint per step -- the first 10 hex digits of
the SHA-1 over observation, reward, done, flags and the float / integer / env state read back after the step -- recorded on the build
of the commit before the change (`recorded_with` = its pgd_source_sha).  The cases are the smallest at which each piece can go wrong:

    respawn        64 envs x 17 slots x 240 beams, respawn traffic (every IDM vehicle drives and changes lanes), uniform(-1, 1)
                   actions, 300 steps, maps 1000 - 1007: the default configuration's kernel, broad phase and search on every step
    trigger        the same with trigger traffic and full throttle straight ahead: groups get triggered, contacts happen
    slots_5_10_15  trigger traffic with exactly the traffic slots 5, 10 and 15 driving (set through the state interface): with three
                   sub-lanes per vehicle these are the groups whose lanes straddle a 16-lane row of the wave
    packed         the default configuration in throughput mode (three envs per wave, one lane per vehicle)
    general_sub4   72 beams, 12 slots: the general kernel, four sub-lanes per vehicle
    safe_sub1      SafePGDriveEnv's configuration, 57 slots: one lane per vehicle, ten rounds of the broad-phase batch

Regenerating the file is only right when the step's results are MEANT to change: run `fingerprint` for every case on the build that
defines the new results (PGD_LIB picks a library) and write the JSON with the same keys.
"""
import hashlib
import json
import os

import numpy as np
import pytest

from pgdrive_amd import _abi
from tests import parity
from tests.parity import closed_engines  # noqa: F401  (autouse: engines are closed when a test ends)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_xlane_v0.json")
N_ENVS = 64

# name -> (steps, library switches, bank / config keywords, action stream, kernel named by pgd_describe_step)
CASES = dict(
    respawn=(300, dict(PGD_PACK=None), dict(traffic_mode="respawn"), "uniform", "specialised for the default"),
    trigger=(300, dict(PGD_PACK=None), dict(), "straight", "specialised for the default"),
    slots_5_10_15=(100, dict(PGD_PACK=None), dict(), "uniform", "specialised for the default"),
    packed=(100, dict(PGD_PACK="1"), dict(traffic_mode="respawn"), "uniform", "throughput mode"),
    general_sub4=(100, dict(PGD_PACK=None), dict(num_traffic=11, num_lasers=72, traffic_mode="respawn"), "uniform", None),
    safe_sub1=(100, dict(PGD_PACK=None), dict(num_traffic=56, accident_prob=0.8, safe_rl_env=True, density=0.05, use_lateral=False),
               "uniform", "specialised for the SafePGDriveEnv"),
)


def _actions(kind, rng, n):
    if kind == "uniform":
        return rng.uniform(-1, 1, size=(n, 1, 2)).astype(np.float32)
    act = np.zeros((n, 1, 2), dtype=np.float32)  # straight ahead at full throttle, a little steering noise so that the envs differ
    act[..., 0] = np.clip(rng.normal(0, 0.05, size=(n, 1)), -1, 1)
    act[..., 1] = 1.0
    return act


def _only_slots_drive(eng, slots):
    """Of the traffic, exactly `slots` drive: they are switched to ACTIVE where the scenario has a vehicle in them, every other traffic
    slot is removed."""
    f, i, ei = eng.get_state()
    st = i[_abi.SI["STATUS"]]
    there = (st == _abi.ST_PENDING) | (st == _abi.ST_ACTIVE)
    for s in range(eng.A, eng.V):
        st[:, s] = np.where(there[:, s], _abi.ST_ACTIVE if s in slots else _abi.ST_REMOVED, st[:, s])
    eng.set_state(f, i, ei)
    return int(there[:, list(slots)].sum())


def fingerprint(name, descs, stats=None):
    """The per-step fingerprints of case `name` on the library in use; `stats` (a dict) receives what happened along the run."""
    import torch
    steps, switches, kw, stream, kernel = CASES[name]
    env = dict(PGD_NO_FIX=None)
    env.update(switches)
    mb, sb, cfg = parity.banks_and_config(descs, N_ENVS, n_maps=8, auto_reset=1, seed=11, **kw)
    eng = parity.engine(cfg, mb, sb, env=env)
    eng.reset(np.arange(N_ENVS) % 8)
    driving = _only_slots_drive(eng, (5, 10, 15)) if name == "slots_5_10_15" else None
    rng = np.random.default_rng(5)
    fp, n_done, n_crash = [], 0, 0
    for _ in range(steps):
        o, r, dn, fl = eng.step(torch.from_numpy(_actions(stream, rng, N_ENVS)).to(eng.device))
        eng.sync()
        h = hashlib.sha1()
        for x in (o, r, dn, fl):
            h.update(x.cpu().numpy().tobytes())
        for x in eng.get_state():
            h.update(x.tobytes())
        fp.append(h.hexdigest()[:10])
        n_done += int(dn.sum())
        n_crash += int(((fl & _abi.F_CRASH_VEHICLE) != 0).sum())
    desc = eng.describe_step()
    assert (kernel in desc) if kernel else ("specialised" not in desc and "throughput" not in desc), desc
    if stats is not None:
        st = eng.get_state()[1][_abi.SI["STATUS"]]
        stats.update(kernel=desc, done=n_done, crash_vehicle=n_crash, active_traffic_at_end=int((st[:, eng.A:] == _abi.ST_ACTIVE).sum()),
                     slots_set_driving=driving, library=eng.L.pgd_source_sha().decode())
    return fp


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_step_results_are_bit_identical_to_the_recorded_ones(descs, golden, name):
    want = golden["cases"][name]
    got = fingerprint(name, descs)
    assert len(got) == len(want) == CASES[name][0]
    differ = [t for t, (a, b) in enumerate(zip(got, want)) if a != b]
    assert not differ, "case %s: %d of %d steps differ from the fingerprints recorded with %s, the first at step %d" % (
        name, len(differ), len(want), golden["recorded_with"], differ[0])
