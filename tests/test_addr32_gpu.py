"""Every result of the engine, bit for bit, against fingerprints recorded before the read-only tables moved into one arena.

The kernels address the tables (maps, lanes, grid cells, scenarios, spawn records, reset images, beam directions) as the arena's base plus
an unsigned 32-bit byte offset instead of one 64-bit pointer per table, and the part of a record's address inside its block in 32 bits.
How an address is formed moves no value: every output bit has to stay what it was.  tests/golden/addr32_v0.json holds, for each case
below, the text of pgd_describe_step and one fingerprint per step -- the first 10 hex digits of the SHA-1 over observation, reward, done,
flags and the float / integer / env state read back after the step (plus the image where a case renders one) -- recorded on the build of
the commit before the change (`recorded_with` = its pgd_source_sha), twice, with identical results.  The cases are small (8 - 32 envs,
100 - 300 steps) and cover every kernel family that reads a table:

    trigger          default kernel, trigger traffic, full throttle straight ahead
    respawn          default kernel, respawn traffic, uniform actions
    resample         auto-reset with resample_scenario=1 over 4 maps: env_map is rewritten, the scenario offset changes mid-run
    partial_reset    pgd_reset with an env list every 25 steps
    general          the general kernel, 12 slots x 72 beams
    packed           throughput mode (three envs per wave), forced with PGD_PACK=1
    safe             SafePGDriveEnv: 57 slots, traffic objects
    marl_8           the 8-seat multi-agent kernel (fused observation)
    marl_40          a 40-seat engine: k_step, then k_observe_env
    topdown          pgd_observe_topdown and pgd_render_topdown (env.render(mode="top_down")) after every step
    reupload         100 steps on 4 scenarios, then a second pgd_upload_scenarios with 8: the arena is rebuilt and every table moves (the
                     scenario tables lead the arena), then 50 more steps

Regenerating the file is only right when the step's results are MEANT to change: run `record` on the build that defines the new results
(`lib` picks a library) and write the JSON with the same keys.
"""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

from pgdrive_amd import _abi
from pgdrive_amd.engine import _np_p
from tests import parity, util
from tests.parity import closed_engines  # noqa: F401  (autouse: engines are closed when a test ends)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "addr32_v0.json")

SAFE = dict(num_traffic=56, accident_prob=0.8, safe_rl_env=True, density=0.05, use_lateral=False)
# name -> (envs, steps, maps, library switches, bank / config keywords, action stream)
SINGLE = dict(
    trigger=(32, 200, 8, dict(PGD_PACK=None), dict(), "straight"),
    respawn=(32, 200, 8, dict(PGD_PACK=None), dict(traffic_mode="respawn"), "uniform"),
    resample=(16, 300, 4, dict(PGD_PACK=None), dict(traffic_mode="respawn", resample_scenario=1), "straight"),
    partial_reset=(16, 100, 8, dict(PGD_PACK=None), dict(traffic_mode="respawn"), "uniform"),
    general=(16, 100, 8, dict(PGD_PACK=None), dict(num_traffic=11, num_lasers=72, traffic_mode="respawn"), "uniform"),
    packed=(32, 100, 8, dict(PGD_PACK="1"), dict(traffic_mode="respawn"), "uniform"),
    safe=(8, 100, 8, dict(PGD_PACK=None), SAFE, "uniform"),
    topdown=(8, 100, 8, dict(PGD_PACK=None), dict(traffic_mode="respawn"), "uniform"),
    reupload=(16, 150, 8, dict(PGD_PACK=None), dict(traffic_mode="respawn"), "uniform"),
)
MARL = dict(marl_8=(16, 8, 200), marl_40=(8, 40, 100))  # name -> (envs, seats, steps)
CASES = list(SINGLE) + list(MARL)


def _actions(kind, rng, n, a=1):
    if kind == "uniform":
        return rng.uniform(-1, 1, size=(n, a, 2)).astype(np.float32)
    act = np.zeros((n, a, 2), dtype=np.float32)  # straight ahead at full throttle, a little steering noise so that the envs differ
    act[..., 0] = np.clip(rng.normal(0, 0.05, size=(n, a)), -1, 1)
    act[..., 1] = 1.0
    return act


def _digest(eng, outs, extra=()):
    h = hashlib.sha1()
    for x in outs:
        h.update(x.cpu().numpy().tobytes())
    for x in eng.get_state():
        h.update(x.tobytes())
    for x in extra:
        h.update(x.cpu().numpy().tobytes())
    return h.hexdigest()[:10]


def _upload_scenarios(eng, sb):
    rc = eng.L.pgd_upload_scenarios(eng.h, _np_p(sb.scenarios), len(sb.scenarios), _np_p(sb.spawns))
    assert rc == 0, "pgd_upload_scenarios: %d" % rc
    eng.scen = sb


def record(name, descs, lib=None):
    """dict(kernel = pgd_describe_step's text, fp = the per-step fingerprints) of case `name` on the library in use (or `lib`)."""
    import torch
    rng = np.random.default_rng(5)
    if name in MARL:
        n, seats, steps = MARL[name]
        _, mb, sb = util.make_marl_banks(num_agents=seats, capacity=seats, kind="roundabout")
        eng = parity.engine(util.marl_config(n, sb, horizon=60), mb, sb, env=dict(PGD_NO_FIX=None), lib=lib)
        draw = lambda: util.marl_actions(rng, n, sb.A)
        n_scen = 8
    else:
        n, steps, n_maps, switches, kw, stream = SINGLE[name]
        env = dict(PGD_NO_FIX=None)
        env.update(switches)
        mb, sb, cfg = parity.banks_and_config(descs, n, n_maps=n_maps, auto_reset=1, seed=11, **kw)
        first = sb
        if name == "reupload":  # the first upload holds the scenarios of the first four maps only
            _, first = util.make_banks(descs, n_maps=4, **{k: v for k, v in kw.items() if k in parity.BANK_KEYS})
        eng = parity.engine(cfg, mb, first, env=env, lib=lib)
        draw = lambda: _actions(stream, rng, n)
        n_scen = len(first.scenarios)
    eng.reset(np.arange(n) % n_scen)
    if name == "topdown":
        eng.enable_topdown()
        eng.enable_render()
    fp = []
    for t in range(steps):
        if name == "partial_reset" and t % 25 == 24:  # a third of the envs, out of order, onto other scenarios
            ids = np.arange(n)[(t // 25) % 3::3][::-1]
            eng.reset((ids + t) % n_scen, env_ids=ids)
        if name == "reupload" and t == 100:
            _upload_scenarios(eng, sb)
        outs = eng.step(torch.from_numpy(draw()).to(eng.device))
        extra = (eng.observe_topdown(), eng.render_topdown()) if name == "topdown" else ()
        eng.sync()
        fp.append(_digest(eng, outs, extra))
    return dict(kernel=eng.describe_step(), fp=fp, library=eng.L.pgd_source_sha().decode())


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_results_are_bit_identical_to_the_ones_recorded_with_pointer_tables(descs, golden, name):
    want = golden["cases"][name]
    got = record(name, descs)
    assert got["kernel"] == want["kernel"], "case %s runs another kernel than the recording" % name
    assert len(got["fp"]) == len(want["fp"]) == (MARL[name][2] if name in MARL else SINGLE[name][1])
    differ = [t for t, (a, b) in enumerate(zip(got["fp"], want["fp"])) if a != b]
    assert not differ, "case %s: %d of %d steps differ from the fingerprints recorded with %s, the first at step %d" % (
        name, len(differ), len(want["fp"]), golden["recorded_with"], differ[0])
