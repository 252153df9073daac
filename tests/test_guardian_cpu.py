"""The expert guardian without a GPU: the float64 restatement of tests/guardian_ref.py against hand-worked cases for every branch of
the rule, the info bits, the slice indices, the config handling of the env layers, the ABI struct, and the derivation of the tolerance
of the traced floats and of the tie band that tests/test_guardian_gpu.py uses."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from pgdrive_amd import _abi, vec_env
from tests import guardian_ref as gr
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D = 72, 90  # a fan whose four windows do not overlap (at 40 beams they do); 18 state floats in front of it


def _row(obs0=0.5, obs1=0.5, fan=None):
    o = np.full((1, D), 0.9, dtype=np.float32)
    o[0, 0], o[0, 1] = obs0, obs1
    for k, v in (fan or {}).items():
        o[0, D - N + k] = v
    return o


def _rule(o, a, e, hd, v, f, s=0.5):
    c, fired = gr.rule_f64(o, N, np.array([a], dtype=np.float32), np.array([e], dtype=np.float32), np.array([hd]), np.array([v]), np.array([f]), s)
    return tuple(float(x) for x in c[0]), {k: bool(x[0]) for k, x in fired.items()}


A, E = (0.25, 0.75), (-0.5, -0.125)  # exact in fp32


def test_save_level_regimes():
    """s > 0.9: the expert drives whatever the row holds; s <= 1e-3: the agent does, whatever the row holds."""
    danger = _row(obs0=0.0, obs1=0.0, fan={k: 0.0 for k in range(N)})
    assert _rule(danger, A, E, -0.2, 50.0, 5.0, s=1.0)[0] == E
    assert _rule(_row(), A, E, 0.2, 50.0, 5.0, s=0.91)[0] == E
    assert _rule(danger, A, E, -0.2, 50.0, 5.0, s=2.0 ** -10)[0] == A
    assert gr.thresholds(1e-3)[1] == 1  # (fp32(1e-3) is above the double 1e-3: the rule runs)
    assert _rule(danger, A, E, -0.2, 50.0, 5.0, s=0.0)[0] == A
    assert gr.thresholds(0.9)[1] == 1 and gr.thresholds(0.91)[1] == 2  # (fp32(0.9) is below the double 0.9: s is compared as a double)
    assert gr.thresholds(0.5)[1:] == (1, 5.0, float(np.float32(0.06)), 0.5)


def test_out_of_road_clauses():
    f = 2.0  # the edge is 0.04 f = 0.08
    # obs0 under the edge counts with hd < 0 only, obs1 with hd > 0 only
    assert _rule(_row(obs0=0.07), A, E, -0.1, 30.0, f) == (E, dict(out=True, slow=False, side=False, front=False))
    assert _rule(_row(obs0=0.07), A, E, +0.1, 30.0, f)[0] == A
    assert _rule(_row(obs1=0.07), A, E, +0.1, 30.0, f)[0] == E
    assert _rule(_row(obs1=0.07), A, E, -0.1, 30.0, f)[0] == A
    assert _rule(_row(obs0=0.09), A, E, -0.1, 30.0, f)[0] == A
    assert _rule(_row(obs0=0.07, obs1=0.07), A, E, 0.0, 30.0, f)[0] == A  # hd = 0: neither side
    # at or under 1e-3 whatever the heading
    assert _rule(_row(obs0=np.float32(1e-3)), A, E, +0.1, 30.0, 1.0)[0] == E
    assert _rule(_row(obs1=np.float32(1e-3)), A, E, -0.1, 30.0, 1.0)[0] == E
    assert _rule(_row(obs1=np.nextafter(np.float32(1e-3), np.float32(1))), A, E, -0.1, 30.0, 1.0)[0] == A
    # v < 5: the expert's steering with throttle 0.5
    assert _rule(_row(obs0=0.07), A, E, -0.1, 4.9, f) == ((E[0], 0.5), dict(out=True, slow=True, side=False, front=False))
    assert _rule(_row(obs0=0.07), A, E, -0.1, 5.0, f)[0] == E


def test_side_and_front_clauses():
    L, R = gr.slices(N)
    thr = float(np.float32(0.06))  # (0.5 + 0.1) / 10
    for beam in (L - 4, L + 5, R - 4, R + 5):
        assert _rule(_row(fan={beam: thr * 0.9}), A, E, 0.1, 30.0, 5.0) == ((E[0], A[1]), dict(out=False, slow=False, side=True, front=False)), beam
        assert _rule(_row(fan={beam: np.float32(thr)}), A, E, 0.1, 30.0, 5.0)[0] == A, beam  # strictly below only
    for beam in (L - 5, L + 6, R - 5, R + 6):  # just outside the side windows
        got = _rule(_row(fan={beam: 0.055}), A, (E[0], 0.5), 0.1, 30.0, 5.0)[0]  # e1 > 0: the front clause cannot fire either
        assert got == A, beam
    # front: a1 >= 0 and e1 <= 0 and a beam of the first or last ten under s
    for beam in (0, 9, N - 10, N - 1):
        assert _rule(_row(fan={beam: 0.4}), A, E, 0.1, 30.0, 5.0) == ((A[0], E[1]), dict(out=False, slow=False, side=False, front=True)), beam
        assert _rule(_row(fan={beam: 0.5}), A, E, 0.1, 30.0, 5.0)[0] == A, beam
        assert _rule(_row(fan={beam: 0.4}), A, (E[0], 0.125), 0.1, 30.0, 5.0)[0] == A, beam    # e1 > 0
        assert _rule(_row(fan={beam: 0.4}), (A[0], -0.25), E, 0.1, 30.0, 5.0)[0] == (A[0], -0.25), beam  # a1 < 0
        assert _rule(_row(fan={beam: 0.4}), (A[0], 0.0), (E[0], 0.0), 0.1, 30.0, 5.0)[0] == (A[0], 0.0), beam  # fires, and changes nothing
    # the out-of-road throttle of a slow car is overwritten by the front clause
    assert _rule(_row(obs0=0.0, fan={0: 0.1}), A, E, -0.1, 3.0, 5.0)[0] == E


@pytest.mark.parametrize("n,left,right", [(40, 10, 30), (72, 18, 54), (240, 60, 180), (241, 60, 180)])
def test_slice_indices(n, left, right):
    assert gr.slices(n) == (left, right) == (n // 4, (3 * n) // 4)
    fan = np.ones((4, n))
    fan[0, left - 4], fan[1, right + 5], fan[2, 9], fan[3, n - 10] = 0.1, 0.2, 0.3, 0.4
    side, front = gr.fan_minima(fan)
    assert side.tolist() == [0.1, 0.2, 1.0, 1.0] or n == 40  # (at 40 beams the front and the right window overlap)
    assert front[2] == 0.3 and front[3] == 0.4
    fan = np.ones((2, n))
    fan[0, left - 5] = fan[0, left + 6] = fan[0, right - 5] = 0.0
    fan[1, 10] = fan[1, n - 11] = 0.0
    side, front = gr.fan_minima(fan)
    assert side[0] == 1.0 and front[1] == 1.0
    assert len(gr.window_beams(n)) == (40 if n > 40 else 30)


def _seq(now_seq, resets, immediate=False):
    """Drive the bookkeeping with steps whose rule corrects (now) or not."""
    state = np.zeros(1, dtype=np.uint8)
    out = []
    for now, rs in zip(now_seq, resets):
        a = np.array([A])
        c = np.array([E]) if now else a
        applied, state, info = gr.bookkeeping(state, np.array([rs]), a, c, immediate)
        out.append((tuple(applied[0]), int(state[0]), int(info[0])))
    return out


def test_info_bits_over_a_sequence():
    """pre / now = 00, 01, 11, 10: nothing, start, takeover (the correction is applied from the second consecutive step on), end."""
    got = _seq([0, 1, 1, 0], [0, 0, 0, 0])
    assert got == [(A, 0, 0), (A, 1, gr.TAKEOVER_START), (E, 1, gr.TAKEOVER), (A, 0, gr.TAKEOVER_END)]


def test_reset_in_the_middle_clears_the_state():
    got = _seq([1, 1, 1, 1], [0, 0, 1, 0])
    assert [g[2] for g in got] == [gr.TAKEOVER_START, gr.TAKEOVER, gr.TAKEOVER_START, gr.TAKEOVER]
    assert [g[0] for g in got] == [A, E, A, E]
    got = _seq([1, 0, 0], [0, 1, 0])  # a reset behind a takeover step: no takeover_end is reported for the new vehicle
    assert [g[2] for g in got] == [gr.TAKEOVER_START, 0, 0]


def test_immediate_applies_in_the_step_that_raises_it():
    got = _seq([0, 1, 1, 0], [0, 0, 0, 0], immediate=True)
    assert [g[0] for g in got] == [A, E, E, A]
    assert [g[2] for g in got] == [0, gr.TAKEOVER_START, gr.TAKEOVER, gr.TAKEOVER_END]  # the info bits are the reference's


def test_a_nan_action_counts_as_changed():
    a = np.array([[np.nan, 0.5]])
    _, state, info = gr.bookkeeping(np.zeros(1), np.zeros(1), a, a)
    assert state[0] == 1 and info[0] == gr.TAKEOVER_START  # nan != nan, as in the reference's float comparison


def test_abi_struct_and_bits_match_the_header():
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "pgdrive_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %u %u %u\\n", ' \
           'sizeof(pgd_guardian_config), offsetof(pgd_guardian_config, expert_in_dim), offsetof(pgd_guardian_config, save_level), ' \
           'offsetof(pgd_guardian_config, seed), offsetof(pgd_guardian_config, tick), offsetof(pgd_guardian_config, mode), ' \
           'PGD_GUARD_LEGACY_LATERAL, PGD_GUARD_DETERMINISTIC, PGD_GUARD_IMMEDIATE); return 0; }\n'
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "g.c")
        open(c, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", os.path.join(td, "g")])
        out = [int(x) for x in subprocess.check_output([os.path.join(td, "g")]).decode().split()]
    G = _abi.GuardianConfig
    assert out[:6] == [C.sizeof(G), G.expert_in_dim.offset, G.save_level.offset, G.seed.offset, G.tick.offset, G.mode.offset]
    assert out[6:] == [_abi.GUARD_LEGACY_LATERAL, _abi.GUARD_DETERMINISTIC, _abi.GUARD_IMMEDIATE] == [gr.LEGACY, gr.DETERMINISTIC, gr.IMMEDIATE]
    assert (_abi.GUARD_TAKEOVER, _abi.GUARD_TAKEOVER_START, _abi.GUARD_TAKEOVER_END) == (gr.TAKEOVER, gr.TAKEOVER_START, gr.TAKEOVER_END)
    from pgdrive_amd import engine, rollout
    assert "pgd_guardian" in engine.EXPORTS and hasattr(engine.Engine, "guardian")
    assert rollout.GUARDIAN_SEED_XOR == gr.SEED_XOR != 0


# ---------------------------------------------------------------------------------------------------------------------
# config handling
# ---------------------------------------------------------------------------------------------------------------------
def _weights(rows, out_cols=4):
    rng = np.random.default_rng(rows)
    shapes = ((rows, 256), (256, ), (256, 256), (256, ), (256, out_cols), (out_cols, ))
    return {k: rng.normal(size=s).astype(np.float32) for k, s in zip(vec_env.SAVER_WEIGHT_KEYS, shapes)}


def test_config_keys_and_defaults():
    d = vec_env.DEFAULT_CONFIG
    assert d["use_saver"] is False and d["save_level"] == 0.5 and d["saver_weights"] is None
    assert d["saver_deterministic"] is False and d["saver_immediate"] is False
    assert "use_saver" not in vec_env.NEUTRAL_KEYS and "save_level" not in vec_env.VISUAL_KEYS
    user = dict(use_saver=True, save_level=0.3, saver_weights="w.npz", use_render=False)
    assert vec_env.strip_reference_only_keys(user) == dict(use_saver=True, save_level=0.3, saver_weights="w.npz")
    c = vec_env.merge_config(d, vec_env.strip_reference_only_keys(user))
    assert c["use_saver"] is True and c["save_level"] == 0.3
    # use_saver=False: a config of before merges to the config of before plus the five neutral keys
    plain = vec_env.merge_config(d, dict(start_seed=5))
    assert plain["use_saver"] is False and plain["start_seed"] == 5


def test_weights_are_checked_against_the_observation_width():
    for rows in (274, 275):
        w = vec_env.load_saver_weights(dict(saver_weights=_weights(rows)), 274)
        assert len(w) == 6 and w[0].shape == (rows, 256) and all(a.dtype == np.float32 and a.flags["C_CONTIGUOUS"] for a in w)
    with pytest.raises(ValueError, match="273 rows"):
        vec_env.load_saver_weights(dict(saver_weights=_weights(273)), 274)
    with pytest.raises(ValueError, match="at least 4 columns"):
        vec_env.load_saver_weights(dict(saver_weights=_weights(274, out_cols=2)), 274)
    part = _weights(274)
    del part["default_policy/fc_2/bias"]
    with pytest.raises(ValueError, match="fc_2/bias"):
        vec_env.load_saver_weights(dict(saver_weights=part), 274)
    with pytest.raises(ValueError, match="examples/ppo_expert/expert_weights.npz"):
        vec_env.load_saver_weights(dict(saver_weights=None), 274)
    fixture = os.path.join(ROOT, "tests", "golden", "expert_weights.npz")
    assert vec_env.load_saver_weights(dict(saver_weights=fixture), 274)[0].shape == (275, 256)  # the reference's expert: the legacy row


def test_refusals_by_name():
    """Each raises before a map is generated or an engine created: no GPU is needed to be refused."""
    from pgdrive_amd.env import PGDriveEnv
    from pgdrive_amd.marl_env import MultiAgentRoundaboutEnv
    from pgdrive_amd.rollout import MultiAgentRolloutCollector
    w = _weights(275)
    base = dict(use_saver=True, saver_weights=w)
    with pytest.raises(ValueError, match="expert_weights.npz"):
        vec_env.PGDriveVecEnv(dict(use_saver=True))
    with pytest.raises(ValueError, match="expert_weights.npz"):
        PGDriveEnv(dict(use_saver=True))
    for extra, name in ((dict(IDM_agent=True), "IDM_agent"), (dict(discrete_action=True), "discrete_action"),
                        (dict(vehicle_config=dict(lidar=dict(gaussian_noise=0.1))), "gaussian_noise"),
                        (dict(vehicle_config=dict(lidar=dict(dropout_prob=0.1))), "dropout_prob"),
                        (dict(vehicle_config=dict(lidar=dict(num_lasers=39))), "fewer than 40"),
                        (dict(vehicle_config=dict(lidar=dict(num_lasers=240, distance=0))), "fewer than 40")):
        with pytest.raises(NotImplementedError, match=name):
            vec_env.PGDriveVecEnv(dict(base, **extra))
    with pytest.raises(NotImplementedError, match="use_saver.*multi-agent"):
        MultiAgentRoundaboutEnv(dict(use_saver=True))

    class TwoSeats:
        A = 2
    with pytest.raises(NotImplementedError, match="guardian"):
        MultiAgentRolloutCollector(TwoSeats(), None, None, T=4, guardian=dict(weights=None))


# ---------------------------------------------------------------------------------------------------------------------
# the traced floats: fp32 emulation against float64 over exactly the poses of the GPU cases
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def banks(descs):
    return util.make_banks(descs, n_maps=gr.N_MAPS, num_traffic=0)


def test_poses_cover_both_sides_of_every_threshold(descs, banks):
    mb, sb = banks
    slow = fast = left = right = capped = free = arcs = 0
    for ci, (rows, n, legacy) in enumerate(gr.KERNEL_CASES):
        p = gr.pose_cases(descs, rows, ci)
        for e in range(rows):
            ld, rec = gr.lane_of(descs, mb, int(p["map"][e]), int(p["lane"][e]))
            hx, hy = np.float32(np.cos(p["theta"][e])), np.float32(np.sin(p["theta"][e]))
            lat, hd, v, f = gr.traced_f64(ld, p["x"][e], p["y"][e], hx, hy, p["speed"][e], 80.0, gr.SAVE_LEVEL)
            assert abs(hd) > 5e-4 and abs(v - 5.0) > 0.5 and 0.0 < lat < 1.0, (ci, e, hd, v, lat)
            slow += v < 5; fast += v > 5; left += hd < 0; right += hd > 0; capped += f == 5.0; free += f < 5.0; arcs += ld["type"] != 0
    assert min(slow, fast, left, right, capped, free, arcs) >= 20, (slow, fast, left, right, capped, free, arcs)
    assert float(sb.spawns["max_speed"][0]) == 80.0


def test_tolerance_of_the_traced_floats_and_the_tie_band(descs, banks):
    """Twice the largest |fp32 emulation - float64| over the poses of the GPU cases: the numbers DESIGN section 28 quotes."""
    tol_lat, tol_f = gr.tolerances(descs, banks[0])
    print("tolerances: lateral float %.3e, f %.3e; tie band around 0.04 f at f = 5: %.3e" % (tol_lat, tol_f, gr.tie_band(tol_f, 0.2)))
    assert 1e-7 < tol_lat < 1e-5 and 1e-6 < tol_f < 5e-4  # fp32 on coordinates of a few hundred metres; f = 1 + |hd| v 80 with hd to 6e-8
    assert abs(tol_lat - 4.52e-6) < 0.01e-6 and abs(tol_f - 1.347e-4) < 0.001e-4, (tol_lat, tol_f)  # as written into DESIGN section 28
    # the crafted rows keep 10 % of the edge between themselves and the edge: far outside the band
    assert gr.tie_band(tol_f, 0.2) < 1e-5 < 0.1 * gr.C_EDGE * 1.0


def test_crafted_rows_are_outside_the_tie_band_and_hit_every_clause():
    rng = np.random.default_rng(3)
    for n in gr.BEAMS:
        Dn = 34 + n
        rows = 56
        f = np.where(np.arange(rows) % 2 == 0, 5.0, rng.uniform(1.5, 4.0, rows))
        hd = np.where(np.arange(rows) % 4 < 2, -0.1, 0.1)
        obs, act = gr.craft_rows(Dn, n, f, gr.SAVE_LEVEL, 0)
        assert obs.dtype == np.float32 and obs.shape == (rows, Dn) and (obs >= 0).all() and (obs <= 1).all()
        edge = gr.C_EDGE * f
        gap = np.minimum(np.abs(obs[:, 0] - edge), np.abs(obs[:, 1] - edge))
        assert (gap > gr.tie_band(1.4e-4, edge)).all()
        e = np.stack([np.full(rows, 0.3), np.where(np.arange(rows) % 3 == 0, 0.2, -0.2)], axis=1)
        _, fired = gr.rule_f64(obs, n, act, e, hd, np.full(rows, 30.0), f, gr.SAVE_LEVEL)
        assert fired["out"].sum() >= 4 and fired["side"].sum() >= 4 and fired["front"].sum() >= 2, (n, {k: int(v.sum()) for k, v in fired.items()})
        assert (~(fired["out"] | fired["side"] | fired["front"])).sum() >= 8
