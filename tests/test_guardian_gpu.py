"""k_guardian (pgdrive_amd/csrc/pgd_guardian.h), Engine.guardian, the env surface (use_saver / save_level) and the collectors' guardian on
the device, against tests/guardian_ref.py:

* the expert's action bit for bit against pgd_mlp_actor_critic, on the plain row and on the row with the lateral float, with a
  normalisation table bound (ignored) and deterministic;
* the traced floats (lateral float, f) against float64 from get_state() within the tolerance tests/test_guardian_cpu.py derives;
* the rule on crafted observation rows around every threshold, teacher-forced on the traced expert action: applied action, state and
  info EQUAL, all rows -- after asserting, by the checker alone, that no row lies inside the tie band of obs < 0.04 f;
* five launches with a reset in the middle; d_applied aliasing d_agent_actions; an env group; the first call inside a graph capture;
* PGDriveVecEnv / PGDriveEnv with use_saver; RolloutCollector with guardian=; the two driving bands.
"""
import os

import numpy as np
import pytest

from pgdrive_amd import _abi
from tests import actor_critic_ref as ar
from tests import guardian_ref as gr
from tests import util
from tests.train_util import KEYS, SENT, Traffic, bits_equal as _bits_equal, dev as _dev, eager_then_graph, make_collector, \
    snapshot as _snapshot, synchronised_rollouts

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "expert_weights.npz")
SF, SI = _abi.SF, _abi.SI
SEED, TICK = 11, 5


@pytest.fixture(scope="module")
def tols(descs):
    mb, _ = util.make_banks(descs, n_maps=gr.N_MAPS, num_traffic=0)
    return gr.tolerances(descs, mb)


def _engine(descs, rows, n):
    from pgdrive_amd.engine import Engine
    mb, sb = util.make_banks(descs, n_maps=gr.N_MAPS, num_traffic=0)
    eng = Engine(_abi.make_config(rows, num_traffic=0, num_lasers=n, seed=2), mb, sb)
    eng.reset(np.arange(rows) % gr.N_MAPS)
    eng.sync()
    return eng, mb, sb


def _pose(eng, descs, sb, p, save_level=gr.SAVE_LEVEL):
    """Write the poses with set_state, read the state back, and form the float64 traced floats from what the engine holds."""
    f, i, ei = eng.get_state()
    f[SF["X"], :, 0], f[SF["Y"], :, 0], f[SF["THETA"], :, 0], f[SF["SPEED"], :, 0] = p["x"], p["y"], p["theta"], p["speed"]
    f[SF["HX"], :, 0] = f[SF["HY"], :, 0] = 0.0  # (derived from THETA by the engine)
    i[SI["LANE"], :, 0] = p["lane"]
    eng.set_state(f, i, ei)
    f, i, ei = eng.get_state()
    rows = eng.N
    out = np.zeros((rows, 4))
    for e in range(rows):
        m = int(sb.scenarios["map"][int(ei[_abi.EI["SCEN"], e])])
        lane = descs[m]["lanes"][int(i[SI["LANE"], e, 0])]
        ms = float(sb.spawns["max_speed"][int(ei[_abi.EI["SCEN"], e]) * sb.V + int(i[SI["SPAWN"], e, 0])])
        out[e] = gr.traced_f64(lane, f[SF["X"], e, 0], f[SF["Y"], e, 0], f[SF["HX"], e, 0], f[SF["HY"], e, 0], f[SF["SPEED"], e, 0], ms, save_level)
    assert (i[SI["LANE"], :, 0] == p["lane"]).all() and np.array_equal(f[SF["X"], :, 0], p["x"])
    return out[:, 0], out[:, 1], out[:, 2], out[:, 3]


def _launch(eng, expert, obs, act, state, prev, save_level=gr.SAVE_LEVEL, alias=False, tail=4, **kw):
    """One launch into sentinel-filled buffers with `tail` rows behind the last -> applied, state, info, trace as numpy."""
    import torch
    rows = eng.N
    a = torch.full((rows + tail, 1, 2), SENT, dtype=torch.float32, device="cuda")
    a[:rows, 0] = _dev(act)
    applied = a if alias else torch.full((rows + tail, 1, 2), SENT, dtype=torch.float32, device="cuda")
    st = torch.full((rows + tail, ), 9, dtype=torch.uint8, device="cuda")
    st[:rows] = _dev(np.asarray(state, dtype=np.uint8))
    info = torch.full((rows + tail, ), 99, dtype=torch.uint8, device="cuda")
    trace = torch.full((rows + tail, 4), SENT, dtype=torch.float32, device="cuda")
    pf = None if prev is None else _dev(np.where(prev, _abi.F_RESET | _abi.F_ARRIVE, _abi.F_ON_BROKEN).astype(np.int32).reshape(rows, 1))
    torch.cuda.synchronize()
    eng.guardian(expert, save_level, a[:rows], st[:rows], applied[:rows], info[:rows], SEED, TICK, prev_flags=pf, trace=trace[:rows],
                 obs=_dev(obs), **kw)
    if kw.get("group", -1) >= 0:
        eng.group_sync(kw["group"])
    eng.sync()
    ap, s, i, tr = applied.cpu().numpy()[:, 0], st.cpu().numpy(), info.cpu().numpy(), trace.cpu().numpy()
    assert (s[rows:] == 9).all() and (i[rows:] == 99).all() and (tr[rows:] == SENT).all() and (ap[rows:] == SENT).all(), "rows past the end were written"
    return ap[:rows], s[:rows], i[:rows], tr[:rows]


def _expert_alone(eng, expert, x, det=False, seed=SEED, tick=TICK):
    """pgd_mlp_actor_critic without a critic on the rows `x`: the expert's action as that kernel writes it."""
    import torch
    rows = x.shape[0]
    a = torch.zeros((rows, 1, 2), dtype=torch.float32, device="cuda")
    lp = torch.zeros((rows, 1), dtype=torch.float32, device="cuda")
    eng.mlp_actor_critic(expert, None, a, lp, None, seed, tick, obs=_dev(x), deterministic=det, in_dim=x.shape[1])
    eng.sync()
    return a.cpu().numpy()[:, 0]


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.int32), np.ascontiguousarray(b, dtype=np.float32).view(np.int32))


def _setup(descs, ci):
    rows, n, legacy = gr.KERNEL_CASES[ci]
    eng, mb, sb = _engine(descs, rows, n)
    lat, hd, v, f = _pose(eng, descs, sb, gr.pose_cases(descs, rows, ci))
    rng = np.random.default_rng(50 + ci)
    p, _ = ar.make_networks(rng, eng.D + (1 if legacy else 0), 4 + ci % 3)
    p[4][:, :2] *= 0.3  # (means around zero: expert throttles of both signs)
    obs, act = gr.craft_rows(eng.D, n, f, gr.SAVE_LEVEL, ci)
    eng.expert_host = p
    return eng, tuple(_dev(w) for w in p), obs, act, (lat, hd, v, f), rng


@pytest.mark.parametrize("ci", range(len(gr.KERNEL_CASES)))
def test_kernel_cases(descs, tols, ci):
    """One engine per (rows, beams, width) of guardian_ref.KERNEL_CASES: expert bits, traced floats, the rule, aliasing, IMMEDIATE."""
    rows, n, legacy = gr.KERNEL_CASES[ci]
    tol_lat, tol_f = tols
    eng, expert, obs, act, (lat, hd, v, f), rng = _setup(descs, ci)
    try:
        # by the checker alone, before the GPU's answer is looked at: no row inside the tie band, none on the other thresholds
        edge = gr.C_EDGE * f
        band = gr.tie_band(tol_f, edge)
        excluded = (np.abs(obs[:, 0].astype(np.float64) - edge) <= band) | (np.abs(obs[:, 1].astype(np.float64) - edge) <= band)
        assert excluded.sum() == 0, np.nonzero(excluded)[0]
        assert (np.abs(hd) > 5e-4).all() and (np.abs(v - 5.0) > 0.5).all()
        state = rng.integers(0, 2, rows)
        prev = rng.integers(0, 4, rows) == 0
        ap, st, info, tr = _launch(eng, expert, obs, act, state, prev)
        # expert, bit for bit
        x = gr.expert_row(obs, tr[:, 2] if legacy else None)
        assert x.shape[1] == eng.D + (1 if legacy else 0)
        assert _same_bits(tr[:, :2], _expert_alone(eng, expert, x)), "the expert's action is not pgd_mlp_actor_critic's"
        if not legacy:
            assert (tr[:, 2] == 0).all()
        a64, tol = gr.expert_f64(x, eng.expert_host, SEED, np.arange(rows), TICK)  # (and against float64: the network and the noise)
        assert (np.abs(tr[:, :2] - a64) < tol).all()
        # traced floats
        e_f = float(np.abs(tr[:, 3] - f).max())
        e_lat = float(np.abs(tr[:, 2] - lat).max()) if legacy else 0.0
        print("case %s: |f - f64| %.3e (tolerance %.3e), |lateral - f64| %.3e (%.3e); f below its cap in %d of %d rows" % (
            gr.KERNEL_CASES[ci], e_f, tol_f, e_lat, tol_lat, int((f < 5.0).sum()), rows))
        assert e_f <= tol_f and e_lat <= tol_lat
        # the rule, teacher-forced on the traced expert action: equal
        w_ap, w_st, w_info, fired = gr.guardian_f64(obs, n, act, tr[:, :2], hd, v, f, gr.SAVE_LEVEL, state, prev)
        assert np.array_equal(ap, w_ap.astype(np.float32)) and np.array_equal(st, w_st) and np.array_equal(info, w_info)
        if rows >= 33:
            assert fired["out"].any() and fired["side"].any() and (~fired["out"]).any() and (info & gr.TAKEOVER).any() and (info & gr.TAKEOVER_END).any()
        # d_applied may alias d_agent_actions
        ap2, st2, info2, tr2 = _launch(eng, expert, obs, act, state, prev, alias=True)
        assert _same_bits(ap2, ap) and np.array_equal(st2, st) and np.array_equal(info2, info) and _same_bits(tr2, tr)
        # IMMEDIATE: the same info bits, the correction applied wherever it was raised; no previous flags at all
        ap3, st3, info3, _ = _launch(eng, expert, obs, act, state, None, immediate=True)
        w_ap, w_st, w_info, _ = gr.guardian_f64(obs, n, act, tr[:, :2], hd, v, f, gr.SAVE_LEVEL, state, np.zeros(rows, bool), immediate=True)
        assert np.array_equal(ap3, w_ap.astype(np.float32)) and np.array_equal(st3, w_st) and np.array_equal(info3, w_info)
    finally:
        eng.close()


def test_normalisation_table_is_ignored_and_deterministic_is_the_mean(descs):
    import torch
    for ci in (0, 1):  # 64 rows x 240 beams, with and without the lateral float
        rows, n, legacy = gr.KERNEL_CASES[ci]
        eng, expert, obs, act, (lat, hd, v, f), rng = _setup(descs, ci)
        try:
            zeros = np.zeros(rows, dtype=np.uint8)
            _, _, _, tr = _launch(eng, expert, obs, act, zeros, None)
            _, _, _, tr_det = _launch(eng, expert, obs, act, zeros, None, deterministic=True)
            x = gr.expert_row(obs, tr[:, 2] if legacy else None)
            assert _same_bits(tr_det[:, :2], _expert_alone(eng, expert, x, det=True))
            assert not _same_bits(tr_det[:, :2], tr[:, :2])
            rec, table = eng.obs_norm_state(eng.D)
            table.copy_(_dev(rng.uniform(0.5, 2.0, size=tuple(table.shape)).astype(np.float32)))
            eng.obs_norm_bind(table, eng.D, 1.5)
            _, _, _, tr_bound = _launch(eng, expert, obs, act, zeros, None)
            eng.obs_norm_bind(None, eng.D, 1.5)
            assert _same_bits(tr_bound, tr), "a bound normalisation table reached the expert"
            torch.cuda.synchronize()
        finally:
            eng.close()


def test_regimes_and_refusals(descs):
    import ctypes as C
    import torch
    from pgdrive_amd.engine import PgdError
    eng, expert, obs, act, (lat, hd, v, f), rng = _setup(descs, 5)  # 15 rows x 72 beams, plain
    try:
        rows = eng.N
        ones = np.ones(rows, dtype=np.uint8)
        for s, name in ((1.0, "expert"), (0.95, "expert"), (2.0 ** -10, "agent"), (0.0, "agent")):
            ap, st, info, tr = _launch(eng, expert, obs, act, ones, None, save_level=s)
            w_ap, w_st, w_info, _ = gr.guardian_f64(obs, 72, act, tr[:, :2], hd, v, f, s, ones, np.zeros(rows, bool))
            assert np.array_equal(ap, w_ap.astype(np.float32)) and np.array_equal(st, w_st) and np.array_equal(info, w_info), s
            assert _same_bits(ap, tr[:, :2] if name == "expert" else act), s
            assert (info == (gr.TAKEOVER if name == "expert" else gr.TAKEOVER_END)).all(), s
        # refused: a value network, an unknown mode bit, a width that is neither D nor D + 1, misaligned buffers
        with pytest.raises(AssertionError):
            eng.guardian(tuple(_dev(w) for w in ar.make_networks(rng, eng.D + 2, 4)[0]), 0.5, _dev(act).view(rows, 1, 2),
                         torch.zeros(rows, dtype=torch.uint8, device="cuda"), torch.zeros((rows, 1, 2), device="cuda"),
                         torch.zeros(rows, dtype=torch.uint8, device="cuda"), 0, 0)
        nets = _abi.ActorCritic()
        nets.w1, nets.b1, nets.w2, nets.b2, nets.w3, nets.b3 = [w.data_ptr() for w in expert]
        nets.out_cols = int(expert[4].shape[1])
        buf = torch.zeros((rows, 2), device="cuda")
        st8 = torch.zeros(rows, dtype=torch.uint8, device="cuda")
        info8 = torch.zeros(rows, dtype=torch.uint8, device="cuda")
        o = _dev(obs)

        def call(cfg, nets=nets, a=buf, applied=buf, stride=eng.D):
            return eng.L.pgd_guardian(eng.h, -1, C.c_void_p(o.data_ptr()), stride, C.byref(nets), C.byref(cfg), C.c_void_p(a.data_ptr()), None,
                                      C.c_void_p(st8.data_ptr()), C.c_void_p(applied.data_ptr()), C.c_void_p(info8.data_ptr()), None)
        good = _abi.GuardianConfig(eng.D, 0.5, 0, 0, 0)
        assert call(good) == 0
        assert call(_abi.GuardianConfig(eng.D, 0.5, 0, 0, 8)) == 1
        assert call(_abi.GuardianConfig(eng.D + 1, 0.5, 0, 0, 0)) == 1
        assert call(_abi.GuardianConfig(eng.D, 0.5, 0, 0, _abi.GUARD_LEGACY_LATERAL)) == 1
        assert call(_abi.GuardianConfig(eng.D, float("nan"), 0, 0, 0)) == 1
        assert call(good, stride=eng.D - 1) == 1
        with_critic = _abi.ActorCritic.from_buffer_copy(nets)
        with_critic.vw1 = with_critic.vb1 = with_critic.vw2 = with_critic.vb2 = with_critic.vw3 = with_critic.vb3 = expert[1].data_ptr()
        assert call(good, nets=with_critic) == 1
        odd = torch.zeros((rows * 2 + 1, ), device="cuda")[1:]
        assert call(good, a=odd) == 1 and call(good, applied=odd) == 1
        eng.sync()
    finally:
        eng.close()
    # refused engines: fewer than 40 beams, several agent seats
    from pgdrive_amd.engine import Engine
    mb, sb = util.make_banks(descs, n_maps=4, num_traffic=0)
    small = Engine(_abi.make_config(4, num_traffic=0, num_lasers=39, seed=2), mb, sb)
    try:
        small.reset(np.arange(4))
        p, _ = ar.make_networks(np.random.default_rng(0), small.D, 4)
        with pytest.raises(PgdError, match="status 1"):
            small.guardian(tuple(_dev(w) for w in p), 0.5, torch.zeros((4, 1, 2), device="cuda"), torch.zeros(4, dtype=torch.uint8, device="cuda"),
                           torch.zeros((4, 1, 2), device="cuda"), torch.zeros(4, dtype=torch.uint8, device="cuda"), 0, 0)
    finally:
        small.close()


def test_sequence_of_five_launches_with_a_reset_in_the_middle(descs):
    """The state lives on the device from launch to launch; launch 2 is handed PGD_F_RESET for a third of the rows."""
    import torch
    eng, expert, obs0, act0, (lat, hd, v, f), rng = _setup(descs, 2)  # 33 rows x 72 beams, the lateral float
    try:
        rows, n = eng.N, 72
        st = torch.zeros(rows, dtype=torch.uint8, device="cuda")
        info = torch.zeros(rows, dtype=torch.uint8, device="cuda")
        trace = torch.zeros((rows, 4), device="cuda")
        applied = torch.zeros((rows, 1, 2), device="cuda")
        w_state = np.zeros(rows, dtype=np.uint8)
        seen = 0
        for k in range(5):
            obs, act = gr.craft_rows(eng.D, n, f, gr.SAVE_LEVEL, 100 + k % 2)  # (two alternating sets: corrections that persist and that end)
            prev = (np.arange(rows) % 3 == 0) if k == 2 else np.zeros(rows, bool)
            pf = _dev(np.where(prev, _abi.F_RESET, 0).astype(np.int32).reshape(rows, 1))
            eng.guardian(expert, gr.SAVE_LEVEL, _dev(act).view(rows, 1, 2), st, applied, info, SEED, k, prev_flags=pf, trace=trace, obs=_dev(obs))
            eng.sync()
            tr = trace.cpu().numpy()
            w_ap, w_state, w_info, _ = gr.guardian_f64(obs, n, act, tr[:, :2], hd, v, f, gr.SAVE_LEVEL, w_state, prev)
            assert np.array_equal(applied.cpu().numpy()[:, 0], w_ap.astype(np.float32)), k
            assert np.array_equal(st.cpu().numpy(), w_state) and np.array_equal(info.cpu().numpy(), w_info), k
            seen |= int(np.bitwise_or.reduce(w_info))
        assert seen == gr.TAKEOVER | gr.TAKEOVER_START | gr.TAKEOVER_END
    finally:
        eng.close()


def test_env_group_launch_writes_its_rows_only(descs):
    eng, expert, obs, act, (lat, hd, v, f), rng = _setup(descs, 0)  # 64 rows
    try:
        rows = eng.N
        state = rng.integers(0, 2, rows)
        whole = _launch(eng, expert, obs, act, state, None, tail=0)
        eng.set_groups(2)
        ap, st, info, tr = _launch(eng, expert, obs, act, state, None, tail=0, group=1)
        lo = slice(0, rows // 2)
        hi = slice(rows // 2, rows)
        assert (ap[lo] == SENT).all() and (info[lo] == 99).all() and (tr[lo] == SENT).all() and np.array_equal(st[lo], state[lo])
        for got, want in zip((ap, st, info, tr), whole):
            assert np.array_equal(got[hi], want[hi])  # (the noise is that of the GLOBAL row)
    finally:
        eng.close()


def test_first_call_inside_a_graph_capture_and_the_device_tick(descs):
    import torch
    rows, n, legacy = gr.KERNEL_CASES[0]
    eng, mb, sb = _engine(descs, rows, n)  # fresh: no guardian launch before the capture
    try:
        rng = np.random.default_rng(9)
        p, _ = ar.make_networks(rng, eng.D + 1, 4)
        expert = tuple(_dev(w) for w in p)
        obs = eng.obs.view(rows, -1).clone()
        act = _dev(rng.uniform(-1, 1, size=(rows, 1, 2)).astype(np.float32))
        st = torch.zeros(rows, dtype=torch.uint8, device="cuda")
        info = torch.zeros(rows, dtype=torch.uint8, device="cuda")
        trace = torch.zeros((rows, 4), device="cuda")
        applied = torch.zeros((rows, 1, 2), device="cuda")
        counter = torch.zeros(1, dtype=torch.int32, device="cuda")
        eng.actor_critic_tick(counter)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):  # (the engine moves to the capture's stream outside the capture; no guardian launch yet)
            eng.lane_keep_actions(torch.zeros((rows, 1, 2), device="cuda"), 0)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()   # (its own capture: the first call on a fresh engine is made inside the capture, nothing runs eagerly in front)
        with torch.no_grad(), torch.cuda.graph(g, stream=s):
            eng.guardian(expert, 1.0, act, st, applied, info, SEED, 3, trace=trace, obs=obs)
            counter.add_(1)
        torch.cuda.synchronize()
        draws = []
        with torch.cuda.stream(s), torch.no_grad():
            for k in range(3):
                g.replay()
                torch.cuda.synchronize()
                draws.append(trace.cpu().numpy().copy())
                assert np.array_equal(info.cpu().numpy(), np.full(rows, gr.TAKEOVER_START if k == 0 else gr.TAKEOVER))
                assert _same_bits(applied.cpu().numpy()[:, 0], act.cpu().numpy()[:, 0] if k == 0 else draws[k][:, :2])  # save_level 1: the expert drives from the second step on
        eng.actor_critic_tick(None)
        del g
        for k in range(3):  # replay k drew with tick 3 + k
            x = gr.expert_row(obs.cpu().numpy(), draws[k][:, 2])
            assert _same_bits(draws[k][:, :2], _expert_alone(eng, expert, x, tick=3 + k)), k
        assert not _same_bits(draws[0][:, :2], draws[1][:, :2])
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# env surface
# ---------------------------------------------------------------------------------------------------------------------
def test_vec_env_with_use_saver(descs):
    """16 envs, 50 steps of an agent that steers hard at full throttle: last_takeover / last_applied_actions equal the calls made by hand
    on a twin env without the guardian; reset() clears the state."""
    import torch
    from pgdrive_amd.rollout import GUARDIAN_SEED_XOR
    from pgdrive_amd.vec_env import PGDriveVecEnv, load_saver_weights
    n = 16
    base = dict(num_envs=n, environment_num=n, start_seed=0, traffic_density=0.1, seed=7)
    env = PGDriveVecEnv(dict(base, use_saver=True, save_level=0.5, saver_weights=FIXTURE))
    twin = PGDriveVecEnv(base)
    try:
        expert = tuple(_dev(w) for w in load_saver_weights(dict(saver_weights=FIXTURE), 274))
        o = env.reset(force_seed=np.arange(n))
        o2 = twin.reset(force_seed=np.arange(n))
        assert _bits_equal(o, o2)
        act = torch.tensor([0.6, 1.0], device="cuda").repeat(n, 1).contiguous()
        st = torch.zeros(n, dtype=torch.uint8, device="cuda")
        info = torch.zeros(n, dtype=torch.uint8, device="cuda")
        applied = torch.zeros((n, 1, 2), device="cuda")
        prev = torch.zeros((n, 1), dtype=torch.int32, device="cuda")
        seen = 0
        n_take = 0
        for t in range(50):
            twin.engine.guardian(expert, 0.5, act.view(n, 1, 2), st, applied, info, 7 ^ GUARDIAN_SEED_XOR, t, prev_flags=prev)
            ob2, r2, d2, f2 = twin.step(applied.view(n, 2))
            prev.copy_(f2.view(n, 1))
            ob, r, d, f = env.step(act)
            torch.cuda.synchronize()
            assert _bits_equal(env.last_takeover, info) and _bits_equal(env.last_applied_actions, applied.view(n, 2)), t
            assert _bits_equal(ob, ob2) and _bits_equal(f, f2), t
            bits = info.cpu().numpy()
            seen |= int(np.bitwise_or.reduce(bits))
            n_take += int((bits & gr.TAKEOVER != 0).sum())
        print("vec env, 16 envs x 50 steps of [0.6, 1]: takeover in %d of 800 env-steps, bits seen %d" % (n_take, seen))
        assert seen & gr.TAKEOVER_START and seen & gr.TAKEOVER and n_take > 0
        assert env.last_takeover.dtype == torch.uint8 and tuple(env.last_applied_actions.shape) == (n, 2)
        env._saver_state.fill_(1)
        env.reset(force_seed=np.arange(n))
        assert int(env._saver_state.sum()) == 0 and int(env.last_takeover.sum()) == 0
        env.step(act)
        torch.cuda.synchronize()
        assert not (env.last_takeover.cpu().numpy() & (gr.TAKEOVER | gr.TAKEOVER_END)).any()  # the first step after a reset can only start one
        assert not hasattr(twin, "last_takeover") and twin.saver is None
    finally:
        env.close()
        twin.close()


def test_vec_env_step_group_runs_the_guardian_on_the_groups_stream():
    """Two env groups stepped one after the other equal the whole env stepped at once: the noise is that of the global row and of the
    group's own step count."""
    import torch
    from pgdrive_amd.vec_env import PGDriveVecEnv
    n = 16
    cfg = dict(num_envs=n, environment_num=n, start_seed=0, traffic_density=0.0, seed=7, use_saver=True, save_level=0.5, saver_weights=FIXTURE)
    whole, split = PGDriveVecEnv(cfg), PGDriveVecEnv(cfg)
    try:
        whole.reset(force_seed=np.arange(n))
        split.reset(force_seed=np.arange(n))
        split.set_groups(2)
        act = torch.tensor([0.6, 1.0], device="cuda").repeat(n, 1).contiguous()
        seen = 0
        for t in range(12):
            ob, _, _, fl = whole.step(act)
            for g in (0, 1):
                ob_g, _, _, fl_g = split.step_group(g, act)
                split.group_sync(g)
                sl = split.group_slice(g)
                torch.cuda.synchronize()
                assert _bits_equal(ob_g, ob[sl]) and _bits_equal(fl_g, fl[sl]), (t, g)
            assert _bits_equal(split.last_takeover, whole.last_takeover) and _bits_equal(split.last_applied_actions, whole.last_applied_actions), t
            seen |= int(np.bitwise_or.reduce(whole.last_takeover.cpu().numpy()))
        assert seen & gr.TAKEOVER
    finally:
        whole.close()
        split.close()


def test_scalar_env_reports_the_three_info_keys():
    from pgdrive_amd.env import PGDriveEnv
    env = PGDriveEnv(dict(environment_num=1, start_seed=0, traffic_density=0.0, use_saver=True, save_level=1.0, saver_weights=FIXTURE,
                          saver_deterministic=True))
    plain = PGDriveEnv(dict(environment_num=1, start_seed=0, traffic_density=0.0))
    try:
        env.reset()
        plain.reset()
        seq = []
        for t in range(4):
            o, r, d, info = env.step([0.0, 1.0])
            assert {"takeover", "takeover_start", "takeover_end"} <= set(info)
            assert info["raw_action"] == (0.0, 1.0)
            seq.append((info["takeover_start"], info["takeover"], info["takeover_end"]))
        assert seq == [(True, False, False)] + [(False, True, False)] * 3  # save_level 1: the expert drives from the second step on
        assert "takeover" not in plain.step([0.0, 1.0])[3]
    finally:
        env.close()
        plain.close()


# ---------------------------------------------------------------------------------------------------------------------
# collectors
# ---------------------------------------------------------------------------------------------------------------------
COL_N, COL_T, COL_SEED = 16, 8, 3
GKEYS = KEYS + ("applied_actions", "takeover", "guardian_trace")


def _Col(descs):
    """16 envs with traffic, the policy steering to one side (the guardian has something to do), the expert of the fixture at save_level 0.5."""
    return Traffic(descs, COL_N, COL_T, COL_SEED, steer_bias=0.5, expert=FIXTURE)


def test_collector_with_guardian(descs):
    import torch
    from pgdrive_amd.rollout import MultiAgentRolloutCollector
    S = _Col(descs)
    want = synchronised_rollouts(S, 3, guardian=True)
    S.eng.close()
    take = sum(int((r["takeover"] & 1).sum()) for r in want)
    print("collector: takeover in %d of %d env-steps" % (take, 3 * COL_N * COL_T))
    assert take > 0

    # (a) eagerly; the takeover state survives from rollout to rollout and is part of state_dict()
    A = _Col(descs)
    col = make_collector("single", A, guardian=A.guardian)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        for k in range(2):
            batch = col.collect()
            got = _snapshot(batch, GKEYS + ("expert_actions", ))
            for key in GKEYS:
                assert _bits_equal(got[key], want[k][key]), "eager collect %d: %s differs from the calls made by hand" % (k, key)
            assert _bits_equal(got["expert_actions"], want[k]["guardian_trace"][..., :2].contiguous())
            assert tuple(batch["applied_actions"].shape) == (COL_T, COL_N, 2) and batch["takeover"].dtype == torch.uint8
    sd = col.state_dict()
    assert sd["guardian_state"].shape == (COL_N, ) and sd["guardian_state"].dtype == np.uint8
    A.eng.close()

    # (b) one eager rollout, then collect() captured in a HIP graph and replayed twice: the device tick advances the expert's noise too
    B = _Col(descs)
    col = make_collector("single", B, guardian=B.guardian)
    eager_then_graph(col.collect, lambda: _snapshot(col.batch, GKEYS), want)
    B.eng.close()

    # the safe collector takes the same argument: the cost critic beside actor and critic changes nothing of what is applied
    from pgdrive_amd.rollout import SafeRolloutCollector
    Ss = _Col(descs)
    col = SafeRolloutCollector(Ss.eng, Ss.pw, Ss.vw, Ss.vw, COL_T, seed=COL_SEED, guardian=Ss.guardian)
    with torch.no_grad():
        got = _snapshot(col.collect(), GKEYS + ("costs", ))
    for key in ("obs", "actions", "logp", "flags", "applied_actions", "takeover", "guardian_trace"):
        assert _bits_equal(got[key], want[0][key]), "safe collector: %s differs from the calls made by hand" % key
    Ss.eng.close()

    # (c) guardian=None: the bytes of today -- and the agent's own stream under the guardian equals them up to the first step whose
    # applied action differs
    Cc = _Col(descs)
    plain = synchronised_rollouts(Cc, 1)[0]
    Cc.eng.close()
    Dd = _Col(descs)
    col = make_collector("single", Dd, guardian=None)
    with torch.no_grad():
        got = _snapshot(col.collect(), KEYS)
    assert set(col.batch) == set(KEYS) and col.state_dict() == {}
    for key in KEYS:
        assert _bits_equal(got[key], plain[key]), "guardian=None: %s differs from today's calls" % key
    with pytest.raises(NotImplementedError, match="guardian"):
        MultiAgentRolloutCollector(Dd.eng, Dd.pw, Dd.vw, COL_T, guardian=Dd.guardian)
    Dd.eng.close()
    w = want[0]
    differs = (w["applied_actions"] != w["actions"]).any(dim=2).cpu().numpy()  # [T, N]
    checked = 0
    for e in range(COL_N):
        first = int(np.argmax(differs[:, e])) if differs[:, e].any() else COL_T - 1
        for key in ("actions", "logp"):
            assert _bits_equal(w[key][:first + 1, e], plain[key][:first + 1, e]), (key, e, first)
        checked += first + 1
    assert checked >= COL_N and differs.any()


# ---------------------------------------------------------------------------------------------------------------------
# bands
# ---------------------------------------------------------------------------------------------------------------------
def _first_episodes(env, steps, seeds):
    """An agent that always commands [0, 1]: how the first episode of every env ends, and the takeover share.  Nothing waits for the
    device inside the loop but one read every 100 steps."""
    import torch
    n = env.num_envs
    env.reset(force_seed=seeds)
    act = torch.tensor([0.0, 1.0], device="cuda").repeat(n, 1).contiguous()
    alive = torch.ones(n, dtype=torch.bool, device="cuda")
    end = torch.zeros(n, dtype=torch.int32, device="cuda")
    take = torch.zeros((), dtype=torch.int64, device="cuda")
    lived = torch.zeros((), dtype=torch.int64, device="cuda")
    for t in range(steps):
        _, _, done, flags = env.step(act)
        if env.saver is not None:
            take += (((env.last_takeover & 1) != 0) & alive).sum()
        lived += alive.sum()
        d = done != 0
        end = torch.where(alive & d, flags, end)
        alive &= ~d
        if t % 100 == 99 and not bool(alive.any()):
            break
    info = env.info_from_flags(end)
    kinds = {k: int(info[k].sum()) for k in ("arrive_dest", "out_of_road", "crash", "max_step")}
    return kinds, int(alive.sum()), int(take), int(lived)


def test_band_save_level_one_the_expert_drives(descs):
    """save_level = 1.0, saver_deterministic, no traffic, the first 32 maps of PGDrive-v0 (seeds 1000 .. 1031): the agent always commands
    [0, 1]; from the second step on the expert drives.  The host-loop expert of test_reference_expert_across_the_map_bank arrives on 100 of
    its 100 maps, and on 32 of 32 of these; here the first step is the agent's.  Measured: 32 of 32 arrive, the takeover bit set in 11150
    of 11182 env-steps (every step but each env's first); DESIGN section 28.  The floor, 26, is well under the measured count."""
    from pgdrive_amd.vec_env import PGDriveVecEnv
    n = 32
    env = PGDriveVecEnv(dict(num_envs=n, environment_num=n, start_seed=1000, traffic_density=0.0, use_saver=True, save_level=1.0,
                             saver_weights=FIXTURE, saver_deterministic=True))
    try:
        kinds, unfinished, take, lived = _first_episodes(env, 3000, 1000 + np.arange(n))
        print("band, save_level 1.0: %s, %d unfinished; takeover in %d of %d env-steps" % (kinds, unfinished, take, lived))
        assert unfinished == 0 and kinds["arrive_dest"] >= 26
        assert take >= lived - n  # every step but each env's first
    finally:
        env.close()


def test_band_save_level_half_sampled_expert(descs):
    """save_level = 0.5, the sampled expert: out-of-road ends are no more frequent than for the same [0, 1] agent unguarded on the same
    seeds.  Counts and the takeover share are printed; measured: guarded 17 arrive and 15 leave the road, the takeover
    bit set in 1475 of 6427 env-steps; unguarded 32 of 32 leave the road.  No other number is fixed."""
    from pgdrive_amd.vec_env import PGDriveVecEnv
    n = 32
    base = dict(num_envs=n, environment_num=n, start_seed=1000, traffic_density=0.0, seed=3)
    guarded = PGDriveVecEnv(dict(base, use_saver=True, save_level=0.5, saver_weights=FIXTURE))
    bare = PGDriveVecEnv(base)
    try:
        kg, ug, take, lived = _first_episodes(guarded, 1500, 1000 + np.arange(n))
        kb, ub, _, lived_b = _first_episodes(bare, 1500, 1000 + np.arange(n))
        print("band, save_level 0.5: guarded %s (%d unfinished, takeover in %d of %d env-steps); unguarded %s (%d unfinished, %d env-steps)" % (
            kg, ug, take, lived, kb, ub, lived_b))
        assert kg["out_of_road"] <= kb["out_of_road"]
    finally:
        guarded.close()
        bare.close()
