"""Partial resets on the GPU: pgd_reset with an env id list (Engine.reset(scen_ids, env_ids=...)), the way a trainer that steps with
auto_reset=0 restarts the envs that finished, in every engine mode.

  protocol 1   a manual restart equals the automatic one (twin A restarts inside the step, twin B is restarted by id between steps);
  protocol 2   envs are independent: what is not listed is bit-identical to a twin that never reset, what is listed is bit-identical to
               a fresh engine's full reset, and the call writes the rows of the listed envs and no others;
  protocol 3   the rows and the integer state a partial reset leaves, against the oracle's orc_reset of the same list.

tests/test_partial_reset_cpu.py states protocol 1 on the oracle alone.  48 - 66 envs, at most 200 steps, horizon 60.
The modes are RESET_MODES of the table in tests/modes.py; step info, top-down images and env groups have tests of their own in the default mode."""
import ctypes as C

import numpy as np
import pytest

from pgdrive_amd import _abi
from tests import parity
from tests.modes import MODES, Setup, assert_same_state, mask_of, state_of, step_all  # noqa: F401
from tests.parity import OBS_TOL, STATE_OBS_TOL, closed_engines  # noqa: F401 (the fixture closes every engine a test made)

pytestmark = pytest.mark.gpu

SF, SI, EI = _abi.SF, _abi.SI, _abi.EI
PGD_ERR_ARG = 1  # include/pgdrive_hip.h
SENTINEL = -7.0  # no observation value: rows are zero or lie in [0, 1]
RESTARTS_FLOOR = {1: 100}  # by agent seats; any multi-agent mode: 30 (the floors of tests/test_partial_reset_cpu.py)

# the modes of tests/modes.py this module runs (the table has grown since: the launch-form tests sweep all of it)
RESET_MODES = ("default", "general", "pack", "ego_only", "imask_40", "safe", "marl8", "marl40", "marl8_rows", "parking", "tollgate")
ORACLE_MODES = ("default", "general", "pack", "safe", "marl8", "marl40")
SHAPE_MODES = ("default", "pack", "marl8")


def raw_reset(eng, scen_ids, env_ids, obs, n=None):
    """pgd_reset through ctypes, without the synchronisations, checks and copies of Engine.reset; returns the status"""
    return eng.L.pgd_reset(eng.h, None if env_ids is None else env_ids.ctypes.data_as(C.c_void_p), scen_ids.ctypes.data_as(C.c_void_p),
                           len(scen_ids) if n is None else n, C.c_void_p(obs.data_ptr()))


# ---------------------------------------------------------------------------------------------------------------------
# Protocol 1
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", RESET_MODES)
def test_manual_restart_equals_the_automatic_one(descs, mode):
    """Twin A: auto_reset=1, resample_scenario=1.  Twin B: auto_reset=0; after every step the envs whose flags carry F_RESET in A are
    restarted by id with the scenario A's EI_SCEN names, into the buffer B's step wrote.  Every step: reward and done bit-identical,
    flags identical but for F_RESET (and F_NEW in the restarted envs), the rows of the envs that did not restart bit-identical (one
    kernel, one state).  After B's restart: float state (as bits), integer state and env counters (without EI_EPISODES, which only
    the restart inside a step counts) identical; the rows of the restarted envs -- A's from the step, B's from the stand-alone
    observation of the id list -- agree as test_fused_observation_equals_stand_alone_kernels lets those two code instances agree:
    1e-6, beams over it counted and bounded by 1e-5 * beams + 2.  B's restart leaves the rows of every unlisted env as they were."""
    import torch
    s = Setup(descs, mode)
    a, b = s.engine(auto_reset=1, resample_scenario=1), s.engine(auto_reset=0)
    ids0 = np.arange(s.n) % s.n_scen
    assert torch.equal(a.reset(ids0), b.reset(ids0))
    s.stagger(a, b)
    actions = s.actions()
    st = dict(beams=0, grazing=0, worst=0.0)
    restarts = calls = 0
    for t in range(200):
        (ao, ar, ad, af), (bo, br, bd, bf) = step_all((a, b), actions(t))
        assert torch.equal(ar, br) and torch.equal(ad, bd), "reward / done differ at step %d" % t
        listed_t = ((af & _abi.F_RESET) != 0).any(dim=1)
        mask = torch.full_like(af, _abi.F_RESET) | torch.where(listed_t[:, None], _abi.F_NEW, 0).to(af.dtype)
        assert torch.equal(af & ~mask, bf & ~mask) and not bool((bf & _abi.F_RESET).any()), "flags differ at step %d" % t
        assert torch.equal(ao[~listed_t], bo[~listed_t]), "rows of running envs differ at step %d" % t
        listed = listed_t.cpu().numpy()
        if listed.any():
            ids = np.nonzero(listed)[0].astype(np.int32)
            scen = a.get_state()[2][EI["SCEN"], ids]
            rows = b.reset(scen, env_ids=ids)
            assert rows is b.obs and torch.equal(rows[~listed_t], bo[~listed_t]), "rows of unlisted envs rewritten at step %d" % t
            parity.rows_close(ao[listed_t], rows[listed_t], st, a.cfg.num_lasers, 1e-6, tail=s.tail)
            assert_same_state(state_of(a), state_of(b), np.ones(s.n, dtype=bool), "after the restart of step %d" % t)
            restarts += len(ids)
            calls += 1
    s.check_name(a); s.check_name(b)
    print("manual = automatic restart:", mode, "restarts", restarts, "in", calls, "calls; rows worst", st["worst"], "grazing", st["grazing"],
          "of", st["beams"], "beams")
    assert restarts >= RESTARTS_FLOOR.get(s.A, 30)
    assert st["worst"] < 1e-6 and st["grazing"] <= 1e-5 * st["beams"] + 2


# ---------------------------------------------------------------------------------------------------------------------
# Protocol 2
# ---------------------------------------------------------------------------------------------------------------------
def fresh_reset(d, scen_of_env):
    """Engine D restarted as a whole: its rows (a clone) and state"""
    rows = d.reset(scen_of_env).clone()
    return rows, state_of(d, skip=("EPISODES", "STEPS_TOTAL"))  # (a fresh engine's step count starts again)


def partial_reset_checked(b, d, ids, scen, what, reset=None):
    """Restart the envs `ids` of engine B with the scenarios `scen` and hold the result to protocol 2: the call writes the rows of
    the listed envs and no others -- neither in the buffer B's last step wrote nor in a second one filled with a sentinel --, the
    state of every unlisted env keeps its bits, and rows and state of the listed envs are those of the fresh engine D after a full
    reset to the same scenarios.  `reset`: the call under test (default: Engine.reset with the id list), (buffer) -> None."""
    import torch
    n = b.N
    listed = mask_of(n, ids)
    lt = torch.from_numpy(listed).to(b.device)
    before_rows, before_state = b.obs.clone(), state_of(b, skip=())
    sent = torch.full_like(b.obs, SENTINEL)
    if reset is None:
        reset = lambda buf: b.reset(scen, env_ids=ids, out=buf)  # noqa: E731
    reset(sent)  # (a restart is a function of the scenario alone: the second call below changes nothing but the buffer)
    reset(b.obs)
    b.sync()
    assert bool((sent[~lt] == SENTINEL).all()), "%s: rows of unlisted envs written in the second buffer" % what
    assert torch.equal(b.obs[~lt], before_rows[~lt]), "%s: rows of unlisted envs rewritten" % what
    assert torch.equal(sent[lt], b.obs[lt])
    assert_same_state(state_of(b, skip=()), before_state, ~listed, what + ", unlisted envs")
    scen_of_env = np.zeros(n, dtype=np.int32)
    scen_of_env[ids] = scen
    d_rows, d_state = fresh_reset(d, scen_of_env)
    assert torch.equal(b.obs[lt], d_rows[lt]), "%s: rows of the listed envs differ from a fresh engine's" % what
    assert_same_state(state_of(b, skip=("EPISODES", "STEPS_TOTAL")), d_state, listed, what + ", listed envs against a fresh engine")
    ei = b.get_state()[2]
    assert np.array_equal(ei[EI["EPISODES"]], before_state[2][EI["EPISODES"]]) and np.array_equal(ei[EI["STEPS_TOTAL"]], before_state[2][EI["STEPS_TOTAL"]])
    return listed


def run_on(s, b, c, actions, t0, n_steps, touched):
    """B and C go on in lock step: outputs and state of every env that was never restarted stay bit-identical."""
    import torch
    keep = torch.from_numpy(~touched).to(b.device)
    for t in range(t0, t0 + n_steps):
        outs_b, outs_c = step_all((b, c), actions(t))
        for xb, xc, name in zip(outs_b, outs_c, parity.OUTPUTS):
            assert torch.equal(xb[keep], xc[keep]), "%s of envs that were not restarted differs at step %d" % (name, t)
    assert_same_state(state_of(b, skip=()), state_of(c, skip=()), ~touched, "after step %d" % (t0 + n_steps))
    return t0 + n_steps


@pytest.mark.parametrize("mode", RESET_MODES)
def test_envs_are_independent(descs, mode):
    """Engines B and C: one configuration (auto_reset=0), one state, one action stream.  B restarts a list of envs after steps 12, 30
    and 48 -- every fifth env from 1, a descending list that straddles the waves of the modes with several envs per wave, and a
    pair at the two ends --, C never does; D is restarted as a whole.  See partial_reset_checked and run_on for what is held."""
    s = Setup(descs, mode)
    b, c, d = s.engine(auto_reset=0), s.engine(auto_reset=0), s.engine(auto_reset=0)
    ids0 = np.arange(s.n) % s.n_scen
    b.reset(ids0); c.reset(ids0)
    actions = s.actions(5)
    touched = np.zeros(s.n, dtype=bool)
    lists = [np.arange(1, s.n, 5), np.arange(s.n - 2, 0, -7), np.array([s.n - 1, 0])]
    t = run_on(s, b, c, actions, 0, 12, touched)
    for k, ids in enumerate(lists):
        ids = ids.astype(np.int32)
        scen = ((ids + 3 + k) % s.n_scen).astype(np.int32)
        touched |= partial_reset_checked(b, d, ids, scen, "%s, list %d" % (mode, k))
        t = run_on(s, b, c, actions, t, 18, touched)
    s.check_name(b); s.check_name(c)
    assert (~touched).sum() >= s.n // 2


def test_step_info_across_a_partial_reset(descs):
    """enable_step_info() on B and C (auto_reset=0: the caller restarts).  After a partial reset of B and one more step, the info
    values of the unlisted envs are C's, and the listed envs' running cost and energy base have restarted: total_cost is the step's own
    cost and step_energy the new episode's whole energy.  After the episodes have ended (horizon 60) the episode statistics of the
    unlisted envs are C's."""
    import torch
    s = Setup(descs, "default")
    b, c, d = s.engine(auto_reset=0), s.engine(auto_reset=0), s.engine(auto_reset=0)
    ib, ic = b.enable_step_info(costs=(1.0, 0.5, 0.25)), c.enable_step_info(costs=(1.0, 0.5, 0.25))
    ids0 = np.arange(s.n) % s.n_scen
    b.reset(ids0); c.reset(ids0)
    actions = s.actions(5)
    touched = np.zeros(s.n, dtype=bool)
    t = run_on(s, b, c, actions, 0, 20, touched)
    with_cost = np.nonzero(ib["total_cost"].cpu().numpy() > 0)[0][:10]
    ids = np.unique(np.concatenate([with_cost, np.arange(1, s.n, 7)])).astype(np.int32)
    lt = torch.from_numpy(mask_of(s.n, ids)).to(b.device)
    assert len(with_cost) > 0 and bool((ib["episode_energy"][lt] > 0).any())
    touched |= partial_reset_checked(b, d, ids, ((ids + 3) % s.n_scen).astype(np.int32), "step info")
    t = run_on(s, b, c, actions, t, 1, touched)
    for k in _abi.STEP_INFO_FIELDS:
        assert torch.equal(ib[k][~lt], ic[k][~lt]), k
    assert torch.equal(ib["final_observation"][~lt], ic["final_observation"][~lt])
    assert torch.equal(ib["total_cost"][lt], ib["cost"][lt]) and torch.equal(ib["step_energy"][lt], ib["episode_energy"][lt])
    assert bool((ib["episode_length"][lt] == 1).all())
    run_on(s, b, c, actions, t, 60, touched)
    for k in _abi.STEP_INFO_FIELDS:
        assert torch.equal(ib[k][~lt], ic[k][~lt]), k
    assert int(ic["ep_count"][~lt].sum()) >= int((~lt).sum())  # every unlisted env has ended an episode by now
    assert "k_step_info" in b.describe_step() and "specialised for the default single-agent" in b.describe_step()


@pytest.mark.parametrize("image", ["render", "observation"])
def test_topdown_images_across_a_partial_reset(descs, image):
    """Top-down images -- the rendered scene with its trails (pgd_render_topdown; pgd_reset ends the listed envs' trails) and the
    bird's-eye observation with its frame history (pgd_observe_topdown; pgd_reset marks the listed envs' history for refilling) --
    of B, of C that never restarts an env, and of the fresh engine D: after a partial reset the listed envs show D's image, the
    unlisted envs C's, bit for bit, and so on over the next steps."""
    import torch
    from pgdrive_amd import render
    s = Setup(descs, "default")
    b, c, d = s.engine(auto_reset=0), s.engine(auto_reset=0), s.engine(auto_reset=0)
    for e in (b, c, d):
        if image == "render":
            e.enable_render(render.make_config(render.parse_kwargs("top_down", dict(film_size=(128, 128), draw_traffic=True))))
        else:
            e.enable_topdown(_abi.make_topdown_config(resolution=42))
    draw = (lambda e: e.render_topdown().clone()) if image == "render" else (lambda e: e.observe_topdown().clone())
    ids0 = np.arange(s.n) % s.n_scen
    b.reset(ids0); c.reset(ids0)
    actions = s.actions(5)
    touched = np.zeros(s.n, dtype=bool)
    t = 0
    for k in range(15):
        t = run_on(s, b, c, actions, t, 1, touched)
        assert torch.equal(draw(b), draw(c))
    ids = np.arange(2, s.n, 5).astype(np.int32)
    touched |= partial_reset_checked(b, d, ids, ((ids + 3) % s.n_scen).astype(np.int32), "top-down " + image)
    lt = torch.from_numpy(touched).to(b.device)
    pb, pc, pd = draw(b), draw(c), draw(d)
    assert torch.equal(pb[~lt], pc[~lt]), "images of unlisted envs differ from the twin that did not reset"
    assert torch.equal(pb[lt], pd[lt]), "images of the listed envs differ from a fresh engine's"
    assert not torch.equal(pb[lt], pc[lt])
    for k in range(6):
        t = run_on(s, b, c, actions, t, 1, touched)
        assert torch.equal(draw(b)[~lt], draw(c)[~lt])
    s.check_name(b)


def test_partial_reset_confined_to_one_env_group(descs):
    """Two env groups on their own streams: group_sync, a partial reset of envs of group 0 (on the engine's stream), then both
    groups go on stepping.  Group 1 and the unlisted envs of group 0 stay bit-identical to the twin that did not reset."""
    import torch
    s = Setup(descs, "default")
    b, c, d = s.engine(auto_reset=0), s.engine(auto_reset=0), s.engine(auto_reset=0)
    ids0 = np.arange(s.n) % s.n_scen
    b.reset(ids0); c.reset(ids0)
    b.set_groups(2); c.set_groups(2)
    actions = s.actions(5)
    touched = np.zeros(s.n, dtype=bool)

    def steps(t0, k):
        keep = torch.from_numpy(~touched).to(b.device)
        for t in range(t0, t0 + k):
            at = torch.from_numpy(actions(t)).to(b.device)
            torch.cuda.synchronize(b.device)
            for e in (b, c):
                e.step_group(0, at); e.step_group(1, at)
            for e in (b, c):
                e.group_sync(0); e.group_sync(1)
            for xb, xc, name in zip((b.obs, b.reward, b.done, b.flags), (c.obs, c.reward, c.done, c.flags), parity.OUTPUTS):
                assert torch.equal(xb[keep], xc[keep]), "%s differs at step %d" % (name, t)
        assert_same_state(state_of(b, skip=()), state_of(c, skip=()), ~touched, "after step %d" % (t0 + k))
        return t0 + k

    t = steps(0, 12)
    ids = np.arange(s.n // 2 - 1, 0, -3).astype(np.int32)  # group 0 only, up to its last env
    touched |= partial_reset_checked(b, d, ids, ((ids + 3) % s.n_scen).astype(np.int32), "env groups")
    steps(t, 18)
    assert not touched[s.n // 2:].any()
    s.check_name(b)


# ---------------------------------------------------------------------------------------------------------------------
# Id list shapes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["first", "last", "strided_descending", "permutation", "two_calls", "lists_overwritten"])
@pytest.mark.parametrize("mode", SHAPE_MODES)
def test_id_list_shapes(descs, mode, shape):
    """[0]; [N - 1]; a strided list in descending order; a permutation of all N envs, which must equal reset(scen_ids) without ids;
    two disjoint lists in two pgd_reset calls back to back with no synchronisation in between (the second call waits for the event
    that guards the pinned staging: both must have taken effect); one call whose two host arrays are overwritten with other valid ids
    as soon as it returns and before the stream is synchronised (the lists are copied before the call returns).  Twelve steps, the
    restart, twelve more steps: checked as in protocol 2."""
    import torch
    s = Setup(descs, mode)
    b, c, d = s.engine(auto_reset=0), s.engine(auto_reset=0), s.engine(auto_reset=0)
    n = s.n
    ids0 = np.arange(n) % s.n_scen
    b.reset(ids0); c.reset(ids0)
    actions = s.actions(9)
    touched = np.zeros(n, dtype=bool)
    t = run_on(s, b, c, actions, 0, 12, touched)
    reset = None
    if shape == "first":
        ids = np.array([0])
    elif shape == "last":
        ids = np.array([n - 1])
    elif shape == "strided_descending":
        ids = np.arange(n - 1, -1, -4)
    elif shape == "permutation":
        ids = np.random.default_rng(2).permutation(n)
    else:
        ids = np.concatenate([np.arange(2, n, 6), np.arange(n - 1, 0, -6)])  # two disjoint lists
        assert len(set(ids.tolist())) == len(ids)
    ids = ids.astype(np.int32)
    scen = ((ids * 5 + 1) % s.n_scen).astype(np.int32)
    if shape == "two_calls":
        half = len(np.arange(2, n, 6))

        def reset(buf):
            b.sync()
            parts = [(ids[:half].copy(), scen[:half].copy()), (ids[half:].copy(), scen[half:].copy())]
            rcs = [raw_reset(b, sc, ev, buf) for ev, sc in parts]  # back to back
            b.sync()
            assert rcs == [0, 0]
    elif shape == "lists_overwritten":
        def reset(buf):
            b.sync()
            ev, sc = ids.copy(), scen.copy()
            rc = raw_reset(b, sc, ev, buf)
            ev[:] = (ev + 1) % n  # other valid ids and scenarios, before anything is synchronised
            sc[:] = (sc + 1) % s.n_scen
            b.sync()
            assert rc == 0
    touched |= partial_reset_checked(b, d, ids, scen, "%s, %s" % (mode, shape), reset)
    if shape == "permutation":  # the same as a reset without ids
        assert torch.equal(b.obs, d.obs)
        scen_of_env = np.zeros(n, dtype=np.int32)
        scen_of_env[ids] = scen
        rows = b.obs.clone()
        assert torch.equal(b.reset(scen_of_env), rows)
        assert_same_state(state_of(b, skip=("EPISODES", "STEPS_TOTAL")), state_of(d, skip=("EPISODES", "STEPS_TOTAL")), touched, "reset without ids")
    else:
        run_on(s, b, c, actions, t, 12, touched)
    s.check_name(b)


# ---------------------------------------------------------------------------------------------------------------------
# Protocol 3
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ORACLE_MODES)
def test_partial_reset_rows_against_the_oracle(descs, mode):
    """A free-running engine (auto_reset=0) whose finished envs are restarted by id after every step, with scenarios that change from
    restart to restart.  The state right after a restart is a function of the scenario alone, so nothing has drifted: the rows the
    call returns for the listed envs are held to orc_reset's rows of the same list at parity.OBS_TOL / STATE_OBS_TOL, and the listed
    envs' integer state and env counters are the oracle's.  A ray-cast value over the tolerance is admitted only by the oracle's
    BEAM margin (parity.compare_rows, as parity.check_reset_rows does); admitted beams are counted as distinct (scenario, seat,
    column) -- a restart repeats what the scenario's last restart showed -- and bounded by the allowance of the full-reset checks
    of these configurations: 2."""
    s = Setup(descs, mode)
    eng, ora = s.engine(auto_reset=0), s.oracle(auto_reset=0)
    ids0 = np.arange(s.n) % s.n_scen
    eng.reset(ids0); ora.reset(ids0)
    s.stagger(eng)
    actions = s.actions(23)
    stats = parity.new_stats()
    o_rows = np.zeros((s.n, s.A, eng.D), dtype=np.float64)
    admitted = set()
    restarts = 0
    counters = [EI[k] for k in ("SCEN", "NEXT_GROUP", "EP_STEPS", "NEXT_AGENT", "AUX")]
    for t in range(200):
        (obs, rew, done, flags), = step_all((eng, ), actions(t))
        fl = flags.cpu().numpy().astype(np.uint32)
        over = ((fl & _abi.F_ALL_DONE) != 0).any(axis=1) if s.A > 1 else done.cpu().numpy()[:, 0] != 0
        if not over.any():
            continue
        ids = np.nonzero(over)[0].astype(np.int32)
        scen = ((ids * 3 + t) % s.n_scen).astype(np.int32)
        g_rows = eng.reset(scen, env_ids=ids).cpu().numpy().astype(np.float64)
        ora.reset(scen, env_ids=ids, out=o_rows)
        n_cases = len(stats["ties"].cases) if "ties" in stats else 0
        parity.compare_rows(eng, ora, stats, g_rows, o_rows, np.repeat(over[:, None], s.A, axis=1), ora.margins())
        scen_of_env = dict(zip(ids.tolist(), scen.tolist()))
        for case in stats["ties"].cases[n_cases:]:
            w = case["where"]
            if case["cls"] in ("BEAM", "BEAM_SLIDE"):
                admitted.add((scen_of_env[w["env"]], w["agent"], w["fan"], w["beam"]))
        (gf, gi, gei), (of, oi, oei) = eng.get_state(), ora.get_state()
        assert np.array_equal(gi[:, over], oi[:, over]), "integer state of the restarted envs differs at step %d" % t
        assert np.array_equal(gei[counters][:, over], oei[counters][:, over]), "env counters of the restarted envs differ at step %d" % t
        restarts += len(ids)
    s.check_name(eng)
    n_adm = stats.get("grazing", 0) + stats.get("det_grazing", 0)
    print("partial reset rows against the oracle:", mode, "restarts", restarts, "beams compared", stats.get("beams", 0) + stats.get("det_beams", 0),
          "admitted", n_adm, "distinct (scenario, seat, column)", len(admitted), "worst not admitted", stats["obs"], "state columns", stats.get("obs_state"))
    parity.report("partial reset rows", stats)
    assert restarts >= RESTARTS_FLOOR.get(s.A, 30)
    assert stats["obs"] < OBS_TOL and stats["obs_state"] < STATE_OBS_TOL
    assert len(admitted) <= 2 and len(stats["ties"].cases) < 200


# ---------------------------------------------------------------------------------------------------------------------
# Zero-row marks
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["marl8", "marl40", "marl8_rows"])
def test_zero_row_marks_across_a_partial_reset(descs, mode):
    """A multi-agent engine zeroes the row of a seat that is not due once and remembers it per env, with the identity of the buffer
    the marks describe.  Steps into buffer X; a partial reset into a sentinel-filled buffer Y -- the marks of the listed envs now
    describe Y, those of every other env still X --; a step into Y, steps into X again, all through the C ABI (no pgd_forget_rows in
    between).  After each step the buffer just written equals, bit for bit, the buffer of a twin created under PGD_NO_ROWZ=1 that
    rewrites every zero row in every call and only ever uses one buffer: in particular every seat that is not due reads zero."""
    import torch
    s = Setup(descs, mode)
    eng, twin = s.engine(auto_reset=0), s.engine(auto_reset=0, env=dict(PGD_NO_ROWZ="1"))
    ids0 = np.arange(s.n) % s.n_scen
    eng.reset(ids0); twin.reset(ids0)
    actions = s.actions(3)
    x, y = eng.obs, torch.full_like(eng.obs, SENTINEL)
    n_zero = 0

    def step(t, buf):
        nonlocal n_zero
        at = torch.from_numpy(actions(t)).to(eng.device)
        eng._follow_stream()
        ptrs = [C.c_void_p(p.data_ptr()) for p in (at, buf, eng.reward, eng.done, eng.flags)]
        assert eng.L.pgd_step(eng.h, *ptrs) == 0
        to, _, _, tf = twin.step(at)
        eng.sync(); twin.sync()
        assert torch.equal(eng.flags, tf)
        not_due = (tf & (_abi.F_REPORT | _abi.F_NEW)) == 0
        assert not bool(buf[not_due].any()), "a seat that is not due does not read zero after step %d" % t
        assert torch.equal(buf, to), "rows differ from the twin without marks at step %d" % t
        n_zero += int(not_due.sum())

    for t in range(40):
        step(t, x)
    ids = np.arange(1, s.n, 3).astype(np.int32)
    scen = ((ids + 2) % s.n_scen).astype(np.int32)
    listed = torch.from_numpy(mask_of(s.n, ids)).to(eng.device)
    eng.sync()
    assert raw_reset(eng, scen, ids, y) == 0
    eng.sync()
    t_rows = twin.reset(scen, env_ids=ids)
    assert bool((y[~listed] == SENTINEL).all()) and torch.equal(y[listed], t_rows[listed])
    step(40, y)
    for t in range(41, 60):
        step(t, x if t % 2 else y)
    s.check_name(eng)
    print("zero-row marks across a partial reset:", mode, "rows that were not due", n_zero)
    assert n_zero > 100


# ---------------------------------------------------------------------------------------------------------------------
# Refusals
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["default", "pack", "marl8"])
def test_refused_calls_leave_the_engine_as_it_was(descs, mode):
    """A duplicate id, an id outside [0, N) and n > N are PGD_ERR_ARG; Engine.reset raises for len(env_ids) != len(scen_ids) before
    it calls the library (which would read the shorter array past its end).  State and rows are bit-identical afterwards."""
    import torch
    s = Setup(descs, mode)
    eng = s.engine(auto_reset=0)
    n = s.n
    eng.reset(np.arange(n) % s.n_scen)
    actions = s.actions(1)
    for t in range(5):
        step_all((eng, ), actions(t))
    before, rows = state_of(eng, skip=()), eng.obs.clone()
    i32 = lambda *v: np.array(v, dtype=np.int32)  # noqa: E731
    cases = dict(duplicate=(i32(3, 5, 3), i32(0, 1, 2), None), duplicate_adjacent=(i32(n - 1, n - 1), i32(0, 1), None),
                 id_is_n=(i32(1, n), i32(0, 1), None), negative_id=(i32(-1, 2), i32(0, 1), None),
                 n_above_N=(np.arange(n + 1, dtype=np.int32) % n, np.zeros(n + 1, dtype=np.int32), n + 1),
                 n_above_N_no_ids=(None, np.zeros(n + 1, dtype=np.int32), n + 1))
    for name, (ev, sc, cnt) in cases.items():
        assert raw_reset(eng, sc, ev, eng.obs, cnt) == PGD_ERR_ARG, name
        eng.sync()
        assert_same_state(state_of(eng, skip=()), before, np.ones(n, dtype=bool), name)
        assert torch.equal(eng.obs, rows), name
    for ev, sc in ((i32(1, 2), i32(0, 1, 2)), (i32(1, 2, 3), i32(0, 1)), (i32(), i32(0))):
        with pytest.raises(ValueError):
            eng.reset(sc, env_ids=ev)
    assert_same_state(state_of(eng, skip=()), before, np.ones(n, dtype=bool), "length mismatch")
    assert torch.equal(eng.obs, rows)
    eng.reset(i32(1, 0), env_ids=i32(n - 1, 0))  # and a good call still goes through
    assert not np.array_equal(state_of(eng, skip=())[0], before[0])
