"""The admission rule of the parity tests (tests/util.py: admissible, oracle/pgd_oracle.h: ORC_MG_*) checked without a GPU.

  * the margin recorder does not move the oracle's results;
  * the margins themselves against plain numpy float64 on hand-made scenes;
  * honest noise is admitted: a surrogate engine (a second oracle whose pose / speed state is moved by up to 1 fp32 ulp before each
    step, outputs rounded to fp32) goes through the very helpers the GPU tests use -- every difference they see is a verified tie and
    the strict asserts pass;
  * planted errors are caught: the same surrogate altered the way a subtly wrong kernel would be makes the strict asserts fail, while
    the count-only form the suite used before (kept here as `old_form_passes`) lets each of them through;
  * the BEAM predicate flags at most 1 % of the beams of oracle-only rollouts (it cannot degenerate into 'everything is a tie').
"""
import ctypes as C

import numpy as np
import pytest

from pgdrive_amd import _abi
from tests import util
from tests import parity
from tests.parity import OBS_TOL, REW_TOL, PARKED_HIT_SHARE, compare_step, int_ties

SF, SI = _abi.SF, _abi.SI
PERTURBED = ("X", "Y", "THETA", "SPEED")  # the continuous inputs of a step; every other field is a copy, a sum or integer-valued bookkeeping


def _single(descs, n_envs, traffic_mode="respawn", **kw):
    from oracle import orc
    mb, sb = util.make_banks(descs, n_maps=8, num_agents=1, num_traffic=16, traffic_mode=traffic_mode,
                             **{k: kw.pop(k) for k in ("accident_prob", "idm_agent") if k in kw})
    cfg = _abi.make_config(n_envs, num_agents=1, num_traffic=16, num_lasers=kw.pop("num_lasers", 240), auto_reset=1, **kw)
    return cfg, mb, sb, (lambda: orc.Oracle(cfg, mb, sb))


def _marl(n_envs):
    from oracle import orc
    d, mb, sb = util.make_marl_banks(num_agents=12, capacity=16, kind="roundabout")
    cfg = util.marl_config(n_envs, sb, horizon=120)
    return cfg, mb, sb, (lambda: orc.Oracle(cfg, mb, sb))


class Surrogate:
    """Engine-shaped wrapper (step / sync / get_state / set_state / cfg / device) of a second oracle: fp32 outputs, state moved by up to
    1 fp32 ulp per perturbed field before each step; `plant` alters its outputs the way a subtly wrong kernel would."""
    device = "cpu"

    def __init__(self, make, cfg, seed=0, plant=None):
        self.o, self.cfg, self.rng, self.plant, self.planted = make(), cfg, np.random.default_rng(seed), plant, 0
        self.o.enable_margins()
        self.A = cfg.num_agents

    def reset(self, ids):
        return self.o.reset(ids).astype(np.float32)

    def set_state(self, f, i, ei):
        f32 = np.asarray(f, dtype=np.float32).copy()
        for name in PERTURBED:
            v = f32[SF[name]]
            step = self.rng.integers(-1, 2, size=v.shape)
            step[v == 0.0] = 0
            f32[SF[name]] = np.where(step > 0, np.nextafter(v, np.float32(np.inf)), np.where(step < 0, np.nextafter(v, np.float32(-np.inf)), v))
        self.o.set_state(f32.astype(np.float64), i, ei)

    def sync(self):
        pass

    def _leader_gaps(self):
        """front gap on the own lane of every active IDM-driven slot, from the state the step starts from (orc_find_front_back)"""
        f, i, ei = self.o.get_state()
        gaps = np.full(i.shape[1:], np.inf)
        objs, dist = np.zeros(6, dtype=np.int32), np.zeros(6, dtype=np.float64)
        for e, s in zip(*np.nonzero(i[SI["STATUS"]] == _abi.ST_ACTIVE)):
            if s < self.A and not self.cfg.idm_agent:
                continue
            lane = i[SI["RLANE"], e, s] if i[SI["RLANE"], e, s] >= 0 else i[SI["LANE"], e, s]
            self.o.L.orc_find_front_back(self.o.h, int(e), int(s), int(lane), 1, objs.ctypes.data_as(C.c_void_p), dist.ctypes.data_as(C.c_void_p))
            if objs[1] >= 0:
                gaps[e, s] = dist[1]
        return gaps, np.abs(f[SF["SPEED"]]) * 3.6

    def step(self, act):
        import torch
        if self.plant == "max_dist":
            gaps, speed = self._leader_gaps()
        obs, rew, done, flags = self.o.step(act.numpy())
        obs, rew = obs.astype(np.float32), rew.astype(np.float32)
        self.state = [x.copy() for x in self.o.get_state()]
        mg = self.o.margins()
        if self.plant == "beam":  # (a) one beam per 10^5 replaced by its neighbour beam's value
            nl = self.cfg.num_lasers
            lid = obs[:, :, -nl:]
            for _ in range(self.rng.poisson(lid.size / 1e5)):
                cand = np.argwhere(np.abs(lid[:, :, 1:] - lid[:, :, :-1]) > 0.01)
                if len(cand):
                    e, a, b = cand[self.rng.integers(len(cand))]
                    lid[e, a, b] = lid[e, a, b + 1]
                    self.planted += 1
        if self.plant == "max_dist":  # (b) a leader search with max_dist 29.9 instead of 30: the leader is dropped, free-road acceleration
            f = self.state[0]
            for e, s in zip(*np.nonzero((gaps > 29.9) & (gaps < 30.0))):
                if self.state[1][SI["STATUS"], e, s] == _abi.ST_ACTIVE:
                    f[SF["ACT1T"], e, s] = f[SF["THROTTLE"], e, s] = 1.0 - (speed[e, s] / f[SF["TARGET_SPEED"], e, s]) ** 10
                    self.planted += 1
        if self.plant == "crash" and not self.planted:  # (c) one CRASH_VEHICLE bit cleared where the SAT gap is < -0.05 m
            hit = ((flags & _abi.F_CRASH_VEHICLE) != 0) & (mg[util.MG["CONTACT"]][:, :self.A] > 0.05)
            if hit.any():
                e, a = np.argwhere(hit)[0]
                flags[e, a] &= ~np.uint32(_abi.F_CRASH_VEHICLE)
                self.planted += 1
        if self.plant == "lane" and not self.planted:  # (d) one SI_LANE moved to the adjacent lane although the vehicle is mid-box
            i = self.state[1]
            mid = (i[SI["STATUS"]] == _abi.ST_ACTIVE) & (mg[util.MG["LANE"]] > 0.5) & np.isfinite(mg[util.MG["LANE"]])
            mid[:, :self.A] = False  # (a traffic vehicle: the agent's lane also feeds its reward)
            if mid.any():
                e, s = np.argwhere(mid)[0]
                i[SI["LANE"], e, s] += 1
                self.planted += 1
        return (torch.from_numpy(obs), torch.from_numpy(rew), torch.from_numpy(done), torch.from_numpy(flags.astype(np.int64)))

    def get_state(self):
        f, i, ei = self.state
        return f.astype(np.float32), i, ei


def _run(make, cfg, n_steps, actions, plant=None, seed=0, park_ego=False):
    """The teacher-forced loop of the GPU tests with the surrogate in the engine's place.  Returns the statistics of the strict form
    (stats, worst, idm_ties, active) and the counts the count-only form of the suite looked at (old)."""
    ora, eng = make(), Surrogate(make, cfg, seed=seed, plant=plant)
    ora.enable_margins()
    n = cfg.num_envs
    ids = np.arange(n) % 8
    o0 = ora.reset(ids)
    assert np.abs(eng.reset(ids) - o0).max() < OBS_TOL
    rng = np.random.default_rng(seed + 100)
    stats = dict(steps=0, flag_mismatch=0, obs=0.0, rew=0.0)
    old = dict(grazing=0, beams=0, flag_mismatch=0, int_mismatch=0, idm_ties=0)
    worst, idm_ties, active = {}, 0, 0
    A = cfg.num_agents
    for t in range(n_steps):
        act = actions(rng, n, A) * (0.0 if park_ego else 1.0)
        compare_step(eng, ora, act, stats)
        mg = stats["ties"].mg
        f, i, ei = ora.get_state()
        gf, gi, gei = eng.get_state()
        agree = (gi == i).all(axis=0) & (gei == ei).all(axis=0)[:, None]
        int_ties(gi, i, gei, ei, mg, stats, stats["ties"].flag_tie)
        tie = util.idm_tie(gf, f, mg)
        if not cfg.idm_agent:
            tie[:, :A] = False
        idm_ties += int((tie & agree).sum())
        active += int((i[SI["STATUS"]][:, A:] == _abi.ST_ACTIVE).sum())
        util.compare_state(gf, f, agree & ~tie, worst, skip=("LASTX", "LASTY", "LASTHX", "LASTHY"))  # (copies of the perturbed input)
        # the count-only form: what differs by more than the tolerance IS the tie
        old["int_mismatch"] += int((gi != i).any(axis=0).sum()) + int((gei != ei).any(axis=0).sum())
        old["idm_ties"] += int((util.throttle_differs(gf, f) & agree).sum())
        f32 = util.round_state_f32(f)
        ora.set_state(f32, i, ei)
        eng.set_state(f32, i, ei)
    old["flag_mismatch"] = stats["flag_mismatch"] + stats.get("flag_ties", 0)
    old["beams"] = stats.get("beams", 0)
    old["grazing"] = stats.get("grazing", 0) + stats.get("beams_not_admitted", 0)
    return dict(stats=stats, worst=worst, idm_ties=idm_ties, active=active, old=old, planted=eng.planted)


def strict_form_passes(r, flag_allowance=0, int_allowance=0):
    s = r["stats"]
    return (s["obs"] < OBS_TOL and s["rew"] < REW_TOL and s["flag_mismatch"] == 0 and s.get("flag_ties", 0) <= flag_allowance and
            s["int_mismatch"] == 0 and s["int_ties"] <= int_allowance and not util.state_failures(r["worst"]) and
            r["idm_ties"] <= 2e-3 * max(r["active"], 1) + 2 and s.get("grazing", 0) <= 1e-5 * s.get("beams", 1) + 2)


def old_form_passes(r):
    """The 'before': mismatches are ties BECAUSE they exceed the tolerance, and only counted (the loosest bounds the suite had: flags
    and integer state of test_marl_roundabout_parity / the fuzz tests, beams and IDM ties of test_teacher_forced_parity)."""
    o = r["old"]
    allowed_flags, allowed_ints = 1, 2
    return (not o["flag_mismatch"] > allowed_flags and not o["int_mismatch"] > allowed_ints and
            o["idm_ties"] <= 2e-3 * max(r["active"], 1) + 2 and
            o["grazing"] <= 1e-5 * o["beams"] + 2)


def _actions_single(rng, n, a):
    return util.driving_actions(rng, n)


# ---------------------------------------------------------------------------------------------------------------------
def test_recording_margins_does_not_move_the_oracle(descs):
    """orc_step with the recorder on and off: obs / reward / done / flags / state bit-identical (single agent with respawn traffic and
    objects, and the 12-of-16 roundabout)."""
    for (cfg, mb, sb, make), actions in ((_single(descs, 32, accident_prob=0.8), _actions_single), (_marl(16), util.marl_actions)):
        a, b = make(), make()
        b.enable_margins()
        ids = np.arange(cfg.num_envs) % 8
        assert np.array_equal(a.reset(ids), b.reset(ids))
        rng = np.random.default_rng(3)
        seen = 0
        for t in range(150):
            act = actions(rng, cfg.num_envs, cfg.num_agents)
            ra, rb = a.step(act), b.step(act)
            for x, y in zip(ra, rb):
                assert np.array_equal(x, y), t
            for x, y in zip(a.get_state(), b.get_state()):
                assert np.array_equal(x, y), t
            seen += int(np.isfinite(b.margins()[1:6]).sum())
        assert seen > 1000  # (and it did record)
        b.enable_margins(False)
        for x, y in zip(a.step(act), b.step(act)):
            assert np.array_equal(x, y)


@pytest.mark.parametrize("case", ["trigger", "respawn", "respawn-parked", "roundabout"])
def test_honest_noise_is_admitted(descs, case):
    """The reference alone stays inside the caps: 64 envs x 300 steps of the surrogate against the unperturbed oracle."""
    if case == "roundabout":
        cfg, mb, sb, make = _marl(64)
        r = _run(make, cfg, 300, util.marl_actions)
    else:
        cfg, mb, sb, make = _single(descs, 64, traffic_mode=case.split("-")[0])
        r = _run(make, cfg, 300, _actions_single, park_ego=case.endswith("parked"))
    print("honest noise", case, r["stats"], "idm ties", r["idm_ties"], "of", r["active"], util.state_failures(r["worst"]), r["old"])
    assert strict_form_passes(r, flag_allowance=2, int_allowance=2), (r["stats"], util.state_failures(r["worst"]))


@pytest.mark.parametrize("plant", ["beam", "max_dist", "crash", "lane"])
def test_planted_errors_are_caught(descs, plant):
    """(a) one beam per 10^5 takes its neighbour's value, (b) the leader search stops at 29.9 m, (c) one CRASH_VEHICLE bit is lost where
    the boxes overlap by more than 5 cm, (d) one lane id is off by one in the middle of a lane box: the strict form fails on each, the
    count-only form the suite had before lets each through."""
    # (the leader plant in trigger mode: there the platoons of the spawn grid drive apart through the 29.9 - 30 m window)
    cfg, mb, sb, make = _single(descs, 64, traffic_mode="trigger" if plant == "max_dist" else "respawn")
    r = _run(make, cfg, 300 if plant == "max_dist" else 200, _actions_single, plant=plant)
    print("planted", plant, r["planted"], r["stats"], "idm ties", r["idm_ties"], "of", r["active"], util.state_failures(r["worst"]), r["old"])
    assert r["planted"] > 0
    assert not strict_form_passes(r, flag_allowance=2, int_allowance=2)
    assert old_form_passes(r)


# ---------------------------------------------------------------------------------------------------------------------
# the margins themselves, against plain numpy float64 on hand-made scenes
# ---------------------------------------------------------------------------------------------------------------------
def _scene(descs, **kw):
    """One env after reset, every slot but the ego's emptied: (cfg, map bank, scenario bank, oracle, f, i, ei)."""
    cfg, mb, sb, make = _single(descs, 1, traffic_mode="trigger", **kw)
    ora = make()
    ora.enable_margins()
    ora.reset([0])
    f, i, ei = ora.get_state()
    i[SI["STATUS"], 0, 1:] = _abi.ST_EMPTY
    return cfg, mb, sb, ora, f, i, ei


def _dims(sb, i, s):
    r = sb.spawns[int(i[SI["SPAWN"], 0, s])]  # (scenario 0: its spawn block starts the table)
    return float(r["length"]), float(r["width"]), int(r["kind"])


def _put(f, i, s, x, y, th, status):
    f[SF["X"], 0, s], f[SF["Y"], 0, s], f[SF["THETA"], 0, s] = x, y, th
    i[SI["STATUS"], 0, s] = status


@pytest.mark.parametrize("shape", ["box", "circle"])
def test_beam_margin_is_the_distance_to_the_corner(descs, shape):
    """A body whose edge runs parallel to a chosen beam at a known distance d (corner d outside the beam: a miss; d inside: a hit), 20 m
    out: the BEAM margin is d to 1e-9 m, and the oracle's reading flips with the side.  Box and circle, headings on both sides of the
    [-3 pi / 2, pi / 2) seam, first / last / a middle beam."""
    cfg, mb, sb, ora, f, i, ei = _scene(descs, **(dict(accident_prob=1.0) if shape == "circle" else {}))
    kinds = [_dims(sb, i, s)[2] for s in range(1, cfg.num_agents + cfg.num_traffic)]
    body = 1 + kinds.index(1 if shape == "circle" else 0)
    length, width, kind = _dims(sb, i, body)
    px, py = f[SF["X"], 0, 0], f[SF["Y"], 0, 0]
    n, R, checked = cfg.num_lasers, float(cfg.lidar_dist), 0
    for th in (-1.5 * np.pi + 1e-3, 0.5 * np.pi - 1e-3, -1.0, 0.3):
        for beam in (0, n - 1, 77):
            ang = th + beam * 2 * np.pi / n
            u, nrm = np.array([np.cos(ang), np.sin(ang)]), np.array([-np.sin(ang), np.cos(ang)])
            for d in (1e-6, 1e-4, 1e-2, 1.0):
                for side in (+1, -1):  # +: the corner lies d off the beam (miss), -: d across it (hit)
                    half = 0.5 * length if shape == "circle" else 0.5 * width
                    c = np.array([px, py]) + 20.0 * u + (half + side * d) * nrm
                    _put(f, i, 0, px, py, th, _abi.ST_ACTIVE)
                    _put(f, i, body, c[0], c[1], ang, _abi.ST_DYING)  # (in the world, not driven)
                    ora.set_state(f, i, ei)
                    obs = ora.observe()
                    # (1 m across the beam: past the middle of a 1.85 m wide box its other corner is the nearer one; past a cone altogether)
                    off = abs(half + side * d)
                    expect = abs(off - half) if shape == "circle" else (d if side > 0 else min(d, 2 * half - d))
                    hit = off < half if shape == "circle" else (side < 0 and d < 2 * half)
                    assert abs(ora.beam_margin(0, 0, 0, beam) - expect) < 1e-9, (th, beam, d, side, ora.beam_margin(0, 0, 0, beam))
                    assert (obs[0, 0, -n + beam] < 1.0) == hit, (th, beam, d, side)
                    assert util.admissible("BEAM", ora.beam_margin(0, 0, 0, beam), R) == (expect < util.tie_eps("BEAM", R))
                    checked += 1
    assert checked == 96


def _np_gap(a, b):
    """signed SAT gap of two rectangles (x, y, heading, half length, half width) in numpy float64"""
    d = np.array([b[0] - a[0], b[1] - a[1]])
    ua, ub = np.array([np.cos(a[2]), np.sin(a[2])]), np.array([np.cos(b[2]), np.sin(b[2])])
    va, vb = np.array([-ua[1], ua[0]]), np.array([-ub[1], ub[0]])
    c, s = abs(ua @ ub), abs(ua[0] * ub[1] - ua[1] * ub[0])
    return max(abs(d @ ua) - (a[3] + b[3] * c + b[4] * s), abs(d @ va) - (a[4] + b[3] * s + b[4] * c),
               abs(d @ ub) - (b[3] + a[3] * c + a[4] * s), abs(d @ vb) - (b[4] + a[3] * s + a[4] * c))


@pytest.mark.parametrize("rel_deg", [0.0, 30.0, 89.0])
def test_contact_margin_is_the_sat_gap_inside_the_sub_steps(descs, rel_deg):
    """The ego rolls at 10 m/s towards a standing vehicle turned by 0 / 30 / 89 degrees, placed so that the boxes are a known distance
    apart (or into each other) after sub-step 2 of 5: the CONTACT margin is the smallest |SAT gap| over the sub-steps the oracle looked
    at (numpy float64 restatement of the sub-step poses and the gap), to 1e-9 m; the crash flag follows the sign."""
    cfg, mb, sb, ora, f, i, ei = _scene(descs)
    length, width, _ = _dims(sb, i, 0)
    ol, ow, kind = _dims(sb, i, 1)
    assert kind == 0
    sp = sb.spawns[int(i[SI["SPAWN"], 0, 0])]
    x0, y0, th = f[SF["X"], 0, 0], f[SF["Y"], 0, 0], f[SF["THETA"], 0, 0]
    v0, dt = 10.0, float(cfg.dt)
    dv = min(4.0 * 2.0 / float(sp["mass"]), float(sp["friction"]) * 9.81 * dt)  # tb = 0: no engine force, brake value 2 (action_forces)
    poses, x, y, v = [], x0, y0, v0
    for k in range(cfg.decision_repeat):
        x += v * np.cos(th) * dt; y += v * np.sin(th) * dt
        v = max(0.0, v - dv)
        poses.append((x, y, th, 0.5 * length, 0.5 * width))
    assert cfg.decision_repeat == 5
    for d in (1e-6, 1e-4, 1e-2):
        for side in (+1, -1):  # +: d apart after sub-step 2, -: d into each other
            oth = th + np.radians(rel_deg)
            lo, hi = 0.0, 30.0
            for _ in range(200):  # the distance ahead at which the gap after sub-step 2 is side * d (the gap grows with the distance)
                mid = 0.5 * (lo + hi)
                g = _np_gap(poses[1], (x0 + mid * np.cos(th), y0 + mid * np.sin(th), oth, 0.5 * ol, 0.5 * ow))
                lo, hi = (mid, hi) if g < side * d else (lo, mid)
            other = (x0 + hi * np.cos(th), y0 + hi * np.sin(th), oth, 0.5 * ol, 0.5 * ow)
            expect, touched = np.inf, False
            for k in range(5):
                g = _np_gap(poses[k], other)
                expect = min(expect, abs(g))
                if g <= 0:
                    touched = True
                    break
            assert touched and abs(expect - d) < 1e-7
            f2, i2 = f.copy(), i.copy()
            f2[SF["SPEED"], 0, 0] = v0
            _put(f2, i2, 1, other[0], other[1], oth, _abi.ST_DYING)
            ora.set_state(f2, i2, ei)
            o_obs, o_rew, o_done, o_flags = ora.step(np.zeros((1, 1, 2), dtype=np.float32))
            mg = ora.margins()
            assert abs(mg[util.MG["CONTACT"], 0, 0] - expect) < 1e-9, (rel_deg, d, side, mg[util.MG["CONTACT"], 0, 0], expect)
            assert abs(mg[util.MG["CONTACT_LEVER"], 0, 0] - (np.hypot(length, width) + np.hypot(ol, ow)) / 2) < 1e-9
            assert o_flags[0, 0] & _abi.F_CRASH_VEHICLE
            assert bool(util.admitted_slots(mg, ("CONTACT",))[0, 0]) == (d < 1e-2)
            ora.reset([0])


def _np_lane_local(l, x, y):
    """lane_local of oracle/pgd_oracle.c on the ABI's lane record, numpy float64"""
    ax, ay, bx, by, dr = (float(l[k]) for k in ("ax", "ay", "bx", "by", "dir"))
    dx, dy = x - ax, y - ay
    if dr == 0.0:
        return dx * bx + dy * by, -dx * by + dy * bx
    phi = by + ((np.arctan2(dy, dx) - by + np.pi) % (2 * np.pi) - np.pi)
    return dr * (phi - by) * bx, dr * (bx - np.hypot(dx, dy))


def _np_lane_position(l, lon, lat):
    ax, ay, bx, by, dr = (float(l[k]) for k in ("ax", "ay", "bx", "by", "dir"))
    if dr == 0.0:
        return ax + lon * bx - lat * by, ay + lon * by + lat * bx
    phi, r = dr * lon / bx + by, bx - lat * dr
    return ax + r * np.cos(phi), ay + r * np.sin(phi)


@pytest.mark.parametrize("where", ["same_lane", "across_lane_end"])
def test_leader_margin_is_the_distance_to_the_search_range_or_the_rival(descs, where):
    """An IDM-driven ego with one leader at 30 m +- d (found / not found), and with two leaders d apart (which one), on its own lane and
    on the lane that follows it: the LEADER margin is d to 1e-9 m (lane coordinates restated in numpy float64 on the same lane
    records)."""
    cfg, mb, sb, ora, f, i, ei = _scene(descs, idm_agent=True)
    lane_id = int(i[SI["LANE"], 0, 0])
    L = mb.lanes[lane_id]
    x0, y0 = f[SF["X"], 0, 0], f[SF["Y"], 0, 0]
    lon0, lat0 = _np_lane_local(L, x0, y0)
    i[SI["TIMER"], 0, 0] = 0
    if where == "across_lane_end":  # the ego 10 m before the end of its lane, the leaders on the lane that follows
        lon0 = float(L["length"]) - 10.0
        x0, y0 = _np_lane_position(L, lon0, lat0)
        lon0, lat0 = _np_lane_local(L, x0, y0)
        f[SF["X"], 0, 0], f[SF["Y"], 0, 0] = x0, y0
        lead_lane = int(L["succ"][0])
        base = float(L["length"]) - lon0
    else:
        lead_lane, base = lane_id, -lon0
    LL = mb.lanes[lead_lane]

    def leader(slot, gap):
        xs, ys = _np_lane_position(LL, gap - base, lat0)
        i[SI["LANE"], 0, slot] = lead_lane
        _put(f, i, slot, xs, ys, float(f[SF["THETA"], 0, 0]), _abi.ST_DYING)
        return _np_lane_local(LL, xs, ys)[0] + base  # the gap as the oracle will compute it

    out2 = np.zeros(2)
    for d in (1e-6, 1e-4, 1e-2, 1.0):
        for sign in (+1, -1):
            i[SI["STATUS"], 0, 1:] = _abi.ST_EMPTY
            lg = leader(1, 30.0 + sign * d)
            ora.set_state(f, i, ei)
            ora.enable_margins()  # (clears the planes)
            ora.L.orc_idm_act(ora.h, 0, 0, out2.ctypes.data_as(C.c_void_p))
            m = ora.margins()[util.MG["LEADER"], 0, 0]
            assert abs(m - abs(lg - 30.0)) < 1e-9 and abs(m - d) < 1e-5, (where, d, sign, m, lg)
            # two leaders d apart, 20 m ahead
            g1, g2 = leader(1, 20.0), leader(2, 20.0 + sign * d)
            ora.set_state(f, i, ei)
            ora.enable_margins()
            ora.L.orc_idm_act(ora.h, 0, 0, out2.ctypes.data_as(C.c_void_p))
            m = ora.margins()[util.MG["LEADER"], 0, 0]
            assert abs(m - abs(g2 - g1)) < 1e-9 and abs(m - d) < 1e-5, (where, d, sign, m, g1, g2)


# ---------------------------------------------------------------------------------------------------------------------
# how much the predicates flag, oracle alone
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("traffic_mode", ["respawn", "trigger"])
def test_share_of_items_the_predicates_flag(descs, traffic_mode):
    """Oracle-only rollout (64 envs, 100 steps): the BEAM predicate flags at most 1 % of the beams (so it cannot degenerate into
    'everything is a tie'); the slot classes are measured the same way and printed (profiles/parity_ties.md).  LEADER on the 10 m
    spawn grid has exact ties and is high in dense scenes: that is why only DIFFERING and admitted slots are excused and the count
    bounds stay."""
    cfg, mb, sb, make = _single(descs, 64, traffic_mode=traffic_mode)
    ora = make()
    ora.enable_margins()
    ora.reset(np.arange(64) % 8)
    rng = np.random.default_rng(0)
    flagged = sampled = 0
    slots = {c: 0 for c in ("CONTACT", "LANE", "LEADER", "NEIGHBOUR", "ROUTE")}
    active = 0
    for t in range(100):
        ora.step(util.driving_actions(rng, 64))
        mg = ora.margins()
        f, i, ei = ora.get_state()
        act = i[SI["STATUS"]] == _abi.ST_ACTIVE
        active += int(act.sum())
        for c in slots:
            slots[c] += int((util.admitted_slots(mg, (c,)) & act).sum())
        for e, b in zip(rng.integers(0, 64, 200), rng.integers(0, cfg.num_lasers, 200)):
            sampled += 1
            flagged += bool(util.admissible("BEAM", ora.beam_margin(e, 0, 0, b), cfg.lidar_dist))
        ora.set_state(util.round_state_f32(f), i, ei)
    print("flagged share,", traffic_mode, ": BEAM %.5f of %d sampled beams;" % (flagged / sampled, sampled),
          {c: round(n / active, 5) for c, n in slots.items()}, "of", active, "active vehicle-steps")
    assert flagged <= 0.01 * sampled


def test_parked_respawn_hit_share(descs):
    """The figure the GPU test's floor for the parked-ego respawn case is half of (tests/parity.py PARKED_HIT_SHARE): the
    oracle alone on the inputs of test_teacher_forced_parity[16-240-respawn-parked]."""
    cfg, mb, sb, make = _single(descs, 64, traffic_mode="respawn")
    ora = make()
    ora.reset(np.arange(64) % 8)
    hits = beams = 0
    for t in range(400):
        o, r, d, fl = ora.step(np.zeros((64, 1, 2), dtype=np.float32))
        hits += int((o[:, :, -240:] < 1.0).sum()); beams += o[:, :, -240:].size
        f, i, ei = ora.get_state()
        ora.set_state(util.round_state_f32(f), i, ei)
    print("parked ego, respawn traffic: %d of %d beams hit (%.4f)" % (hits, beams, hits / beams))
    assert abs(hits / beams - PARKED_HIT_SHARE) < 5e-4


def test_engine_keywords_are_split_strictly(descs):
    """parity.banks_and_config (the half of parity.engines that needs no GPU): a key that neither the scenario bank nor make_config
    takes is an error -- it used to be dropped, and the test then ran the default configuration --, and for keyword sets of the suite
    the PgdConfig is _abi.make_config's byte for byte and the scenarios are util.make_banks', with the keys both take handed to both."""
    for bad in (dict(lidar_range=40.0), dict(seed=3, crash_vehicle_penalti=1.0)):
        with pytest.raises(TypeError, match=sorted(bad)[0]):
            parity.banks_and_config(descs, 16, **bad)
    for n_maps, bank_kw, cfg_kw in [
            (8, dict(traffic_mode="respawn"), dict(seed=3, resample_scenario=1)),
            (16, dict(num_traffic=56, accident_prob=0.8, density=0.05), dict(num_traffic=56, safe_rl_env=True, use_lateral=False, seed=3)),
            (16, dict(traffic_mode="respawn", idm_agent=1), dict(seed=4, idm_steer_lag=0.2, idm_agent=1)),
            (8, dict(random_agent_model=True), dict(num_lasers=16, lane_line_lasers=33, lane_line_dist=20.0, random_agent_model=True)),
            (8, dict(auto_termination=True, traffic_mode="respawn"), dict(discrete_action=True, increment_steering=True, num_lasers=60)),
            (8, {}, {})]:
        mb, sb, cfg = parity.banks_and_config(descs, 16, n_maps=n_maps, **dict(bank_kw, **cfg_kw))
        assert bytes(cfg) == bytes(_abi.make_config(16, **cfg_kw)), cfg_kw
        mb_ref, sb_ref = util.make_banks(descs, n_maps=n_maps, **bank_kw)
        assert sb.scenarios.tobytes() == sb_ref.scenarios.tobytes() and sb.spawns.tobytes() == sb_ref.spawns.tobytes(), bank_kw
        assert len(mb.descs) == n_maps
