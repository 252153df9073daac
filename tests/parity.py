"""The harness of the GPU parity tests (tests/test_parity_gpu.py, tests/test_parity_wide_gpu.py; tests/test_ties_cpu.py drives it with a
surrogate engine on the CPU): the tolerances, how engines and oracles are built and closed, the comparison of one step against the
oracle with its margin-verified ties (the tie rule itself is tests/util.py), and one loop per comparison protocol -- teacher-forced
against the oracle, twin engines in lock step, the all-maps campaign.  The loops live here; the assertions stay in the tests.

Tolerances: observations are fp32 values in [0,1] -> 1e-5 abs vs the fp64 oracle; rewards 1e-4 (a difference of two
~100 m lane coordinates in fp32); poses 1e-3 m / 1e-4 rad after one step from an identical state; done / flags bit-exact.
"""
import inspect
import os

import numpy as np
import pytest

from pgdrive_amd import _abi, scenario
from tests import util

OBS_TOL = 2.5e-5  # ray-cast columns (lidar, side / lane-line fans): SURVEY 8c's 0.5 mm at the shortest fan range in the suite (20 m)
STATE_OBS_TOL = 1e-5  # every other column (ego state, navigation, neighbour rows): SURVEY 8c's 1e-5, asserted separately
REW_TOL = 2e-4


# ---------------------------------------------------------------------------------------------------------------------
# Building engines: keywords split by signature (an unknown one is an error, not the default configuration), library switches set for
# the construction only, everything handed out closed when the test ends.
# ---------------------------------------------------------------------------------------------------------------------
def _named(*funcs):
    return {p.name for fn in funcs for p in inspect.signature(fn).parameters.values() if p.kind == p.POSITIONAL_OR_KEYWORD}


# what util.make_banks takes by name or hands on (ScenarioBank -> build_scenario), without the arguments they fill in themselves
BANK_KEYS = _named(util.make_banks, scenario.ScenarioBank.__init__, scenario.build_scenario) - {
    "self", "descs", "seeds", "desc", "map_index", "seed", "traffic_seed", "n_maps"}
CONFIG_KEYS = _named(_abi.make_config) - {"num_envs"}


def banks_and_config(descs, n_envs, n_maps=8, **kw):
    """(map bank, scenario bank, PgdConfig) for `kw`: every key goes to util.make_banks, to _abi.make_config or (num_agents,
    num_traffic, random_agent_model, idm_agent) to both; a key neither takes is a TypeError.  Needs no GPU."""
    unknown = sorted(set(kw) - BANK_KEYS - CONFIG_KEYS)
    if unknown:
        raise TypeError("neither the scenario bank nor make_config takes %s" % ", ".join(unknown))
    mb, sb = util.make_banks(descs, n_maps=n_maps, **{k: v for k, v in kw.items() if k in BANK_KEYS})
    return mb, sb, _abi.make_config(n_envs, **{k: v for k, v in kw.items() if k in CONFIG_KEYS})


_open_engines = []


def _setenv(name, value):
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = value


def engine(cfg, mb, sb, env=None, **kw):
    """An Engine created with the library switches `env` (name -> value, None = unset) in the environment: pgd_create reads them, so
    they are put back right after the construction, whatever happens.  The engine is closed when the test ends (closing)."""
    from pgdrive_amd.engine import Engine
    saved = {k: os.environ.get(k) for k in env or {}}
    try:
        for k, v in (env or {}).items():
            _setenv(k, v)
        eng = Engine(cfg, mb, sb, **kw)
    finally:
        for k, v in saved.items():
            _setenv(k, v)
    return closing(eng)


def closing(x):
    """`x` (an engine, or an env that owns one) is closed by close_engines(), i.e. when the test ends."""
    _open_engines.append(x)
    return x


def oracle(cfg, mb, sb):
    from oracle import orc
    ora = orc.Oracle(cfg, mb, sb)
    ora.enable_margins()  # every mismatch the tests tolerate is checked against the oracle's decision margins (tests/util.py)
    ora.map_bank, ora.scen_bank = mb, sb
    return ora


def engines(descs, n_envs, n_maps=8, env=None, **kw):
    """(engine, oracle, config) on the first `n_maps` maps of `descs`; `kw` as in banks_and_config, `env` as in engine."""
    mb, sb, cfg = banks_and_config(descs, n_envs, n_maps, **kw)
    return engine(cfg, mb, sb, env=env), oracle(cfg, mb, sb), cfg


def close_engines():
    while _open_engines:
        _open_engines.pop().close()


@pytest.fixture(autouse=True)
def closed_engines():
    """Imported by the parity test modules: every engine a test got from engine() / engines() / closing() is closed when the test
    ends, pass or fail (a red test does not leave its device memory to the tests after it)."""
    yield
    close_engines()


def new_stats():
    return dict(steps=0, flag_mismatch=0, obs=0.0, rew=0.0)


def driving_with_bursts(rng, n):
    """t -> util.driving_actions, every fourth step with every third env at full steering and throttle (episodes end quickly)"""
    def actions(t):
        act = util.driving_actions(rng, n)
        if t % 4 == 0:
            act[::3, 0, :] = 1.0
        return act
    return actions


def fan_layout(cfg):
    """The ray-cast columns of an observation row: (first column, beams, fan, neighbour rank) with fan 0 = lidar, 1 = side detector,
    2 = lane-line detector (oracle/pgd_oracle.h orc_beam_margin) and rank -1 = the agent's own fan, k = the fan inside the state vector
    of neighbour row k (MA_OTHERS_STATE); and the row width the layout is for."""
    nl, ks, km = cfg.num_lasers, cfg.side_lasers, cfg.lane_line_lasers
    toll = bool(cfg.marl_flags & _abi.MA_TOLLGATE)
    sl = (ks or 2) + 6 + km + (2 if cfg.random_agent_model else 0) + (0 if toll else 10)
    others_state = bool(cfg.marl_flags & _abi.MA_OTHERS_STATE)
    D = sl + (sl if others_state else 4) * cfg.num_others + nl + (2 if toll else 0)
    out = []
    for rank in [-1] + (list(range(cfg.num_others)) if others_state else []):
        off = sl * (rank + 1)
        if ks:
            out.append((off, ks, 1, rank))
        if km:
            out.append((off + (ks or 2) + 6, km, 2, rank))
    if nl:
        out.append((D - (2 if toll else 0) - nl, nl, 0, -1))  # TollGateObservation appends its two floats BEHIND the lidar
    return out, D


def admit_beams(eng, ora, ties, where, layout, lead_tie=None, diff=None):
    """`where`: (env, agent, column) of ray-cast values that differ by more than OBS_TOL (`diff`: by how much).  A beam is a tie only
    where the oracle's geometry says so:
      * its BEAM margin (a box corner / circle / range end / broad-phase radius / the origin on a boundary within eps of the beam, up
        to where the beam ends) is admissible;
      * or the beam slides along the face it ends on: OBS_TOL is SURVEY 8c's 0.5 mm displacement of the geometry for a beam that meets
        its surface head-on; at an angle phi the same displacement moves the reading 1 / sin(phi) times as far (found by
        tests/test_ties_cpu.py: 1 fp32 ulp of pose, 1.5e-5 m, moves a beam that meets a rear face at 0.02 rad by 1.3 mm).  Such a beam is
        admitted where its difference, taken normal to the surface, keeps the tolerance: diff * sin(phi) <= OBS_TOL;
      * or, for lidar beams, it passes within the distance a vehicle with a verified LEADER tie can have moved (another acceleration
        on the two sides: at most g * T^2 / 2, brake limited by friction <= 1 in dynamics()) of that vehicle.
    Returns the admitted ones as a bool array; everything else stays in the numeric comparison and fails there."""
    cfg = eng.cfg
    ranges = {0: cfg.lidar_dist, 1: cfg.side_dist, 2: cfg.lane_line_dist}
    ok = np.zeros(len(where), dtype=bool)
    T = float(cfg.dt) * cfg.decision_repeat
    shift = 0.5 * 9.81 * T * T
    for k, (e, a, col) in enumerate(where):
        start, n, fan, rank = next(x for x in layout if x[0] <= col < x[0] + x[1])
        slot = a if rank < 0 else ora.neighbour_slot(e, a, rank)
        if slot < 0:
            continue
        m = ora.beam_margin(e, a, fan, col - start, slot)
        sin_phi = ora.beam_incidence(e, a, fan, col - start, slot) if diff is not None else 1.0
        if diff is not None and diff[k] * sin_phi <= OBS_TOL:  # (first: what it explains is no near-tie and is listed apart)
            ok[k] = True
            ties.add("BEAM_SLIDE", diff[k] * sin_phi * ranges[fan], dict(env=int(e), agent=int(a), fan=fan, beam=int(col - start), slide_sin=sin_phi))
        elif util.admissible("BEAM", m, ranges[fan]):
            ok[k] = True
            ties.add("BEAM", m, dict(env=int(e), agent=int(a), fan=fan, beam=int(col - start)))
        elif fan == 0 and lead_tie is not None and lead_tie[e].any():
            for body in np.nonzero(lead_tie[e])[0]:
                dist = ora.beam_body_dist(e, slot, int(body), col - start)
                if body != slot and dist < shift + util.tie_eps("BEAM", ranges[0]):
                    ok[k] = True
                    ties.add("LEADER", dist, dict(env=int(e), agent=int(a), beam=int(col - start), moved_body=int(body)))
                    break
    return ok


def beam_flagged_sample(ora, ties, o_obs, layout, rng, k=64):
    """Share of compared beams the BEAM predicate WOULD flag, estimated on k random lidar beams per step (must stay small: the predicate
    may not degenerate into 'everything is a tie'; bounded at 1 % by tests/test_ties_cpu.py)."""
    lid = [x for x in layout if x[2] == 0]
    if not lid:
        return
    start, n = lid[0][0], lid[0][1]
    N, A = o_obs.shape[:2]
    for e, a, b in zip(rng.integers(0, N, k), rng.integers(0, A, k), rng.integers(0, n, k)):
        if o_obs[e, a].any():  # (an empty agent seat has a zero row and no beams)
            ties.sampled += 1
            ties.flagged += bool(util.admissible("BEAM", ora.beam_margin(e, a, 0, b), ora.cfg.lidar_dist))


def flag_ties(eng, stats, same, mg):
    """Rows whose done / flags differ: a tie (stats["flag_ties"]) only where a CONTACT / ROUTE / LANE decision of that agent was a near-tie
    in the oracle, else stats["flag_mismatch"] (== 0 in every test)."""
    ties = stats["ties"]
    A = eng.cfg.num_agents
    flag_tie = ~same & util.admitted_slots(mg, ("CONTACT", "ROUTE", "LANE"))[:, :A]
    for cls in ("CONTACT", "ROUTE", "LANE"):
        ties.add_slots(cls, ~same & util.admitted_slots(mg, (cls,))[:, :A], mg)
    stats["flag_ties"] = stats.get("flag_ties", 0) + int(flag_tie.sum())
    stats["flag_mismatch"] += int((~same & ~flag_tie).sum())
    for e, a in np.argwhere(~same & ~flag_tie):
        ties.reject("flags", dict(env=int(e), agent=int(a), margins={c: float(mg[util.MG[c], e, a]) for c in ("CONTACT", "ROUTE", "LANE")}))
    return flag_tie


# which near-tie can explain a differing integer field of a slot (oracle/pgd_oracle.c: where each is written)
_INT_FIELD_CLASSES = dict(LANE=("LANE",), CK0=("ROUTE", "LANE"), CK1=("ROUTE", "LANE"), RLANE=("LANE", "LEADER"), TIMER=("LEADER", "LANE"),
                          VFLAGS=("CONTACT", "LANE"), STATUS=("LANE", "CONTACT", "ROUTE"), SPAWN=("ROUTE", "CONTACT"))


def int_ties(gi, i, gei, ei, mg, stats, flag_tie=None):
    """Integer state (status / lanes / checkpoints / timers / counters) that differs after one teacher-forced step.  A slot is a tie where
    EVERY differing field has a near-tie of a class that writes it (_INT_FIELD_CLASSES): LANE (the lane pick feeds everything else of the
    slot, off-lane removal), CONTACT (line / crash bits of SI_VFLAGS), ROUTE (checkpoints, arrival, respawn place), LEADER (routing
    lane / timer of an IDM vehicle).  Discrete outcomes cascade inside an env within the step (an episode end resets every slot, a
    finish frees a seat for a respawn, the ego's lane triggers traffic): a differing slot without a near-tie of its own is a tie only
    if the same env has a verified one (a differing slot or a differing done / flags row).  Returns (ties, mismatches): slots + env
    records."""
    ties = stats["ties"]
    bad = (gi != i).any(axis=0)
    own = bad.copy()
    for name, k in _abi.SI.items():
        differs = gi[k] != i[k]
        adm = util.admitted_slots(mg, _INT_FIELD_CLASSES[name])
        own &= ~differs | adm
        for cls in _INT_FIELD_CLASSES[name]:
            ties.add_slots(cls, differs & util.admitted_slots(mg, (cls,)), mg)
    env_ok = own.any(axis=1)
    if flag_tie is not None:
        env_ok |= flag_tie.any(axis=1)
    bad_env = (gei != ei).any(axis=0)
    n_bad = int(bad.sum()) + int(bad_env.sum())
    n_tie = int((bad & env_ok[:, None]).sum()) + int((bad_env & env_ok).sum())
    for e, s_ in np.argwhere(bad & ~env_ok[:, None]):
        ties.reject("int_state", dict(env=int(e), slot=int(s_), fields=[k for k, v in _abi.SI.items() if gi[v, e, s_] != i[v, e, s_]],
                                      margins={c: float(mg[util.MG[c], e, s_]) for c in ("LANE", "CONTACT", "ROUTE", "LEADER")}))
    stats["int_ties"] = stats.get("int_ties", 0) + n_tie
    stats["int_mismatch"] = stats.get("int_mismatch", 0) + n_bad - n_tie
    return n_tie, n_bad - n_tie


def compare_rows(eng, ora, stats, g_obs, o_obs, same, mg):
    """The observation rows of one step (float64 arrays [N, A, D]) where the discrete outcome agrees (`same`): non-ray columns into
    stats["obs"] / ["obs_state"]; ray-cast columns over OBS_TOL into stats["grazing"] / ["det_grazing"] if admit_beams admits them,
    else into stats["obs"] as well."""
    ties = stats.setdefault("ties", util.Ties(os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0]))
    layout, D = fan_layout(eng.cfg)
    assert D == g_obs.shape[2]
    nl = eng.cfg.num_lasers
    if nl:
        lo = [x for x in layout if x[2] == 0][0][0]
        ties.beams += int(same.sum()) * nl
        ties.hits += int((o_obs[same][:, lo:lo + nl] < 1.0).sum())
        beam_flagged_sample(ora, ties, o_obs, layout, ties.rng)
    # numeric comparison only where the discrete outcome agrees (a flipped flag changes reward / reset / obs wholesale)
    if same.any():
        dfull = np.where(same[:, :, None], np.abs(g_obs - o_obs), 0.0)
        fan = np.zeros(D, dtype=bool)  # ray-cast columns: side fan, lane-line fan, lidar
        lidar = np.zeros(D, dtype=bool)
        for start, n, kind, rank in layout:
            fan[start:start + n] = True
            lidar[start:start + n] = kind == 0
        stats["obs"] = max(stats["obs"], float(dfull[:, :, ~fan].max()))
        stats["obs_state"] = max(stats.get("obs_state", 0.0), float(dfull[:, :, ~fan].max()))  # the non-ray columns on their own
        # a beam grazing a box corner can flip hit <-> miss between fp32 and fp64 (the slab test compares two nearly equal
        # parameters): such a beam is a tie only if the oracle's geometry confirms it; ties are counted and bounded by the callers,
        # every other beam must agree to OBS_TOL
        over = np.argwhere((dfull > OBS_TOL) & fan[None, None, :])
        if len(over):
            lead_tie = None
            if eng.cfg.num_traffic or eng.cfg.idm_agent:
                lead_tie = util.idm_tie(eng.get_state()[0], ora.get_state()[0], mg)
            ok = admit_beams(eng, ora, ties, over, layout, lead_tie, diff=dfull[over[:, 0], over[:, 1], over[:, 2]])
            stats["beams_not_admitted"] = stats.get("beams_not_admitted", 0) + int((~ok).sum())
            for (e, a, col), adm in zip(over, ok):
                if not adm:  # a finding: kept for the report (and it stays in stats["obs"])
                    ties.reject("beam", dict(env=int(e), agent=int(a), column=int(col), engine=float(g_obs[e, a, col]), oracle=float(o_obs[e, a, col])))
                if adm:
                    dfull[e, a, col] = 0.0
                    key = ("grazing", "beams") if lidar[col] else ("det_grazing", "det_beams")
                    stats[key[0]] = stats.get(key[0], 0) + 1
        n_rows = int(same.sum())
        if nl:
            stats["beams"] = stats.get("beams", 0) + n_rows * nl
            stats.setdefault("grazing", 0)
        if int(fan.sum()) - nl:
            stats["det_beams"] = stats.get("det_beams", 0) + n_rows * (int(fan.sum()) - nl)
            stats.setdefault("det_grazing", 0)
        stats["obs"] = max(stats["obs"], float(dfull[:, :, fan].max()) if fan.any() else 0.0)


def check_reset_rows(eng, ora, g0, o0, allowance, name="reset rows"):
    """The first observation after a reset: values over OBS_TOL are allowed only in ray-cast columns whose BEAM margin (from the state
    the oracle holds after the reset) admits them, and at most `allowance` of those."""
    stats = new_stats()
    same = np.ones(o0.shape[:2], dtype=bool)
    compare_rows(eng, ora, stats, np.asarray(g0, dtype=np.float64), o0, same, ora.margins())
    n_ties = stats.get("grazing", 0) + stats.get("det_grazing", 0)
    print(name, "worst not admitted", stats["obs"], "admitted beams", n_ties, stats["ties"])
    assert stats["obs"] < OBS_TOL and n_ties <= allowance, stats


def compare_step(eng, ora, act, stats):
    """One step on both sides.  Discrete outcomes must agree; what does not is a tie only where the oracle's margins say so
    (tests/util.py: admissible): rows whose done / flags differ go to stats["flag_ties"] if a CONTACT / ROUTE / LANE decision of that
    agent was a near-tie, else to stats["flag_mismatch"] (asserted == 0 by every caller); ray-cast values over OBS_TOL go to
    stats["grazing"] / ["det_grazing"] if admit_beams admits them, else they stay in stats["obs"]."""
    if not getattr(ora, "margins_on", False):
        ora.enable_margins()
    import torch
    ties = stats.setdefault("ties", util.Ties(os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0]))
    o_obs, o_rew, o_done, o_flags = ora.step(act)
    mg = ties.mg = ora.margins()  # (callers take the step's margins from here)
    g_obs, g_rew, g_done, g_flags = eng.step(torch.from_numpy(act).to(eng.device))
    eng.sync()
    g_obs, g_rew = g_obs.cpu().numpy().astype(np.float64), g_rew.cpu().numpy().astype(np.float64)
    g_done, g_flags = g_done.cpu().numpy(), g_flags.cpu().numpy().astype(np.uint32)
    same = (g_flags == o_flags) & (g_done == o_done)
    for name, bit in (("n_new", _abi.F_NEW), ("n_all_done", _abi.F_ALL_DONE), ("n_report", _abi.F_REPORT),
                      ("n_crash_object", _abi.F_CRASH_OBJECT), ("n_crash_vehicle", _abi.F_CRASH_VEHICLE)):
        stats[name] = stats.get(name, 0) + int(((o_flags & bit) != 0).sum())
    stats["steps"] += same.size
    ties.flag_tie = flag_ties(eng, stats, same, mg)
    compare_rows(eng, ora, stats, g_obs, o_obs, same, mg)
    if same.any():
        stats["rew"] = max(stats["rew"], float(np.abs(g_rew - o_rew)[same].max()))
    return o_done


def report(name, stats):
    """The line every parity test prints beside its own: beams compared, beams with a hit, items admitted per class with their largest
    margin, the share of sampled beams the BEAM predicate would flag."""
    t = stats.get("ties")
    if t is not None:
        print(name, "ties:", t.summary(), "flag_ties", stats.get("flag_ties", 0))
        t.dump()
    return t


# Share of the compared lidar beams with a hit (oracle value < 1), respawn traffic, from oracle-only runs of the same inputs
# (profiles/parity_ties.md): ego driving 26 %, floor 10 %; ego parked: see PARKED_HIT_SHARE, floor half of it.  Trigger mode: ~0.2 %,
# printed only.
DRIVING_HIT_FLOOR = 0.10
PARKED_HIT_SHARE = 0.1276  # tests/test_ties_cpu.py::test_parked_respawn_hit_share holds this figure to the oracle
PARKED_HIT_FLOOR = 0.5 * PARKED_HIT_SHARE


def teleport_to_objects(mb, sb, scen_ids, f, i, back=9.0):
    """Put every env's ego `back` metres (along the lane) behind a traffic object that sits on a road of its route."""
    from pgdrive_amd import mapdata
    V = sb.V
    moved = 0
    for e, sc in enumerate(scen_ids):
        sp = sb.spawns[sc * V:(sc + 1) * V]
        d = mb.descs[int(sb.scenarios["map"][sc])]
        route = list(sp[0]["ckpt_road"][:sp[0]["n_ckpt"] - 1])
        for k in range(1, V):
            if sp[k]["lane"] < 0 or sp[k]["group"] != -2:
                continue
            lane = d["lanes"][int(sp[k]["lane"])]
            if lane["road"] not in route:
                continue
            lon, lat = mapdata.lane_local_coordinates(lane, (float(sp[k]["x"]), float(sp[k]["y"])))
            if lon < back + 3:
                continue
            x, y = mapdata.lane_position(lane, lon - back, lat)
            th = mapdata.lane_heading_at(lane, lon - back)
            ck = route.index(lane["road"])
            f[_abi.SF["X"], e, 0], f[_abi.SF["Y"], e, 0], f[_abi.SF["THETA"], e, 0] = x, y, th
            f[_abi.SF["LASTX"], e, 0], f[_abi.SF["LASTY"], e, 0] = x, y
            f[_abi.SF["LASTHX"], e, 0], f[_abi.SF["LASTHY"], e, 0] = np.cos(th), np.sin(th)
            f[_abi.SF["SPEED"], e, 0] = 8.0
            i[_abi.SI["LANE"], e, 0] = int(sp[k]["lane"])
            i[_abi.SI["CK0"], e, 0] = ck
            i[_abi.SI["CK1"], e, 0] = ck + 1 if ck + 1 < sp[0]["n_ckpt"] - 1 else ck
            moved += 1
            break
    return moved


def np_obb_overlap(ax, ay, ath, al, aw, bx, by, bth, bl, bw):
    """Closed-rectangle SAT on arrays (chassis boxes length x width at heading th)."""
    dx, dy = bx - ax, by - ay
    aux, auy, bux, buy = np.cos(ath), np.sin(ath), np.cos(bth), np.sin(bth)
    ac, as_ = np.abs(aux * bux + auy * buy), np.abs(aux * buy - auy * bux)
    ahl, ahw, bhl, bhw = al / 2, aw / 2, bl / 2, bw / 2
    sep = (np.abs(dx * aux + dy * auy) > ahl + bhl * ac + bhw * as_) | (np.abs(dy * aux - dx * auy) > ahw + bhl * as_ + bhw * ac) | \
          (np.abs(dx * bux + dy * buy) > bhl + ahl * ac + ahw * as_) | (np.abs(dy * bux - dx * buy) > bhw + ahl * as_ + ahw * ac)
    return ~sep


# ---------------------------------------------------------------------------------------------------------------------
# Protocol 1: teacher-forced against the oracle.  Each step starts from the same fp32-rounded state on both sides.
# ---------------------------------------------------------------------------------------------------------------------
class ForcedStep:
    """What teacher_forced yields after a step: t, the oracle's done (o_done), the step's margins (mg), the oracle's state
    (f, i, ei) and -- read from the device only when asked for -- the engine's (gf, gi, gei)."""
    def __init__(self, t, eng, ora, stats, o_done):
        self.t, self.eng, self.stats, self.o_done = t, eng, stats, o_done
        self.ties = stats["ties"]
        self.mg = self.ties.mg
        self.f, self.i, self.ei = ora.get_state()
        self._g = None

    def _engine_state(self, k):
        if self._g is None:
            self._g = self.eng.get_state()
        return self._g[k]

    gf, gi, gei = (property(lambda self, k=k: self._engine_state(k)) for k in range(3))

    @property
    def agree(self):
        """[N, V] slots whose integer state (and their env's counters) is the oracle's"""
        return (self.gi == self.i).all(axis=0) & (self.gei == self.ei).all(axis=0)[:, None]

    def idm_tie(self, agree, skip_slots=0):
        """util.idm_tie of the step without the first `skip_slots` slots (agents that do not run the IDM policy); the agreeing ones are
        noted as LEADER ties"""
        tie = util.idm_tie(self.gf, self.f, self.mg)
        tie[:, :skip_slots] = False
        self.ties.add_slots("LEADER", tie & agree, self.mg)
        return tie

    def int_ties(self):
        return int_ties(self.gi, self.i, self.gei, self.ei, self.mg, self.stats, self.ties.flag_tie)

    def pose_error(self, mask):
        """largest |engine - oracle| of X / Y / THETA / SPEED over the slots of `mask`"""
        worst = 0.0
        if mask.any():
            for fld in ("X", "Y", "THETA", "SPEED"):
                dlt = np.abs(self.gf[_abi.SF[fld]].astype(np.float64) - self.f[_abi.SF[fld]])[mask]
                if fld == "THETA":  # heading_theta lives in [-3 pi / 2, pi / 2): a value on the seam may wrap on one side only
                    dlt = np.minimum(dlt, np.abs(dlt - 2 * np.pi))
                worst = max(worst, float(dlt.max()))
        return worst

    def compare_state(self, mask, worst):
        return util.compare_state(self.gf, self.f, mask, worst)


def teacher_forced(eng, ora, stats, n_steps, actions):
    """Generator: per step t draws actions(t) (a float32 array), runs compare_step and yields a ForcedStep; when the caller's loop
    body is done, the oracle's state rounded to fp32 is set on both sides."""
    for t in range(n_steps):
        step = ForcedStep(t, eng, ora, stats, compare_step(eng, ora, actions(t), stats))
        yield step
        f32 = util.round_state_f32(step.f)
        ora.set_state(f32, step.i, step.ei)
        eng.set_state(f32, step.i, step.ei)


def single_teacher_forced(descs, num_traffic, num_lasers, traffic_mode="trigger", ego="driving"):
    """The single-agent teacher-forced test: 64 envs x 400 steps on the first 8 maps of `descs`; outputs and the next state must agree."""
    n_envs = 64
    eng, ora, cfg = engines(descs, n_envs, num_traffic=num_traffic, num_lasers=num_lasers, traffic_mode=traffic_mode)
    scen_ids = np.arange(n_envs) % 8
    o0 = ora.reset(scen_ids)
    g0 = eng.reset(scen_ids).cpu().numpy()
    assert np.abs(g0 - o0).max() < OBS_TOL
    rng = np.random.default_rng(0)
    stats = new_stats()
    pose = 0.0
    worst = {}  # every float field of the state, in units of its tolerance (tests/util.py STATE_TOL)
    idm_ties = active = 0
    for s in teacher_forced(eng, ora, stats, 400, lambda t: util.driving_actions(rng, n_envs) * (0.0 if ego == "parked" else 1.0)):
        agree = s.agree
        # an IDM leader exactly MAX_DIST = 30 m ahead on the 10 m spawn grid is found / not found by the last bit of a lane
        # coordinate: that vehicle gets another throttle on the two sides (counted and bounded, as in the campaign) -- where the
        # oracle's LEADER margin confirms the near-tie; any other differing throttle stays in compare_state
        tie = s.idm_tie(agree, skip_slots=cfg.num_agents)
        idm_ties += int((tie & agree).sum())
        active += int((s.i[_abi.SI["STATUS"]][:, cfg.num_agents:] == _abi.ST_ACTIVE).sum())
        if agree.any():
            pose = max(pose, s.pose_error(agree & ~tie))
        s.compare_state(agree & ~tie, worst)
    print("teacher-forced parity:", traffic_mode, ego, stats, "pose", pose, "idm ties", idm_ties, "of", active,
          "state fields (x tolerance):", {k: round(v, 3) for k, v in worst.items()})
    ties = report("teacher-forced parity", stats)
    print("n_crash_vehicle", stats["n_crash_vehicle"], "lidar hit share", ties.hits / max(ties.beams, 1))
    if traffic_mode == "respawn":
        assert ties.hits >= (PARKED_HIT_FLOOR if ego == "parked" else DRIVING_HIT_FLOOR) * ties.beams
        assert ego == "parked" or stats["n_crash_vehicle"] > 0
    assert stats["obs"] < OBS_TOL and stats["obs_state"] < STATE_OBS_TOL and stats["rew"] < REW_TOL and pose < 1e-3
    assert not util.state_failures(worst), util.state_failures(worst)
    assert idm_ties <= 2e-3 * max(active, 1) + 2
    assert stats["flag_mismatch"] == 0 and stats.get("flag_ties", 0) == 0  # done / flags bit-exact (north star); no tie class occurs on these 8 maps
    assert stats.get("grazing", 0) <= 1e-5 * stats.get("beams", 1) + 2


def marl_teacher_forced(num_agents, capacity, kind="roundabout", **cfg_kw):
    """The multi-agent teacher-forced test: 32 envs x 300 steps on the map `kind`, `cfg_kw` on top of util.marl_config."""
    d, mb, sb = util.make_marl_banks(num_agents=num_agents, capacity=capacity, kind=kind)
    n_envs = 32
    cfg = util.marl_config(n_envs, sb, horizon=120, **cfg_kw)  # short horizon so that the episode end / reset path is exercised
    eng, ora = engine(cfg, mb, sb), oracle(cfg, mb, sb)
    ids = np.arange(n_envs) % 8
    o0 = ora.reset(ids)
    g0 = eng.reset(ids).cpu().numpy()
    assert np.abs(g0 - o0).max() < OBS_TOL
    rng = np.random.default_rng(5)
    A = sb.A
    stats = new_stats()
    seen = dict(new=0, dying=0, all_done=0, report=0)
    worst = {}
    for s in teacher_forced(eng, ora, stats, 300, lambda t: util.marl_actions(rng, n_envs, A)):
        # discrete state (status / lanes / ids / counters) must be bit-exact, up to box-overlap tests that sit on an fp32
        # rounding boundary (measured: 1 line-contact flip in ~77 k agent-steps); every step restarts from the oracle state
        s.int_ties()
        seen["id_mismatch"] = seen.get("id_mismatch", 0) + int((s.gf[_abi.SF["AGENT_ID"]] != s.f[_abi.SF["AGENT_ID"]].astype(np.float32)).sum())
        seen["dying"] += int((s.i[_abi.SI["STATUS"]] == _abi.ST_DYING).sum())
        s.compare_state(s.agree, worst)
    print("marl parity:", stats, seen, "state fields (x tolerance):", {k: round(v, 3) for k, v in worst.items()})
    report("marl parity", stats)
    assert not util.state_failures(worst), util.state_failures(worst)
    assert stats["obs"] < OBS_TOL and stats["rew"] < REW_TOL
    # the only tie class seen in the multi-agent runs: a car whose box touches a line box exactly (fp32 vs fp64 SAT), one
    # agent-step in 153,600 of the 12-of-16 configuration; every other configuration is bit-exact.  Such a row is admitted only where the
    # oracle's CONTACT / ROUTE / LANE margin confirms the near-tie (at most the one seen before); anything else: 0
    assert stats["flag_mismatch"] == 0 and stats["flag_ties"] <= 1
    assert stats["int_mismatch"] == 0 and seen["id_mismatch"] == 0
    assert stats["int_ties"] <= 1
    assert seen["dying"] > 0 and stats["n_new"] > 0 and stats["n_all_done"] > 0 and stats["n_report"] > 1000


# ---------------------------------------------------------------------------------------------------------------------
# Protocol 2: twin engines in lock step, and the three strengths at which the suite compares them.
# ---------------------------------------------------------------------------------------------------------------------
OUTPUTS = ("obs", "reward", "done", "flags")


def twins(a, b, n_steps, actions, copy_state=None):
    """Generator: per step t draws actions(t), copies the whole state of engine `copy_state` (None, a or b) into b -- from b itself it
    only clears what pgd_set_state clears --, uploads the action once, steps a then b, clones the four outputs, syncs both and yields
    (t, outputs of a, outputs of b)."""
    import torch
    for t in range(n_steps):
        act = actions(t)
        if copy_state is not None:
            b.set_state(*copy_state.get_state())
        at = torch.from_numpy(act).to(a.device)
        outs_a = [x.clone() for x in a.step(at)]
        outs_b = [x.clone() for x in b.step(at)]
        a.sync(); b.sync()
        yield t, outs_a, outs_b


def same_bits(t, outs_a, outs_b, a=None, b=None, names=OUTPUTS):
    """Same bits: the outputs, and with the engines given the whole state (floats compared as numbers and as int32 views)."""
    import torch
    for xa, xb, name in zip(outs_a, outs_b, names):
        assert torch.equal(xa, xb), "%s differs at step %d" % (name, t)
    if a is not None:
        (fa, ia, ea), (fb, ib, eb) = a.get_state(), b.get_state()
        assert (ia == ib).all() and (ea == eb).all(), "integer state differs at step %d" % t
        assert np.array_equal(fa, fb) and (fa.view(np.int32) == fb.view(np.int32)).all(), "state differs at step %d" % t


def same_outcome(t, outs_a, outs_b, a, b, obs_tol=None, rew_tol=None, state_tol=None):
    """Same discrete outcome, floats to rounding: done / flags / integer state equal; obs, reward and the float state within the
    caller's tolerances (one left off is not compared)."""
    import torch
    (o1, r1, d1, f1), (o2, r2, d2, f2) = outs_a, outs_b
    assert torch.equal(d1, d2) and torch.equal(f1, f2), "flags differ at step %d" % t
    assert obs_tol is None or float((o1 - o2).abs().max()) < obs_tol, "obs differs at step %d" % t
    assert rew_tol is None or float((r1 - r2).abs().max()) < rew_tol, "reward differs at step %d" % t
    (g1, i1, e1), (g2, i2, e2) = a.get_state(), b.get_state()
    assert (i1 == i2).all() and (e1 == e2).all(), "integer state differs at step %d" % t
    assert state_tol is None or np.abs(g1 - g2).max() < state_tol, "float state differs at step %d" % t


def same_rows(t, outs_a, outs_b, st, nl, tol, tail=0):
    """Same discrete outcome, rows to `tol` with grazing beams counted: reward / done / flags equal bit for bit; of the rows' `nl`
    lidar columns (`tail` columns from the end) those off by more than `tol` go to st["grazing"] of st["beams"], the largest
    difference of everything else to st["worst"]."""
    same_bits(t, outs_a[1:], outs_b[1:], names=OUTPUTS[1:])
    rows_close(outs_a[0], outs_b[0], st, nl, tol, tail)


def rows_close(xa, xb, st, nl, tol, tail=0):
    dd = np.abs(xa.cpu().numpy().astype(np.float64) - xb.cpu().numpy())
    D = dd.shape[-1]
    beams = dd[..., D - tail - nl:D - tail]
    st["beams"] += beams.size
    st["grazing"] += int((beams > tol).sum())
    beams[beams > tol] = 0.0
    st["worst"] = max(st["worst"], float(dd.max()))


# ---------------------------------------------------------------------------------------------------------------------
# Protocol 3: the all-maps campaign (tests/test_parity_wide_gpu.py::test_all_maps_campaign, tests/parity_campaign.py).
# ---------------------------------------------------------------------------------------------------------------------
def stream_actions(mode, rng, n):
    if mode == "driving":
        return util.driving_actions(rng, n)
    if mode == "uniform":
        return rng.uniform(-1, 1, size=(n, 1, 2)).astype(np.float32)
    act = np.zeros((n, 1, 2), np.float32)  # drive straight, full throttle
    act[..., 1] = 1.0
    act[..., 0] = rng.normal(0, 0.05, size=(n, 1))
    return act


def campaign(eng, ora, name, steps, actions, threads):
    """Teacher-forced single-agent run with every tie class counted (profiles/r01_parity_campaign.md): grazing lidar beams, a body
    exactly on the 50 m neighbour radius, an IDM leader exactly MAX_DIST = 30 m ahead on the 10 m spawn grid.  Returns (stats, worst
    state fields in units of their tolerance); the callers assert on them."""
    import torch
    st = dict(steps=0, flag_mismatch=0, obs=0.0, rew=0.0, pose=0.0, beams=0, grazing=0, int_mismatch=0, int_ties=0, done=0, active=0,
              radius_rows=0, idm_ties=0)
    ties = st.setdefault("ties", util.Ties(name))
    worst = {}
    for t in range(steps):
        act = actions(t)
        oo, orw, od, ofl = ora.step(act, threads=threads)
        mg = ties.mg = ora.margins()
        go, grw, gd, gfl = eng.step(torch.from_numpy(act).to(eng.device))
        eng.sync()
        go = go.cpu().numpy().astype(np.float64)
        grw = grw.cpu().numpy().astype(np.float64)
        gd, gfl = gd.cpu().numpy(), gfl.cpu().numpy().astype(np.uint32)
        same = (gfl == ofl) & (gd == od)
        st["steps"] += same.size
        ties.flag_tie = flag_ties(eng, st, same, mg)  # (done / flags that differ: verified ties or flag_mismatch; both asserted 0 by the test)
        st["done"] += int(od.sum())
        head = np.where(same[:, :, None], np.abs(go - oo), 0.0)[:, 0, :34]
        # neighbour block alone differs: a body on the 50 m radius or two equally distant ones -- only where the oracle's NEIGHBOUR
        # margin of the row confirms it; any other such row stays in the comparison
        flip = (head[:, 18:].max(axis=1) > OBS_TOL) & (head[:, :18].max(axis=1) <= OBS_TOL)
        flip &= util.admissible("NEIGHBOUR", mg[util.MG["NEIGHBOUR"]][:, 0])
        ties.add_slots("NEIGHBOUR", np.pad(flip[:, None], ((0, 0), (0, mg.shape[2] - 1))), mg)
        st["radius_rows"] += int(flip.sum())
        go_cmp = go.copy()
        go_cmp[flip, 0, 18:34] = oo[flip, 0, 18:34]
        compare_rows(eng, ora, st, go_cmp, oo, same, mg)  # beams over OBS_TOL: margin-verified grazing or st["obs"]
        st["rew"] = max(st["rew"], float(np.abs(grw - orw)[same].max()))
        s = ForcedStep(t, eng, ora, st, od)
        agree = s.agree
        s.int_ties()
        st["active"] += int((s.i[0, :, 1:] == 2).sum())
        tie = s.idm_tie(agree)
        st["idm_ties"] += int((tie & agree).sum())
        st["pose"] = max(st["pose"], s.pose_error(agree & ~tie))
        s.compare_state(agree & ~tie, worst)  # all 26 float fields, not the pose alone
        f32 = util.round_state_f32(s.f)
        ora.set_state(f32, s.i, s.ei)
        eng.set_state(f32, s.i, s.ei)
    return st, worst
