"""Checker of the expert guardian (pgd_guardian, pgdrive_amd/csrc/pgd_guardian.h): a float64 restatement of the rule include/pgdrive_hip.h
states, the traced floats (the lateral float of the expert's row, hd, f) in float64 and as an fp32 emulation in the kernel's operation
order, and the cases the CPU and the GPU tests share -- poses written with set_state and crafted observation rows.

Rounding recipe (the header's): the regimes compare save_level, an fp32 number, as a double; 10 s and (s + 0.1) / 10 are formed in double
and rounded to fp32 once; 0.04, 1e-3 and 5 are fp32 constants.  Observation floats and actions are fp32 numbers and enter as they are.
The one comparison whose two sides the kernel and this checker compute differently is obs < 0.04 f: the kernel's f is fp32, this one's
float64 -- hence the tie band (tie_band).
"""
import math

import numpy as np

from pgdrive_amd import _abi, mapdata
from tests import actor_critic_ref as ar

F32 = np.float32
C_EDGE, C_OBS, C_SLOW = float(F32(0.04)), float(F32(1e-3)), 5.0
EPS = 2.0 ** -23
TAKEOVER, TAKEOVER_START, TAKEOVER_END = 1, 2, 4
LEGACY, DETERMINISTIC, IMMEDIATE = 1, 2, 4
SEED_XOR = 0x6a7d1a4b  # the collectors' guardian seed = their seed ^ this (pgdrive_amd/rollout.py: GUARDIAN_SEED_XOR)
# the ABI this checker restates (an engine without the guardian has none of these names: every test that uses the checker fails there)
assert (_abi.GUARD_TAKEOVER, _abi.GUARD_TAKEOVER_START, _abi.GUARD_TAKEOVER_END) == (TAKEOVER, TAKEOVER_START, TAKEOVER_END)
assert (_abi.GUARD_LEGACY_LATERAL, _abi.GUARD_DETERMINISTIC, _abi.GUARD_IMMEDIATE) == (LEGACY, DETERMINISTIC, IMMEDIATE)

ROW_COUNTS = (1, 15, 16, 17, 33, 64)
BEAMS = (40, 72, 240, 241)


# ---------------------------------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------------------------------
def thresholds(save_level):
    """(s as a double, regime 0 / 1 / 2, 10 s, (s + 0.1) / 10, s) -- the last three as the fp32 numbers the kernel compares with."""
    s = float(F32(save_level))
    return s, (2 if s > 0.9 else (1 if s > 1e-3 else 0)), float(F32(10.0 * s)), float(F32((s + 0.1) / 10.0)), s


def slices(n):
    """(left, right): the centres of the side windows, the integer parts of n / 4 and n / 4 * 3."""
    return int(n / 4), int(n / 4 * 3)


def fan_minima(fan):
    """(side, front) minima of the fans [rows, n]: beams [L - 4, L + 5] and [R - 4, R + 5]; [0, 9] and [n - 10, n - 1]."""
    n = fan.shape[1]
    L, R = slices(n)
    side = np.minimum(fan[:, L - 4:L + 6].min(axis=1), fan[:, R - 4:R + 6].min(axis=1))
    front = np.minimum(fan[:, :10].min(axis=1), fan[:, n - 10:].min(axis=1))
    return side, front


def rule_f64(obs, n, a, e, hd, v, f, save_level):
    """The corrected (steer, thr) [rows, 2] and the clauses that fired (dict of bool arrays).  obs [rows, D] (the fan = its last n floats),
    a the agent's action, e the expert's, hd / v / f per row."""
    obs = np.asarray(obs, dtype=np.float64)
    a, e = np.asarray(a, dtype=np.float64), np.asarray(e, dtype=np.float64)
    rows = obs.shape[0]
    s, regime, ten_s, side_thr, front_thr = thresholds(save_level)
    steer, thr = a[:, 0].copy(), a[:, 1].copy()
    fired = dict(out=np.zeros(rows, bool), slow=np.zeros(rows, bool), side=np.zeros(rows, bool), front=np.zeros(rows, bool))
    if regime == 2:
        return np.stack([e[:, 0], e[:, 1]], axis=1), fired
    if regime == 1:
        edge = C_EDGE * np.asarray(f, dtype=np.float64)
        o0, o1 = obs[:, 0], obs[:, 1]
        out = ((o0 < edge) & (hd < 0)) | ((o1 < edge) & (hd > 0)) | (o0 <= C_OBS) | (o1 <= C_OBS)
        slow = out & (np.asarray(v) < C_SLOW)
        steer = np.where(out, e[:, 0], steer)
        thr = np.where(out, np.where(slow, 0.5, e[:, 1]), thr)
        side_min, front_min = fan_minima(obs[:, obs.shape[1] - n:])
        side = side_min < side_thr
        steer = np.where(side, e[:, 0], steer)
        front = (a[:, 1] >= 0) & (e[:, 1] <= 0) & (front_min < front_thr)
        thr = np.where(front, e[:, 1], thr)
        fired = dict(out=out, slow=slow, side=side, front=front)
    return np.stack([steer, thr], axis=1), fired


def bookkeeping(state, prev_reset, a, corrected, immediate=False):
    """(applied [rows, 2], new state, info bits) from the takeover state before the call, the reset marks of the previous step, the agent's
    action and the rule's."""
    a, c = np.asarray(a, dtype=np.float64), np.asarray(corrected, dtype=np.float64)
    pre = (np.asarray(state) != 0) & ~np.asarray(prev_reset, dtype=bool)
    now = (a[:, 0] != c[:, 0]) | (a[:, 1] != c[:, 1])
    take = pre & now
    info = take * TAKEOVER + (~pre & now) * TAKEOVER_START + (pre & ~now) * TAKEOVER_END
    use = now if immediate else take
    return np.where(use[:, None], c, a), now.astype(np.uint8), info.astype(np.uint8)


def guardian_f64(obs, n, a, e, hd, v, f, save_level, state, prev_reset, immediate=False):
    c, fired = rule_f64(obs, n, a, e, hd, v, f, save_level)
    applied, new_state, info = bookkeeping(state, prev_reset, a, c, immediate)
    return applied, new_state, info, fired


def expert_f64(rows_x, weights, seed, g_rows, tick, deterministic=False):
    """(the expert's action in float64, its tolerance per element): the network, the counter-hash noise and the propagated tolerance of
    tests/actor_critic_ref.py."""
    mean, ls, _ = ar.heads_f64(rows_x, weights)
    z = np.zeros_like(mean) if deterministic else ar.noise_f64(seed, g_rows, tick)
    return ar.sample_f64(mean, ls, z)[0], ar.tol_action(mean, ls, z)


def expert_row(obs, lateral=None):
    """The expert's input rows: obs, or obs[0..7] | lateral | obs[8..]."""
    obs = np.asarray(obs)
    return obs if lateral is None else np.concatenate([obs[:, :8], np.asarray(lateral, dtype=obs.dtype)[:, None], obs[:, 8:]], axis=1)


# ---------------------------------------------------------------------------------------------------------------------
# traced floats: float64 from the lane description, fp32 from the lane record in the kernel's operation order
# ---------------------------------------------------------------------------------------------------------------------
def lateral_float(lat):
    return float(np.clip((lat * 2 / 4.5 + 1.0) / 2.0, 0.0, 1.0))


def heading_diff_f64(lane, x, y, hx, hy):
    """vehicle.heading_diff(lane) - 0.5: half the cosine between the heading and the lane's lateral direction."""
    if lane["type"] == 0:
        dx, dy = lane["direction"]
        lx, ly = -dy, dx
    elif lane["direction"] < 0:
        lx, ly = x - lane["center"][0], y - lane["center"][1]
    else:
        lx, ly = lane["center"][0] - x, lane["center"][1] - y
    ln, fn = math.hypot(lx, ly), math.hypot(hx, hy)
    if ln * fn == 0.0:
        return -0.5
    return float(np.clip((hx * lx + hy * ly) / (ln * fn), -1.0, 1.0)) * 0.5 + 0.5 - 0.5


def traced_f64(lane, x, y, hx, hy, speed_ms, max_speed, save_level):
    """(lateral float, hd, v [km/h], f) in float64 from fp32 state values and the lane description."""
    x, y, hx, hy = float(x), float(y), float(hx), float(hy)
    _, lat = mapdata.lane_local_coordinates(lane, (x, y))
    hd = heading_diff_f64(lane, x, y, hx, hy)
    v = min(abs(float(speed_ms)) * 3.6, 100000.0)
    f = min(1.0 + abs(hd) * v * float(max_speed), thresholds(save_level)[2])
    return lateral_float(lat), hd, v, f


def traced_f32(rec, x, y, hx, hy, speed_ms, max_speed, save_level):
    """The same four numbers as the kernel forms them: every operation rounded to fp32, in the order of lane_local, heading_diff (a / b as
    a * (1 / b), the build's division), gd_lateral and gd_factor.  rec: the lane's record of the map bank (fp32 fields)."""
    x, y, hx, hy = F32(x), F32(y), F32(hx), F32(hy)
    ax, ay, bx, by, dr = F32(rec["ax"]), F32(rec["ay"]), F32(rec["bx"]), F32(rec["by"]), F32(rec["dir"])
    dx, dy = F32(x - ax), F32(y - ay)
    if dr == 0:
        lat = F32(F32(dy * bx) - F32(dx * by))
        lx, ly = F32(-by), bx
    else:
        lat = F32(dr * F32(bx - F32(np.sqrt(F32(F32(dx * dx) + F32(dy * dy))))))
        lx, ly = (dx, dy) if dr < 0 else (F32(ax - x), F32(ay - y))
    lateral = F32(np.clip(F32(F32(F32(F32(lat * F32(2.0)) * F32(F32(1.0) / F32(4.5))) + F32(1.0)) * F32(0.5)), F32(0.0), F32(1.0)))
    ln = F32(np.sqrt(F32(F32(lx * lx) + F32(ly * ly))))
    fn = F32(np.sqrt(F32(F32(hx * hx) + F32(hy * hy))))
    den = F32(ln * fn)
    if den == 0:
        hd = F32(-0.5)
    else:
        c = F32(F32(F32(hx * lx) + F32(hy * ly)) * F32(F32(1.0) / den))
        hd = F32(F32(F32(np.clip(c, F32(-1.0), F32(1.0))) * F32(0.5) + F32(0.5)) - F32(0.5))
    v = F32(min(F32(abs(F32(speed_ms)) * F32(3.6)), F32(100000.0)))
    f = F32(min(F32(F32(1.0) + F32(F32(abs(hd) * v) * F32(max_speed))), F32(thresholds(save_level)[2])))
    return float(lateral), float(hd), float(v), float(f)


# ---------------------------------------------------------------------------------------------------------------------
# the shared cases
# ---------------------------------------------------------------------------------------------------------------------
N_MAPS = 4
# (rows, beams, legacy row): the tile edges and the second workgroup, every beam count, both widths
KERNEL_CASES = ((64, 240, True), (64, 240, False), (33, 72, True), (17, 40, False), (16, 241, True), (15, 72, False), (1, 40, True))
SAVE_LEVEL = 0.5
# (speed [m/s], heading offset from the lane [rad]): slow and nearly aligned -- f below its cap, v on both sides of 5 km/h, hd on both sides
# of 0 -- and fast and oblique -- f at its cap
POSES = ((0.9, 0.012), (0.9, -0.012), (1.6, 0.008), (1.6, -0.008), (12.0, 0.25), (20.0, -0.3), (1.0, 0.2), (3.0, -0.004))


def pose_cases(descs, rows, seed):
    """Poses of `rows` envs, env e on map e % N_MAPS of `descs`: a point on a lane of the map, a heading near the lane's, a speed.
    -> dict of arrays x, y, theta (fp32), speed (fp32, m/s), lane (map-local id), map."""
    rng = np.random.default_rng(1000 + seed)
    out = dict(x=[], y=[], theta=[], speed=[], lane=[], map=[])
    for e in range(rows):
        m = e % N_MAPS
        lanes = descs[m]["lanes"]
        ok = [k for k, l in enumerate(lanes) if l["length"] > 12.0]
        k = int(ok[rng.integers(len(ok))])
        l = lanes[k]
        lon = float(rng.uniform(3.0, l["length"] - 3.0))
        lat = float(rng.uniform(-1.4, 1.4))
        spd, da = POSES[(e + seed) % len(POSES)]
        scale = float(rng.uniform(0.6, 1.0))
        px, py = mapdata.lane_position(l, lon, lat)
        out["x"].append(px); out["y"].append(py)
        out["theta"].append(mapdata.lane_heading_at(l, lon) + da * scale)
        out["speed"].append(spd * scale if spd > 5.0 else spd)
        out["lane"].append(k); out["map"].append(m)
    return {k: np.asarray(v, dtype=(np.int32 if k in ("lane", "map") else np.float32)) for k, v in out.items()}


def window_beams(n):
    L, R = slices(n)
    return set(range(L - 4, L + 6)) | set(range(R - 4, R + 6)) | set(range(10)) | set(range(n - 10, n))


def craft_rows(D, n, f, save_level, seed):
    """Observation rows [rows, D] (fp32) around every threshold of the rule, and agent actions [rows, 2]: obs0 / obs1 10 % to either side
    of 0.04 f and at 1e-3 and the next fp32 number, fan minima to either side of and exactly at (s + 0.1) / 10 and s, zeros just outside
    the windows.  `f`: float64 per row."""
    rng = np.random.default_rng(2000 + seed)
    rows = len(f)
    s, _, _, side_thr, front_thr = thresholds(save_level)
    obs = rng.uniform(0.3, 1.0, size=(rows, D)).astype(F32)
    fan0 = D - n
    obs[:, fan0:] = rng.uniform(min(max(front_thr, side_thr) + 0.05, 0.99), 1.0, size=(rows, n)).astype(F32)
    act = rng.uniform(-1.0, 1.0, size=(rows, 2)).astype(F32)
    L, R = slices(n)
    inside = window_beams(n)
    edge = C_EDGE * np.asarray(f, dtype=np.float64)
    for r in range(rows):
        c = (r + seed) % 14

        def outside(beam):
            if 0 <= beam < n and beam not in inside:
                obs[r, fan0 + beam] = 0.0
        if c == 0: obs[r, 0] = F32(edge[r] * 0.9)
        elif c == 1: obs[r, 0] = F32(edge[r] * 1.1)
        elif c == 2: obs[r, 1] = F32(edge[r] * 0.9)
        elif c == 3: obs[r, 1] = F32(edge[r] * 1.1)
        elif c == 4: obs[r, 0] = F32(1e-3)
        elif c == 5: obs[r, 1] = np.nextafter(F32(1e-3), F32(1.0))
        elif c == 6: obs[r, fan0 + L - 4] = F32(side_thr * 0.9); outside(L - 5)
        elif c == 7: obs[r, fan0 + L + 5] = F32(side_thr); outside(L + 6)
        elif c == 8: obs[r, fan0 + R - 4] = F32(side_thr * 0.5); outside(R - 5)
        elif c == 9: obs[r, fan0 + R + 5] = np.nextafter(F32(side_thr), F32(0.0)); outside(R + 6)
        elif c == 10: obs[r, fan0 + 9] = F32(front_thr * 0.9); act[r, 1] = abs(act[r, 1]); outside(10)
        elif c == 11: obs[r, fan0 + n - 10] = F32(front_thr * 0.9); act[r, 1] = -abs(act[r, 1]) - F32(0.01); outside(n - 11)
        elif c == 12: obs[r, fan0] = F32(front_thr); act[r, 1] = 0.0
        # 13: nothing near
    return obs, act


def tie_band(tol_f, edge):
    """Half width of the band around 0.04 f inside which the kernel's fp32 comparison may differ from this checker's: the error of f
    times 0.04, and the rounding of the fp32 product."""
    return C_EDGE * tol_f + 2.0 * EPS * np.abs(edge)


def lane_of(descs, bank, m, k):
    """(description, record) of lane k of map m."""
    return descs[m]["lanes"][k], bank.lanes[int(bank.maps[m]["lane_off"]) + k]


def tolerances(descs, bank, max_speed=80.0):
    """(tol_lateral, tol_f): twice the largest |fp32 emulation - float64| over the poses of KERNEL_CASES (seed = the case's index)."""
    worst_l = worst_f = 0.0
    for ci, (rows, n, legacy) in enumerate(KERNEL_CASES):
        p = pose_cases(descs, rows, ci)
        for e in range(rows):
            ld, rec = lane_of(descs, bank, int(p["map"][e]), int(p["lane"][e]))
            hx, hy = F32(np.cos(p["theta"][e])), F32(np.sin(p["theta"][e]))
            a = traced_f64(ld, p["x"][e], p["y"][e], hx, hy, p["speed"][e], max_speed, SAVE_LEVEL)
            b = traced_f32(rec, p["x"][e], p["y"][e], hx, hy, p["speed"][e], max_speed, SAVE_LEVEL)
            worst_l, worst_f = max(worst_l, abs(a[0] - b[0])), max(worst_f, abs(a[3] - b[3]))
    return 2.0 * worst_l, 2.0 * worst_f
