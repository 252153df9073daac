"""The checker of pgdrive_amd/csrc/pgd_timelimit.h (pgd_mlp_terminal_value, pgd_gae_bootstrap, pgd_cost_gae_bootstrap), in plain numpy:

* truncated_ref       a literal restatement of the step's done rule (reward_done of pgd_dynamics.h: pgdrive_env.py:162-194,
                      safe_pgdrive_env.py:49-56) plus the horizon line of pgd_step.h, from which "the clock alone ended the episode" follows;
* gae_bootstrap_f64 / gae_bootstrap_by_segments_f64 / cost_gae_bootstrap_f64
                      the recursion of include/pgdrive_hip.h in float64, the same cut by definition -- every episode segment through the
                      plain actor_critic_ref.gae_f64 with its own bootstrap --, and the cost form on safe_ppo_ref's costs and books;
* gae_bootstrap_f32   the kernels' ARITHMETIC in float32 (k_gae's fma forms with the select).  Never compared with the device: its
                      purpose is the measured tolerance below;
* the seeded histories of tests/test_timelimit_gpu.py (bootstrap_cases / build_bootstrap / build_cost_bootstrap) and the truncation
  patterns of the terminal-value launch (trunc_pattern).

Tolerance.  TOL_GAE_BOOTSTRAP is MEASURED: the largest |float32 emulation - float64| over exactly the histories of the GPU test, both
forms, both lambdas, advantages and returns, doubled (tests/test_timelimit_cpu.py measures it again and holds the emulation within the
recorded figure).  It is not actor_critic_ref.TOL_GAE: a truncated end adds gamma term_value, N(0, 2), to the one-step target where
pgd_gae has 0, and the cost form's histories are its own.
"""
import numpy as np

from tests import actor_critic_ref as ar
from tests import safe_ppo_ref as sr

F_ARRIVE, F_OUT_OF_ROAD, F_CRASH_VEHICLE, F_CRASH_OBJECT, F_CRASH_BUILDING, F_MAX_STEP = 1, 2, 4, 8, 16, 32
CAUSE_BITS = (F_ARRIVE, F_OUT_OF_ROAD, F_CRASH_VEHICLE, F_CRASH_OBJECT, F_CRASH_BUILDING, F_MAX_STEP)

# max |float32 emulation - float64| over bootstrap_cases() x TRUNC_MODES x GAE_LAM, reward form and cost form, adv and ret: 5.107e-6
# (rewards N(0, 1) or the costs of the flags, values and terminal values N(0, 2), T up to 33)
TOL_GAE_BOOTSTRAP_MEASURED = 5.11e-6
TOL_GAE_BOOTSTRAP = 2.0 * TOL_GAE_BOOTSTRAP_MEASURED

_f32 = ar._f32


# ---------------------------------------------------------------------------------------------------------------------
# the predicate
# ---------------------------------------------------------------------------------------------------------------------
def truncated_ref(flags, done, safe_rl_env):
    """One step's (flags, done) as python ints -> bool.  reward_done: done = arrive or out_of_road or crash_vehicle or crash_object or
    crash_building; safe_rl_env: a step with crash_vehicle or crash_object is not terminal.  The horizon line: max_step sets done.  The
    done is a truncation when the step reports one, the clock is among its causes and reward_done's own rule says "not done"."""
    arrive, oor = bool(flags & F_ARRIVE), bool(flags & F_OUT_OF_ROAD)
    crash, crash_obj, building = bool(flags & F_CRASH_VEHICLE), bool(flags & F_CRASH_OBJECT), bool(flags & F_CRASH_BUILDING)
    done_out = arrive or oor or crash or crash_obj or building
    if safe_rl_env and (crash or crash_obj):
        done_out = False
    max_step = bool(flags & F_MAX_STEP)
    return bool(done) and max_step and not done_out


# ---------------------------------------------------------------------------------------------------------------------
# float64
# ---------------------------------------------------------------------------------------------------------------------
def gae_bootstrap_f64(reward, value, done, term_value, gamma, lam):
    """The recursion of include/pgdrive_hip.h (pgd_gae_bootstrap) in float64; gamma, lam as the float32 the device is given.
    value[t + 1] behind a done is never read (a select)."""
    r, v, tv = [np.asarray(a, dtype=np.float64) for a in (reward, value, term_value)]
    d = np.asarray(done) != 0
    g, gl = float(np.float32(gamma)), float(np.float32(gamma)) * float(np.float32(lam))
    adv = np.zeros_like(r)
    a = np.zeros(r.shape[1:])
    for t in range(r.shape[0] - 1, -1, -1):
        vb = np.where(d[t], tv[t], v[t + 1])
        a = r[t] + g * vb - v[t] + gl * np.where(d[t], 0.0, a)
        adv[t] = a
    return adv, adv + v[:-1]


def gae_bootstrap_by_segments_f64(reward, value, done, term_value, trunc, gamma, lam):
    """The same, cut by definition: every episode segment of every row through the plain gae_f64 (no done inside) with its own
    bootstrap -- term_value at a truncated end, 0 at a terminal one, value[T] at the rollout's end.  2-d arrays [T, rows]."""
    r, v, tv = [np.asarray(a, dtype=np.float64) for a in (reward, value, term_value)]
    d, tr = np.asarray(done) != 0, np.asarray(trunc) != 0
    T, rows = r.shape
    adv = np.zeros_like(r)
    for q in range(rows):
        s = 0
        while s < T:
            e = s
            while e < T - 1 and not d[e, q]:
                e += 1
            boot = (tv[e, q] if tr[e, q] else 0.0) if d[e, q] else v[T, q]
            seg_v = np.concatenate([v[s:e + 1, q], [boot]])[:, None]
            a, _ = ar.gae_f64(r[s:e + 1, q][:, None], seg_v, np.zeros((e + 1 - s, 1), dtype=np.uint8), gamma, lam)
            adv[s:e + 1, q] = a[:, 0]
            s = e + 1
    return adv, adv + v[:-1]


def cost_gae_bootstrap_f64(flags, done, cost_value, term_cost_value, costs, gamma, lam, run):
    """pgd_cost_gae_bootstrap in float64: safe_ppo_ref.cost_gae_f64's dict with cadv / cret from the bootstrap recursion."""
    ref = sr.cost_gae_f64(flags, done, cost_value, costs, gamma, lam, run)
    ref["cadv"], ref["cret"] = gae_bootstrap_f64(ref["cost"], cost_value, done, term_cost_value, gamma, lam)
    return ref


# ---------------------------------------------------------------------------------------------------------------------
# the kernels' arithmetic in float32
# ---------------------------------------------------------------------------------------------------------------------
def gae_bootstrap_f32(reward, value, done, term_value, gamma, lam):
    """k_gae_bootstrap: delta = fma(gamma, done ? term_value : v[t + 1], reward) - v[t]; adv = fma(gamma lam, done ? 0 : adv, delta);
    ret = adv + v[t]; float32 (actor_critic_ref.gae_f32's forms with the select)."""
    r, v, tv = [_f32(a).astype(np.float64) for a in (reward, value, term_value)]
    d = np.asarray(done) != 0
    g = float(np.float32(gamma))
    gl = float(_f32(np.float32(gamma) * np.float32(lam)))
    adv, ret = np.zeros(r.shape, dtype=np.float32), np.zeros(r.shape, dtype=np.float32)
    a = np.zeros(r.shape[1:], dtype=np.float64)
    for t in range(r.shape[0] - 1, -1, -1):
        vb = np.where(d[t], tv[t], v[t + 1])
        delta = _f32(_f32(g * vb + r[t]).astype(np.float64) - v[t]).astype(np.float64)
        a = _f32(gl * np.where(d[t], 0.0, a) + delta).astype(np.float64)
        adv[t] = a
        ret[t] = _f32(a + v[t])
    return adv, ret


# ---------------------------------------------------------------------------------------------------------------------
# the histories of the GPU test
# ---------------------------------------------------------------------------------------------------------------------
TRUNC_MODES = ("none", "all", "bernoulli")   # which of the dones are truncations
COSTS = sr.NONDYADIC


def bootstrap_cases():
    """actor_critic_ref.gae_cases(): T in (1, 2, 33) x rows in (1, 63, 64, 65, 4099) x the five done patterns."""
    return ar.gae_cases()


def _trunc_of(rng, done, mode):
    d = np.asarray(done) != 0
    if mode == "none":
        return np.zeros_like(d)
    if mode == "all":
        return d.copy()
    return d & (rng.uniform(size=d.shape) < 0.5)


def build_bootstrap(T, rows, pattern, mode):
    """(reward, value, done) of actor_critic_ref.build_gae plus trunc (bool [T, rows], a subset of the dones) and term_value float32
    [T, rows]: N(0, 2) at a truncated end -- a critic's output --, exactly 0 everywhere else, as pgd_mlp_terminal_value writes it."""
    reward, value, done = ar.build_gae(T, rows, pattern)
    rng = np.random.default_rng([T, rows, ar.GAE_DONES.index(pattern), TRUNC_MODES.index(mode), 41])
    trunc = _trunc_of(rng, done, mode)
    term_value = np.where(trunc, rng.normal(0, 2, size=(T, rows)), 0.0).astype(np.float32)
    return reward, value, done, trunc, term_value


def build_cost_bootstrap(T, rows, pattern, mode):
    """The cost side of the same history: flags int32 [T, rows] -- the eight combinations of the three cost bits and every other
    defined bit at random; PGD_F_MAX_STEP exactly at the truncated ends, no cause of a termination there --, done and trunc of
    build_bootstrap, cost_value float32 [T + 1, rows] N(0, 2), term_cost_value, run float32 [rows]."""
    _, _, done, trunc, _ = build_bootstrap(T, rows, pattern, mode)
    rng = np.random.default_rng([T, rows, ar.GAE_DONES.index(pattern), TRUNC_MODES.index(mode), 43])
    combo = rng.integers(0, 8, size=(T, rows))
    flags = ((combo & 1) * sr.F_OUT_OF_ROAD + ((combo >> 1) & 1) * sr.F_CRASH_VEHICLE + ((combo >> 2) & 1) * sr.F_CRASH_OBJECT).astype(np.int64)
    for bit in sr.OTHER_FLAG_BITS:
        if bit != F_MAX_STEP:
            flags |= np.where(rng.random((T, rows)) < 0.5, bit, 0)
    flags = np.where(trunc, (flags & ~(F_ARRIVE | F_OUT_OF_ROAD | F_CRASH_BUILDING)) | F_MAX_STEP, flags).astype(np.int32)
    cost_value = rng.normal(0, 2, size=(T + 1, rows)).astype(np.float32)
    term_cost_value = np.where(trunc, rng.normal(0, 2, size=(T, rows)), 0.0).astype(np.float32)
    run = rng.uniform(0, 10, size=rows).astype(np.float32)
    return flags, done, trunc, cost_value, term_cost_value, run


def emulation_error(cases=None):
    """max |gae_bootstrap_f32 - gae_bootstrap_f64| over the histories of the GPU test: every case x TRUNC_MODES x GAE_LAM, the reward
    form and the cost form (the costs of the flags as rewards), advantages and returns."""
    worst = 0.0
    for c in (bootstrap_cases() if cases is None else cases):
        for mode in TRUNC_MODES:
            r, v, d, _, tv = build_bootstrap(mode=mode, **c)
            fl, _, _, cv, tcv, _ = build_cost_bootstrap(mode=mode, **c)
            cost = sr.costs_of_flags(fl, COSTS)
            for lam in ar.GAE_LAM:
                for rew, val, term in ((r, v, tv), (cost, cv, tcv)):
                    a64, r64 = gae_bootstrap_f64(rew, val, d, term, ar.GAE_GAMMA, lam)
                    a32, r32 = gae_bootstrap_f32(rew, val, d, term, ar.GAE_GAMMA, lam)
                    assert np.isfinite(a32).all() and np.isfinite(r32).all()
                    worst = max(worst, float(np.abs(a32 - a64).max()), float(np.abs(r32 - r64).max()))
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# truncation patterns of the terminal-value launch (tiles of 16 rows)
# ---------------------------------------------------------------------------------------------------------------------
TV_ROWS = (1, 15, 16, 17, 33)
TV_WIDTHS = (4, 35, 274, 319, 320, 321, 324, 416)
TV_PATTERNS = ("none", "all", "one_per_tile", "last_row", "gap")
TV_GAP_ROWS = 48   # three tiles: the pattern "gap" leaves the middle one without a truncated row


def trunc_pattern(rows, pattern):
    """bool [rows]: none, all, one row per tile of 16 (another position in every tile), only the last row, or -- three tiles -- some
    rows of the first and the last tile and none of the middle one."""
    m = np.zeros(rows, dtype=bool)
    if pattern == "all":
        m[:] = True
    elif pattern == "one_per_tile":
        for j in range(0, rows, 16):
            m[min(rows - 1, j + (5 * (j // 16) + 3) % 16)] = True
    elif pattern == "last_row":
        m[-1] = True
    elif pattern == "gap":
        assert rows >= 33
        m[[0, 7, 15]] = True
        m[[32, rows - 1]] = True
    return m


def flags_of(trunc, rng, safe_rl_env=False):
    """(flags int32, done uint8) [rows] whose predicate is `trunc`: truncated rows hold PGD_F_MAX_STEP, done and no cause (with
    safe_rl_env some hold a crash, which is a cost there); the others are a mix of running rows, terminations, terminations that fall on
    the time limit's step, and PGD_F_MAX_STEP without a done (never written by the step; the predicate is still defined)."""
    n = len(trunc)
    kind = rng.integers(0, 4, size=n)
    last = F_OUT_OF_ROAD | (F_CRASH_BUILDING if safe_rl_env else F_CRASH_VEHICLE)
    cause = np.array([F_ARRIVE, F_OUT_OF_ROAD, F_CRASH_BUILDING, last])[rng.integers(0, 4, size=n)]
    flags = np.where(kind == 0, 0, np.where(kind == 1, cause, np.where(kind == 2, cause | F_MAX_STEP, F_MAX_STEP)))
    done = np.where(kind == 0, 0, np.where(kind == 3, 0, 1))
    tflags = np.full(n, F_MAX_STEP)
    if safe_rl_env:
        tflags = tflags | np.array([0, F_CRASH_VEHICLE, F_CRASH_OBJECT, F_CRASH_VEHICLE | F_CRASH_BUILDING])[rng.integers(0, 4, size=n)]
    flags = np.where(trunc, tflags, flags) | (1 << 16) * done | np.where(rng.random(n) < 0.5, 256, 0)
    done = np.where(trunc, 1, done)
    flags = np.where(trunc, flags | (1 << 16), flags)
    got = np.array([truncated_ref(int(f), int(d), safe_rl_env) for f, d in zip(flags, done)])
    assert np.array_equal(got, np.asarray(trunc, dtype=bool))
    return flags.astype(np.int32), done.astype(np.uint8)
