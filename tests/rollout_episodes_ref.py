"""Float64 / numpy checker of pgd_rollout_episodes (include/pgdrive_hip.h states the rule), in two routines that share nothing but the
predicates:

* by_definition: every row's series is cut into episodes, each episode's return is formed by sequential np.float32 adds (exactly what
  the device does: the samples are bit-exact), and the record is plain numpy statistics over the list of samples;
* kernel_order: the rows side by side step by step, a row's samples in shifted sums, the rows of a wave, the partials and the waves merged
  by Chan's update in the order of the two kernels.

Shared by tests/test_rollout_episodes_cpu.py and tests/test_rollout_episodes_gpu.py."""
import numpy as np

from tests import return_norm_ref as rn

F_RESET, F_REPORT, F_NEW = rn.F_RESET, rn.F_REPORT, 1 << 18
CAUSES = ("arrive", "out_of_road", "crash_vehicle", "crash_object", "crash_building", "max_step")   # bits 0 .. 5 of the flags
FIELDS = ("episodes", "return_mean", "return_m2", "return_min", "return_max", "length_sum", "length_max") + CAUSES + ("cut", "steps", "calls")
INIT = np.array([0.0, 0.0, 0.0, np.inf, -np.inf] + [0.0] * 11)
INTEGER_SLOTS = (0, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)   # compared with ==
BITWISE_SLOTS = (3, 4)                                       # return_min, return_max: samples, bit for bit
TOL_STATS = rn.TOL_STATS
WAVE, MERGE_THREADS = 64, 256

# the shapes of the exact-input tests: around a wave, several workgroups; (1, 16449): 258 partials, a second pass of the merge's threads
EXACT_SHAPES = tuple((T, rows) for T in (1, 2, 16) for rows in (1, 63, 64, 65, 257, 1000)) + ((1, 16449), )


def predicates(done, flags, seats):
    """-> acted, ends (bool arrays of done's shape)."""
    done, f = np.asarray(done) != 0, np.asarray(flags).astype(np.int64)
    if not seats:
        return np.ones(done.shape, bool), done
    acted = (f & F_REPORT) != 0
    cont = acted & ~done & ((f & F_RESET) == 0)
    return acted, acted & ~cont


# ---------------------------------------------------------------------------------------------------------------------
# by definition
# ---------------------------------------------------------------------------------------------------------------------
def moments(x):
    """n, mean, sum of squared deviations of the samples x (float64, two passes).  Samples that are all equal: their value and 0 (what
    any order of exact operations gives; the two-pass mean of n equal values may round)."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    if x.size == 0:
        return 0.0, 0.0, 0.0
    if (x == x[0]).all():
        return float(x.size), float(x[0]), 0.0
    m = float(x.mean())
    return float(x.size), m, float(((x - m) ** 2).sum())


def record_of(samples, steps):
    """The record of one call from its list of samples (R, L, f, d)."""
    rec = INIT.copy()
    rec[14], rec[15] = steps, 1.0
    if not samples:
        return rec
    R = np.array([s[0] for s in samples], np.float32)
    L = np.array([s[1] for s in samples], np.int64)
    f = np.array([s[2] for s in samples], np.int64)
    d = np.array([s[3] for s in samples], np.int64)
    rec[0], rec[1], rec[2] = moments(R)
    rec[3], rec[4] = R.min(), R.max()
    rec[5], rec[6] = L.sum(), L.max()
    for c in range(len(CAUSES)):
        rec[7 + c] = ((f >> c) & 1).sum()
    rec[13] = (d == 0).sum()
    return rec


def by_definition(reward, done, flags, ret_carry, len_carry, seats=False):
    """One call -> dict(samples: the list of (R float32, L, f, d) of the episodes that ended, rows in order and t in order within a row;
    call: the call's record; ret_carry, len_carry; ep_return float32, ep_length int32 [T, rows]; steps)."""
    reward, done, flags = np.asarray(reward, np.float32), np.asarray(done), np.asarray(flags)
    T = reward.shape[0]
    reward, done, flags = reward.reshape(T, -1), done.reshape(T, -1), flags.reshape(T, -1)
    rows = reward.shape[1]
    acted, ends = predicates(done, flags, seats)
    ret_out, len_out = np.array(ret_carry, np.float32).reshape(-1).copy(), np.array(len_carry, np.int32).reshape(-1).copy()
    ep_return, ep_length = np.zeros((T, rows), np.float32), np.zeros((T, rows), np.int32)
    samples = []
    for r in range(rows):
        R, L = np.float32(ret_out[r]), int(len_out[r])
        for t in range(T):
            if acted[t, r]:
                R = np.float32(R + reward[t, r])   # one float32 add
                L += 1
            if ends[t, r]:
                samples.append((R, L, int(flags[t, r]), int(done[t, r])))
                ep_return[t, r], ep_length[t, r] = R, L
                R, L = np.float32(0.0), 0
        ret_out[r], len_out[r] = R, L
    steps = int(acted.sum())
    return dict(samples=samples, call=record_of(samples, steps), ret_carry=ret_out, len_carry=len_out, ep_return=ep_return, ep_length=ep_length,
                steps=steps)


def merge_record(record, call):
    """The running record after a call, from the call's own: Chan's update, min, max, sums; a call without an episode moves steps and
    calls only."""
    out = np.array(record, np.float64)
    if call[0] > 0:
        out[0], out[1], out[2] = rn.chan(record[0], record[1], record[2], call[0], call[1], call[2])
        out[3], out[4] = min(record[3], call[3]), max(record[4], call[4])
        out[5], out[6] = record[5] + call[5], max(record[6], call[6])
        out[7:14] = record[7:14] + call[7:14]
    out[14], out[15] = record[14] + call[14], record[15] + 1.0
    return out


# ---------------------------------------------------------------------------------------------------------------------
# in the kernels' order
# ---------------------------------------------------------------------------------------------------------------------
def _merge(a, b):
    """a + b over the last axis of [..., 15] statistics (slots 0 .. 14 of a record), as the kernels' ep_merge."""
    o = np.empty_like(a)
    tot = a[..., 0] + b[..., 0]
    w = np.where(b[..., 0] > 0, b[..., 0] / np.where(tot > 0, tot, 1.0), 0.0)
    delta = b[..., 1] - a[..., 1]
    o[..., 0] = tot
    o[..., 1] = a[..., 1] + delta * w
    o[..., 2] = a[..., 2] + b[..., 2] + delta * delta * (a[..., 0] * w)
    o[..., 3], o[..., 4] = np.minimum(a[..., 3], b[..., 3]), np.maximum(a[..., 4], b[..., 4])
    o[..., 5], o[..., 6] = a[..., 5] + b[..., 5], np.maximum(a[..., 6], b[..., 6])
    o[..., 7:15] = a[..., 7:15] + b[..., 7:15]
    return o


def _wave_merge(s):
    """[..., 64, 15] -> [..., 15]: lane l with lane l + 32, 16, .. 1."""
    k = WAVE // 2
    while k >= 1:
        s = _merge(s[..., :k, :], s[..., k:2 * k, :])
        k //= 2
    return s[..., 0, :]


def kernel_order(reward, done, flags, ret_carry, len_carry, seats=False):
    """One call -> dict(call, ret_carry, len_carry, ep_return, ep_length), the statistics formed as the kernels form them."""
    reward, done, flags = np.asarray(reward, np.float32), np.asarray(done), np.asarray(flags)
    T = reward.shape[0]
    reward, done, flags = reward.reshape(T, -1), done.reshape(T, -1), flags.reshape(T, -1).astype(np.int64)
    rows = reward.shape[1]
    acted, ends = predicates(done, flags, seats)
    R, L = np.array(ret_carry, np.float32).reshape(-1).copy(), np.array(len_carry, np.int64).reshape(-1).copy()
    ep_return, ep_length = np.zeros((T, rows), np.float32), np.zeros((T, rows), np.int32)
    n, K, s1, s2 = np.zeros(rows), np.zeros(rows), np.zeros(rows), np.zeros(rows)
    stat = np.zeros((rows, 15))
    stat[:, 3], stat[:, 4] = np.inf, -np.inf
    for t in range(T):
        a, e = acted[t], ends[t]
        with np.errstate(invalid="ignore"):
            R = np.where(a, R + reward[t], R).astype(np.float32)   # (a selection: a NaN behind a row that did not act reaches nothing)
        L = L + a
        x = R.astype(np.float64)
        K = np.where(n == 0, x, K)
        dx = x - K
        s1, s2, n = np.where(e, s1 + dx, s1), np.where(e, s2 + dx * dx, s2), n + e
        stat[:, 3], stat[:, 4] = np.where(e, np.minimum(stat[:, 3], x), stat[:, 3]), np.where(e, np.maximum(stat[:, 4], x), stat[:, 4])
        stat[:, 5] += np.where(e, L, 0)
        stat[:, 6] = np.where(e, np.maximum(stat[:, 6], L), stat[:, 6])
        for c in range(len(CAUSES)):
            stat[:, 7 + c] += e & (((flags[t] >> c) & 1) != 0)
        stat[:, 13] += e & (done[t] == 0)
        stat[:, 14] += a
        ep_return[t], ep_length[t] = np.where(e, R, np.float32(0.0)), np.where(e, L, 0)
        R, L = np.where(e, np.float32(0.0), R).astype(np.float32), np.where(e, 0, L)
    q = s1 / np.maximum(n, 1.0)
    stat[:, 0], stat[:, 1], stat[:, 2] = n, np.where(n > 0, K + q, 0.0), np.where(n > 0, np.maximum(s2 - s1 * q, 0.0), 0.0)
    empty = np.zeros(15)
    empty[3], empty[4] = np.inf, -np.inf
    n_part = (rows + WAVE - 1) // WAVE
    lanes = np.tile(empty, (n_part * WAVE, 1))
    lanes[:rows] = stat
    partial = _wave_merge(lanes.reshape(n_part, WAVE, 15))
    threads = np.tile(empty, (MERGE_THREADS, 1))
    for first in range(0, n_part, MERGE_THREADS):   # thread i: partials i, i + 256, .. in order
        chunk = partial[first:first + MERGE_THREADS]
        threads[:len(chunk)] = _merge(threads[:len(chunk)], chunk)
    waves = _wave_merge(threads.reshape(MERGE_THREADS // WAVE, WAVE, 15))
    total = waves[0]
    for k in range(1, len(waves)):
        total = _merge(total, waves[k])
    return dict(call=np.concatenate([total, [1.0]]), ret_carry=R, len_carry=L.astype(np.int32), ep_return=ep_return, ep_length=ep_length)


# ---------------------------------------------------------------------------------------------------------------------
# comparing records
# ---------------------------------------------------------------------------------------------------------------------
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def check_record(got, want, where):
    """Every integer slot with ==; return_min / return_max bit for bit (they are samples); mean within TOL_STATS of sqrt(m2 / episodes) and
    m2 within TOL_STATS relative -- return_norm_ref's criterion.  Where the samples are all equal (m2 == 0 in `want`: one sample, or equal
    ones) every operation of either order is exact: mean and m2 are then compared with ==.  -> the error."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    for k in INTEGER_SLOTS:
        assert got[k] == want[k], (where, FIELDS[k], got[k], want[k])
    for k in BITWISE_SLOTS:
        assert bits(got[k:k + 1])[0] == bits(want[k:k + 1])[0], (where, FIELDS[k], got[k], want[k])
    if want[2] == 0.0:
        assert got[1] == want[1] and got[2] == 0.0, (where, "equal samples", got[:3], want[:3])
        return 0.0
    sd = np.sqrt(want[2] / want[0])
    err = max(abs(got[1] - want[1]) / sd, abs(got[2] - want[2]) / want[2])
    assert err < TOL_STATS, (where, err, got[:3], want[:3])
    return err


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
def cause_flags(rng, shape):
    """Step flags of single-agent rows: the six causes at random at EVERY entry (only those of an end may count) and line bits."""
    return (rng.integers(0, 64, size=shape) | (rng.integers(0, 64, size=shape) << 8)).astype(np.int32)


def exact_case(T, rows, dones, seed=0):
    """Integer rewards in [-8, 8], dones at rate 0.2 ("some"), everywhere ("all") or nowhere ("none"), integer carries: every running
    return is an integer below 2^24 in size, exact in float32 in any order.  -> reward, done, flags, ret_carry, len_carry."""
    rng = np.random.default_rng([seed, T, rows])
    reward = rng.integers(-8, 9, size=(T, rows)).astype(np.float32)
    done = dict(some=rng.uniform(size=(T, rows)) < 0.2, all=np.ones((T, rows), bool), none=np.zeros((T, rows), bool))[dones].astype(np.uint8)
    return reward, done, cause_flags(rng, (T, rows)), rng.integers(-40, 41, size=rows).astype(np.float32), rng.integers(0, 9, size=rows).astype(np.int32)


def general_case(T, rows, seed=0, p_done=0.1):
    """Normal rewards and carries.  -> reward, done, flags, ret_carry, len_carry."""
    rng = np.random.default_rng([seed, T, rows, 1])
    reward = (rng.normal(size=(T, rows)) * 3.0 + 0.5).astype(np.float32)
    done = (rng.uniform(size=(T, rows)) < p_done).astype(np.uint8)
    return reward, done, cause_flags(rng, (T, rows)), rng.normal(size=rows).astype(np.float32), rng.integers(0, 50, size=rows).astype(np.int32)


def seat_case(T, rows, seed=0):
    """Seats that change hands (return_norm_ref.seat_history: agents that start mid-rollout, end by done, are cut by PGD_F_RESET without
    a done, follow each other in a seat), dones also at entries at which nobody acted (they must not count), and NaN as the reward of
    every entry that did not act.  -> reward, done, flags, ret_carry, len_carry."""
    rng = np.random.default_rng([seed, T, rows, 2])
    flags, done = rn.seat_history(rng, T, rows)
    acted = rn.acted(flags)
    done = (done | (~acted & (rng.uniform(size=(T, rows)) < 0.3))).astype(np.uint8)
    reward = (rng.normal(size=(T, rows)) * 3.0).astype(np.float32)
    reward[~acted] = np.nan
    return reward, done, flags, rng.normal(size=rows).astype(np.float32), rng.integers(0, 50, size=rows).astype(np.int32)
