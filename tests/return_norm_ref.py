"""Float64 checker of pgd_return_norm (include/pgdrive_hip.h states the rule), written from its formulas: the running discounted return
of every row, its samples, Chan's merge into the record (count, mean, m2, scale) and the scaled rewards; plain and with step flags.
Shared by tests/test_return_norm_cpu.py and tests/test_return_norm_gpu.py."""
import numpy as np

F_RESET, F_REPORT = 1 << 16, 1 << 17
RECORD_INIT = (1e-4, 0.0, 1e-4, 1.0)   # count, mean, m2, scale: RunningMeanStd(mean 0, variance 1, count 1e-4), m2 = variance * count
TOL_STATS = 1e-12                      # mean (relative to sqrt(m2 / count)) and m2 (relative), device against checker on the same samples

# the shapes of the exact-input tests: around a wave, a workgroup of the merge launch, several workgroups
EXACT_T = (1, 2, 16)
EXACT_ROWS = (1, 63, 64, 65, 257, 1000)
EXACT_GAMMA = 0.5


def fma32(a, b, c):
    """fma(a, b, c) in float32: the product of two float32 is exact in the 64-bit significand of a long double, the sum is rounded there
    once and to float32 once (a double rounding needs a sum within 2^-40 of a float32 tie)."""
    ld = np.longdouble
    return (np.asarray(a, np.float32).astype(ld) * np.asarray(b, np.float32).astype(ld) + np.asarray(c, np.float32).astype(ld)).astype(np.float32)


def acted(flags):
    return (np.asarray(flags).astype(np.int64) & F_REPORT) != 0


def cont(flags, done):
    return acted(flags) & (np.asarray(done) == 0) & ((np.asarray(flags).astype(np.int64) & F_RESET) == 0)


def running_returns(reward, done, gamma, carry, flags=None, fp32=False):
    """The recursion of the rule over a rollout [T, rows...]: -> (R [T, ...] float64, the value that is a sample where `sampled`;
    sampled [T, ...] bool; carry_out [...]).  fp32: R is formed as the device forms it, by one float32 fma per step (else in float64)."""
    reward, done = np.asarray(reward), np.asarray(done)
    T = reward.shape[0]
    R = np.array(carry, dtype=np.float32 if fp32 else np.float64)
    out = np.zeros(reward.shape, dtype=np.float64)
    sampled = np.ones(reward.shape, dtype=bool) if flags is None else acted(flags)
    g = np.float32(gamma) if fp32 else float(gamma)
    for t in range(T):
        with np.errstate(invalid="ignore"):
            Rn = fma32(g, R, reward[t]) if fp32 else g * R + reward[t].astype(np.float64)
        out[t] = np.where(sampled[t], Rn, 0.0)
        keep = (done[t] == 0) if flags is None else cont(flags[t], done[t])
        R = np.where(sampled[t] & keep, Rn, 0).astype(R.dtype)   # (a selection: a NaN behind a row that did not act reaches nothing)
    return out, sampled, R


def moments(x):
    """n, mean, sum of squared deviations of the samples x (float64, two passes)."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    if x.size == 0:
        return 0, 0.0, 0.0
    m = float(x.mean())
    return x.size, m, float(((x - m) ** 2).sum())


def chan(count, mean, m2, n, bmean, bm2):
    """Chan's parallel update of (count, mean, m2) by a batch (n, bmean, bm2); n = 0: unchanged."""
    if n == 0:
        return count, mean, m2
    delta, tot = bmean - mean, count + n
    return tot, mean + delta * n / tot, m2 + bm2 + delta * delta * count * n / tot


def scale_of(count, m2, eps):
    return 1.0 / np.sqrt(m2 / count + eps)


def scaled_rewards(reward, scale, clip, flags=None):
    """reward * (float) scale in float32, clamped, 0 where no agent acted."""
    reward = np.asarray(reward, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        x = reward * np.float32(scale)
        if clip > 0:
            x = np.minimum(np.maximum(x, np.float32(-clip)), np.float32(clip))
    return x if flags is None else np.where(acted(flags), x, np.float32(0.0)).astype(np.float32)


def return_norm_f64(reward, done, gamma, carry, record, flags=None, eps=1e-8, clip=10.0, freeze=False, fp32=False, samples=None):
    """One call of pgd_return_norm -> dict(carry, record (4 float64), scaled (float32), samples (the call's samples, flat)).  `samples`:
    take these as the call's samples instead of the recursion's (the device's own, reconstructed by a test)."""
    R, sampled, carry_out = running_returns(reward, done, gamma, carry, flags, fp32)
    x = R[sampled] if samples is None else np.asarray(samples, dtype=np.float64).reshape(-1)
    count, mean, m2, scale = [float(v) for v in record]
    if not freeze:
        count, mean, m2 = chan(count, mean, m2, *moments(x))
        scale = float(scale_of(count, m2, eps))
    else:
        carry_out = np.array(carry, dtype=carry_out.dtype)
    return dict(carry=carry_out, record=np.array([count, mean, m2, scale]), scaled=scaled_rewards(reward, scale, clip, flags), samples=x)


def vecnormalize_stepwise(reward, done, gamma, eps, clip):
    """VecNormalize's norm_reward rule, one step at a time (ret = ret * gamma + reward; ret_rms.update(ret) over the envs;
    ret[done] = 0), from a fresh RunningMeanStd -- and then every step of the call scaled by the FINAL variance.
    -> (scaled float32 [T, N], (count, mean, var))."""
    reward = np.asarray(reward, dtype=np.float64)
    T, N = reward.shape
    mean, var, count = 0.0, 1.0, 1e-4
    ret = np.zeros(N)
    for t in range(T):
        ret = ret * gamma + reward[t]
        bmean, bvar, bcount = ret.mean(), ret.var(), N
        delta, tot = bmean - mean, count + bcount
        new_mean = mean + delta * bcount / tot
        m2 = var * count + bvar * bcount + delta ** 2 * count * bcount / tot
        mean, var, count = new_mean, m2 / tot, tot
        ret = np.where(done[t] != 0, 0.0, ret)
    return scaled_rewards(reward, 1.0 / np.sqrt(var + eps), clip), (count, mean, var)


def exact_case(T, rows, dones, seed=0):
    """Integer rewards in [-8, 8] and dones at rate 0.2 ("some"), everywhere ("all") or nowhere ("none"): with gamma = 0.5 every running
    return is an integer multiple of 2^-k, k < 24 + the steps since the last done, small enough to be exact in float32 over the T of
    the tests (held by test_return_norm_cpu.py)."""
    rng = np.random.default_rng([seed, T, rows])
    reward = rng.integers(-8, 9, size=(T, rows)).astype(np.float32)
    done = dict(some=rng.uniform(size=(T, rows)) < 0.2, all=np.ones((T, rows), bool), none=np.zeros((T, rows), bool))[dones].astype(np.uint8)
    return reward, done


def seat_history(rng, T, rows, p_acted=0.7, p_done=0.15, p_reset=0.05):
    """Step flags of seats that change hands: PGD_F_REPORT where an agent acted, dones among those, PGD_F_RESET with and without a done,
    and other bits that must not matter.  -> flags int32 [T, rows], done uint8 [T, rows]."""
    act = rng.uniform(size=(T, rows)) < p_acted
    done = (act & (rng.uniform(size=(T, rows)) < p_done)).astype(np.uint8)
    reset = rng.uniform(size=(T, rows)) < p_reset
    noise = rng.integers(0, 1 << 14, size=(T, rows))   # (causes and line bits)
    flags = (noise | np.where(act, F_REPORT, 0) | np.where(reset, F_RESET, 0) | np.where(rng.uniform(size=(T, rows)) < 0.1, 1 << 18, 0)).astype(np.int32)
    return flags, done
