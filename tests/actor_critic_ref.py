"""The checker of pgdrive_amd/csrc/pgd_actor_critic.h (k_mlp_actor_critic, k_gae), in plain numpy:

* heads_f64 / noise_f64 / sample_f64 / gae_f64
                     the float64 restatement: numpy_expert.py:38-45 (mean, log_std = split(fc_out); action = mean + exp(log_std) z),
                     numpy_expert.py:62-78 (the value network), the Box-Muller noise of the header from the counter hash
                     (policy_ref.pgd_rng), the log-probability, and GAE -- what tests/test_actor_critic_gpu.py holds the device against;
* emulate_heads / noise_f32 / emulate_sample / gae_f32
                     the kernels' ARITHMETIC in float32 (policy_ref's fma chains and tanh; the heads' lane partition; log as log2 times
                     a constant, exp as exp2 of a scaled argument -- what the library's build flags make of logf / expf).  Never compared
                     with the device: its purpose is the half-tolerance rule of tests/test_actor_critic_cpu.py;
* the LDS formula of the header restated (lds_bytes), from which the largest accepted in_dim is DERIVED (max_in_dim);
* the seeded cases of the GPU module (all_cases / build_case, gae_cases / build_gae) and every noise draw they use (all_draws).

Tolerances.  Head outputs (mean, log_std, value): policy_ref.TOL_EXACT.  TOL_Z and TOL_GAE are MEASURED by the emulation over exactly
the draws / shapes of the GPU tests and doubled (a case may use half its tolerance in emulation); action and log-probability follow
from those two through the formulas (tol_action, tol_logp).
"""
import zlib

import numpy as np

from tests import policy_ref as pr

H = pr.H
K_SEED, K_STREAM = 0xac7012c1, 0x5a3b1e0d   # AC_KEY_SEED, AC_KEY_STREAM of the header
LOG_2PI = float(np.log(2.0 * np.pi))
EPS = 2.0 ** -23

# max |z(float32 emulation) - z(float64)| over all_draws(): 1.37e-6 (tests/test_actor_critic_cpu.py measures it again and holds it
# below half of TOL_Z).  The largest |z| over those draws is 4.5; the error is mostly R times the rounding of the angle 2 pi u2 (2.4e-7).
TOL_Z_MEASURED = 1.37e-6
TOL_Z = 2.0 * TOL_Z_MEASURED
# max |float32 recursion - float64| over gae_cases() with both lambdas, advantages and returns: 4.87e-6 (rewards N(0, 1), values
# N(0, 2), T up to 33)
TOL_GAE_MEASURED = 4.87e-6
TOL_GAE = 2.0 * TOL_GAE_MEASURED

LOG_STD_RANGE = (-3.0, 1.0)
LOG_STD_SCALE, LOG_STD_BIAS = 0.4, -1.0   # the log_std columns of the head: w3[:, 2:4] *= scale, b3[2:4] = bias + 0.1 N(0, 1)


# ---------------------------------------------------------------------------------------------------------------------
# LDS of k_mlp_actor_critic (pgd_actor_critic.h: ac_lds_bytes) and the acceptance limit that follows from it
# ---------------------------------------------------------------------------------------------------------------------
def lds_bytes(in_dim):  # X tile | H1 | H2 | the head's weights [4][256], f32
    kp = (in_dim + 3) & ~3
    xs = kp + ((2 - kp) % 32 + 32) % 32
    return 4 * (16 * (xs + 2 * (H + 2)) + 4 * H)


def max_in_dim():
    k = 4
    while k < 4096 and lds_bytes(k + 1) <= pr.LDS_LIMIT:
        k += 1
    return k


PROLOGUE_SWITCH = 320  # rows of up to 320 floats (padded to a multiple of four) take the first form of the row prologue


# ---------------------------------------------------------------------------------------------------------------------
# float64
# ---------------------------------------------------------------------------------------------------------------------
def _hidden_f64(x, weights):
    w1, b1, w2, b2 = [np.asarray(w, dtype=np.float64) for w in weights[:4]]
    return np.tanh(np.tanh(np.asarray(x, dtype=np.float64) @ w1 + b1) @ w2 + b2)


def heads_f64(x, policy, value=None):
    """(mean [rows, 2], log_std [rows, 2], value [rows] or None): numpy_expert.py:38-45 and 62-78 in float64."""
    o = _hidden_f64(x, policy) @ np.asarray(policy[4], dtype=np.float64)[:, :4] + np.asarray(policy[5], dtype=np.float64)[:4]
    v = None
    if value is not None:
        v = (_hidden_f64(x, value) @ np.asarray(value[4], dtype=np.float64)[:, :1] + np.asarray(value[5], dtype=np.float64)[:1])[:, 0]
    return o[:, :2], o[:, 2:4], v


def draws(seed, rows, tick):
    """(r1, r2) of the header for the global rows `rows` (array): two draws of the counter hash, as uint64 arrays."""
    g = np.asarray(rows, dtype=np.uint64)
    s = (int(seed) & pr.M32) ^ K_SEED
    t = int(tick) & pr.M32
    return pr.pgd_rng(s, g, K_STREAM, t), pr.pgd_rng(s, g, K_STREAM, t ^ 0x80000000)


def units(seed, rows, tick):
    """u1, u2 = ((r >> 9) + 0.5) * 2^-23: 24 significant bits at most -- the same number in float32 and float64."""
    r1, r2 = draws(seed, rows, tick)
    return ((r1 >> np.uint64(9)).astype(np.float64) + 0.5) / 8388608.0, ((r2 >> np.uint64(9)).astype(np.float64) + 0.5) / 8388608.0


def noise_f64(seed, rows, tick):
    """z [n, 2]: R = sqrt(-2 log u1), z0 = R cos(2 pi u2), z1 = R sin(2 pi u2)."""
    u1, u2 = units(seed, rows, tick)
    R = np.sqrt(-2.0 * np.log(u1))
    return np.stack([R * np.cos(2.0 * np.pi * u2), R * np.sin(2.0 * np.pi * u2)], axis=1)


def sample_f64(mean, log_std, z):
    """(action [rows, 2], logp [rows]) from z."""
    a = mean + np.exp(log_std) * z
    return a, -0.5 * (z ** 2).sum(axis=1) - log_std.sum(axis=1) - LOG_2PI


def tol_action(mean, log_std, z):
    """|d action| <= d mean + exp(log_std) (|z| d log_std + d z) + the roundings of expf (2.5 ulp), the product and the sum."""
    e = np.exp(log_std)
    return pr.TOL_EXACT + e * (np.abs(z) * pr.TOL_EXACT + TOL_Z) + 4.0 * EPS * (np.abs(mean) + e * np.abs(z))


def tol_logp(log_std, z):
    """|d logp| <= (|z0| + |z1|) d z + d z^2 + 2 d log_std + the roundings of the four terms."""
    az = np.abs(z).sum(axis=1)
    return az * TOL_Z + TOL_Z ** 2 + 2.0 * pr.TOL_EXACT + 4.0 * EPS * (0.5 * (z ** 2).sum(axis=1) + np.abs(log_std).sum(axis=1) + LOG_2PI)


def gae_f64(reward, value, done, gamma, lam):
    """The recursion of include/pgdrive_hip.h (pgd_gae) in float64; gamma, lam as the float32 the device is given."""
    r, v = np.asarray(reward, dtype=np.float64), np.asarray(value, dtype=np.float64)
    nt = 1.0 - (np.asarray(done) != 0).astype(np.float64)
    g, gl = float(np.float32(gamma)), float(np.float32(gamma)) * float(np.float32(lam))
    adv = np.zeros_like(r)
    a = np.zeros(r.shape[1:])
    for t in range(r.shape[0] - 1, -1, -1):
        a = r[t] + g * v[t + 1] * nt[t] - v[t] + gl * nt[t] * a
        adv[t] = a
    return adv, adv + v[:-1]


def gae_by_definition_f64(reward, value, done, gamma, lam):
    """adv[t] = sum_{l >= 0} (gamma lam)^l delta[t + l], the sum cut behind the first done at or after t (O(T^2))."""
    r, v = np.asarray(reward, dtype=np.float64), np.asarray(value, dtype=np.float64)
    d = np.asarray(done) != 0
    g, gl = float(np.float32(gamma)), float(np.float32(gamma)) * float(np.float32(lam))
    T = r.shape[0]
    delta = r + g * v[1:] * (1.0 - d) - v[:-1]
    adv = np.zeros_like(r)
    for t in range(T):
        alive = np.ones(r.shape[1:], dtype=bool)
        w = 1.0
        for k in range(t, T):
            adv[t] += np.where(alive, w * delta[k], 0.0)
            alive &= ~d[k]
            w *= gl
    return adv, adv + v[:-1]


# ---------------------------------------------------------------------------------------------------------------------
# the kernels' arithmetic in float32
# ---------------------------------------------------------------------------------------------------------------------
_f32 = pr._f32


def _dots(h2, w, lanes):
    """Dot products of 256 over `lanes` lanes each (lane p takes k = p, p + lanes, ...), then a butterfly sum; f32."""
    h64, w64 = h2.astype(np.float64), w.astype(np.float64)
    part = np.zeros((lanes, h2.shape[0], w.shape[1]), dtype=np.float32)
    for k in range(H):
        part[k % lanes] = _f32(part[k % lanes].astype(np.float64) + h64[:, k, None] * w64[None, k, :])
    d = lanes >> 1
    while d:
        part = _f32(part + part[np.arange(lanes) ^ d])
        d >>= 1
    return part[0]


def _hidden_f32(x, weights):
    w1, b1, w2, b2 = [_f32(w) for w in weights[:4]]
    h1 = pr.tanh_f32(_f32(pr._fma_chain(_f32(x), w1) + b1))
    return pr.tanh_f32(_f32(pr._fma_chain(h1, w2) + b2))


def emulate_heads(x, policy, value=None):
    """(mean, log_std, value) as k_mlp_actor_critic computes them: the actor's four dot products on four lanes each, the critic's one
    on sixteen."""
    o = _f32(_dots(_hidden_f32(x, policy), _f32(policy[4])[:, :4], 4) + _f32(policy[5])[:4])
    v = None
    if value is not None:
        v = _f32(_dots(_hidden_f32(x, value), _f32(value[4])[:, :1], 16) + _f32(value[5])[:1])[:, 0]
    return o[:, :2], o[:, 2:4], v


def noise_f32(seed, rows, tick):
    """z [n, 2] float32: -2 logf(u1) = log2(u1) * (-2 ln 2) (the hardware's log2, one rounding each), the angle float32(2 pi) * u2
    rounded once, sinf / cosf and the square root rounded to float32."""
    u1, u2 = units(seed, rows, tick)
    l2 = _f32(np.log2(u1))
    R = _f32(np.sqrt(_f32(l2.astype(np.float64) * float(np.float32(-2.0 * np.log(2.0)))).astype(np.float64)))
    th = _f32(float(np.float32(2.0 * np.pi)) * u2).astype(np.float64)
    cs, sn = _f32(np.cos(th)), _f32(np.sin(th))
    return np.stack([_f32(R.astype(np.float64) * cs), _f32(R.astype(np.float64) * sn)], axis=1)


def emulate_sample(mean, log_std, z):
    """action = fma(exp2(log_std * log2 e), z, mean); logp = -log(2 pi) - (log_std0 + log_std1 + 0.5 (z0^2 + z1^2)); float32."""
    m, ls, z = _f32(mean).astype(np.float64), _f32(log_std), _f32(z).astype(np.float64)
    e = _f32(np.exp2(_f32(ls.astype(np.float64) * float(np.float32(np.log2(np.e)))).astype(np.float64))).astype(np.float64)
    a = _f32(e * z + m)
    q = _f32(z[:, 0] * z[:, 0] + _f32(z[:, 1] * z[:, 1]).astype(np.float64)).astype(np.float64)
    s = _f32(0.5 * q + _f32(ls[:, 0] + ls[:, 1]).astype(np.float64)).astype(np.float64)
    return a, _f32(-float(np.float32(LOG_2PI)) - s)


def gae_f32(reward, value, done, gamma, lam):
    """k_gae: delta = fma(gamma nt, v[t + 1], reward) - v[t]; adv = fma(gamma lam nt, adv, delta); ret = adv + v[t]; float32."""
    r, v = _f32(reward).astype(np.float64), _f32(value).astype(np.float64)
    nt = 1.0 - (np.asarray(done) != 0).astype(np.float64)
    g = float(np.float32(gamma))
    gl = float(_f32(np.float32(gamma) * np.float32(lam)))
    adv, ret = np.zeros(r.shape, dtype=np.float32), np.zeros(r.shape, dtype=np.float32)
    a = np.zeros(r.shape[1:], dtype=np.float64)
    for t in range(r.shape[0] - 1, -1, -1):
        delta = _f32(_f32(g * nt[t] * v[t + 1] + r[t]).astype(np.float64) - v[t]).astype(np.float64)
        a = _f32(gl * nt[t] * a + delta).astype(np.float64)
        adv[t] = a
        ret[t] = _f32(a + v[t])
    return adv, ret


# ---------------------------------------------------------------------------------------------------------------------
# cases of the network kernel
# ---------------------------------------------------------------------------------------------------------------------
WIDTHS = (4, 5, 35, 274, 275, PROLOGUE_SWITCH - 1, PROLOGUE_SWITCH, PROLOGUE_SWITCH + 1, 324)  # + max_in_dim()
SWEEP_ROWS = 48
ROW_COUNTS = pr.ROW_COUNTS  # 1, 15, 16, 17, 33, 4099
ROW_WIDTH = 274
OUT_COLS = (4, 5, 6)


def make_networks(rng, in_dim, out_cols):
    """(policy, value) weights: policy_ref.make_weights with a head of out_cols columns -- real values in columns 0..3, NaN beyond
    (never read), the log_std columns scaled and biased into LOG_STD_RANGE -- and a value network with a head of one column."""
    p = pr.make_weights(rng, in_dim, 1.0, out_cols, nan_unused=False)
    p[4][:, 2:4] *= np.float32(LOG_STD_SCALE)
    p[5][2:4] += np.float32(LOG_STD_BIAS)
    p[4][:, 4:] = np.nan
    p[5][4:] = np.nan
    v = pr.make_weights(rng, in_dim, 1.0, 1, nan_unused=False)
    return p, v


def build_case(name, in_dim, rows, scaling="unit", out_cols=4, seed=0, tick=0):
    """(x [rows, stride] float32 with NaN padding, policy, value): a pure function of its arguments; `seed` and `tick` are also the
    noise's."""
    rng = np.random.default_rng([zlib.crc32(name.encode()), in_dim, rows, pr.SCALINGS.index(scaling), out_cols, seed])
    x = pr.make_inputs(rng, rows, in_dim, scaling)
    p, v = make_networks(rng, in_dim, out_cols)
    return x, p, v


def sweep_cases():
    for i, k in enumerate(WIDTHS + (max_in_dim(), )):
        for j, sc in enumerate(("unit", "normalised")):
            yield dict(name="sweep", in_dim=k, rows=SWEEP_ROWS, scaling=sc, out_cols=OUT_COLS[(i + j) % 3], seed=i, tick=(0, 1, 2 ** 31, 2 ** 32 - 1)[(i + j) % 4])


def row_cases():
    for n in ROW_COUNTS:
        yield dict(name="rows", in_dim=ROW_WIDTH, rows=n, scaling="unit", out_cols=4, seed=n, tick=n)


def other_cases():
    yield dict(name="permute", in_dim=35, rows=40, scaling="normalised", out_cols=5, seed=3, tick=9)
    yield dict(name="permute", in_dim=324, rows=40, scaling="normalised", out_cols=4, seed=4, tick=10)
    yield dict(name="groups", in_dim=274, rows=16, scaling="unit", out_cols=4, seed=5, tick=11)       # 8 envs x 2 groups ... 16 envs
    yield dict(name="marl", in_dim=274, rows=30, scaling="unit", out_cols=6, seed=6, tick=12)         # 6 envs x 5 seats, 2 groups
    yield dict(name="nocritic", in_dim=275, rows=24, scaling="unit", out_cols=6, seed=7, tick=13)
    yield dict(name="boundary", in_dim=max_in_dim(), rows=20, scaling="normalised", out_cols=5, seed=11, tick=3)  # a fresh engine's first launch


def all_cases():
    for gen in (sweep_cases, row_cases, other_cases):
        for c in gen():
            yield c


# the noise test proper (w3 = 0, b3 = 0: the action IS z): (engine rows, env_base, seed, tick)
NOISE_ROWS = 4099
NOISE_RUNS = [(NOISE_ROWS, 0, 0, 0), (NOISE_ROWS, 0, 0, 1), (NOISE_ROWS, 0, 1, 0), (NOISE_ROWS, 0, 0xdeadbeef, 2 ** 31),
              (NOISE_ROWS, 0, 5, 2 ** 32 - 1), (33, 1000, 0, 0), (33, 3000000, 9, 77)]


def all_draws():
    """(seed, global rows, tick) of every noise draw the GPU tests compare against float64."""
    for n, base, seed, tick in NOISE_RUNS:
        yield seed, base + np.arange(n), tick
    for c in all_cases():
        yield c["seed"], np.arange(c["rows"]), c["tick"]


# ---------------------------------------------------------------------------------------------------------------------
# cases of GAE
# ---------------------------------------------------------------------------------------------------------------------
GAE_T = (1, 2, 33)
GAE_ROWS = (1, 63, 64, 65, 4099)
GAE_DONES = ("none", "all", "bernoulli", "first", "last")
GAE_LAM = (0.0, 0.95)
GAE_GAMMA = 0.99


def gae_cases():
    for T in GAE_T:
        for rows in GAE_ROWS:
            for pattern in GAE_DONES:
                yield dict(T=T, rows=rows, pattern=pattern)


def build_gae(T, rows, pattern):
    """(reward [T, rows] f32, value [T + 1, rows] f32, done [T, rows] uint8): rewards N(0, 1), values N(0, 2)."""
    rng = np.random.default_rng([T, rows, GAE_DONES.index(pattern)])
    reward = rng.normal(0, 1, size=(T, rows)).astype(np.float32)
    value = rng.normal(0, 2, size=(T + 1, rows)).astype(np.float32)
    done = np.zeros((T, rows), dtype=np.uint8)
    if pattern == "all":
        done[:] = 1
    elif pattern == "bernoulli":
        done[:] = rng.uniform(size=(T, rows)) < 0.1
    elif pattern == "first":
        done[0] = 1
    elif pattern == "last":
        done[-1] = 1
    return reward, value, done
