"""The checker of pgdrive_amd/csrc/pgd_ppo.h (pgd_ppo_grad, pgd_adv_stats, pgd_adam), in plain numpy:

* loss_and_grads_f64 / adv_stats_f64 / adam_f64
                     the formulas of include/pgdrive_hip.h in float64, the backward pass derived by hand (tests/test_ppo_update_cpu.py
                     holds it against torch autograd) -- what tests/test_ppo_update_gpu.py holds the device against;
* emulate_grads / emulate_adv_stats / emulate_adam
                     the kernels' ARITHMETIC and summation order in float32 (fma chains in k order on the matrix cores; tanh through
                     exp2 and a reciprocal; the row loss in double from the fp32 heads; weight gradients as fma chains over the rows of
                     a partition of 1024, the partitions in order; tile sums of 16 rows, the tiles 16-strided).  Never compared with the
                     device: its purpose is to MEASURE the tolerances and the half-tolerance rule of the CPU test;
* the seeded cases of the GPU module.

Errors are normalised per entry by the float64 sum of the absolute values of the entry's contributions (`norm` below: for a gradient
the backward pass with every sum replaced by the sum of the absolute values of its terms, for a mean sum |term| / n), so that
cancellation does not hide in an absolute number.  An entry whose
contributions are all zero must be exactly zero.

Tolerances: each *_MEASURED constant is the largest normalised error of the emulation against float64 over exactly the cases named in
its comment; the tolerance is twice that; the CPU test measures again and holds the emulation below half of the tolerance.
"""
import collections
import functools
import zlib

import numpy as np

from tests import actor_critic_ref as ar
from tests import policy_ref as pr

H = pr.H
LOG_2PI = float(np.log(2.0 * np.pi))
LOG_2PIE = LOG_2PI + 1.0
PART = 1024          # PPO_PART of the header: rows per partial sum of a weight gradient
CLIP, VF_COEF, ENT_COEF = 0.2, 0.5, 0.01
GRAD_NAMES = ("w1", "b1", "w2", "b2", "w3", "b3")

# Gradients and statistics: the largest normalised error of emulate_grads against loss_and_grads_f64 over compared_cases() (the width
# sweep, the row counts, the list forms, the case without a critic, the three-partition case and the split of the 1027-row case of the
# GPU module; every gradient entry of both networks / the six statistics), taken per ROW CLASS: a sum over n rows averages the rows'
# roundings, so one figure set by the single-row cases would leave the large cases -- those that cross the kernels' tile and partition
# boundaries -- an order of magnitude of slack.  Classes by live rows n: "few" n < 16 (less than a tile), "tile" 16 <= n < 1024,
# "part" n >= 1024 (more than one partition of the weight-gradient reduction).
ROW_CLASSES = (("few", 1, 15), ("tile", 16, 1023), ("part", 1024, 1 << 30))
TOL_GRAD_MEASURED = dict(few=5.163e-7, tile=1.283e-7, part=4.129e-8)
TOL_STAT_MEASURED = dict(few=8.191e-7, tile=2.152e-7, part=3.227e-8)


def row_class(n):
    return [name for name, lo, hi in ROW_CLASSES if lo <= n <= hi][0]


def tolerances(n):
    """(TOL_GRAD, TOL_STAT) of a minibatch of n live rows: twice the measured figures of its row class."""
    return 2.0 * TOL_GRAD_MEASURED[row_class(n)], 2.0 * TOL_STAT_MEASURED[row_class(n)]


# max normalised error of emulate_adv_stats over ADV_COUNTS with and without an index (mean: by sum |adv| / n; 1 / (std + 1e-8): relative)
TOL_ADV_MEASURED = 1.149e-7
TOL_ADV = 2.0 * TOL_ADV_MEASURED
# max normalised error of three emulate_adam steps over adam_cases() (p: by |p| + |step|; m, v: by their two terms)
TOL_ADAM_MEASURED = 3.461e-6
TOL_ADAM = 2.0 * TOL_ADAM_MEASURED
# L(before) - L(after) of ten adam_f64 steps of the float64 reference on the minibatch closed_loop_case() (in_dim 35, 64 rows, lr 3e-4)
CLOSED_LOOP_D = 0.11347946

_f32 = pr._f32
_f64 = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731


# ---------------------------------------------------------------------------------------------------------------------
# float64
# ---------------------------------------------------------------------------------------------------------------------
def _forward_f64(x, net):
    w1, b1, w2, b2, w3, b3 = [_f64(w) for w in net]
    h1 = np.tanh(_f64(x) @ w1 + b1)
    h2 = np.tanh(h1 @ w2 + b2)
    return h1, h2


def _backward_f64(x, h1, h2, d_out, n_out, net, heads):
    """(grads in the weights' shapes, norms of the same shapes) from dL/d(head outputs) [n, heads] and the sums of the absolute values
    of ITS terms, n_out.  The norms are the backward pass with every sum replaced by the sum of the absolute values of its terms -- down to
    the single products dOut W3 (1 - h2^2) W2 (1 - h1^2) x --, so the cancellation inside a row's 256-term sums counts as well.  The two
    differences the kernels form count as sums too: an activation is h = 1 - 2 / (e^2x + 1) (mlp_tanh), terms 1 and 1 - h, so it enters
    a norm as 2 - h, not |h| (its error is a few ulp of ONE however small h is); tanh' = 1 - h h enters as 1 + h h."""
    w2, w3 = _f64(net[2]), _f64(net[4])
    out_cols = w3.shape[1]
    dz2 = (d_out @ w3[:, :heads].T) * (1.0 - h2 * h2)
    dz1 = (dz2 @ w2.T) * (1.0 - h1 * h1)
    nz2 = (n_out @ np.abs(w3[:, :heads]).T) * (1.0 + h2 * h2)
    nz1 = (nz2 @ np.abs(w2).T) * (1.0 + h1 * h1)
    x = _f64(x)
    dw3, nw3 = np.zeros((H, out_cols)), np.zeros((H, out_cols))
    dw3[:, :heads], nw3[:, :heads] = h2.T @ d_out, (2.0 - h2).T @ n_out
    db3, nb3 = np.zeros(out_cols), np.zeros(out_cols)
    db3[:heads], nb3[:heads] = d_out.sum(axis=0), n_out.sum(axis=0)
    g = [x.T @ dz1, dz1.sum(axis=0), h1.T @ dz2, dz2.sum(axis=0), dw3, db3]
    nrm = [np.abs(x).T @ nz1, nz1.sum(axis=0), (2.0 - h1).T @ nz2, nz2.sum(axis=0), nw3, nb3]
    return g, nrm


def row_terms_f64(mean, ls, action, logp_old, adv, adv_stats, clip):
    """Per live row: (A, logp, r, flows, z, e) of the header, float64; clip as the float32 the device is given."""
    A = _f64(adv)
    if adv_stats is not None:
        A = (A - float(adv_stats[0])) * float(adv_stats[1])
    e = np.exp(-ls)
    z = (_f64(action) - mean) * e
    logp = -0.5 * (z ** 2).sum(axis=1) - ls.sum(axis=1) - LOG_2PI
    r = np.exp(logp - _f64(logp_old))
    c = float(np.float32(clip))
    rc = np.clip(r, 1.0 - c, 1.0 + c)
    return A, logp, r, (r * A <= rc * A), z, e, rc


def loss_and_grads_f64(x, action, logp_old, adv, ret, policy, value, clip=CLIP, vf_coef=VF_COEF, ent_coef=ENT_COEF, adv_stats=None):
    """The live rows of one minibatch in (x [n, in_dim], action [n, 2], logp_old, adv, ret [n]) -> dict(stats [8], loss, policy / value:
    six gradients each (value None without a critic), policy_norm / value_norm, stat_norm [8])."""
    n = int(np.asarray(x).shape[0])
    in_dim = np.asarray(policy[0]).shape[0]
    out_cols = np.asarray(policy[4]).shape[1]
    vf, ce = float(np.float32(vf_coef)), float(np.float32(ent_coef))
    zero = lambda net, oc: [np.zeros((in_dim, H)), np.zeros(H), np.zeros((H, H)), np.zeros(H), np.zeros((H, oc)), np.zeros(oc)]  # noqa: E731
    if n == 0:
        return dict(stats=np.zeros(8), stat_norm=np.zeros(8), loss=0.0, policy=zero(policy, out_cols), policy_norm=zero(policy, out_cols),
                    value=None if value is None else zero(value, 1), value_norm=None if value is None else zero(value, 1))
    x = _f64(np.asarray(x)[:, :in_dim])
    h1, h2 = _forward_f64(x, policy)
    o = h2 @ _f64(policy[4])[:, :4] + _f64(policy[5])[:4]
    mean, ls = o[:, :2], o[:, 2:4]
    A, logp, r, flows, z, e, rc = row_terms_f64(mean, ls, action, logp_old, adv, adv_stats, clip)
    g = np.where(flows, -A * r / n, 0.0)
    d_out = np.concatenate([g[:, None] * z * e, g[:, None] * (z * z - 1.0) - ce / n], axis=1)
    # dOut's own terms: z = (a - mean) e is a difference -- |a| + |mean| stands for it --, and dL/dlogp carries exp(logp - logp_old),
    # whose error is r times that of a difference of two numbers of logp's size
    nz = (np.abs(_f64(action)) + np.abs(mean)) * e
    ng = (np.abs(g) * (1.0 + np.abs(logp) + np.abs(_f64(logp_old))))[:, None]
    n_out = np.concatenate([ng * nz * e, ng * (nz * nz + 1.0) + ce / n], axis=1)
    pg, pn = _backward_f64(x, h1, h2, d_out, n_out, policy, 4)
    ent = ls.sum(axis=1) + LOG_2PIE
    terms = [np.full(n, float(n)), -np.minimum(r * A, rc * A), np.zeros(n), ent, _f64(logp_old) - logp, (~flows).astype(np.float64), r, np.zeros(n)]
    # the terms' own contributions: logp_old - logp is a difference of two numbers of logp's size, and r = exp of that difference
    # carries its error times r -- so the ratio and the surrogate count with the factor 1 + |logp| + |logp_old|
    cond = 1.0 + np.abs(logp) + np.abs(_f64(logp_old))
    term_norms = [None, np.abs(terms[1]) * cond, None, np.abs(ls).sum(axis=1) + LOG_2PIE, np.abs(logp) + np.abs(_f64(logp_old)), None, r * cond, None]
    vg = vn = None
    if value is not None:
        vh1, vh2 = _forward_f64(x, value)
        v = (vh2 @ _f64(value[4])[:, :1] + _f64(value[5])[:1])[:, 0]
        err = v - _f64(ret)
        terms[2] = 0.5 * err * err
        term_norms[2] = 0.5 * (np.abs(v) + np.abs(_f64(ret))) ** 2
        vg, vn = _backward_f64(x, vh1, vh2, (vf * err / n)[:, None], (vf * (np.abs(v) + np.abs(_f64(ret))) / n)[:, None], value, 1)   # (v - ret: a difference)
    stats = np.array([t.sum() / n for t in terms])
    stat_norm = np.array([np.abs(t if q is None else q).sum() / n for t, q in zip(terms, term_norms)])
    stats[0], stat_norm[0] = n, n
    loss = stats[1] + vf * stats[2] - ce * stats[3]
    return dict(stats=stats, stat_norm=stat_norm, loss=float(loss), policy=pg, policy_norm=pn, value=vg, value_norm=vn)


def adv_stats_f64(adv):
    """(mean, 1 / (std + 1e-8)) of the live advantages, population std; no entries: (0, 1)."""
    a = _f64(adv).reshape(-1)
    if a.size == 0:
        return np.array([0.0, 1.0])
    return np.array([a.mean(), 1.0 / (a.std() + 1e-8)])


def adam_f64(p, g, m, v, t, lr, betas=(0.9, 0.999), eps=1e-5, max_grad_norm=0.0):
    """Step number t (1, 2, ...) of the header's Adam on float64 copies -> (p, m, v); the hyper-parameters as the float32 the device is given."""
    p, g, m, v = _f64(p), _f64(g), _f64(m), _f64(v)
    lr, b1, b2, eps, mx = [float(np.float32(q)) for q in (lr, betas[0], betas[1], eps, max_grad_norm)]
    if mx > 0.0:
        g = g * min(1.0, mx / (np.sqrt((g * g).sum()) + 1e-6))
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    return p - lr * (m / (1.0 - b1 ** t)) / (np.sqrt(v / (1.0 - b2 ** t)) + eps), m, v


def normalised_error(got, want, norm):
    """max |got - want| / norm over the entries with norm > 0; entries with norm == 0 must be exactly `want` (zero)."""
    got, want, norm = _f64(got), _f64(want), _f64(norm)
    assert got.shape == want.shape == norm.shape, (got.shape, want.shape, norm.shape)
    assert np.isfinite(got).all(), "non-finite output"
    dead = norm == 0.0
    assert (got[dead] == want[dead]).all(), "an entry without contributions is not exactly zero"
    if dead.all():
        return 0.0
    return float((np.abs(got - want)[~dead] / norm[~dead]).max())


# ---------------------------------------------------------------------------------------------------------------------
# the kernels' arithmetic in float32
# ---------------------------------------------------------------------------------------------------------------------
LOG2E_F32 = float(np.float32(np.log2(np.e)))


def tanh_dev(x):
    """mlp_tanh as the library's build compiles it: e = exp2(2 x log2 e) with the argument rounded to float32, 2 / (e + 1) as 2 times
    a rounded reciprocal."""
    x = np.clip(_f32(x), np.float32(-pr.CLAMP), np.float32(pr.CLAMP))
    arg = _f32(_f32(np.float32(2.0) * x).astype(np.float64) * LOG2E_F32)
    e = _f32(np.exp2(arg.astype(np.float64)))
    rcp = _f32(1.0 / _f32(e + np.float32(1.0)).astype(np.float64))
    return _f32(np.float32(1.0) - _f32(np.float32(2.0) * rcp))


def _one_minus_sq(h):
    return _f32(1.0 - h.astype(np.float64) ** 2)  # fma(-h, h, 1): one rounding


def _ordered_sum(terms, strides=16):
    """terms [n, k] float32 -> [k]: tiles of 16 rows summed in row order, thread u takes tiles u, u + strides, ... in order, the `strides`
    values of u in order (k_ppo_stats: 16; k_ppo_stats_cat: 8)."""
    n, k = terms.shape
    tiles = (n + 15) // 16
    pad = np.zeros((tiles * 16, k), dtype=np.float32)
    pad[:n] = terms
    ts = np.zeros((tiles, k), dtype=np.float32)
    for q in range(16):
        ts = _f32(ts + pad[q::16])
    red = np.zeros((strides, k), dtype=np.float32)
    for t in range(tiles):
        red[t % strides] = _f32(red[t % strides] + ts[t])
    out = np.zeros(k, dtype=np.float32)
    for u in range(strides):
        out = _f32(out + red[u])
    return out


def _wgrad(a, dz):
    """a^T dz: an fma chain over the rows of each partition of 1024 in row order, the partitions summed in order; float32."""
    out = np.zeros((a.shape[1], dz.shape[1]), dtype=np.float32)
    for r0 in range(0, a.shape[0], PART):
        out = _f32(out + pr._fma_chain(np.ascontiguousarray(a[r0:r0 + PART].T), dz[r0:r0 + PART]))
    return out


# What a head of a network is to the emulation: its live columns; out(h2, w3, b3) -> the head's outputs [n, cols] as its kernel forms them;
# how dH2 = dOut W3^T starts -- from_zero False: dO_0 W3_0 as a PRODUCT, then fma with the columns behind it (ppo_rows_tile); True: fma over
# all columns from zero (k_ppo_rows_cat) -- two recurrences on purpose, they round differently; and the strides of its tile sums.
Head = collections.namedtuple("Head", "cols out from_zero strides")


def gaussian_head(heads, lanes):
    """The vector-ALU head of k_ppo_rows: `heads` dot products of 256 over `lanes` lanes each (the actor: 4 and 4; a critic: 1 and 16)."""
    return Head(heads, lambda h2, w3, b3: _f32(ar._dots(h2, w3[:, :heads], lanes) + b3[:heads]), False, 16)


def _emulate_net(x, net, d_out_fn, head):
    w1, b1, w2, b2, w3, b3 = [_f32(w) for w in net]
    out_cols = w3.shape[1]
    x = _f32(x)
    h1 = tanh_dev(_f32(pr._fma_chain(x, w1) + b1))
    h2 = tanh_dev(_f32(pr._fma_chain(h1, w2) + b2))
    d_out, extra = d_out_fn(head.out(h2, w3, b3))
    acc = np.zeros((x.shape[0], H), dtype=np.float32) if head.from_zero else None
    for k in range(head.cols):
        prod = d_out[:, k, None].astype(np.float64) * w3[None, :, k].astype(np.float64)
        acc = _f32(prod) if acc is None else _f32(acc.astype(np.float64) + prod)
    dz2 = _f32(acc.astype(np.float64) * _one_minus_sq(h2).astype(np.float64))
    dz1 = _f32(pr._fma_chain(dz2, np.ascontiguousarray(w2.T)).astype(np.float64) * _one_minus_sq(h1).astype(np.float64))
    ones = np.ones((x.shape[0], 1), dtype=np.float32)
    dw3 = np.zeros((H, out_cols), dtype=np.float32)
    dw3[:, :head.cols] = _wgrad(d_out, h2).T
    db3 = np.zeros(out_cols, dtype=np.float32)
    db3[:head.cols] = _ordered_sum(d_out, head.strides)
    return [_wgrad(x, dz1), _wgrad(ones, dz1)[0], _wgrad(h1, dz2), _wgrad(ones, dz2)[0], dw3, db3], extra


def emulate_update(x, ret, policy, value, actor, head, critic_head, vf_coef):
    """What emulate_grads of either head is around its row loss `actor(o) -> (dOut [n, cols], the five loss terms [n, 5])`: the actor's
    network, the critic's (value None: none) with its loss, and the statistics.  x: float32 [n, in_dim], n >= 1."""
    n = x.shape[0]
    inv, vf = np.float32(1.0 / n), np.float32(vf_coef)
    pg, t = _emulate_net(x, policy, actor, head)
    stats = np.zeros(8, dtype=np.float32)
    stats[0] = n
    stats[[1, 3, 4, 5, 6]] = _f32(_ordered_sum(t, head.strides) * inv)
    vg = None
    if value is not None:
        def critic(o):
            err = _f32(o[:, 0] - _f32(ret))
            lv = _f32(_f32(np.float32(0.5) * err) * err)
            return _f32(_f32(vf * err) * inv)[:, None], lv[:, None]
        vg, lv = _emulate_net(x, value, critic, critic_head)
        stats[2] = _f32(_ordered_sum(lv, critic_head.strides)[0] * inv)
    return dict(stats=stats, policy=pg, value=vg)


def emulate_grads(x, action, logp_old, adv, ret, policy, value, clip=CLIP, vf_coef=VF_COEF, ent_coef=ENT_COEF, adv_stats=None):
    """loss_and_grads_f64's outputs (stats, policy, value) as the kernels compute them; rows in minibatch order, n >= 1."""
    n = int(np.asarray(x).shape[0])
    in_dim = np.asarray(policy[0]).shape[0]
    x = _f32(np.asarray(x)[:, :in_dim])
    inv = float(np.float32(1.0 / n))
    ce = float(np.float32(ent_coef))

    def actor(o):  # the row loss in double from the fp32 heads
        o64 = o.astype(np.float64)
        A, logp, r, flows, z, e, rc = row_terms_f64(o64[:, :2], o64[:, 2:4], action, logp_old, adv,
                                                    None if adv_stats is None else _f32(adv_stats), clip)
        g = np.where(flows, -A * r * inv, 0.0)
        d = _f32(np.concatenate([g[:, None] * z * e, g[:, None] * (z * z - 1.0) - ce * inv], axis=1))
        t = _f32(np.stack([-np.minimum(r * A, rc * A), _f32(_f32(o[:, 2] + o[:, 3]) + np.float32(LOG_2PIE)), _f64(logp_old) - logp,
                           (~flows).astype(np.float64), r], axis=1))
        return d, t

    return emulate_update(x, ret, policy, value, actor, gaussian_head(4, 4), gaussian_head(1, 16), vf_coef)


def _thread_strided(terms, fma_sq=False, threads=256):
    """sum of terms (float32): thread i takes entries i, i + 256, ... in order (fma_sq: fma(x, x, s)), a butterfly per wave of 64, the four
    waves in order."""
    n = terms.shape[0]
    pad = np.zeros(((n + threads - 1) // threads + 1) * threads, dtype=np.float32)
    pad[:n] = terms
    s = np.zeros(threads, dtype=np.float32)
    for row in pad.reshape(-1, threads):
        r64 = row.astype(np.float64)
        s = _f32(s.astype(np.float64) + (r64 * r64 if fma_sq else r64))
    w = s.reshape(4, 64)
    d = 32
    while d:
        w = _f32(w + w[:, np.arange(64) ^ d])
        d >>= 1
    return np.float32(_f32(_f32(w[0, 0] + w[1, 0]) + w[2, 0]) + w[3, 0])


def emulate_adv_stats(adv):
    a = _f32(adv).reshape(-1)
    n = a.size
    if n == 0:
        return np.array([0.0, 1.0], dtype=np.float32)
    mean = np.float32(float(_thread_strided(a)) / n)
    s2 = _thread_strided(_f32(a - mean), fma_sq=True)
    return np.array([mean, np.float32(1.0 / (np.sqrt(float(s2) / n) + 1e-8))], dtype=np.float32)


def emulate_adam(p, g, m, v, t, lr, betas=(0.9, 0.999), eps=1e-5, max_grad_norm=0.0):
    p, g, m, v = _f32(p), _f32(g), _f32(m), _f32(v)
    lr, b1, b2, eps, mx = [np.float32(q) for q in (lr, betas[0], betas[1], eps, max_grad_norm)]
    scale = np.float32(1.0)
    if mx > 0.0:
        scale = np.float32(min(1.0, float(mx) / (np.sqrt(float(_thread_strided(g, fma_sq=True))) + 1e-6)))
    c1 = np.float32(1.0 / (1.0 - float(b1) ** t))
    c2 = np.float32(1.0 / (1.0 - float(b2) ** t))
    g = _f32(g * scale)
    m = _f32(float(b1) * m.astype(np.float64) + _f32(np.float32(1.0 - b1) * g).astype(np.float64))
    v = _f32(float(b2) * v.astype(np.float64) + _f32(_f32(np.float32(1.0 - b2) * g) * g).astype(np.float64))
    step = float(lr) * (m.astype(np.float64) * float(c1)) / (np.sqrt(v.astype(np.float64) * float(c2)) + float(eps))
    return _f32(p.astype(np.float64) - step), m, v


# ---------------------------------------------------------------------------------------------------------------------
# cases of pgd_ppo_grad
# ---------------------------------------------------------------------------------------------------------------------
WIDTHS = (4, 5, 35, 274, 275, 416)
ROW_COUNTS = (1, 15, 16, 17, 33, 1027)   # 1027: one past a multiple of 16 and 64, and beyond the partition of 1024 rows
OUT_COLS = (4, 5, 6)
SWEEP_ROWS = 33
ROW_WIDTH = 274
ADV_STATS = (0.15, 1.3)   # the (mean, 1 / std) handed to the kernel in the cases that normalise
BRANCHES = ("cut_pos", "cut_neg", "in_pos", "in_neg")   # A > 0 with r > 1 + clip; A < 0 with r < 1 - clip; both signs inside the band


def build_case(name, in_dim, rows, scaling="unit", out_cols=4, seed=0, normalise=False):
    """The rows of one minibatch, in order: dict(x [rows, stride] float32 with NaN padding, action, logp_old, adv, ret, policy, value,
    adv_stats, branch [rows]).  Row i belongs to branch i % 4 by CONSTRUCTION: logp_old = logp_f64 - log(r) with r drawn at least 0.02
    inside or outside the band, |A| in [0.1, 2] -- no row sits within 1e-3 of a discontinuity of the gradient."""
    rng = np.random.default_rng([zlib.crc32(name.encode()), in_dim, rows, pr.SCALINGS.index(scaling), out_cols, seed])
    x = pr.make_inputs(rng, rows, in_dim, scaling)
    p, v = ar.make_networks(rng, in_dim, out_cols)
    mean, ls, val = ar.heads_f64(x[:, :in_dim], p, v)
    z = np.clip(rng.normal(0, 1, size=(rows, 2)), -3, 3)
    action = (mean + np.exp(ls) * z).astype(np.float32)
    zz = (action.astype(np.float64) - mean) * np.exp(-ls)
    logp = -0.5 * (zz ** 2).sum(axis=1) - ls.sum(axis=1) - LOG_2PI
    branch = np.arange(rows) % 4
    u = rng.uniform(size=rows)
    r = np.select([branch == 0, branch == 1], [1.0 + CLIP + 0.05 + 0.45 * u, 1.0 - CLIP - 0.05 - 0.45 * u], 1.0 - CLIP + 0.02 + (2 * CLIP - 0.04) * u)
    A = rng.uniform(0.1, 2.0, size=rows) * np.where((branch == 0) | (branch == 2), 1.0, -1.0)
    s = ADV_STATS if normalise else None
    adv = (A / s[1] + s[0] if normalise else A).astype(np.float32)
    ret = (val + rng.normal(0, 1, size=rows)).astype(np.float32)
    return dict(x=x, action=action, logp_old=(logp - np.log(r)).astype(np.float32), adv=adv, ret=ret, policy=p, value=v,
                adv_stats=None if s is None else np.array(s, dtype=np.float32), branch=branch, in_dim=in_dim)


def sweep_cases():
    for i, k in enumerate(WIDTHS):
        for j, sc in enumerate(("unit", "normalised")):
            yield dict(name="sweep", in_dim=k, rows=SWEEP_ROWS, scaling=sc, out_cols=OUT_COLS[(i + j) % 3], seed=i, normalise=bool((i + j) % 2))


def row_cases():
    for i, n in enumerate(ROW_COUNTS):
        yield dict(name="rows", in_dim=ROW_WIDTH, rows=n, scaling=("unit", "normalised")[i % 2], out_cols=OUT_COLS[i % 3], seed=n, normalise=bool(i % 2))


def grad_cases():
    for gen in (sweep_cases, row_cases):
        for c in gen():
            yield c


# the list forms: one case, its first `count` rows listed, split into n_mb strided minibatches (n_mb 1: the whole list); count 5 with
# n_mb 7 has minibatches of one row and empty ones
LIST_CASE = dict(name="list", in_dim=35, rows=100, scaling="normalised", out_cols=5, seed=4, normalise=True)
LIST_COUNTS = (100, 5)
LIST_MB = (3, 7)
NOCRITIC_CASE = dict(name="nocritic", in_dim=275, rows=40, scaling="unit", out_cols=6, seed=7, normalise=False)


PART_CASE = dict(name="parts", in_dim=35, rows=2049, scaling="unit", out_cols=4, seed=8, normalise=True)   # three partitions of 1024 rows
SPLIT_CASE = dict(name="rows", in_dim=ROW_WIDTH, rows=1027, scaling="normalised", out_cols=OUT_COLS[5 % 3], seed=1027, normalise=True)  # row_cases()' last
SPLIT_MB = 2   # its two strided halves (514 and 513 rows: no partition boundary inside) against the whole (one inside)


def list_subsets():
    """(count, n_mb, j, the rows of LIST_CASE in minibatch j) of every comparison of the list-form test."""
    for count in LIST_COUNTS:
        yield count, 1, 0, np.arange(count)
        for n_mb in LIST_MB:
            for j in range(n_mb):
                yield count, n_mb, j, np.arange(j, count, n_mb)


def subset_case(case, sel):
    """The rows `sel` of a case of either head: every per-row array it has (`action` the Gaussian's, `index` the categorical's)."""
    out = dict(case)
    for key in ("x", "action", "index", "logp_old", "adv", "ret", "branch"):
        if key in case:
            out[key] = case[key][sel]
    return out


def reference_of(case, critic=True):
    k = case["in_dim"]
    return loss_and_grads_f64(case["x"][:, :k], case["action"], case["logp_old"], case["adv"], case["ret"], case["policy"],
                              case["value"] if critic else None, adv_stats=case["adv_stats"])


def emulation_of(case, critic=True):
    k = case["in_dim"]
    return emulate_grads(case["x"][:, :k], case["action"], case["logp_old"], case["adv"], case["ret"], case["policy"],
                         case["value"] if critic else None, adv_stats=case["adv_stats"])


def compared_cases():
    """(label, case arrays, float64 reference) of EVERY comparison of tests/test_ppo_update_gpu.py that uses the recorded tolerances: the width
    sweep, the row counts, the list forms, the case without a critic, the three-partition case and the split of the 1027-row case.  What the tolerances are measured over."""
    for c in grad_cases():
        case, ref = case_and_reference(c)
        yield str(c), case, ref, True
    full, _ = case_and_reference(LIST_CASE)
    for count, n_mb, j, sel in list_subsets():
        if len(sel):
            sub = subset_case(full, sel)
            yield "list: count %d, minibatch %d of %d" % (count, j, n_mb), sub, reference_of(sub), True
    case, _ = case_and_reference(NOCRITIC_CASE)
    yield "no critic", case, reference_of(case, critic=False), False
    case, ref = case_and_reference(PART_CASE)
    yield str(PART_CASE), case, ref, True
    full, _ = case_and_reference(SPLIT_CASE)
    for j in range(SPLIT_MB):
        sub = subset_case(full, np.arange(j, SPLIT_CASE["rows"], SPLIT_MB))
        yield "split: minibatch %d of %d of the 1027 rows" % (j, SPLIT_MB), sub, reference_of(sub), True


def _key(c):
    return tuple(sorted(c.items()))


@functools.lru_cache(maxsize=None)
def _case_and_reference(key):
    c = build_case(**dict(key))
    k = c["in_dim"]
    return c, loss_and_grads_f64(c["x"][:, :k], c["action"], c["logp_old"], c["adv"], c["ret"], c["policy"], c["value"], adv_stats=c["adv_stats"])


def case_and_reference(c):
    """(the case's arrays, its float64 reference), computed once and shared; neither is modified by its users."""
    return _case_and_reference(_key(c))


def grad_errors(got, ref):
    """(largest normalised gradient error, largest normalised statistics error) of outputs `got` (dict: stats, policy, value) against `ref`."""
    eg = 0.0
    for net in ("policy", "value"):
        if ref[net] is None:
            continue
        for g, w, nrm in zip(got[net], ref[net], ref[net + "_norm"]):
            eg = max(eg, normalised_error(np.asarray(g).reshape(np.shape(w)), w, nrm))
    assert float(got["stats"][0]) == ref["stats"][0] and float(got["stats"][7]) == 0.0
    es = normalised_error(np.asarray(got["stats"])[1:7], ref["stats"][1:7], ref["stat_norm"][1:7])
    return eg, es


def stat_errors(got, ref):
    """The normalised error of each statistics slot 1 .. 6 (what grad_errors takes the maximum of), for a test's printout."""
    norm = np.where(ref["stat_norm"][1:7] > 0, ref["stat_norm"][1:7], 1.0)
    return np.abs(_f64(got["stats"])[1:7] - ref["stats"][1:7]) / norm


def closed_loop_case():
    return dict(name="closed", in_dim=35, rows=64, scaling="unit", out_cols=4, seed=1, normalise=False)


# ---------------------------------------------------------------------------------------------------------------------
# cases of pgd_adv_stats and pgd_adam
# ---------------------------------------------------------------------------------------------------------------------
ADV_COUNTS = (0, 1, 2, 63, 64, 65, 4099)


def build_adv(count, with_index):
    """(adv [n_rows] float32 with NaN in every unlisted row, index [n_list] int32 or None, n_list): advantages N(0.3, 1.5)."""
    rng = np.random.default_rng([count, int(with_index)])
    n_list = count + 7
    if not with_index:
        adv = np.full(n_list, np.nan, dtype=np.float32)
        adv[:count] = rng.normal(0.3, 1.5, size=count)
        return adv, None, n_list
    n_rows = 2 * count + 11
    index = rng.permutation(n_rows)[:n_list].astype(np.int32)
    adv = np.full(n_rows, np.nan, dtype=np.float32)
    adv[index[:count]] = rng.normal(0.3, 1.5, size=count)
    return adv, index, n_list


ADAM_SIZES = (1, 63, 64, 65, 1027, 140000)
ADAM_NORMS = ("below", "above", "off")   # |g| = max_grad_norm / 10, 10 max_grad_norm (never within 1 % of the threshold), no clipping
ADAM_MAX_NORM = 0.5
ADAM_HYPER = dict(lr=3e-4, betas=(0.9, 0.999), eps=1e-5)


def adam_cases():
    for n in ADAM_SIZES:
        for mode in ADAM_NORMS:
            yield dict(n_elem=n, mode=mode)


def build_adam(n_elem, mode):
    """(p [n], three gradients [3, n], max_grad_norm): p N(0, 0.1); each gradient scaled to the norm its mode names."""
    rng = np.random.default_rng([n_elem, ADAM_NORMS.index(mode)])
    p = rng.normal(0, 0.1, size=n_elem).astype(np.float32)
    g = rng.normal(0, 1, size=(3, n_elem))
    target = dict(below=ADAM_MAX_NORM / 10.0, above=ADAM_MAX_NORM * 10.0, off=1.0)[mode]
    g = (g / np.sqrt((g * g).sum(axis=1, keepdims=True)) * target).astype(np.float32)
    return p, g, (0.0 if mode == "off" else ADAM_MAX_NORM)


def adam_errors(run):
    """`run(p, g, m, v, t, max_norm) -> (p, m, v)` applied three times against adam_f64 from the same float32 state: the largest
    normalised error of p, m, v over adam_cases().  The reference restarts from the run's own float32 state at every step, so a step's
    error is not carried into the next comparison."""
    worst = 0.0
    for c in adam_cases():
        p, g, mx = build_adam(**c)
        m, v = np.zeros_like(p), np.zeros_like(p)
        b1, b2 = [float(np.float32(b)) for b in ADAM_HYPER["betas"]]
        for t in (1, 2, 3):
            p64, m64, v64 = adam_f64(p, g[t - 1], m, v, t, max_grad_norm=mx, **ADAM_HYPER)
            gs = _f64(g[t - 1]) * (min(1.0, float(np.float32(mx)) / (np.sqrt((_f64(g[t - 1]) ** 2).sum()) + 1e-6)) if mx > 0 else 1.0)
            nm = b1 * np.abs(_f64(m)) + (1 - b1) * np.abs(gs)
            nv = b2 * np.abs(_f64(v)) + (1 - b2) * gs * gs
            npar = np.abs(_f64(p)) + np.abs(p64 - _f64(p))
            p, m, v = run(p, g[t - 1], m, v, t, mx)
            worst = max(worst, normalised_error(p, p64, npar), normalised_error(m, m64, nm), normalised_error(v, v64, nv))
    return worst
