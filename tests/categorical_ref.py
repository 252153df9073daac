"""The checker of pgdrive_amd/csrc/pgd_categorical.h (pgd_mlp_actor_critic_cat, _cat_rows, pgd_ppo_grad_cat), in plain numpy, after the
protocol of tests/ppo_ref.py:

* forward_f64 / loss_and_grads_f64
                     the formulas of include/pgdrive_hip.h in float64 -- two independent categorical heads over the 256-256 tanh network,
                     the sampling from the same u (tests/actor_critic_ref.units: the kernel's two draws), the backward pass by hand
                     (tests/test_categorical_cpu.py holds it against torch.distributions.Categorical and autograd);
* emulate_forward / emulate_grads
                     the kernels' ARITHMETIC and summation orders in float32 (the logit tile: four k-ordered fma chains of 64, ((P0 + P1) +
                     P2) + P3 + b3; softmax, the running sum of the probabilities in index order; the row loss in double from the fp32
                     logits; dOut W3^T as an fma chain over the columns; weight gradients and tile sums as ppo_ref's, the tile sums
                     8-strided).  Never compared with the device: it exists to MEASURE the tolerances;
* the seeded cases of tests/test_categorical_gpu.py.

Tolerances: each TOL_*_MEASURED is the largest normalised error of the emulation against float64 over exactly the GPU module's cases
(forward_cases() / compared_grad_cases()); the tolerance is twice that; the CPU test measures again and holds the emulation below half of
the tolerance.  Gradient and statistic errors are normalised as in ppo_ref (the float64 sum of the absolute contributions of an entry), per
row class few / tile / part.  logp is normalised by 1 + |l_s[i_s]| + |lse_s| + |l_t[i_t]| + |lse_t|, the sizes of the four numbers it is
the combination of.

Near-ties.  The device's index may differ from the float64 reference's only where the reference itself says that fp32 cannot decide:
  sampling  index = #{j < K_head - 1 : c_j <= u}, c_j = p_0 + ... + p_j.  The device's c_j differs from the float64 c_j by at most
            sum_{i <= j} p_i (|dl_i| + |dlse|)      the logits' own error dl (TOL_LOGIT: the bound pgd_mlp_policy's head outputs are
                                                    held to, policy_ref.TOL_EXACT) through softmax; lse is 1-Lipschitz in max |dl|
                                                    -> at most 2 TOL_LOGIT c_j <= 2 TOL_LOGIT
            + K roundings of the partial sums, each at most EPS / 2 of a number <= 1 (+ its own error)  -> K EPS
            + per p_i: expf (2 ulp), the rounding of its argument l_i - lse (|logp_i| EPS / 2, and p |log p| <= 0.37) and of lse
              (|lse| EPS, |lse| <= 8 for the cases' logits)  -> at most 16 EPS over a head
            MARGIN(K) = 2 TOL_LOGIT + (K + 16) EPS.  A device index i' != i is admitted iff |u - c_j| <= MARGIN for EVERY boundary j
            between the two (j = min(i, i') .. max(i, i') - 1).
  argmax    the device may pick i' != i iff l[i] - l[i'] <= 2 TOL_LOGIT (each logit moves by at most TOL_LOGIT).
Such rows are left out of the logp comparison as well, and a case may have at most NEAR_TIE_CAP = 1 % of its rows NEAR a tie in the
reference (near_tie_rows: any boundary of a row within MARGIN, or its top two logits within 2 TOL_LOGIT); the CPU test asserts that with
the reference alone for every seeded case.
"""
import functools
import zlib

import numpy as np

from tests import actor_critic_ref as ar
from tests import policy_ref as pr
from tests import ppo_ref as pp

H = pr.H
EPS = 2.0 ** -23
CAT_COLS = 16
TOL_LOGIT = pr.TOL_EXACT
ARGMAX_GAP = 2.0 * TOL_LOGIT
NEAR_TIE_CAP = 0.01
CLIP, VF_COEF, ENT_COEF = pp.CLIP, pp.VF_COEF, pp.ENT_COEF
LOGIT_SCALE = 3.0   # the head's weights of make_networks are policy_ref's times this: logits of standard deviation about 1.5

# logp of the forward launch: the largest normalised error of emulate_forward against forward_f64 over forward_cases()
TOL_CAT_LOGP_MEASURED = 2.329e-7
TOL_CAT_LOGP = 2.0 * TOL_CAT_LOGP_MEASURED
# gradients and statistics of pgd_ppo_grad_cat: the largest normalised error of emulate_grads against loss_and_grads_f64 over
# compared_grad_cases(), per row class (ppo_ref.ROW_CLASSES)
TOL_GRAD_MEASURED = dict(few=3.229e-7, tile=1.090e-7, part=3.335e-8)
TOL_STAT_MEASURED = dict(few=9.387e-8, tile=8.562e-8, part=4.109e-8)

_f32 = pr._f32
_f64 = pp._f64


def margin(K):
    return 2.0 * TOL_LOGIT + (K + 16) * EPS


def tolerances(n):
    """(TOL_GRAD, TOL_STAT) of a minibatch of n live rows: twice the measured figures of its row class."""
    c = pp.row_class(n)
    return 2.0 * TOL_GRAD_MEASURED[c], 2.0 * TOL_STAT_MEASURED[c]


def grid_value(index, K):
    """(float) i * (2.0f / (float) (K - 1)) - 1.0f: one fp32 multiplication, one fp32 subtraction, the quotient correctly rounded."""
    return _f32(_f32(_f32(index) * np.float32(2.0 / (K - 1))) - np.float32(1.0))


# ---------------------------------------------------------------------------------------------------------------------
# float64
# ---------------------------------------------------------------------------------------------------------------------
def head_f64(l):
    """logits [n, K_head] -> (logp_j [n, K_head], p_j, H_head [n], lse [n])."""
    m = l.max(axis=1, keepdims=True)
    lse = m + np.log(np.exp(l - m).sum(axis=1, keepdims=True))
    logp = l - lse
    p = np.exp(logp)
    return logp, p, -(p * logp).sum(axis=1), lse[:, 0]


def logits_f64(x, policy, bins):
    K = sum(bins)
    in_dim = np.asarray(policy[0]).shape[0]
    h1, h2 = pp._forward_f64(np.asarray(x)[:, :in_dim], policy)
    return h1, h2, h2 @ _f64(policy[4])[:, :K] + _f64(policy[5])[:K]


def forward_f64(x, policy, value, bins, u=None):
    """The forward launch in float64: u [n, 2] the two draws of every row (None: PGD_AC_DETERMINISTIC) -> dict(logits [n, K], index [n, 2],
    logp [n], value [n] or None, norm [n] (what a logp error is normalised by), cum (per head: c_j [n, K_head - 1]), u)."""
    ks, kt = bins
    _, _, l = logits_f64(x, policy, bins)
    n = l.shape[0]
    index = np.zeros((n, 2), dtype=np.int64)
    logp, norm, cum = np.zeros(n), np.ones(n), []
    for hd, lh in enumerate((l[:, :ks], l[:, ks:ks + kt])):
        lp, p, _, lse = head_f64(lh)
        c = np.cumsum(p, axis=1)[:, :-1]
        cum.append(c)
        i = lh.argmax(axis=1) if u is None else (c <= _f64(u)[:, hd, None]).sum(axis=1)
        index[:, hd] = i
        logp += lp[np.arange(n), i]
        norm += np.abs(lh[np.arange(n), i]) + np.abs(lse)
    v = None
    if value is not None:
        in_dim = np.asarray(value[0]).shape[0]
        v = (ar._hidden_f64(np.asarray(x)[:, :in_dim], value) @ _f64(value[4])[:, :1] + _f64(value[5])[:1])[:, 0]
    return dict(logits=l, index=index, logp=logp, value=v, norm=norm, cum=cum, u=None if u is None else _f64(u), bins=bins)


def near_tie_rows(ref):
    """[n] bool: the rows of a float64 forward result at which fp32 may decide otherwise (the module's docstring)."""
    ks, kt = ref["bins"]
    l, near = ref["logits"], np.zeros(ref["logits"].shape[0], dtype=bool)
    for hd, lh in enumerate((l[:, :ks], l[:, ks:ks + kt])):
        if ref["u"] is None:
            top = np.sort(lh, axis=1)
            near |= (top[:, -1] - top[:, -2]) <= ARGMAX_GAP
        else:
            near |= (np.abs(ref["cum"][hd] - ref["u"][:, hd, None]) <= margin(ks + kt)).any(axis=1)
    return near


def admitted_differences(ref, got_index):
    """[n] bool: the rows at which `got_index` [n, 2] differs from the reference's; every one of them must be an admitted near-tie
    (AssertionError otherwise)."""
    ks, kt = ref["bins"]
    got = np.asarray(got_index).astype(np.int64)
    assert got.shape == ref["index"].shape
    assert (got >= 0).all() and (got[:, 0] < ks).all() and (got[:, 1] < kt).all(), "an index outside its head"
    l = ref["logits"]
    differs = np.zeros(l.shape[0], dtype=bool)
    for hd, lh in enumerate((l[:, :ks], l[:, ks:ks + kt])):
        for r in np.flatnonzero(got[:, hd] != ref["index"][:, hd]):
            i, j = int(ref["index"][r, hd]), int(got[r, hd])
            if ref["u"] is None:
                ok = lh[r, i] - lh[r, j] <= ARGMAX_GAP
            else:
                ok = (np.abs(ref["cum"][hd][r, min(i, j):max(i, j)] - ref["u"][r, hd]) <= margin(ks + kt)).all()
            assert ok, "row %d, head %d: index %d, the reference says %d, and no near-tie lies between them" % (r, hd, j, i)
            differs[r] = True
    return differs


def row_terms_f64(l, index, logp_old, adv, adv_stats, clip, bins):
    """Per live row from the logits l [n, K] (float64): (A, logp, r, flows, rc, logp_j [n, K], p_j [n, K], H_head [n, K] (a row's H of the
    head column j belongs to), onehot [n, K], H [n])."""
    ks, kt = bins
    n = l.shape[0]
    index = np.asarray(index).astype(np.int64)
    lpj, pj, hh, onehot = np.zeros_like(l), np.zeros_like(l), np.zeros_like(l), np.zeros_like(l)
    logp, Htot = np.zeros(n), np.zeros(n)
    for hd, (a, b) in enumerate(((0, ks), (ks, ks + kt))):
        lp, p, Hh, _ = head_f64(l[:, a:b])
        i = np.clip(index[:, hd], 0, b - a - 1)
        lpj[:, a:b], pj[:, a:b], hh[:, a:b] = lp, p, Hh[:, None]
        onehot[np.arange(n), a + i] = 1.0
        logp += lp[np.arange(n), i]
        Htot += Hh
    A = _f64(adv)
    if adv_stats is not None:
        A = (A - float(adv_stats[0])) * float(adv_stats[1])
    r = np.exp(logp - _f64(logp_old))
    c = float(np.float32(clip))
    rc = np.clip(r, 1.0 - c, 1.0 + c)
    return A, logp, r, (r * A <= rc * A), rc, lpj, pj, hh, onehot, Htot


def loss_and_grads_f64(x, index, logp_old, adv, ret, policy, value, bins, clip=CLIP, vf_coef=VF_COEF, ent_coef=ENT_COEF, adv_stats=None):
    """ppo_ref.loss_and_grads_f64 with the categorical head: the live rows of one minibatch in (x [n, in_dim], index [n, 2], logp_old, adv,
    ret [n]) -> dict(stats [8], loss, policy / value: six gradients each, policy_norm / value_norm, stat_norm [8])."""
    n = int(np.asarray(x).shape[0])
    in_dim = np.asarray(policy[0]).shape[0]
    out_cols = np.asarray(policy[4]).shape[1]
    K = sum(bins)
    vf, ce = float(np.float32(vf_coef)), float(np.float32(ent_coef))
    zero = lambda oc: [np.zeros((in_dim, H)), np.zeros(H), np.zeros((H, H)), np.zeros(H), np.zeros((H, oc)), np.zeros(oc)]  # noqa: E731
    if n == 0:
        return dict(stats=np.zeros(8), stat_norm=np.zeros(8), loss=0.0, policy=zero(out_cols), policy_norm=zero(out_cols),
                    value=None if value is None else zero(1), value_norm=None if value is None else zero(1))
    x = _f64(np.asarray(x)[:, :in_dim])
    h1, h2, l = logits_f64(x, policy, bins)
    A, logp, r, flows, rc, lpj, pj, hh, onehot, Htot = row_terms_f64(l, index, logp_old, adv, adv_stats, clip, bins)
    g = np.where(flows, -A * r / n, 0.0)
    d_out = g[:, None] * (onehot - pj) + (ce / n) * pj * (lpj + hh)
    # dOut's own terms: dL/dlogp carries exp(logp - logp_old), whose error is r times that of a difference of two numbers of logp's size
    cond = 1.0 + np.abs(logp) + np.abs(_f64(logp_old))
    n_out = (np.abs(g) * cond)[:, None] * (onehot + pj) + (ce / n) * pj * (np.abs(lpj) + hh)
    pg, pn = pp._backward_f64(x, h1, h2, d_out, n_out, policy, K)
    terms = [np.full(n, float(n)), -np.minimum(r * A, rc * A), np.zeros(n), Htot, _f64(logp_old) - logp, (~flows).astype(np.float64), r, np.zeros(n)]
    term_norms = [None, np.abs(terms[1]) * cond, None, 2.0 * Htot, np.abs(logp) + np.abs(_f64(logp_old)), None, r * cond, None]
    vg = vn = None
    if value is not None:
        vh1, vh2 = pp._forward_f64(x, value)
        v = (vh2 @ _f64(value[4])[:, :1] + _f64(value[5])[:1])[:, 0]
        err = v - _f64(ret)
        terms[2] = 0.5 * err * err
        term_norms[2] = 0.5 * (np.abs(v) + np.abs(_f64(ret))) ** 2
        vg, vn = pp._backward_f64(x, vh1, vh2, (vf * err / n)[:, None], (vf * (np.abs(v) + np.abs(_f64(ret))) / n)[:, None], value, 1)
    stats = np.array([t.sum() / n for t in terms])
    stat_norm = np.array([np.abs(t if q is None else q).sum() / n for t, q in zip(terms, term_norms)])
    stats[0], stat_norm[0] = n, n
    loss = stats[1] + vf * stats[2] - ce * stats[3]
    return dict(stats=stats, stat_norm=stat_norm, loss=float(loss), policy=pg, policy_norm=pn, value=vg, value_norm=vn)


# ---------------------------------------------------------------------------------------------------------------------
# the kernels' arithmetic in float32
# ---------------------------------------------------------------------------------------------------------------------
def _hidden_dev(x, net):
    w1, b1, w2, b2 = [_f32(w) for w in net[:4]]
    h1 = pp.tanh_dev(_f32(pr._fma_chain(_f32(x), w1) + b1))
    return h1, pp.tanh_dev(_f32(pr._fma_chain(h1, w2) + b2))


def emulate_logits(h2, w3, b3, K):
    """The logit tile: wave w's fma chain over k = 64 w .. 64 w + 63 from zero, ((P0 + P1) + P2) + P3 + b3."""
    w3 = _f32(w3)[:, :K]
    P = [pr._fma_chain(np.ascontiguousarray(h2[:, 64 * w:64 * w + 64]), np.ascontiguousarray(w3[64 * w:64 * w + 64])) for w in range(4)]
    return _f32(_f32(_f32(_f32(P[0] + P[1]) + P[2]) + P[3]) + _f32(b3)[:K])


def emulate_forward(x, policy, bins, u=None):
    """(index [n, 2], logp [n] float32) as k_mlp_actor_critic_cat computes them."""
    ks, kt = bins
    in_dim = np.asarray(policy[0]).shape[0]
    _, h2 = _hidden_dev(np.asarray(x)[:, :in_dim], policy)
    l = emulate_logits(h2, policy[4], policy[5], ks + kt)
    n = l.shape[0]
    index, logp = np.zeros((n, 2), dtype=np.int64), []
    for hd, lh in enumerate((l[:, :ks], l[:, ks:ks + kt])):
        m = lh.max(axis=1, keepdims=True)
        e = _f32(np.exp(_f32(lh - m).astype(np.float64)))
        s = np.zeros(n, dtype=np.float32)
        for j in range(lh.shape[1]):
            s = _f32(s + e[:, j])
        lse = _f32(m[:, 0] + _f32(np.log(s.astype(np.float64))))
        lp = _f32(lh - lse[:, None])
        p = _f32(np.exp(lp.astype(np.float64)))
        if u is None:
            i = lh.argmax(axis=1)
        else:
            c, i = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.int64)
            for j in range(lh.shape[1] - 1):
                c = _f32(c + p[:, j])
                i += c <= _f32(u)[:, hd]
        index[:, hd] = i
        logp.append(lp[np.arange(n), i])
    return index, _f32(logp[0] + logp[1])


def cat_head(K):
    """The head of k_ppo_rows_cat for the emulation (ppo_ref.Head): K logits off the matrix cores, dOut W3^T as fma from zero over the K
    columns, the tile sums 8-strided."""
    return pp.Head(K, lambda h2, w3, b3: emulate_logits(h2, w3, b3, K), True, 8)


# its critic: k_ppo_rows' dot product on sixteen lanes; one column from zero, 8-strided sums
CRITIC_HEAD = pp.gaussian_head(1, 16)._replace(from_zero=True, strides=8)


def emulate_grads(x, index, logp_old, adv, ret, policy, value, bins, clip=CLIP, vf_coef=VF_COEF, ent_coef=ENT_COEF, adv_stats=None):
    """loss_and_grads_f64's outputs (stats, policy, value) as the kernels compute them; rows in minibatch order, n >= 1."""
    n = int(np.asarray(x).shape[0])
    in_dim = np.asarray(policy[0]).shape[0]
    x = _f32(np.asarray(x)[:, :in_dim])
    inv = float(np.float32(1.0 / n))
    ce = float(np.float32(ent_coef))

    def actor(o):  # the row loss in double from the fp32 logits, rounded once
        A, logp, r, flows, rc, lpj, pj, hh, onehot, Htot = row_terms_f64(o.astype(np.float64), index, logp_old, adv,
                                                                         None if adv_stats is None else _f32(adv_stats), clip, bins)
        g = np.where(flows, -A * r * inv, 0.0)
        d = _f32(g[:, None] * (onehot - pj) + (ce * inv) * (pj * (lpj + hh)))
        t = _f32(np.stack([-np.minimum(r * A, rc * A), Htot, _f64(logp_old) - logp, (~flows).astype(np.float64), r], axis=1))
        return d, t

    return pp.emulate_update(x, ret, policy, value, actor, cat_head(sum(bins)), CRITIC_HEAD, vf_coef)


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
def make_networks(rng, in_dim, out_cols, K):
    """(policy, value): policy_ref.make_weights with a head of out_cols columns -- logits in columns 0 .. K - 1 (times LOGIT_SCALE), NaN
    beyond (never read) -- and a value network with a head of one column."""
    p = pr.make_weights(rng, in_dim, 1.0, out_cols, nan_unused=False)
    p[4][:, :K] *= np.float32(LOGIT_SCALE)
    p[4][:, K:] = np.nan
    p[5][K:] = np.nan
    return p, pr.make_weights(rng, in_dim, 1.0, 1, nan_unused=False)


# the forward launch: rows {1, 15, 16, 17, 33} x in_dim {4, 19, 274, 416} x bins {(2, 2), (5, 5), (3, 13), (8, 8)} x out_cols {K, 16, 19},
# a handful of combinations; `seed` and `tick` are also the noise's
FORWARD_CASES = (
    dict(rows=1, in_dim=4, bins=(2, 2), out_cols=4, scaling="unit", seed=1, tick=0),
    dict(rows=15, in_dim=19, bins=(5, 5), out_cols=16, scaling="normalised", seed=2, tick=3),
    dict(rows=16, in_dim=274, bins=(3, 13), out_cols=16, scaling="unit", seed=3, tick=1),
    dict(rows=17, in_dim=416, bins=(8, 8), out_cols=19, scaling="unit", seed=4, tick=2 ** 31),
    dict(rows=33, in_dim=274, bins=(5, 5), out_cols=10, scaling="normalised", seed=5, tick=7),
    dict(rows=33, in_dim=19, bins=(2, 2), out_cols=19, scaling="unit", seed=6, tick=0xfffffff0),
)


def _key(c):
    return tuple(sorted(c.items()))


@functools.lru_cache(maxsize=None)
def _forward_case(key):
    c = dict(key)
    rng = np.random.default_rng([zlib.crc32(b"cat_forward"), c["in_dim"], c["rows"], sum(c["bins"]), c["out_cols"], c["seed"]])
    x = pr.make_inputs(rng, c["rows"], c["in_dim"], c["scaling"])
    p, v = make_networks(rng, c["in_dim"], c["out_cols"], sum(c["bins"]))
    u = np.stack(ar.units(c["seed"], np.arange(c["rows"]), c["tick"]), axis=1)
    return dict(x=x, policy=p, value=v, u=u, sampled=forward_f64(x, p, v, c["bins"], u), argmax=forward_f64(x, p, v, c["bins"], None))


def forward_case(c):
    """dict(x [rows, stride] with NaN padding, policy, value, u [rows, 2] (the draws of rows 0 .. rows - 1: env_base 0), sampled / argmax:
    the float64 references), computed once and shared; not modified by its users."""
    return _forward_case(_key(c))


def logp_error(got_logp, ref, skip):
    """The largest normalised logp error over the rows that are not in `skip`."""
    keep = ~np.asarray(skip)
    if not keep.any():
        return 0.0
    got = _f64(got_logp)
    assert np.isfinite(got).all()
    return float((np.abs(got - ref["logp"]) / ref["norm"])[keep].max())


BRANCHES = pp.BRANCHES
ADV_STATS = pp.ADV_STATS
# pgd_ppo_grad_cat: live rows {1, 16, 17, 1025} (1025 crosses PPO_PART), out_cols = K and > K
GRAD_CASES = (
    dict(rows=1, in_dim=19, bins=(2, 2), out_cols=4, scaling="unit", seed=1, normalise=False),
    dict(rows=16, in_dim=274, bins=(5, 5), out_cols=10, scaling="normalised", seed=2, normalise=True),
    dict(rows=17, in_dim=416, bins=(3, 13), out_cols=19, scaling="unit", seed=3, normalise=False),
    dict(rows=1025, in_dim=35, bins=(8, 8), out_cols=16, scaling="unit", seed=4, normalise=True),
)
# a sweep of the four widths and the four bin pairs at 33 rows (three tiles, the last with one row) and one more case of each other
# class: a class's figure is the MAXIMUM of the emulation's error over its cases, and the maximum of two or three samples says little about
# the spread of a quantity that is a few roundings of fp32 in size (ppo_ref measures every class over a dozen cases and more)
SWEEP_CASES = tuple(dict(rows=33, in_dim=k, bins=b, out_cols=sum(b) + 3 * (i % 2), scaling=("unit", "normalised")[i % 2], seed=10 + i, normalise=bool(i % 2))
                    for i, (k, b) in enumerate(((4, (2, 2)), (19, (5, 5)), (274, (3, 13)), (416, (8, 8)), (274, (8, 8)), (19, (3, 13)))))
MORE_CASES = (dict(rows=15, in_dim=274, bins=(5, 5), out_cols=16, scaling="unit", seed=20, normalise=True),
              dict(rows=7, in_dim=416, bins=(3, 13), out_cols=16, scaling="normalised", seed=21, normalise=False),
              dict(rows=1040, in_dim=19, bins=(5, 5), out_cols=10, scaling="normalised", seed=22, normalise=False))
NOCRITIC_CASE = dict(rows=17, in_dim=35, bins=(5, 5), out_cols=12, scaling="normalised", seed=5, normalise=False)
LIST_CASE = dict(rows=40, in_dim=35, bins=(5, 5), out_cols=16, scaling="normalised", seed=6, normalise=True)
LIST_COUNT, LIST_MB = 37, 3   # its first 37 rows listed, in three strided minibatches


@functools.lru_cache(maxsize=None)
def _grad_case(key):
    c = dict(key)
    rows, in_dim, bins = c["rows"], c["in_dim"], c["bins"]
    rng = np.random.default_rng([zlib.crc32(b"cat_grad"), in_dim, rows, sum(bins), c["out_cols"], c["seed"]])
    x = pr.make_inputs(rng, rows, in_dim, c["scaling"])
    p, v = make_networks(rng, in_dim, c["out_cols"], sum(bins))
    index = np.stack([rng.integers(0, bins[0], size=rows), rng.integers(0, bins[1], size=rows)], axis=1).astype(np.int32)
    _, _, l = logits_f64(x, p, bins)
    logp = row_terms_f64(l, index, np.zeros(rows), np.zeros(rows), None, CLIP, bins)[1]
    val = (ar._hidden_f64(x[:, :in_dim], v) @ _f64(v[4])[:, :1] + _f64(v[5])[:1])[:, 0]
    branch = np.arange(rows) % 4
    uu = rng.uniform(size=rows)
    r = np.select([branch == 0, branch == 1], [1.0 + CLIP + 0.05 + 0.45 * uu, 1.0 - CLIP - 0.05 - 0.45 * uu], 1.0 - CLIP + 0.02 + (2 * CLIP - 0.04) * uu)
    A = rng.uniform(0.1, 2.0, size=rows) * np.where((branch == 0) | (branch == 2), 1.0, -1.0)
    s = ADV_STATS if c["normalise"] else None
    adv = (A / s[1] + s[0] if s else A).astype(np.float32)
    ret = (val + rng.normal(0, 1, size=rows)).astype(np.float32)
    return dict(x=x, index=index, logp_old=(logp - np.log(r)).astype(np.float32), adv=adv, ret=ret, policy=p, value=v,
                adv_stats=None if s is None else np.array(s, dtype=np.float32), branch=branch, in_dim=in_dim, bins=bins)


def grad_case(c):
    """The rows of one minibatch, in order (ppo_ref.build_case's construction with sampled indices in place of actions: row i belongs to
    branch i % 4 -- cut above, cut below, inside the band with either sign of A), computed once and shared."""
    return _grad_case(_key(c))


subset_case = pp.subset_case


@functools.lru_cache(maxsize=None)
def _reference(key, critic, sel):
    case = grad_case(dict(key))
    if sel is not None:
        case = subset_case(case, np.asarray(sel))
    return reference_of(case, critic)


def reference_of(case, critic=True):
    k = case["in_dim"]
    return loss_and_grads_f64(case["x"][:, :k], case["index"], case["logp_old"], case["adv"], case["ret"], case["policy"],
                              case["value"] if critic else None, case["bins"], adv_stats=case["adv_stats"])


def emulation_of(case, critic=True):
    k = case["in_dim"]
    return emulate_grads(case["x"][:, :k], case["index"], case["logp_old"], case["adv"], case["ret"], case["policy"],
                         case["value"] if critic else None, case["bins"], adv_stats=case["adv_stats"])


def list_subsets():
    """(j, the rows of LIST_CASE in strided minibatch j of LIST_MB over its first LIST_COUNT rows)."""
    for j in range(LIST_MB):
        yield j, np.arange(j, LIST_COUNT, LIST_MB)


def compared_grad_cases():
    """(label, case arrays, float64 reference, critic) of EVERY comparison of tests/test_categorical_gpu.py that uses the recorded
    tolerances.  The references are computed once and shared."""
    for c in GRAD_CASES + SWEEP_CASES + MORE_CASES:
        yield str(c), grad_case(c), _reference(_key(c), True, None), True
    yield "no critic", grad_case(NOCRITIC_CASE), _reference(_key(NOCRITIC_CASE), False, None), False
    for j, sel in list_subsets():
        yield "list: minibatch %d of %d" % (j, LIST_MB), subset_case(grad_case(LIST_CASE), sel), _reference(_key(LIST_CASE), True, tuple(sel)), True


grad_errors, stat_errors = pp.grad_errors, pp.stat_errors
