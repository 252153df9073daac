"""The checker of pgdrive_amd/csrc/pgd_guided.h (pgd_ppo_grad_guided), in plain numpy, on tests/ppo_ref.py:

* loss_and_grads_guided_f64   the formulas of include/pgdrive_hip.h in float64: ppo_ref.loss_and_grads_f64's expressions, the guided bit
                              u selecting the surrogate away and the imitation term in (tests/test_guided_cpu.py holds it against torch
                              autograd and, with no guided row, against ppo_ref.loss_and_grads_f64 for equality); one, two or three networks;
* emulate_grads_guided        the kernels' arithmetic and summation order in float32 through ppo_ref._emulate_net's d_out_fn hook.  Never
                              compared with the device: it MEASURES the tolerances;
* the seeded cases of tests/test_guided_gpu.py, each built on ppo_ref.build_case (its ratios stay off the clip band).

Errors are normalised as ppo_ref describes; the imitation term's own contributions enter the norms as the surrogate's do: zt = (target -
mean) e is a difference, |target| + |mean| stands for it.

Tolerances: per row class of ppo_ref.ROW_CLASSES, TOL_*_MEASURED is the largest normalised error of the emulation against float64 over
exactly guided_cases(); the GPU tolerance is twice that (the margin covers the device's exp / tanh forms, which the emulation restates);
tests/test_guided_cpu.py measures again and holds the emulation below half of the tolerance."""
import functools
import zlib

import numpy as np

from tests import ppo_ref as rf

ar, pr = rf.ar, rf.pr
_f32, _f64 = rf._f32, rf._f64
LOG_2PI, LOG_2PIE = rf.LOG_2PI, rf.LOG_2PIE
CVF_COEF = 0.25
N_STATS = 12
MEAN_SLOTS = (1, 2, 3, 4, 5, 6, 7, 9)   # the statistics that are means: compared under the tolerance; 0, 8, 10, 11 are exact

# The largest normalised error of emulate_grads_guided against loss_and_grads_guided_f64 over guided_cases() -- in_dim 4, 274, 416 at 33
# rows; 1, 15, 16, 17, 33, 1027 rows at in_dim 274; out_cols 4, 5, 6; the mask patterns of PATTERNS at 33 rows; target stride 2 and 4;
# keep_surrogate on and off; bc_coef 1, 0.5 and 0; two and three networks and one without a critic; the two strided halves of the 1027
# rows -- per row class (every gradient entry of every network / the eight means of the twelve statistics), measured on the CPU by
# tests/test_guided_cpu.py's measure().
TOL_GRAD_MEASURED = dict(few=8.286e-7, tile=1.224e-7, part=4.550e-8)
TOL_STAT_MEASURED = dict(few=1.633e-7, tile=3.046e-7, part=3.466e-8)
# bc_loss(before) - bc_loss(after) of ten adam_f64 steps of the float64 reference on ppo_ref.closed_loop_case() (in_dim 35, 64 rows,
# lr 3e-4) with every row guided, no surrogate, bc_coef 1, the target of loop_case()
GUIDED_LOOP_D = 1.68897300


def tolerances(n):
    """(TOL_GRAD, TOL_STAT) of a minibatch of n live rows: twice the measured figures of its row class."""
    return 2.0 * TOL_GRAD_MEASURED[rf.row_class(n)], 2.0 * TOL_STAT_MEASURED[rf.row_class(n)]


# ---------------------------------------------------------------------------------------------------------------------
# float64
# ---------------------------------------------------------------------------------------------------------------------
def _critic_f64(x, net, ret, coef, n):
    """(L terms, their norms, gradients, norms) of a critic-shaped network on the targets `ret`: ppo_ref.loss_and_grads_f64's lines."""
    vh1, vh2 = rf._forward_f64(x, net)
    v = (vh2 @ _f64(net[4])[:, :1] + _f64(net[5])[:1])[:, 0]
    err = v - _f64(ret)
    vg, vn = rf._backward_f64(x, vh1, vh2, (coef * err / n)[:, None], (coef * (np.abs(v) + np.abs(_f64(ret))) / n)[:, None], net, 1)
    return 0.5 * err * err, 0.5 * (np.abs(v) + np.abs(_f64(ret))) ** 2, vg, vn


def loss_and_grads_guided_f64(x, action, logp_old, adv, ret, policy, value, target, guided, bc_coef=1.0, keep_surrogate=False, clip=rf.CLIP,
                              vf_coef=rf.VF_COEF, ent_coef=rf.ENT_COEF, adv_stats=None, cost=None, cost_ret=None, cvf_coef=CVF_COEF):
    """The live rows of one minibatch -> dict(stats [12], stat_norm [12], loss, policy / value / cost: six gradients each (None without
    the network), *_norm).  target [n, >= 2] (columns 0, 1 are read, and only where `guided` [n] bool holds), guided None: every row."""
    n = int(np.asarray(x).shape[0])
    in_dim = np.asarray(policy[0]).shape[0]
    out_cols = np.asarray(policy[4]).shape[1]
    vf, ce, cvf, bc = [float(np.float32(q)) for q in (vf_coef, ent_coef, cvf_coef, bc_coef)]
    zero = lambda oc: [np.zeros((in_dim, rf.H)), np.zeros(rf.H), np.zeros((rf.H, rf.H)), np.zeros(rf.H), np.zeros((rf.H, oc)), np.zeros(oc)]  # noqa: E731
    if n == 0:
        out = dict(stats=np.zeros(N_STATS), stat_norm=np.zeros(N_STATS), loss=0.0, policy=zero(out_cols), policy_norm=zero(out_cols))
        for name, net in (("value", value), ("cost", cost)):
            out[name], out[name + "_norm"] = (None, None) if net is None else (zero(1), zero(1))
        return out
    u = np.ones(n, dtype=bool) if guided is None else np.asarray(guided, dtype=bool)
    s = ~u | bool(keep_surrogate)
    x = _f64(np.asarray(x)[:, :in_dim])
    h1, h2 = rf._forward_f64(x, policy)
    o = h2 @ _f64(policy[4])[:, :4] + _f64(policy[5])[:4]
    mean, ls = o[:, :2], o[:, 2:4]
    A, logp, r, flows, z, e, rc = rf.row_terms_f64(mean, ls, action, logp_old, adv, adv_stats, clip)
    g = np.where(flows & s, -A * r / n, 0.0)
    tgt = np.where(u[:, None], _f64(target)[:, :2], 0.0)   # (selected: a free row's target may be NaN)
    zt = (tgt - mean) * e
    c = np.where(u, bc / n, 0.0)[:, None]
    d_out = np.concatenate([g[:, None] * z * e - c * zt * e, g[:, None] * (z * z - 1.0) - ce / n + c * (1.0 - zt * zt)], axis=1)
    nz = (np.abs(_f64(action)) + np.abs(mean)) * e
    nzt = (np.abs(tgt) + np.abs(mean)) * e
    ng = (np.abs(g) * (1.0 + np.abs(logp) + np.abs(_f64(logp_old))))[:, None]
    n_out = np.concatenate([ng * nz * e + c * nzt * e, ng * (nz * nz + 1.0) + ce / n + c * (1.0 + nzt * nzt)], axis=1)
    pg, pn = rf._backward_f64(x, h1, h2, d_out, n_out, policy, 4)
    ent = ls.sum(axis=1) + LOG_2PIE
    nlp = 0.5 * (zt * zt).sum(axis=1) + ls.sum(axis=1) + LOG_2PI
    cond = 1.0 + np.abs(logp) + np.abs(_f64(logp_old))
    sel = lambda t: np.where(s, t, 0.0)  # noqa: E731
    n_s, n_g = int(s.sum()), int(u.sum())
    # slot: (terms, their norms (None: the terms' absolute values), the count its mean is over)
    slots = {1: (sel(-np.minimum(r * A, rc * A)), sel(np.abs(np.minimum(r * A, rc * A)) * cond), n_s),
             3: (ent, np.abs(ls).sum(axis=1) + LOG_2PIE, n),
             4: (sel(_f64(logp_old) - logp), sel(np.abs(logp) + np.abs(_f64(logp_old))), n_s),
             5: (sel((~flows).astype(np.float64)), None, n_s),
             6: (sel(r), sel(r * cond), n_s),
             9: (np.where(u, nlp, 0.0), np.where(u, 0.5 * (nzt * nzt).sum(axis=1) + np.abs(ls).sum(axis=1) + LOG_2PI, 0.0), n_g)}
    out = dict(policy=pg, policy_norm=pn)
    for name, net, targets, coef, slot in (("value", value, ret, vf, 2), ("cost", cost, cost_ret, cvf, 7)):
        out[name] = out[name + "_norm"] = None
        if net is not None:
            lv, lvn, out[name], out[name + "_norm"] = _critic_f64(x, net, targets, coef, n)
            slots[slot] = (lv, lvn, n)
    stats, stat_norm = np.zeros(N_STATS), np.zeros(N_STATS)
    for k, (t, q, cnt) in slots.items():
        if cnt:
            stats[k], stat_norm[k] = t.sum() / cnt, np.abs(t if q is None else q).sum() / cnt
    stats[0] = stat_norm[0] = n
    stats[8] = stat_norm[8] = n_g
    out.update(stats=stats, stat_norm=stat_norm, loss=float(stats[1] * (n_s / n) + vf * stats[2] - ce * stats[3] + bc * stats[9] * (n_g / n) +
                                                           cvf * stats[7]))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the kernels' arithmetic in float32
# ---------------------------------------------------------------------------------------------------------------------
def emulate_grads_guided(x, action, logp_old, adv, ret, policy, value, target, guided, bc_coef=1.0, keep_surrogate=False, clip=rf.CLIP,
                         vf_coef=rf.VF_COEF, ent_coef=rf.ENT_COEF, adv_stats=None, cost=None, cost_ret=None, cvf_coef=CVF_COEF):
    """loss_and_grads_guided_f64's outputs (stats, policy, value, cost) as the kernels compute them; rows in minibatch order, n >= 1."""
    n = int(np.asarray(x).shape[0])
    in_dim = np.asarray(policy[0]).shape[0]
    x = _f32(np.asarray(x)[:, :in_dim])
    inv32 = np.float32(1.0 / n)
    inv, ce, bc = float(inv32), float(np.float32(ent_coef)), float(np.float32(bc_coef))
    u = np.ones(n, dtype=bool) if guided is None else np.asarray(guided, dtype=bool)
    s = ~u | bool(keep_surrogate)
    tgt = np.where(u[:, None], _f64(_f32(target))[:, :2], 0.0)

    def actor(o):  # ppo_rows_tile<NORM, true>'s row lane: in double from the fp32 heads, dOut rounded once
        o64 = o.astype(np.float64)
        mean, ls = o64[:, :2], o64[:, 2:4]
        A, logp, r, flows, z, e, rc = rf.row_terms_f64(mean, ls, action, logp_old, adv, None if adv_stats is None else _f32(adv_stats), clip)
        g = np.where(flows, -A * r * inv, 0.0)[:, None]
        sc = s[:, None]
        zt = (tgt - mean) * e
        c = bc * inv
        d_mean = np.where(sc, g * z * e, 0.0)
        d_ls = np.where(sc, g * (z * z - 1.0), 0.0) - ce * inv
        d_mean = np.where(u[:, None], d_mean - c * zt * e, d_mean)
        d_ls = np.where(u[:, None], d_ls + c * (1.0 - zt * zt), d_ls)
        nlp = 0.5 * (zt * zt).sum(axis=1) + ls.sum(axis=1) + LOG_2PI
        t = _f32(np.stack([np.where(s, -np.minimum(r * A, rc * A), 0.0), _f32(_f32(o[:, 2] + o[:, 3]) + np.float32(LOG_2PIE)),
                           np.where(s, _f64(logp_old) - logp, 0.0), (s & ~flows).astype(np.float64), np.where(s, r, 0.0),
                           u.astype(np.float64), np.where(u, nlp, 0.0)], axis=1))
        return _f32(np.concatenate([d_mean, d_ls], axis=1)), t

    pg, t = rf._emulate_net(x, policy, actor, rf.gaussian_head(4, 4))
    tot = rf._ordered_sum(t, 16)
    n_g = int(tot[5])
    n_s = n if keep_surrogate else n - n_g
    inv_s = np.float32(1.0 / n_s) if n_s else np.float32(0.0)
    stats = np.zeros(N_STATS, dtype=np.float32)
    stats[0], stats[8] = n, n_g
    stats[[1, 4, 5, 6]] = _f32(tot[[0, 2, 3, 4]] * inv_s)
    stats[3] = np.float32(tot[1] * inv32)
    stats[9] = np.float32(tot[6] * np.float32(1.0 / n_g)) if n_g else 0.0
    out = dict(policy=pg)
    for name, net, targets, coef, slot in (("value", value, ret, vf_coef, 2), ("cost", cost, cost_ret, cvf_coef, 7)):
        out[name] = None
        if net is not None:
            def critic(o, targets=targets, coef=np.float32(coef)):   # ppo_ref.emulate_update's critic
                err = _f32(o[:, 0] - _f32(targets))
                lv = _f32(_f32(np.float32(0.5) * err) * err)
                return _f32(_f32(coef * err) * inv32)[:, None], lv[:, None]
            out[name], lv = rf._emulate_net(x, net, critic, rf.gaussian_head(1, 16))
            stats[slot] = np.float32(rf._ordered_sum(lv, 16)[0] * inv32)
    out["stats"] = stats
    return out


def grad_errors(got, ref):
    """(largest normalised gradient error over every entry of every network `ref` has, largest normalised error of the eight means);
    n, n_g and the two reserved slots are exact."""
    eg = 0.0
    for net in ("policy", "value", "cost"):
        if ref.get(net) is None:
            continue
        for g, w, nrm in zip(got[net], ref[net], ref[net + "_norm"]):
            eg = max(eg, rf.normalised_error(np.asarray(g).reshape(np.shape(w)), w, nrm))
    st = np.asarray(got["stats"])
    assert st.shape == (N_STATS, ) and float(st[0]) == ref["stats"][0] and float(st[8]) == ref["stats"][8] and st[10] == 0.0 and st[11] == 0.0
    m = list(MEAN_SLOTS)
    return eg, rf.normalised_error(st[m], ref["stats"][m], ref["stat_norm"][m])


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
# the guided rows of a minibatch of n rows by pattern: (mask bytes [n] or None for a null mask, mask_bits)
PATTERNS = {
    "none": lambda n: (np.zeros(n, np.uint8), 1),
    "null": lambda n: (None, 1),
    "ones": lambda n: (np.ones(n, np.uint8), 1),
    "alternating": lambda n: ((np.arange(n) % 2 == 0).astype(np.uint8), 1),
    "single0": lambda n: ((np.arange(n) == 0).astype(np.uint8), 1),
    "single15": lambda n: ((np.arange(n) == 15).astype(np.uint8), 1),
    "single16": lambda n: ((np.arange(n) == 16).astype(np.uint8), 1),
    "bytes246_bits1": lambda n: (np.array([2, 4, 6], np.uint8)[np.arange(n) % 3], 1),   # no low bit: every row free
    "bytes246_bits3": lambda n: (np.array([2, 4, 6], np.uint8)[np.arange(n) % 3], 3),   # 2 and 6 guided, 4 free
}
PATTERN_ROWS, PATTERN_WIDTH = 33, 274


def _base(name, in_dim, rows, i):
    return dict(name=name, in_dim=in_dim, rows=rows, scaling=("unit", "normalised")[i % 2], out_cols=rf.OUT_COLS[i % 3], seed=i, normalise=bool(i % 2))


def guided_cases_rows():
    """Tile edges and one past the partition of 1024 rows, every other row guided; three networks at 17 and 1027 rows."""
    return [dict(base=_base("guided-rows", PATTERN_WIDTH, rows, i), pattern="alternating", stride=(4, 2)[i % 2], keep=bool(i % 2),
                 bc_coef=(1.0, 0.5)[i % 2], nets=3 if rows in (17, 1027) else 2) for i, rows in enumerate(rf.ROW_COUNTS)]


def guided_cases():
    """Every comparison of tests/test_guided_gpu.py that uses the recorded tolerances, as dicts of build_guided's arguments."""
    out = []
    for i, pattern in enumerate(PATTERNS):   # the mask patterns at 33 rows, stride and keep_surrogate alternating
        out.append(dict(base=_base("guided-pattern", PATTERN_WIDTH, PATTERN_ROWS, i), pattern=pattern, stride=(2, 4)[i % 2], keep=bool(i % 3 == 1),
                        bc_coef=1.0, nets=2))
    out += guided_cases_rows()
    for i, in_dim in enumerate((4, 416)):     # the narrowest input and the LDS limit
        out.append(dict(base=_base("guided-width", in_dim, PATTERN_ROWS, i), pattern=("alternating", "null")[i], stride=(2, 4)[i], keep=False,
                        bc_coef=1.0, nets=(2, 3)[i]))
    alt = _base("guided-switch", PATTERN_WIDTH, PATTERN_ROWS, 1)
    out.append(dict(base=alt, pattern="alternating", stride=2, keep=True, bc_coef=0.0, nets=2))    # bc_coef 0, the surrogate kept: plain PPO's gradient
    out.append(dict(base=alt, pattern="alternating", stride=4, keep=False, bc_coef=0.0, nets=2))   # bc_coef 0, masking only
    out.append(dict(base=alt, pattern="null", stride=4, keep=True, bc_coef=1.0, nets=1))           # no critic
    for j in range(SPLIT_MB):                 # the strided halves of the 1027-row case (no partition boundary inside; the whole has one)
        out.append(dict(split_whole(), split=(j, SPLIT_MB)))
    return out


SPLIT_MB = 2


def split_whole():
    """The 1027-row case of guided_cases(): the whole of the strided-split comparison."""
    return [c for c in guided_cases_rows() if c["base"]["rows"] == 1027][0]


def build_guided(base, pattern, stride, keep, bc_coef, nets, split=None):
    """ppo_ref.build_case(**base) plus: target [rows, stride] float32 -- mean + std * N(0, 1) clipped at 3 in columns 0, 1 of the guided
    rows, NaN in every free row and in columns 2, 3 --, mask / mask_bits of the pattern, guided [rows] bool, the cost critic and its
    targets, and the switches.  nets 1: no critic; 3: with the cost critic.  split (j, n_mb): the rows j, j + n_mb, ... of that case."""
    c = dict(rf.build_case(**base))
    rows, k = base["rows"], base["in_dim"]
    rng = np.random.default_rng([zlib.crc32(b"guided"), k, rows, list(PATTERNS).index(pattern), stride, base["seed"]])
    mask, bits = PATTERNS[pattern](rows)
    u = np.ones(rows, dtype=bool) if mask is None else (mask & bits) != 0
    mean, ls, _ = ar.heads_f64(c["x"][:, :k], c["policy"], c["value"])
    tgt = np.full((rows, stride), np.nan, dtype=np.float32)
    tgt[u, :2] = (mean + np.exp(ls) * np.clip(rng.normal(0, 1, size=(rows, 2)), -3, 3))[u]
    _, cost = ar.make_networks(rng, k, 4)
    val, cost_ret = ar.heads_f64(c["x"][:, :k], c["policy"], cost)[2], None
    cost_ret = (val + rng.normal(0, 1, size=rows)).astype(np.float32)
    c.update(target=tgt, mask=mask, mask_bits=bits, guided=u, cost=cost, cost_ret=cost_ret, keep=keep, bc_coef=bc_coef, nets=nets,
             stride=stride)
    return c if split is None else subset(c, np.arange(split[0], rows, split[1]))


def subset(case, sel):
    out = rf.subset_case(case, sel)
    for key in ("target", "guided", "cost_ret"):
        out[key] = case[key][sel]
    out["mask"] = None if case["mask"] is None else case["mask"][sel]
    return out


def _args(c):
    k = c["in_dim"]
    return (c["x"][:, :k], c["action"], c["logp_old"], c["adv"], c["ret"], c["policy"], c["value"] if c["nets"] >= 2 else None, c["target"],
            c["guided"]), dict(bc_coef=c["bc_coef"], keep_surrogate=c["keep"], adv_stats=c["adv_stats"], cost=c["cost"] if c["nets"] == 3 else None,
                               cost_ret=c["cost_ret"] if c["nets"] == 3 else None)


def reference_of(c):
    a, kw = _args(c)
    return loss_and_grads_guided_f64(*a, **kw)


def emulation_of(c):
    a, kw = _args(c)
    return emulate_grads_guided(*a, **kw)


def _key(c):
    return tuple(sorted((k, tuple(sorted(v.items())) if isinstance(v, dict) else v) for k, v in c.items()))


@functools.lru_cache(maxsize=None)
def _case_and_reference(key):
    c = build_guided(**{k: dict(v) if k == "base" else v for k, v in key})
    return c, reference_of(c)


def case_and_reference(c):
    """(the case's arrays, its float64 reference), computed once and shared; neither is modified by its users."""
    return _case_and_reference(_key(c))


def loop_case():
    """ppo_ref.closed_loop_case() with every row guided by a null mask: the target is the case's own policy's mean shifted by (0.3, -0.2)
    -- an expert that steers and brakes otherwise than the agent."""
    c = dict(rf.build_case(**rf.closed_loop_case()))
    k = c["in_dim"]
    mean, _, _ = ar.heads_f64(c["x"][:, :k], c["policy"], c["value"])
    c["target"] = (mean + np.array([0.3, -0.2])).astype(np.float32)
    return c
