"""The checker of pgdrive_amd/csrc/pgd_safe.h (pgd_cost_gae, pgd_lagrange, pgd_adv_mix, pgd_ppo_grad_cost), in plain numpy:

* float64 restatements of the formulas of include/pgdrive_hip.h -- the costs of a rollout from its flags, the episode-cost bookkeeping,
  GAE on the costs, the multiplier step, the mixed advantage;
* the three-network loss as two uses of ppo_ref.loss_and_grads_f64: actor and critic on the advantage the policy sees, and the cost
  critic as "the critic" on cost_ret with cvf_coef;
* float32 emulations of the stated summation orders where a result is not exact (the bookkeeping's running sums);
* the cases of tests/test_safe_ppo_gpu.py, so that tests/test_safe_ppo_cpu.py measures the emulation over the very same inputs.

Tolerances: TOL_EP is twice what the float32 emulation of the bookkeeping is away from float64 over cost_gae_cases() with the costs
NONDYADIC, per entry and relative to the sum of the entry's |terms| (tests/test_safe_ppo_cpu.py measures it and holds the emulation
within half of the constant).  pgd_lagrange and pgd_adv_mix are single roundings of double results: one float32 ulp, no constant.
"""
import numpy as np

from tests import actor_critic_ref as ar
from tests import ppo_ref as rf

F_OUT_OF_ROAD, F_CRASH_VEHICLE, F_CRASH_OBJECT = 2, 4, 8
# every other flag bit include/pgdrive_hip.h defines (pgdrive_amd/_abi.py: F_*)
OTHER_FLAG_BITS = (1, 16, 32, 256, 512, 1024, 2048, 4096, 8192, 1 << 14, 1 << 16, 1 << 17, 1 << 18, 1 << 19)

DYADIC = (1.0, 0.5, 0.25)       # every sum of these is exact in float32
NONDYADIC = (0.3, 0.7, 1.1)
CVF_COEF = 0.75                  # the cost critic's coefficient in the cases (another number than ppo_ref.VF_COEF)

TOL_EP_MEASURED = 1.978e-7       # tests/test_safe_ppo_cpu.py::test_the_bookkeeping_emulation_keeps_half_of_the_tolerance measures it
TOL_EP = 2.0 * TOL_EP_MEASURED


def _f32(a):
    return np.asarray(a, dtype=np.float32)


def _f64(a):
    return np.asarray(a, dtype=np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# (2) costs, bookkeeping, GAE
# ---------------------------------------------------------------------------------------------------------------------
def costs_of_flags(flags, costs):
    """cost = out_of_road ? c0 : crash_vehicle ? c1 : crash_object ? c2 : 0 -- a selection of the three floats as float32."""
    f = np.asarray(flags).astype(np.int64)
    c = _f32(costs)
    return np.where(f & F_OUT_OF_ROAD, c[0], np.where(f & F_CRASH_VEHICLE, c[1], np.where(f & F_CRASH_OBJECT, c[2], np.float32(0.0)))).astype(np.float32)


def bookkeeping(cost, done, run, dtype=np.float64):
    """The forward scan over t in `dtype`: run += cost; at a done: ep_sum += run, ep_count += 1, run = 0 -> (run, ep_sum, ep_count,
    and the sum of |terms| behind every entry of run and ep_sum, for normalising an error)."""
    cost, done = np.asarray(cost), np.asarray(done) != 0
    T, rows = cost.shape
    rn, es, ec = np.asarray(run).astype(dtype).copy(), np.zeros(rows, dtype=dtype), np.zeros(rows, dtype=np.int32)
    rn_abs, es_abs = np.abs(_f64(run)).copy(), np.zeros(rows)
    for t in range(T):
        rn = (rn + cost[t].astype(dtype)).astype(dtype)
        rn_abs = rn_abs + np.abs(_f64(cost[t]))
        d = done[t]
        es = np.where(d, (es + rn).astype(dtype), es)
        es_abs = np.where(d, es_abs + rn_abs, es_abs)
        ec = ec + d.astype(np.int32)
        rn = np.where(d, dtype(0.0), rn)
        rn_abs = np.where(d, 0.0, rn_abs)
    return rn, es, ec, rn_abs, es_abs


def cost_gae_f64(flags, done, cost_value, costs, gamma, lam, run):
    """pgd_cost_gae in float64 -> dict(cost (float32, exact), cadv, cret, run, ep_sum, ep_count, run_norm, ep_norm)."""
    cost = costs_of_flags(flags, costs)
    rn, es, ec, rn_abs, es_abs = bookkeeping(cost, done, run)
    cadv, cret = ar.gae_f64(cost, cost_value, done, gamma, lam)
    return dict(cost=cost, cadv=cadv, cret=cret, run=rn, ep_sum=es, ep_count=ec, run_norm=rn_abs, ep_norm=es_abs)


def emulate_bookkeeping(cost, done, run):
    """The kernel's order in float32: one thread per row, t ascending, every sum rounded."""
    rn, es, ec, _, _ = bookkeeping(_f32(cost), done, _f32(run), dtype=np.float32)
    return rn, es, ec


def bookkeeping_error(got_run, got_sum, ref):
    """The largest error of the running and the finished sums against float64, each relative to the sum of its |terms|."""
    return max(rf.normalised_error(got_run, ref["run"], ref["run_norm"]), rf.normalised_error(got_sum, ref["ep_sum"], ref["ep_norm"]))


COST_T = (1, 2, 7)
COST_ROWS = (1, 63, 64, 65, 130)
DONE_MODES = ("random", "every", "none")


def cost_gae_cases():
    """(T, rows, done mode): every T and row count with random dones, and the largest shape with a done in every step and with none."""
    for T in COST_T:
        for rows in COST_ROWS:
            yield T, rows, "random"
    yield COST_T[-1], COST_ROWS[-1], "every"
    yield COST_T[-1], COST_ROWS[-1], "none"


def build_cost_rollout(T, rows, done_mode, dyadic):
    """flags int32 [T, rows] -- entry i has cost-bit combination i % 8, every other defined bit at random --, done uint8, cost_value
    float32 [T + 1, rows], run float32 [rows] (multiples of 0.25 when `dyadic`)."""
    rng = np.random.default_rng([T, rows, DONE_MODES.index(done_mode), int(dyadic)])
    combo = (np.arange(T * rows) + rng.integers(0, 8)) % 8
    flags = ((combo & 1) * F_OUT_OF_ROAD + ((combo >> 1) & 1) * F_CRASH_VEHICLE + ((combo >> 2) & 1) * F_CRASH_OBJECT).astype(np.int64)
    for bit in OTHER_FLAG_BITS:
        flags |= np.where(rng.random(T * rows) < 0.5, bit, 0)
    flags = rng.permutation(flags).reshape(T, rows).astype(np.int32)
    done = dict(random=rng.random((T, rows)) < 0.3, every=np.ones((T, rows), dtype=bool), none=np.zeros((T, rows), dtype=bool))[done_mode]
    cost_value = rng.normal(0, 1, size=(T + 1, rows)).astype(np.float32)
    run = (rng.integers(0, 40, size=rows) * 0.25 if dyadic else rng.uniform(0, 10, size=rows)).astype(np.float32)
    return flags, done.astype(np.uint8), cost_value, run


# ---------------------------------------------------------------------------------------------------------------------
# (3) the multiplier
# ---------------------------------------------------------------------------------------------------------------------
def lagrange_f64(ep_sum, ep_count, state, cost_limit, lr, lambda_max):
    """One pgd_lagrange step on a float64 copy of the four-float state; the scalars as the float32 the device is given.  E = 0: the
    state as it was."""
    st = _f64(state).copy()
    E = int(np.asarray(ep_count).astype(np.int64).sum())
    if E == 0:
        return st
    limit, lr, lmax = [float(np.float32(q)) for q in (cost_limit, lr, lambda_max)]
    jc = float(_f64(ep_sum).sum()) / E
    st[0] = min(lmax, max(0.0, st[0] + lr * (jc - limit)))
    st[1], st[2] = jc, float(E)
    return st


LAG_ROWS = (1, 64, 65, 4099)
LAG_MOVES = ("up", "down", "clamp_zero", "clamp_max")
LAG_MAX = 5.0


def build_lagrange(rows, move):
    """(ep_sum float32, ep_count int32, state float32 [4], cost_limit, lr) whose step from state[0] goes up, goes down, is held at 0 or is
    held at LAG_MAX.  Rows without an episode hold sum 0."""
    rng = np.random.default_rng([rows, LAG_MOVES.index(move)])
    count = rng.integers(0, 4, size=rows).astype(np.int32)
    count[rng.integers(0, rows)] = 2
    ep_sum = np.where(count > 0, rng.uniform(0, 3, size=rows) * count, 0.0).astype(np.float32)
    jc = float(ep_sum.astype(np.float64).sum()) / int(count.sum())
    limit, lr, lam0 = dict(up=(0.5 * jc, 0.05, 1.0), down=(1.5 * jc, 0.05, 1.0), clamp_zero=(jc + 50.0, 0.5, 0.3),
                           clamp_max=(jc - 50.0, 0.5, 4.0))[move]
    return ep_sum, count, np.array([lam0, np.nan, 0.0, 0.0], dtype=np.float32), limit, lr


def ulp32(x):
    """The spacing of float32 at |x| (at least that of the smallest normal number)."""
    return np.spacing(np.maximum(np.abs(_f32(x)), np.float32(1.17549435e-38))).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# (4) the advantage the policy sees
# ---------------------------------------------------------------------------------------------------------------------
def adv_mix_f64(adv, cadv, adv_stats, cadv_stats, lam):
    """((adv - m) s - lambda (cadv - m_c)) / (1 + lambda) in float64 -> (out, the bound of one float32 rounding: one ulp at
    max(|term 1|, |term 2|) / (1 + lambda), which holds the result however the two terms cancel)."""
    m, s = (0.0, 1.0) if adv_stats is None else (float(adv_stats[0]), float(adv_stats[1]))
    mc = 0.0 if cadv_stats is None else float(cadv_stats[0])
    lam = float(np.float32(lam))
    t1, t2 = (_f64(adv) - m) * s, lam * (_f64(cadv) - mc)
    return (t1 - t2) / (1.0 + lam), ulp32(np.maximum(np.abs(t1), np.abs(t2)) / (1.0 + lam))


MIX_N = (1, 63, 64, 65, 4099)
MIX_LAMBDA = (0.0, 0.37, 100.0)


def build_mix(n):
    rng = np.random.default_rng([n, 77])
    return rng.normal(0.2, 1.5, size=n).astype(np.float32), rng.uniform(-1, 3, size=n).astype(np.float32), \
        np.array([0.2, 0.7], dtype=np.float32), np.array([0.9, 1.3], dtype=np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# (5) three networks
# ---------------------------------------------------------------------------------------------------------------------
GRAD_WIDTHS = (4, 35, 274, 416)


def grad_cases():
    """ppo_ref's cases at the widths 4, 35, 274, 416 (33 rows each, out_cols 4, 5, 6) and its row counts 1 .. 1027 at width 274."""
    return [c for c in rf.grad_cases() if c["in_dim"] in GRAD_WIDTHS]


def f64_cases():
    """The cases whose three gradient sets tests/test_safe_ppo_gpu.py holds against float64: per width the first case and those of the
    width's largest row count."""
    out = []
    for k in GRAD_WIDTHS:
        cases = [c for c in grad_cases() if c["in_dim"] == k]
        top = max(c["rows"] for c in cases)
        out += [c for j, c in enumerate(cases) if j == 0 or c["rows"] == top]
    return out


def cost_side(c):
    """The cost critic and its targets of ppo_ref case `c`: (six weights of the value network's shapes, cost_ret float32 [rows]).  The
    targets are drawn as ppo_ref.build_case draws `ret`: the network's own float64 output plus unit normal noise.  ppo_ref.tolerances, which
    the comparison with float64 uses, were measured on targets of that kind; targets with a common offset from the outputs make every
    dL/dv of one sign and the bias gradients a sum of 1027 like-signed terms, whose float32 rounding in row order (6e-7 of the sum in the
    emulation and on the device alike) is no property of the third network."""
    rng = np.random.default_rng([c["in_dim"], c["rows"], c["seed"], 1234])
    _, cw = ar.make_networks(rng, c["in_dim"], 4)
    case, _ = rf.case_and_reference(c)
    _, _, v = ar.heads_f64(case["x"][:, :c["in_dim"]], case["policy"], cw)
    return cw, (v + rng.normal(0, 1, size=c["rows"])).astype(np.float32)


def loss_and_grads3_f64(x, action, logp_old, adv, ret, cost_ret, policy, value, cost_net, clip=rf.CLIP, vf_coef=rf.VF_COEF, cvf_coef=CVF_COEF,
                        ent_coef=rf.ENT_COEF, adv_stats=None):
    """The three-network loss L = L_pi + vf_coef L_v - ent_coef mean(H) + cvf_coef L_c and its gradients: ppo_ref.loss_and_grads_f64 for actor
    and critic, and once more with the cost critic as "the critic" on cost_ret -> (main, cost): two of its dicts; stats[7] of the device
    is cost["stats"][2], the cost critic's gradients are cost["value"]."""
    main = rf.loss_and_grads_f64(x, action, logp_old, adv, ret, policy, value, clip=clip, vf_coef=vf_coef, ent_coef=ent_coef, adv_stats=adv_stats)
    cost = rf.loss_and_grads_f64(x, action, logp_old, adv, cost_ret, policy, cost_net, clip=clip, vf_coef=cvf_coef, ent_coef=ent_coef,
                                 adv_stats=adv_stats)
    return main, cost


def split_outputs(stats, policy, value, cost):
    """The outputs of pgd_ppo_grad_cost as the two dicts ppo_ref.grad_errors compares: (actor and critic with stats[7] taken out, the
    cost critic as "the critic" with stats[7] in slot 2)."""
    s = _f64(stats)
    main = dict(stats=np.concatenate([s[:7], [0.0]]), policy=policy, value=value)
    cs = np.concatenate([s[:2], [s[7]], s[3:7], [0.0]])
    return main, dict(stats=cs, policy=policy, value=cost)
