"""The categorical head on the device (pgdrive_amd/csrc/pgd_categorical.h) against tests/categorical_ref.py: the forward launch, the
sampling frequencies and the tick rule, the row-list form, pgd_ppo_grad_cat against float64, the observation binding, and the collectors
and the learner with the head -- the smallest shapes at which each mechanism can go wrong."""
import functools

import numpy as np
import pytest

from tests import categorical_ref as cf
from tests import train_util as tu
from tests.ppo_util import Problem, check, into_sentinels, shapes
from tests.train_util import SENT, bits_equal, dev

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def load_descs():
    from pgdrive_amd import bank
    return bank.load_descriptions()


@functools.lru_cache(maxsize=None)
def _engine(n):
    """n envs, ego only, no lidar: the network kernels only need its row count."""
    return tu.ego_engine(load_descs(), n)


def _forward(eng, x, pw, vw, bins, seed, tick, rows=None, count=None, **kw):
    """One forward launch into sentinel-filled buffers -> (actions, index, logp, value) as tensors, synchronised."""
    import torch
    n = eng.N
    out = [torch.full((n, 1, 2), SENT, device="cuda"), torch.full((n, 1, 2), -7, dtype=torch.int32, device="cuda"),
           torch.full((n, 1), SENT, device="cuda"), torch.full((n, 1), SENT, device="cuda")]
    in_dim = int(pw[0].shape[0])
    if rows is None:
        eng.mlp_actor_critic_cat(pw, vw, bins, out[0], out[1], out[2], out[3], seed, tick, obs=x, in_dim=in_dim, **kw)
    else:
        eng.mlp_actor_critic_cat_rows(pw, vw, bins, rows, count, out[0], out[1], out[2], out[3], seed, tick, obs=x, in_dim=in_dim, **kw)
    eng.sync()
    torch.cuda.synchronize()
    return [t.view(n, -1) if t.dim() == 3 else t.view(n) for t in out]


# ---------------------------------------------------------------------------------------------------------------------
# 1. the forward launch against float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", cf.FORWARD_CASES, ids=lambda c: "rows%d-in%d-bins%dx%d-cols%d" % (c["rows"], c["in_dim"], *c["bins"], c["out_cols"]))
def test_forward_against_float64(c):
    import torch
    case = cf.forward_case(c)
    eng = _engine(c["rows"])
    x = dev(case["x"])   # (strided: the rows are wider than in_dim, NaN in the padding)
    pw, vw = tuple(dev(w) for w in case["policy"]), tuple(dev(w) for w in case["value"])
    (ks, kt), n = c["bins"], c["rows"]
    for det, ref in ((False, case["sampled"]), (True, case["argmax"])):
        act, idx, logp, value = _forward(eng, x, pw, vw, c["bins"], c["seed"], c["tick"], deterministic=det)
        got = idx.cpu().numpy()
        skip = cf.admitted_differences(ref, got)
        assert int(skip.sum()) <= int(cf.NEAR_TIE_CAP * n)
        e = cf.logp_error(logp.cpu().numpy(), ref, skip)
        print("%s %s: logp %.3f of %.2e, %d near-ties" % (c, "argmax" if det else "sampled", e / cf.TOL_CAT_LOGP, cf.TOL_CAT_LOGP, int(skip.sum())))
        assert e < cf.TOL_CAT_LOGP
        want = np.stack([cf.grid_value(got[:, 0], ks), cf.grid_value(got[:, 1], kt)], axis=1)   # exact from the index
        assert (tu.np_bits(act.cpu().numpy()) == tu.np_bits(want)).all()
        # the critic's output: mlp_actor_critic's bits on the same inputs
        a2, l2, v2 = [torch.full(s, SENT, device="cuda") for s in ((n, 1, 2), (n, 1), (n, 1))]
        gw = tuple(torch.nan_to_num(w) for w in pw) if c["out_cols"] >= 4 else pw
        eng.mlp_actor_critic(gw, vw, a2, l2, v2, c["seed"], c["tick"], obs=x, in_dim=c["in_dim"])
        eng.sync()
        assert bits_equal(value, v2.view(n))
        # PGD_AC_EMIT_INDEX: the same indices, written as floats
        act_i, idx_i, logp_i, _ = _forward(eng, x, pw, vw, c["bins"], c["seed"], c["tick"], deterministic=det, emit_index=True)
        assert bits_equal(idx_i, idx) and bits_equal(logp_i, logp) and bits_equal(act_i, idx.float())
        # no critic: value untouched
        _, idx_n, logp_n, value_n = _forward(eng, x, pw, None, c["bins"], c["seed"], c["tick"], deterministic=det)
        assert bits_equal(idx_n, idx) and bits_equal(logp_n, logp) and bool((value_n == SENT).all())


def test_forward_refusals():
    from pgdrive_amd.engine import PgdArgError, PgdError
    c = cf.FORWARD_CASES[1]
    case = cf.forward_case(c)
    eng = _engine(c["rows"])
    x, pw, vw = dev(case["x"]), tuple(dev(w) for w in case["policy"]), tuple(dev(w) for w in case["value"])
    for bins in ((1, 5), (5, 1), (9, 8)):
        with pytest.raises(ValueError):
            _forward(eng, x, pw, vw, bins, 0, 0)
    bad = __import__("torch").zeros((c["rows"], 1, 2), device="cuda")   # action_index must be int32
    with pytest.raises(PgdArgError):
        eng.mlp_actor_critic_cat(pw, vw, c["bins"], bad.clone(), bad, bad[..., 0].clone(), bad[..., 1].clone(), 0, 0, obs=x, in_dim=c["in_dim"])
    narrow = tuple(dev(w) for w in cf.forward_case(cf.FORWARD_CASES[0])["policy"])
    with pytest.raises((PgdArgError, PgdError)):
        _forward(_engine(1), dev(cf.forward_case(cf.FORWARD_CASES[0])["x"]), narrow, None, (3, 3), 0, 0)   # w3 has 4 columns


# ---------------------------------------------------------------------------------------------------------------------
# 2. sampling frequencies, the tick and the device counter
# ---------------------------------------------------------------------------------------------------------------------
def test_sampling_frequencies_and_ticks():
    """Zero w3 and a chosen b3: fixed probabilities.  16384 rows x 4 ticks; each bin's count within 5 binomial standard deviations
    sqrt(n p (1 - p)) of n p (derived, not measured)."""
    import torch
    N, in_dim, bins = 16384, 4, (5, 3)
    eng = _engine(N)
    rng = np.random.default_rng(11)
    p, v = cf.make_networks(rng, in_dim, 8, 8)
    p[4][:] = 0.0
    probs = (np.array([0.05, 0.4, 0.25, 0.1, 0.2]), np.array([0.7, 0.01, 0.29]))
    p[5][:] = np.concatenate([np.log(probs[0]), np.log(probs[1]) + 2.0]).astype(np.float32)   # (a head's logits may carry any offset)
    pw, vw = tuple(dev(w) for w in p), tuple(dev(w) for w in v)
    x = dev(rng.uniform(size=(N, in_dim)).astype(np.float32))
    ticks, draws = (0, 1, 2, 3), []
    for tick in ticks:
        _, idx, logp, _ = _forward(eng, x, pw, vw, bins, 77, tick)
        draws.append(idx.cpu().numpy())
        lp = np.log(probs[0])[draws[-1][:, 0]] + np.log(probs[1])[draws[-1][:, 1]]
        assert np.abs(logp.cpu().numpy() - lp).max() < 1e-5
    assert all((draws[0] != d).any() for d in draws[1:])   # another tick, other indices
    got = np.concatenate(draws)
    n = got.shape[0]
    for hd in range(2):
        counts = np.bincount(got[:, hd], minlength=bins[hd])
        assert counts.shape[0] == bins[hd]   # never outside the head
        sigma = np.sqrt(n * probs[hd] * (1.0 - probs[hd]))
        z = (counts - n * probs[hd]) / sigma
        print("head %d: counts %s, z %s" % (hd, counts, np.round(z, 2)))
        assert (np.abs(z) < 5.0).all()
    # tick + counter equals the summed argument, bit for bit
    counter = torch.tensor([2], dtype=torch.int32, device="cuda")
    eng.actor_critic_tick(counter)
    try:
        _, idx_c, logp_c, _ = _forward(eng, x, pw, vw, bins, 77, 1)
    finally:
        eng.actor_critic_tick(None)
    _, idx_3, logp_3, _ = _forward(eng, x, pw, vw, bins, 77, 3)
    assert bits_equal(idx_c, idx_3) and bits_equal(logp_c, logp_3)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the row-list form
# ---------------------------------------------------------------------------------------------------------------------
def test_row_list_form():
    import torch
    c = cf.FORWARD_CASES[4]   # 33 rows: three tiles
    case = cf.forward_case(c)
    n = c["rows"]
    eng = _engine(n)
    pw, vw = tuple(dev(w) for w in case["policy"]), tuple(dev(w) for w in case["value"])
    full = _forward(eng, dev(case["x"]), pw, vw, c["bins"], c["seed"], c["tick"])
    listed = np.array([32, 0, 5, 17, 16, 15, 31, 2, 9, 20, 21, 22, 23, 24, 25, 26, 27, 3], dtype=np.int32)   # unordered, more than one tile
    for count in (len(listed), 0, n):
        rows_np = np.arange(n, dtype=np.int32) if count == n else np.concatenate([listed, np.full(n - len(listed), 10 ** 6, dtype=np.int32)])
        x = case["x"].copy()
        x[np.setdiff1d(np.arange(n), rows_np[:count])] = np.nan   # a NaN observation in an unlisted row reaches nothing
        got = _forward(eng, dev(x), pw, vw, c["bins"], c["seed"], c["tick"], rows=dev(rows_np), count=dev(np.array([count], dtype=np.int32)))
        on = np.zeros(n, dtype=bool)
        on[rows_np[:count]] = True
        on_t = torch.from_numpy(on).cuda()
        for g, f in zip(got, full):
            assert bits_equal(g[on_t], f[on_t]), "a listed row differs from the full launch"
            assert bool((g[~on_t] == 0).all()), "an unlisted row is not cleared"


# ---------------------------------------------------------------------------------------------------------------------
# 4. pgd_ppo_grad_cat against float64
# ---------------------------------------------------------------------------------------------------------------------
def _grad(eng, P, start=0, stride=1, rows=None, critic=True, ent_coef=cf.ENT_COEF):
    """One ppo_grad_cat into sentinel-filled buffers and NaN-filled scratch (ppo_util.into_sentinels)."""
    k = P.case["in_dim"]
    rows = P.n_list if rows is None else rows
    need = eng.ppo_cat_work_bytes(k, rows, critic)
    assert need >= eng.ppo_work_bytes(k, rows, critic) > 0

    def call(pg, vg, stats, work):
        eng.ppo_grad_cat(P.pw, P.vw if critic else None, pg, vg if critic else None, P.case["bins"], P.t["x"], P.t["index"], P.t["logp_old"],
                         P.t["adv"], P.t["ret"], stats, work, start=start, stride=stride, rows=rows, index=P.index, count=P.count,
                         n_list=P.n_list, adv_stats=P.stats_in, clip=cf.CLIP, vf_coef=cf.VF_COEF, ent_coef=ent_coef, in_dim=k)
        eng.sync()

    return into_sentinels(P, critic, (need + 3) // 4, call)


def _check(got, ref, what, K):
    check(got, ref, what, live=K, tolerances=cf.tolerances)


@pytest.mark.parametrize("c", cf.GRAD_CASES + cf.SWEEP_CASES + cf.MORE_CASES, ids=lambda c: "rows%d-in%d-bins%dx%d-cols%d" % (c["rows"], c["in_dim"], *c["bins"], c["out_cols"]))
def test_grad_against_float64(c):
    """Live rows 1, 16, 17, 1025; the case's rows scattered over a larger rollout full of NaN, listed by an index with a count; padding
    columns of obs and of the head hold NaN; ent_coef > 0; rows on both sides of the clip; the same call twice gives the same bytes."""
    case = cf.grad_case(c)
    n = c["rows"]
    eng = _engine(1)
    ref = cf.reference_of(case)
    rng = np.random.default_rng(n)
    n_rows = 2 * n + 5
    where = np.sort(rng.permutation(n_rows)[:n])
    index = np.concatenate([where, rng.integers(0, n_rows, size=7)])   # (entries beyond the count: never followed)
    P = Problem(case, n_rows=n_rows, where=where, index=index, count=n)
    got = _grad(eng, P)
    _check(got, ref, str(c), sum(c["bins"]))
    again = _grad(eng, P)
    assert all(bits_equal(a, b) for a, b in zip(got["raw"], again["raw"]))
    if n > 1:   # without index and count: position = row, the rows in place
        plain = _grad(eng, Problem(case))
        _check(plain, ref, "%s, no index" % (c, ), sum(c["bins"]))


def test_grad_list_forms_no_critic_and_empty():
    eng = _engine(1)
    full = cf.grad_case(cf.LIST_CASE)
    K = sum(full["bins"])
    P = Problem(full, count=cf.LIST_COUNT)   # the rows beyond the count stay in the arrays and are not live
    for j, sel in cf.list_subsets():
        ref = cf.reference_of(cf.subset_case(full, sel))
        rows = -(-(cf.LIST_CASE["rows"] - j) // cf.LIST_MB)
        _check(_grad(eng, P, start=j, stride=cf.LIST_MB, rows=rows), ref, "list: minibatch %d" % j, K)
    case = cf.grad_case(cf.NOCRITIC_CASE)
    _check(_grad(eng, Problem(case), critic=False), cf.reference_of(case, critic=False), "no critic", sum(case["bins"]))
    empty = _grad(eng, Problem(full, count=0))   # n = 0: all zeros
    assert all(bool((t == 0).all()) for t in empty["raw"])


def test_refusals_of_the_row_list_and_gradient_calls():
    """The one tensor check for the new calls: a wrong-shape or host `action_index`, a short or unaligned `work`, a
    host tensor among the rollout's -- refused before the library is called, and nothing is written."""
    import torch
    from pgdrive_amd.engine import PgdArgError
    c = cf.FORWARD_CASES[4]
    case = cf.forward_case(c)
    n = c["rows"]
    eng = _engine(n)
    x, pw, vw = dev(case["x"]), tuple(dev(w) for w in case["policy"]), tuple(dev(w) for w in case["value"])
    rows, count = dev(np.arange(n, dtype=np.int32)), dev(np.array([n], dtype=np.int32))
    act, logp, value = torch.full((n, 1, 2), SENT, device="cuda"), torch.full((n, 1), SENT, device="cuda"), torch.full((n, 1), SENT, device="cuda")
    good = torch.zeros((n, 1, 2), dtype=torch.int32, device="cuda")
    for bad_index in (good[:n - 1], good[..., 0], good.cpu(), good.long()):
        with pytest.raises(PgdArgError):
            eng.mlp_actor_critic_cat_rows(pw, vw, c["bins"], rows, count, act, bad_index, logp, value, 0, 0, obs=x, in_dim=c["in_dim"])
    with pytest.raises(PgdArgError):
        eng.mlp_actor_critic_cat_rows(pw, vw, c["bins"], rows[:n - 1], count, act, good, logp, value, 0, 0, obs=x, in_dim=c["in_dim"])
    with pytest.raises(PgdArgError):
        eng.mlp_actor_critic_cat_rows(pw, vw, c["bins"], rows, None, act, good, logp, value, 0, 0, obs=x, in_dim=c["in_dim"])
    torch.cuda.synchronize()
    assert all(bool((t == SENT).all()) for t in (act, logp, value))
    # the gradient call
    g = cf.GRAD_CASES[1]
    gcase = cf.grad_case(g)
    P = Problem(gcase)
    k, oc, m = g["in_dim"], g["out_cols"], g["rows"]
    ps, vs = shapes(k, oc)
    pg = [torch.full(s, SENT, device="cuda") for s in ps]
    vg = [torch.full(s, SENT, device="cuda") for s in vs]
    stats = torch.full((8, ), SENT, device="cuda")
    need = eng.ppo_cat_work_bytes(k, m)
    work = torch.zeros((need // 4 + 8, ), device="cuda")

    def call(index=P.t["index"], logp_old=P.t["logp_old"], work=work, stats=stats, bins=g["bins"]):
        eng.ppo_grad_cat(P.pw, P.vw, pg, vg, bins, P.t["x"], index, logp_old, P.t["adv"], P.t["ret"], stats, work, in_dim=k)

    for kw in (dict(index=P.t["index"][:, 0]), dict(index=P.t["index"][:m - 1]), dict(index=P.t["index"].cpu()), dict(index=P.t["index"].float()),
               dict(work=work[:need // 4 - 4]), dict(work=work[1:]), dict(work=work.cpu()), dict(logp_old=P.t["logp_old"].cpu()),
               dict(stats=stats[:7])):
        with pytest.raises(PgdArgError):
            call(**kw)
    with pytest.raises(ValueError):
        call(bins=(9, 9))
    torch.cuda.synchronize()
    assert all(bool((t == SENT).all()) for t in [stats] + pg + vg)
    call()   # (and the same arguments, unbroken, are accepted)
    eng.sync()
    assert float(stats[0]) == m


# ---------------------------------------------------------------------------------------------------------------------
# 5. the observation binding
# ---------------------------------------------------------------------------------------------------------------------
def test_bound_launches_equal_unbound_launches_on_normalised_rows():
    import torch
    c = cf.GRAD_CASES[2]   # 17 rows, in_dim 416
    case = cf.grad_case(c)
    k, n = c["in_dim"], c["rows"]
    eng = _engine(n)
    kp = (k + 3) & ~3
    rng = np.random.default_rng(5)
    table = np.zeros((2, kp), dtype=np.float32)
    table[0, :k], table[1, :k] = rng.normal(0.5, 0.2, size=k), rng.uniform(0.5, 2.0, size=k)
    clip = np.float32(1.5)
    raw = case["x"].copy()
    pre = raw.copy()
    pre[:, :k] = np.clip((raw[:, :k] - table[0, :k]) * table[1, :k], -clip, clip)   # one fp32 subtraction, one fp32 multiplication
    pw, vw = tuple(dev(w) for w in case["policy"]), tuple(dev(w) for w in case["value"])
    want_f = _forward(eng, dev(pre), pw, vw, c["bins"], 9, 4)
    pre_case = dict(case, x=pre)
    want_g = _grad(eng, Problem(pre_case))
    tab = dev(table)
    eng.obs_norm_bind(tab, k, float(clip))
    try:
        got_f = _forward(eng, dev(raw), pw, vw, c["bins"], 9, 4)
        got_g = _grad(eng, Problem(case))
    finally:
        eng.obs_norm_bind(None)
    assert all(bits_equal(a, b) for a, b in zip(got_f, want_f))
    assert all(bits_equal(a, b) for a, b in zip(got_g["raw"], want_g["raw"]))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# 6. collectors and learner
# ---------------------------------------------------------------------------------------------------------------------
N_ENVS, T_STEPS, BINS = 64, 8, (5, 5)


def _cat_networks(D, out_cols=10, seed=0):
    rng = np.random.default_rng(seed)
    p, v = cf.make_networks(rng, D, out_cols, sum(BINS))
    p[4][:, :sum(BINS)] *= np.float32(0.2)   # (near-uniform heads: every bin is drawn)
    return tuple(dev(np.nan_to_num(w)) for w in p), tuple(dev(w) for w in v)


def _single(discrete, gaussian=False, **kw):
    from pgdrive_amd.rollout import RolloutCollector
    eng = tu.ego_engine(load_descs(), N_ENVS, auto_reset=1, horizon=5, seed=5, discrete_action=discrete, discrete_steering_dim=BINS[0],
                        discrete_throttle_dim=BINS[1])
    eng.reset(np.arange(N_ENVS) % 4)
    eng.sync()
    if gaussian:
        S = type("S", (), {})()
        tu._networks(S, eng.D)
        return eng, RolloutCollector(eng, S.pw, S.vw, T_STEPS, seed=3, **kw), S.pw, S.vw
    pw, vw = _cat_networks(eng.D)
    return eng, RolloutCollector(eng, pw, vw, T_STEPS, seed=3, action_head="categorical", bins=BINS, **kw), pw, vw


@pytest.mark.parametrize("discrete", [False, True], ids=["grid_value_on_a_continuous_engine", "emit_index_on_a_discrete_engine"])
def test_collect_equals_the_engine_calls_by_hand(discrete):
    """collect() twice against step, mlp_actor_critic_cat, gae made one at a time into fresh buffers (the carry of row T included)."""
    import torch
    eng, col, pw, vw = _single(discrete)
    assert col.emit_index == discrete
    first = eng.obs.view(N_ENVS, -1).clone()
    got = [tu.snapshot(col.collect(), tu.KEYS + ("action_index", )) for _ in range(2)]
    # the same engine again, by hand
    eng2 = tu.ego_engine(load_descs(), N_ENVS, auto_reset=1, horizon=5, seed=5, discrete_action=discrete, discrete_steering_dim=BINS[0],
                         discrete_throttle_dim=BINS[1])
    eng2.reset(np.arange(N_ENVS) % 4)
    eng2.sync()
    assert bits_equal(eng2.obs.view(N_ENVS, -1), first)

    def evaluate(obs, tick):
        a, i = torch.full((N_ENVS, 1, 2), SENT, device="cuda"), torch.full((N_ENVS, 1, 2), -7, dtype=torch.int32, device="cuda")
        lp, v = torch.full((N_ENVS, 1), SENT, device="cuda"), torch.full((N_ENVS, 1), SENT, device="cuda")
        eng2.mlp_actor_critic_cat(pw, vw, BINS, a, i, lp, v, 3, tick, obs=obs, emit_index=discrete)
        torch.cuda.synchronize()
        return a, i, lp, v

    obs = eng2.obs.clone()
    a, i, lp, v = evaluate(obs, 0)
    for k in range(2):
        rec = {key: [] for key in tu.KEYS[:7] + ("action_index", )}
        for t in range(T_STEPS):
            for key, x in (("obs", obs.view(N_ENVS, -1)), ("actions", a.view(N_ENVS, 2)), ("action_index", i.view(N_ENVS, 2)),
                           ("logp", lp.view(N_ENVS)), ("values", v.view(N_ENVS))):
                rec[key].append(x)
            obs, rew, done, flags = eng2.step(a, out=eng2.make_outputs())
            torch.cuda.synchronize()
            for key, x in (("rewards", rew), ("dones", done), ("flags", flags)):
                rec[key].append(x.view(N_ENVS))
            a, i, lp, v = evaluate(obs, k * T_STEPS + t + 1)
        rec["values"].append(v.view(N_ENVS))
        want = {key: torch.stack(x) for key, x in rec.items()}
        want["advantages"], want["returns"] = eng2.gae(want["rewards"], want["values"], want["dones"], 0.99, 0.95)
        torch.cuda.synchronize()
        tu.assert_same(got[k], want, "rollout %d" % k, need=tu.KEYS + ("action_index", ))
        idx = got[k]["action_index"].cpu().numpy()
        assert idx.min() == 0 and idx.max() == BINS[0] - 1   # every env drew, inside the heads
        if discrete:
            assert bits_equal(got[k]["actions"], got[k]["action_index"].float())
        else:
            assert (tu.np_bits(got[k]["actions"].cpu().numpy()) == tu.np_bits(cf.grid_value(idx, BINS[0]))).all()


def test_captured_iteration_equals_eager_and_draws_new_indices():
    """collect(); update() eagerly four times on one engine; on a twin: once eagerly, then captured and replayed three times."""
    import torch
    from pgdrive_amd.learner import PPOLearner
    keys = ("action_index", "actions", "logp", "values", "rewards", "advantages")

    def build():
        eng, col, _, _ = _single(False, episode_stats=True)
        L = PPOLearner(col, ent_coef=0.01, **tu.LEARN_KW)
        col.prime()
        return col, L

    col, L = build()
    want = []
    for _ in range(4):
        batch = col.collect()
        L.update(batch)
        want.append(dict(tu.snapshot(batch, keys), params=L.params.clone(), stats=L.stats.clone()))
    assert not bits_equal(want[1]["action_index"], want[2]["action_index"])   # new indices per iteration
    assert bool(torch.isfinite(want[3]["params"]).all()) and not bits_equal(want[0]["params"], want[3]["params"])
    col2, L2 = build()

    def iteration():
        L2.update(col2.collect())

    def state():
        torch.cuda.synchronize()
        return dict({k: col2.batch[k].clone() for k in keys}, params=L2.params.clone(), stats=L2.stats.clone())

    tu.eager_then_graph(iteration, state, want, replays=3, need=keys + ("params", "stats"))
    assert col2.episode_summary()["steps"] == 4 * T_STEPS * N_ENVS


def test_multi_agent_collector_on_the_roundabout():
    import torch
    from pgdrive_amd.learner import PPOLearner
    from pgdrive_amd.rollout import MultiAgentRolloutCollector
    class FourEnvs(tu.Roundabout):
        N, CUT_ENVS = 4, (2, 3)

    S = FourEnvs(T=T_STEPS)
    eng = S.eng
    pw, vw = _cat_networks(eng.D)
    col = MultiAgentRolloutCollector(eng, pw, vw, T_STEPS, seed=3, action_head="categorical", bins=BINS)
    L = PPOLearner(col, **tu.LEARN_KW)
    before = L.params.clone()
    batch = col.collect()
    L.update(batch)
    torch.cuda.synchronize()
    mask = batch["mask"].bool()
    idx = batch["action_index"]
    assert int(mask.sum()) > 0 and int(batch["count"]) == int(mask.sum())
    assert bool((idx[~mask] == 0).all()) and bool((batch["logp"][~mask] == 0).all())   # seats that are not due: cleared
    assert int(idx[mask].min()) >= 0 and int(idx[mask].max()) == BINS[0] - 1 and bool((batch["logp"][mask] < 0).all())
    want = cf.grid_value(idx.cpu().numpy(), BINS[0])
    want[~mask.cpu().numpy()] = 0.0
    assert (tu.np_bits(batch["actions"].cpu().numpy()) == tu.np_bits(want)).all()
    assert bool(torch.isfinite(L.params).all()) and not bits_equal(before, L.params)
    assert float(L.stats[0, 0]) > 0 and 0.0 < float(L.stats[0, 3]) <= np.log(BINS[0]) + np.log(BINS[1]) + 1e-5   # mean entropy of two heads


def test_gaussian_collectors_keep_their_bytes_next_to_a_categorical_one():
    """A Gaussian collector run after the categorical entry points were used in the same process, against a second Gaussian collector on a
    twin engine that ran first: the same bytes."""
    import warnings
    _, first, _, _ = _single(False, gaussian=True)
    a = tu.snapshot(first.collect(), tu.KEYS)
    _, cat, _, _ = _single(False)
    cat.collect()
    _, second, _, _ = _single(False, gaussian=True)
    b = tu.snapshot(second.collect(), tu.KEYS)
    tu.assert_same(b, a, "the Gaussian collector behind a categorical one", need=tu.KEYS)
    assert "action_index" not in second.batch
    with warnings.catch_warnings(record=True) as seen:   # a discrete engine with the Gaussian head: today's behaviour, one warning
        warnings.simplefilter("always")
        _, disc, _, _ = _single(True, gaussian=True)
    assert len(seen) == 1 and "categorical" in str(seen[0].message)
    assert bool(np.isfinite(disc.collect()["rewards"].cpu().numpy()).all())


def test_target_kl_stops_on_a_batch_that_exceeds_it():
    """logp_old shifted by +1 in every row: the first minibatch's estimate mean(logp_old - logp) is 1 > 1.5 x 0.1, so no step is applied."""
    import torch
    from pgdrive_amd import _abi
    from pgdrive_amd.learner import PPOLearner
    eng, col, _, _ = _single(False)
    L = PPOLearner(col, target_kl=0.1, epochs=2, minibatches=2, lr=3e-4)
    batch = dict(col.collect())
    batch["logp"] = batch["logp"] + 1.0
    before = L.params.clone()
    stats = L.update(batch)
    torch.cuda.synchronize()
    gate = dict(zip(_abi.ADAM_GATE, L.gate.cpu().numpy().tolist()))
    assert gate["stopped"] == 1 and gate["applied"] == 0 and bits_equal(before, L.params)
    assert abs(float(stats[0, 4]) - 1.0) < 1e-4 and float(stats[1, 0]) == 0.0   # the first minibatch's estimate; the later calls find no live row


def test_ten_steps_raise_the_probability_of_the_rewarded_bin():
    """One fixed minibatch whose advantages are positive exactly where steering index k was taken: ten ppo_grad_cat + adam steps raise the
    mean p_k.  Deterministic, no environment in the loop."""
    import torch
    from pgdrive_amd.learner import flat_layout
    eng = _engine(1)
    c = dict(rows=64, in_dim=35, bins=(5, 5), out_cols=10, scaling="unit", seed=9, normalise=False)
    case = cf.grad_case(c)
    k_bin, n, in_dim = 3, c["rows"], c["in_dim"]
    adv = np.where(case["index"][:, 0] == k_bin, 1.0, -0.25).astype(np.float32)
    assert 0 < (adv > 0).sum() < n
    layout, total = flat_layout(in_dim, c["out_cols"])
    params, grads, m, v = [torch.zeros(total, device="cuda") for _ in range(4)]
    views = lambda flat: tuple(flat[o:o + int(np.prod(s))].view(s) for _, s, o in layout)  # noqa: E731
    wv, gv = views(params), views(grads)
    for dst, src in zip(wv, list(case["policy"]) + list(case["value"])):
        dst.copy_(dev(np.nan_to_num(src)).view(dst.shape))
    x, idx, ret = dev(case["x"]), dev(case["index"]), dev(case["ret"])
    step = torch.zeros(4, dtype=torch.int32, device="cuda")
    stats = torch.zeros(8, device="cuda")
    work = torch.empty((eng.ppo_cat_work_bytes(in_dim, n) + 3) // 4, device="cuda")

    def mean_pk():
        w = [t.cpu().numpy() for t in wv[:6]]
        _, _, l = cf.logits_f64(case["x"], w, c["bins"])
        return float(cf.head_f64(l[:, :5])[1][:, k_bin].mean()), l

    p0, l = mean_pk()
    logp_old = dev(cf.row_terms_f64(l, case["index"], np.zeros(n), adv, None, cf.CLIP, c["bins"])[1].astype(np.float32))
    for _ in range(10):
        eng.ppo_grad_cat(wv[:6], wv[6:], gv[:6], gv[6:], c["bins"], x, idx, logp_old, dev(adv), ret, stats, work, in_dim=in_dim)
        eng.adam(params, grads, m, v, step, 1e-3, eps=1e-5, max_grad_norm=0.5)
    eng.sync()
    torch.cuda.synchronize()
    p1, _ = mean_pk()
    print("mean p_k: %.4f -> %.4f" % (p0, p1))
    assert bool(torch.isfinite(params).all()) and p1 > p0 + 1e-3
