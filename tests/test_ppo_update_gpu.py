"""pgd_ppo_grad, pgd_adv_stats, pgd_adam (pgdrive_amd/csrc/pgd_ppo.h) and pgdrive_amd.learner.PPOLearner on the device, against the float64
restatement of tests/ppo_ref.py:

* gradients and statistics at every width and row count of the checker's cases, out_cols 4, 5, 6 with NaN in the unused head columns,
  both input scalings; plain, and through a permuted index with the count read from device memory;
* the list forms: strided splits whose n_j-weighted gradients give the full-list gradient, an empty minibatch;
* NaN in every unlisted row of every array, garbage in the list behind the count, NaN in the observation columns behind in_dim;
* no critic (the critic's gradient buffers keep their sentinel); the same bytes twice;
* pgd_adv_stats and pgd_adam (three eager steps against float64; the same three steps as replays of a one-step graph, bit for bit);
* the closed loop: PPOLearner.update against the same Engine calls made by hand, collect + update from a HIP graph, the loss going
  down; a multi-agent rollout whose minibatches the host recomputes from the mask.

Errors are normalised per entry as tests/ppo_ref.py describes.  Tolerances, each twice what the float32 emulation of the kernels'
summation order measures over the same cases (tests/test_ppo_update_cpu.py): gradients / statistics by the minibatch's live rows -- fewer
than 16: 1.03e-6 / 1.64e-6; 16 to 1023: 2.57e-7 / 4.30e-7; 1024 and more: 8.26e-8 / 6.45e-8 --, TOL_ADV 2.30e-7, TOL_ADAM 6.92e-6.
"""
import numpy as np
import pytest

from tests import actor_critic_ref as ar
from tests import ppo_ref as rf
from tests.ppo_util import Problem as _Problem, check as _check, grad as _grad, shapes as _shapes
from tests.train_util import ERR_ARG, EVERY_LEARNER, SENT, Traffic, assert_same, dev as _dev, eager_then_graph, ego_engine, learner_state, make_collector, update_by_hand

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(descs):
    """One env, ego only, no lidar: the update kernels need the engine for its device and stream only."""
    e = ego_engine(descs, 1)
    yield e
    e.close()


def _weighted_sum_equals(parts, full, ref_full, what):
    """sum_j n_j g_j / n against the device's gradient g of the whole list.  Every g_j is within its tolerance times norm_j of float64 and
    sum_j n_j norm_j = n norm (the norms are sums over rows, too), so the weighted sum is within the largest of the parts' tolerances
    times norm of float64; g is within its own."""
    n = sum(n_j for n_j, _ in parts)
    assert n == int(ref_full["stats"][0])
    tol = max(rf.tolerances(n_j)[0] for n_j, _ in parts if n_j) + rf.tolerances(n)[0]
    total = [np.zeros(q.shape) for q in full["policy"] + full["value"]]
    for n_j, g in parts:
        for acc, q in zip(total, g["policy"] + g["value"]):
            acc += n_j * q.astype(np.float64)
    worst = 0.0
    for acc, w, nrm in zip(total, full["policy"] + full["value"], ref_full["policy_norm"] + ref_full["value_norm"]):
        err = np.abs(acc / n - w)
        assert (err <= tol * nrm).all(), (what, float((err / (nrm + 1e-300)).max()), tol)
        worst = max(worst, float((err / (nrm + 1e-300)).max()))
    print("%s: weighted sum of the parts against the whole: %.3f of %.2e" % (what, worst / tol, tol))


def _listed(case, seed):
    """The case's rows scattered over a larger rollout behind a permuted index; the list is longer than its count, and what lies behind
    the count is garbage."""
    rows = case["x"].shape[0]
    rng = np.random.default_rng(seed)
    n_rows = 2 * rows + 5
    where = rng.permutation(n_rows)[:rows]
    index = np.concatenate([where, [0x7fffffff, -5, n_rows, 1 << 20, -(1 << 30), 3, 0, 1, 2]]).astype(np.int32)
    return _Problem(case, n_rows=n_rows, where=where, index=index, count=rows)


# ---------------------------------------------------------------------------------------------------------------------
# gradients and statistics against float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_dim", rf.WIDTHS)
def test_width_sweep(eng, in_dim):
    """Every width in both scalings, out_cols cycling through 4, 5, 6 (NaN in the unused head columns), NaN behind in_dim in every row."""
    for c in rf.sweep_cases():
        if c["in_dim"] != in_dim:
            continue
        case, ref = rf.case_and_reference(c)
        assert c["out_cols"] == 4 or np.isnan(case["policy"][4][:, 4:]).all()
        _check(_grad(eng, _Problem(case)), ref, str(c))


@pytest.mark.parametrize("rows", rf.ROW_COUNTS)
def test_row_counts_plain_and_listed(eng, rows):
    """1 .. 1027 rows (the last tile partly empty; 1027 crosses the partition of 1024 rows): index null, and the same rows behind a permuted
    index with the count in device memory, a grid larger than the count, NaN in every unlisted row and garbage behind the count."""
    for c in rf.row_cases():
        if c["rows"] != rows:
            continue
        case, ref = rf.case_and_reference(c)
        plain = _grad(eng, _Problem(case))
        _check(plain, ref, "plain %s" % c)
        listed = _grad(eng, _listed(case, rows))
        _check(listed, ref, "listed %s" % c)
        # the same rows in the same order: the same bits, wherever they lie in the rollout
        for a, b in zip(plain["raw"], listed["raw"]):
            assert np.array_equal(a.cpu().numpy().view(np.int32), b.cpu().numpy().view(np.int32))


def test_strided_splits_sum_to_the_full_list_and_an_empty_minibatch_is_zero(eng):
    """The first `count` rows of one case behind a permuted index, the count in device memory: the whole list, and its split into 3 and
    into 7 strided minibatches -- each against float64 over its own rows, and sum_j n_j g_j / n against the device's full-list gradient.
    Count 5 in 7 minibatches: minibatches of one row, and empty ones whose outputs are exactly zero."""
    case, _ = rf.case_and_reference(rf.LIST_CASE)
    P = _listed(case, 9)
    got, refs = {}, {}
    for count, n_mb, j, sel in rf.list_subsets():
        P.count = _dev(np.array([count], dtype=np.int32))
        g = _grad(eng, P, start=j, stride=n_mb, rows=max(1, -(-(P.n_list - j) // n_mb)))
        assert g["stats"][0] == len(sel)
        if len(sel) == 0:
            for q in g["policy"] + g["value"]:
                assert (q == 0).all()
            assert (g["stats"] == 0).all()
        else:
            refs[(count, n_mb, j)] = rf.reference_of(rf.subset_case(case, sel))
            _check(g, refs[(count, n_mb, j)], "count %d, minibatch %d of %d" % (count, j, n_mb))
        got[(count, n_mb, j)] = (len(sel), g)
    assert any(n == 0 for n, _ in got.values()) and any(n == 1 for n, _ in got.values())
    for count in rf.LIST_COUNTS:
        for n_mb in rf.LIST_MB:
            _weighted_sum_equals([got[(count, n_mb, j)] for j in range(n_mb)], got[(count, 1, 0)][1], refs[(count, 1, 0)],
                                 "count %d in %d" % (count, n_mb))
    P.count = _dev(np.array([0], dtype=np.int32))  # nothing is live anywhere
    g = _grad(eng, P)
    for q in g["policy"] + g["value"]:
        assert (q == 0).all()
    assert (g["stats"] == 0).all()


def test_partitions_of_the_row_reduction(eng):
    """2049 rows: three partitions of the weight-gradient reduction, plain and behind an index (the same bits).  And the 1027 rows of the
    row-count case, whose 1024th row ends a partition, against their two strided halves of 514 and 513 rows, which have no partition
    boundary inside: a row lost or taken twice at a boundary shows in the weighted sum."""
    case, ref = rf.case_and_reference(rf.PART_CASE)
    plain = _grad(eng, _Problem(case))
    _check(plain, ref, "plain %s" % rf.PART_CASE)
    listed = _grad(eng, _listed(case, 5))
    for a, b in zip(plain["raw"], listed["raw"]):
        assert np.array_equal(a.cpu().numpy().view(np.int32), b.cpu().numpy().view(np.int32))
    case, ref = rf.case_and_reference(rf.SPLIT_CASE)
    P = _listed(case, 6)
    whole = _grad(eng, P)
    _check(whole, ref, "the 1027 rows")
    parts = []
    for j in range(rf.SPLIT_MB):
        sel = np.arange(j, rf.SPLIT_CASE["rows"], rf.SPLIT_MB)
        g = _grad(eng, P, start=j, stride=rf.SPLIT_MB, rows=-(-(P.n_list - j) // rf.SPLIT_MB))
        _check(g, rf.reference_of(rf.subset_case(case, sel)), "half %d of the 1027 rows" % j)
        parts.append((len(sel), g))
    _weighted_sum_equals(parts, whole, ref, "1027 rows in 2")


def test_the_first_call_of_a_fresh_engine_is_capturable(descs):
    """Nothing is allocated inside pgd_ppo_grad and the scratch is the caller's: its very first call on an engine, at a width whose LDS
    lies above the default limit (274 inputs: 56,704 bytes), is made inside a graph capture; the replay gives the eager call's bytes."""
    import torch
    from pgdrive_amd import _abi
    from pgdrive_amd.engine import Engine
    from tests import util
    c = [c for c in rf.row_cases() if c["rows"] == 33][0]
    case, ref = rf.case_and_reference(c)
    k = c["in_dim"]
    assert rf.ar.lds_bytes(k) + 1024 > 49152
    mb, sb = util.make_banks(descs, n_maps=4, num_traffic=0)
    fresh = Engine(_abi.make_config(1, num_agents=1, num_traffic=0, num_lasers=0, seed=2), mb, sb)
    try:
        P = _Problem(case)
        ps, vs = _shapes(k, case["policy"][4].shape[1])
        pg, vg = [torch.full(s, SENT, device="cuda") for s in ps], [torch.full(s, SENT, device="cuda") for s in vs]
        stats = torch.full((8, ), SENT, device="cuda")
        work = torch.empty(fresh.ppo_work_bytes(k, c["rows"]) // 4 + 1, device="cuda")
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()   # (its own capture: the first call on a fresh engine is made inside the capture, nothing runs eagerly in front)
        with torch.cuda.graph(graph, stream=s):
            fresh.ppo_grad(P.pw, P.vw, pg, vg, P.t["x"], P.t["action"], P.t["logp_old"], P.t["adv"], P.t["ret"], stats, work, in_dim=k,
                           adv_stats=P.stats_in, clip=rf.CLIP, vf_coef=rf.VF_COEF, ent_coef=rf.ENT_COEF)
        torch.cuda.synchronize()
        assert bool((stats == SENT).all()), "the capture itself ran the kernels"
        with torch.cuda.stream(s):
            graph.replay()
        torch.cuda.synchronize()
        got = dict(stats=stats.cpu().numpy(), policy=[g.cpu().numpy() for g in pg], value=[g.cpu().numpy() for g in vg])
        _check(got, ref, "first call, captured")
        eager = _grad(fresh, P)
        for a, b in zip(eager["raw"], [stats] + pg + vg):
            assert torch.equal(a, b), "the replay of the captured first call differs from the eager call"
        del graph
    finally:
        fresh.close()


def test_no_critic_and_the_same_bytes_twice(eng):
    import torch
    case, _ = rf.case_and_reference(rf.NOCRITIC_CASE)
    ref = rf.reference_of(case, critic=False)
    P = _listed(case, 3)
    got = _grad(eng, P, critic=False)
    for g in got["value"]:
        assert (g == SENT).all(), "no critic, but a critic gradient buffer was written"
    assert got["stats"][2] == 0.0
    got_cmp = dict(stats=got["stats"], policy=got["policy"], value=None)
    _check(got_cmp, ref, "no critic")
    with_critic = _grad(eng, P)
    for a, b in zip(with_critic["raw"][1:7], got["raw"][1:7]):
        assert torch.equal(a, b), "the actor's gradient depends on the critic's presence"
    again = _grad(eng, P)
    for a, b in zip(with_critic["raw"], again["raw"]):
        assert torch.equal(a, b), "not the same bytes twice"
    # a scratch that is one byte too small, a misaligned one: PGD_ERR_ARG and nothing written; shapes the call refuses have no scratch size
    assert _grad(eng, P, short_by=1, expect=ERR_ARG) is None
    assert _grad(eng, P, shift=1, expect=ERR_ARG) is None
    assert eng.L.pgd_ppo_work_bytes(417, 16, 1) == 0 and eng.L.pgd_ppo_work_bytes(3, 16, 1) == 0 and eng.L.pgd_ppo_work_bytes(35, 0, 1) == 0
    assert eng.L.pgd_ppo_work_bytes(416, 16, 1) > eng.L.pgd_ppo_work_bytes(416, 16, 0) > 0


# ---------------------------------------------------------------------------------------------------------------------
# pgd_adv_stats, pgd_adam
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_index", [False, True])
def test_adv_stats(eng, with_index):
    import torch
    for n in rf.ADV_COUNTS:
        adv, index, n_list = rf.build_adv(n, with_index)
        live = adv[:n] if index is None else adv[index[:n]]
        want = rf.adv_stats_f64(live)
        out = torch.full((2, ), SENT, dtype=torch.float32, device="cuda")
        got = eng.adv_stats(_dev(adv), out=out, index=_dev(index) if index is not None else None, count=_dev(np.array([n], dtype=np.int32)),
                            n_list=n_list)
        eng.sync()
        g = got.cpu().numpy().astype(np.float64)
        assert np.isfinite(g).all()
        if n == 0:
            assert g[0] == 0.0 and g[1] == 1.0
            continue
        scale = np.array([np.abs(live.astype(np.float64)).mean(), want[1]])
        err = float((np.abs(g - want) / scale).max())
        print("adv_stats, %d live entries, index %s: %.3f of TOL_ADV" % (n, with_index, err / rf.TOL_ADV))
        assert err < rf.TOL_ADV, (n, with_index, err)
        again = eng.adv_stats(_dev(adv), index=_dev(index) if index is not None else None, count=_dev(np.array([n], dtype=np.int32)), n_list=n_list)
        eng.sync()
        assert torch.equal(again, got)


def test_adam_three_steps_and_three_replays_of_one_graph(eng):
    import torch
    state = {}

    def run(p, g, m, v, t, mx):
        if t == 1:
            state.update(p=_dev(p), m=_dev(m), v=_dev(v), step=torch.zeros(4, dtype=torch.int32, device="cuda"))
        eng.adam(state["p"], _dev(g), state["m"], state["v"], state["step"], max_grad_norm=mx, **rf.ADAM_HYPER)
        eng.sync()
        assert int(state["step"][0]) == t
        return state["p"].cpu().numpy(), state["m"].cpu().numpy(), state["v"].cpu().numpy()

    worst = rf.adam_errors(run)
    print("adam: %.3f of TOL_ADAM (%.2e)" % (worst / rf.TOL_ADAM, worst))
    assert worst < rf.TOL_ADAM
    # the same three steps as three replays of ONE captured step: the step number is read on the device
    for c in (dict(n_elem=1027, mode="above"), dict(n_elem=65, mode="off")):
        p0, g, mx = rf.build_adam(**c)
        eager = dict(p=_dev(p0), m=torch.zeros(c["n_elem"], device="cuda"), v=torch.zeros(c["n_elem"], device="cuda"),
                     step=torch.zeros(4, dtype=torch.int32, device="cuda"))
        for t in range(3):
            eng.adam(eager["p"], _dev(g[t]), eager["m"], eager["v"], eager["step"], max_grad_norm=mx, **rf.ADAM_HYPER)
        eng.sync()
        cap = dict(p=_dev(p0), m=torch.zeros(c["n_elem"], device="cuda"), v=torch.zeros(c["n_elem"], device="cuda"),
                   step=torch.zeros(4, dtype=torch.int32, device="cuda"))
        gbuf = _dev(g[0])
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()   # (its own capture: nothing runs eagerly in front, and the host writes the gradient between the replays)
        with torch.cuda.graph(graph, stream=s):
            eng.adam(cap["p"], gbuf, cap["m"], cap["v"], cap["step"], max_grad_norm=mx, **rf.ADAM_HYPER)
        torch.cuda.synchronize()
        assert int(cap["step"][0]) == 0, "the capture itself took a step"
        with torch.cuda.stream(s):
            for t in range(3):
                gbuf.copy_(_dev(g[t]))
                graph.replay()
        torch.cuda.synchronize()
        for key in ("p", "m", "v", "step"):
            assert torch.equal(eager[key], cap[key]), (c, key)
        assert int(cap["step"][0]) == 3
        del graph


# ---------------------------------------------------------------------------------------------------------------------
# the closed loop
# ---------------------------------------------------------------------------------------------------------------------
CL_N, CL_T, CL_SEED = 8, 8, 3
CL_KW = dict(lr=3e-4, epochs=2, minibatches=2)


def _Single(descs):
    S = Traffic(descs, CL_N, CL_T, CL_SEED)
    S.col = make_collector("single", S)
    return S


def test_single_agent_update_by_hand_from_a_graph_and_into_the_next_rollout(descs):
    import torch
    from pgdrive_amd.learner import PPOLearner
    # (a) update() against the same Engine calls made by hand, over 3 iterations; what the next rollout does with the new weights
    A, B = _Single(descs), _Single(descs)
    LA, LB = PPOLearner(A.col, **CL_KW), PPOLearner(B.col, **CL_KW)
    assert A.col.policy_weights[0].data_ptr() == LA.params.data_ptr(), "the collector does not read the learner's buffer"
    want = []
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        for it in range(3):
            old_p = [w.clone() for w in LA.policy_weights], [w.clone() for w in LA.value_weights]
            batch = A.col.collect()
            stats = LA.update(batch)
            assert stats.shape == (4, 8)
            want.append(learner_state(LA))
            update_by_hand(B.eng, LB, B.col.collect(), **CL_KW)
            assert_same(want[-1], learner_state(LB), "iteration %d, against the calls made by hand" % it, need=EVERY_LEARNER)
            st = stats.cpu().numpy()
            assert np.isfinite(st).all() and (st[:, 0] == CL_T * CL_N // 2).all() and int(LA.step[0]) == 4 * (it + 1)
            assert not torch.equal(old_p[0][0], LA.policy_weights[0]) and not torch.equal(old_p[1][0], LA.value_weights[0])
            if it == 0:
                # the next rollout: row 0 is the carry, evaluated with the OLD weights and not again; row 1 is evaluated with the new ones
                carry_v = A.col.values[CL_T].clone()
            if it == 1:
                assert torch.equal(A.col.values[0], carry_v), "the carry row was evaluated again"
                ev = dict(a=torch.zeros((CL_N, 1, 2), device="cuda"), lp=torch.zeros((CL_N, 1), device="cuda"), v=torch.zeros((CL_N, 1), device="cuda"))
                A.eng.mlp_actor_critic(old_p[0], old_p[1], ev["a"], ev["lp"], ev["v"], CL_SEED, 0, obs=A.col._obs[1], deterministic=True)
                new_v = torch.zeros((CL_N, 1), device="cuda")
                A.eng.mlp_actor_critic(LA.policy_weights, LA.value_weights, ev["a"], ev["lp"], new_v, CL_SEED, 0, obs=A.col._obs[1], deterministic=True)
                torch.cuda.synchronize()
                assert torch.equal(A.col.values[1].view(-1), ev["v"].view(-1)), "row 1 of the rollout was not evaluated with the weights it ran with"
                assert not torch.equal(ev["v"], new_v)
    A.eng.close()
    B.eng.close()
    # (b) one collect() + update() captured in a graph behind one eager iteration, replayed twice
    G = _Single(descs)
    LG = PPOLearner(G.col, **CL_KW)
    eager_then_graph(lambda: LG.update(G.col.collect()), lambda: learner_state(LG), want, need=EVERY_LEARNER)
    G.eng.close()


def test_ten_updates_on_one_minibatch_lower_the_loss(eng):
    """The fixed minibatch of ppo_ref.closed_loop_case(): ten ppo_grad + adam steps lower L, evaluated in float64 from the downloaded
    weights, by at least half of what ten float64 steps do (tests/test_ppo_update_cpu.py measures CLOSED_LOOP_D)."""
    import torch
    from pgdrive_amd import learner
    c = rf.closed_loop_case()
    case = rf.build_case(**c)
    k = c["in_dim"]
    layout, total = learner.flat_layout(k, 4)
    params = torch.zeros(total, device="cuda")
    views = [params[o:o + int(np.prod(sh))].view(sh) for _, sh, o in layout]
    for dst, src in zip(views, list(case["policy"]) + list(case["value"])):
        dst.copy_(_dev(src))
    grads = torch.zeros(total, device="cuda")
    gviews = [grads[o:o + int(np.prod(sh))].view(sh) for _, sh, o in layout]
    m, v, step = torch.zeros(total, device="cuda"), torch.zeros(total, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
    stats = torch.zeros(8, device="cuda")
    work = torch.empty(eng.ppo_work_bytes(k, c["rows"]) // 4 + 1, device="cuda")
    arrays = [_dev(case[q]) for q in ("x", "action", "logp_old", "adv", "ret")]

    def loss():
        torch.cuda.synchronize()
        w = [t.cpu().numpy() for t in views]
        return rf.loss_and_grads_f64(case["x"][:, :k], case["action"], case["logp_old"], case["adv"], case["ret"], w[:6], w[6:], ent_coef=0.0)["loss"]

    first = loss()
    for _ in range(10):
        eng.ppo_grad(views[:6], views[6:], gviews[:6], gviews[6:], arrays[0], arrays[1], arrays[2], arrays[3], arrays[4], stats, work, in_dim=k,
                     ent_coef=0.0)
        eng.adam(params, grads, m, v, step, 3e-4, eps=1e-5, max_grad_norm=0.5)
    last = loss()
    print("ten updates: L %.6f -> %.6f (float64 reference: -%.6f)" % (first, last, rf.CLOSED_LOOP_D))
    assert first - last >= 0.5 * rf.CLOSED_LOOP_D


def test_multi_agent_update_follows_the_device_side_index_and_count():
    """Roundabout, 2 envs, T = 8, one epoch of two minibatches.  update() with batch["index"] / batch["count"] as they lie on the device
    equals, bit for bit, the same launches made by hand with the weights downloaded in front of every minibatch; and what each of those
    launches gives -- statistics and every gradient -- equals loss_and_grads_f64 over the entries the host recomputes from the mask, with
    the weights that minibatch saw.  (The test reads the count for checking; update() never does.)
    These minibatches are the device's own rollout, so no recorded case covers them: the emulation runs on these very rows, and the device
    may be twice as far from float64 as the emulation is there, or as it was on the recorded cases of the same row class if that is more."""
    import torch
    from pgdrive_amd import learner as lm
    from pgdrive_amd.engine import Engine
    from pgdrive_amd.learner import PPOLearner
    from pgdrive_amd.rollout import MultiAgentRolloutCollector
    from tests import util
    N, T, A = 2, 8, 5
    _, mb, sb = util.make_marl_banks(num_agents=A)
    eng = Engine(util.marl_config(N, sb, horizon=40, seed=5), mb, sb)
    try:
        eng.reset(np.arange(N) % len(sb.scenarios))
        p, v = ar.make_networks(np.random.default_rng(0), eng.D, 4)
        p[5][1] = 0.5
        p[5][2:4] += 1.0
        col = MultiAgentRolloutCollector(eng, tuple(_dev(w) for w in p), tuple(_dev(w) for w in v), T, seed=CL_SEED)
        L = PPOLearner(col, lr=3e-4, epochs=1, minibatches=2, ent_coef=0.01)
        batch = col.collect()
        torch.cuda.synchronize()
        # the hand-made twin: its own flat buffers, starting from the learner's weights
        layout, total = lm.flat_layout(eng.D, 4)
        flat = {q: torch.zeros(total, device="cuda") for q in ("p", "g", "m", "v")}
        flat["p"].copy_(L.params)
        views = {q: [flat[q][o:o + int(np.prod(sh))].view(sh) for _, sh, o in layout] for q in ("p", "g")}
        step = torch.zeros(4, dtype=torch.int32, device="cuda")
        stats_update = L.update(batch).clone()
        torch.cuda.synchronize()
        mask = batch["mask"].cpu().numpy().reshape(-1) != 0
        listed = np.flatnonzero(mask)
        count = int(batch["count"][0])
        assert count == len(listed) and count >= 4 and np.array_equal(batch["index"][:count].cpu().numpy(), listed)
        arr = {q: batch[q].cpu().numpy() for q in ("obs", "actions", "logp", "advantages", "returns")}
        obs = arr["obs"].reshape(T * N * A, -1)
        act, lpo, adv, ret = arr["actions"].reshape(-1, 2), arr["logp"].reshape(-1), arr["advantages"].reshape(-1), arr["returns"].reshape(-1)
        s64, s_dev = rf.adv_stats_f64(adv[listed]), L.adv_stats.cpu().numpy()
        scale = np.array([np.abs(adv[listed]).mean(), s64[1]])
        tol_a = 2.0 * max(float((np.abs(rf.emulate_adv_stats(adv[listed]) - s64) / scale).max()), rf.TOL_ADV_MEASURED)
        assert (np.abs(s_dev - s64) / scale).max() < tol_a, (s_dev, s64, tol_a)
        for j in range(2):
            sel = listed[j::2]
            w = [t.cpu().numpy().copy() for t in views["p"]]   # the weights minibatch j sees
            st = torch.zeros(8, device="cuda")
            for g in views["g"]:   # (the views only: the padding between them stays zero, as in the learner's buffer)
                g.fill_(SENT)
            eng.ppo_grad(views["p"][:6], views["p"][6:], views["g"][:6], views["g"][6:], batch["obs"], batch["actions"], batch["logp"],
                         batch["advantages"], batch["returns"], st, L.work, start=j, stride=2, rows=L.plan[j][2], index=batch["index"],
                         count=batch["count"], n_list=L.n_list, adv_stats=L.adv_stats, ent_coef=0.01)
            eng.sync()
            got = dict(stats=st.cpu().numpy(), policy=[g.cpu().numpy() for g in views["g"][:6]], value=[g.cpu().numpy() for g in views["g"][6:]])
            assert np.array_equal(got["stats"], stats_update[j].cpu().numpy()), "minibatch %d: update() saw other statistics" % j
            ref = rf.loss_and_grads_f64(obs[sel], act[sel], lpo[sel], adv[sel], ret[sel], w[:6], w[6:], ent_coef=0.01, adv_stats=s_dev)
            emu = rf.emulate_grads(obs[sel], act[sel], lpo[sel], adv[sel], ret[sel], w[:6], w[6:], ent_coef=0.01, adv_stats=s_dev)
            tol_g, tol_s = [2.0 * max(e, m) for e, m in zip(rf.grad_errors(emu, ref), [t / 2.0 for t in rf.tolerances(len(sel))])]
            eg, es = rf.grad_errors(got, ref)
            print("multi-agent minibatch %d of 2 (%d of %d listed transitions): gradients %.2e (tolerance %.2e), statistics %.2e (%.2e)" % (
                j, len(sel), count, eg, tol_g, es, tol_s))
            assert got["stats"][0] == len(sel) and eg < tol_g and es < tol_s, (j, eg, tol_g, es, tol_s)
            eng.adam(flat["p"], flat["g"], flat["m"], flat["v"], step, 3e-4, eps=1e-5, max_grad_norm=0.5)
        eng.sync()
        assert torch.equal(flat["p"], L.params) and torch.equal(flat["g"], L.grads) and torch.equal(flat["m"], L.m) and torch.equal(step, L.step), \
            "update() is not the launches made by hand"
    finally:
        eng.close()
