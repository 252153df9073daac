"""pgd_ppo_grad_guided (pgdrive_amd/csrc/pgd_guided.h) and the learners' guide= switch on the device, against the float64 restatement of
tests/guided_ref.py:

* no guided row: the gradients and stats[0:8] of pgd_ppo_grad (with and without a critic) and of pgd_ppo_grad_cost, ==;
* every case of guided_ref.guided_cases() -- the widths, the row counts, the mask patterns, target stride 2 and 4 with NaN in what is
  not read, keep_surrogate on and off, bc_coef 0, one to three networks -- against float64: every gradient entry, all twelve statistics;
* mask and target are followed by ROW under a permuted index; guided bits and NaN targets beyond the count change nothing;
* strided splits sum to the whole; a bound normalisation table; the first call of a fresh engine captured, three replays;
* the collector's takeover bits are the rows whose applied action differs from the sampled one; update() of the guided learners against
  the same Engine calls made by hand, eagerly and from a graph; ten guided steps lower bc_loss.  (guide=None makes the parent's
  calls: tests/test_guided_cpu.py, on tests/recording_engine.py.)

Errors are normalised as tests/ppo_ref.py describes.  Tolerances, each twice what the float32 emulation of the kernels' order measures
over the same cases (tests/test_guided_cpu.py): gradients / statistics by the minibatch's live rows -- fewer than 16: 1.66e-6 / 3.27e-7;
16 to 1023: 2.45e-7 / 6.09e-7; 1024 and more: 9.10e-8 / 6.93e-8."""
import os

import numpy as np
import pytest

from tests import guided_ref as gr
from tests import ppo_ref as rf
from tests.train_util import (EVERY_LEARNER, LAGRANGIAN, SENT, Traffic, assert_same, bits_equal, dev, eager_then_graph, ego_engine, learner_state,
                              make_collector)

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "expert_weights.npz")


@pytest.fixture(scope="module")
def eng(descs):
    """One env, ego only, no lidar: the update kernels need the engine for its device and stream only."""
    e = ego_engine(descs, 1)
    yield e
    e.close()


class Problem:
    """The rollout arrays of a guided case on the device: n_rows rows, of which `where` hold the case's rows in minibatch order; every
    other row holds NaN in every float array, `junk_target` in its target and `junk_mask` in its mask byte."""
    def __init__(self, case, n_rows=None, where=None, index=None, count=None, junk_mask=0xff, junk_target=np.nan, mask="case"):
        rows = case["x"].shape[0]
        self.case, self.n_rows = case, rows if n_rows is None else n_rows
        where = np.arange(rows) if where is None else np.asarray(where)

        def scatter(a, fill):
            full = np.full((self.n_rows, ) + a.shape[1:], fill, dtype=a.dtype)
            full[where] = a
            return dev(full)

        self.t = {k: scatter(case[k], np.nan) for k in ("x", "action", "logp_old", "adv", "ret", "cost_ret")}
        self.t["target"] = scatter(case["target"], junk_target)
        m = case["mask"] if isinstance(mask, str) else mask
        self.mask = None if m is None else scatter(m, junk_mask)
        self.index = dev(np.asarray(index, dtype=np.int32)) if index is not None else None
        self.count = dev(np.array([count], dtype=np.int32)) if count is not None else None
        self.n_list = len(index) if index is not None else self.n_rows
        self.stats_in = dev(case["adv_stats"]) if case["adv_stats"] is not None else None
        self.pw, self.vw, self.cw = [tuple(dev(w) for w in case[k]) for k in ("policy", "value", "cost")]


def _shapes(k, oc, critic):
    oc = 1 if critic else oc
    return [(k, 256), (256, ), (256, 256), (256, ), (256, oc), (oc, )]


def run(e, P, call="guided", nets=None, start=0, stride=1, rows=None):
    """One gradient call through the Engine into sentinel-filled buffers -> dict(stats, policy, value, cost: numpy; raw: the tensors).
    call: "guided" (pgd_ppo_grad_guided with the case's switches) or "plain" (pgd_ppo_grad; with three networks pgd_ppo_grad_cost)."""
    import torch
    c = P.case
    nets = c["nets"] if nets is None else nets
    k, oc = c["in_dim"], c["policy"][4].shape[1]
    rows = P.n_list if rows is None else rows
    need = e.ppo_cost_work_bytes(k, rows) if nets == 3 else e.ppo_work_bytes(k, rows, nets == 2)
    assert need > 0
    g = {name: [torch.full(s, SENT, dtype=torch.float32, device="cuda") for s in _shapes(k, oc, name != "policy")] for name in ("policy", "value", "cost")}
    stats = torch.full((12 if call == "guided" else 8, ), SENT, dtype=torch.float32, device="cuda")
    work = torch.full(((need + 3) // 4, ), float("nan"), dtype=torch.float32, device="cuda")
    mb = dict(start=start, stride=stride, rows=rows, index=P.index, count=P.count, n_list=P.n_list, adv_stats=P.stats_in, clip=rf.CLIP,
              vf_coef=rf.VF_COEF, ent_coef=rf.ENT_COEF, in_dim=k)
    t, vw = P.t, P.vw if nets >= 2 else None
    if call == "guided":
        cost = dict(cost_weights=P.cw, cost_grads=g["cost"], cost_ret=t["cost_ret"], cvf_coef=gr.CVF_COEF) if nets == 3 else {}
        e.ppo_grad_guided(P.pw, vw, g["policy"], g["value"], t["x"], t["action"], t["logp_old"], t["adv"], t["ret"], stats, work, t["target"],
                          mask=P.mask, mask_bits=c["mask_bits"], bc_coef=c["bc_coef"], keep_surrogate=c["keep"], **cost, **mb)
    elif nets == 3:
        e.ppo_grad_cost(P.pw, vw, P.cw, g["policy"], g["value"], g["cost"], t["x"], t["action"], t["logp_old"], t["adv"], t["ret"], t["cost_ret"],
                        stats, work, cvf_coef=gr.CVF_COEF, **mb)
    else:
        e.ppo_grad(P.pw, vw, g["policy"], g["value"], t["x"], t["action"], t["logp_old"], t["adv"], t["ret"], stats, work, **mb)
    e.sync()
    out = dict(stats=stats.cpu().numpy(), raw=[stats] + g["policy"] + g["value"] + g["cost"])
    for i, name in enumerate(("policy", "value", "cost")):
        out[name] = [q.cpu().numpy() for q in g[name]]
        written = i < nets
        for q in out[name]:
            assert (not (q == SENT).any()) if written else (q == SENT).all(), "%s: gradient buffers %s" % (name, "not written" if written else "touched")
    return out


def check(got, ref, what):
    """Every gradient entry of every network and the twelve statistics against float64, under the tolerances of the minibatch's row class."""
    eg, es = gr.grad_errors(got, ref)
    tol_g, tol_s = gr.tolerances(int(ref["stats"][0]))
    print("%s: gradients %.3f of %.2e, statistics %.3f of %.2e; stats %s" % (what, eg / tol_g, tol_g, es / tol_s, tol_s, got["stats"]))
    assert eg < tol_g and es < tol_s, (what, eg, tol_g, es, tol_s)
    assert (got["policy"][4][:, 4:] == 0).all() and (got["policy"][5][4:] == 0).all(), (what, "unused head columns")


def same_bits(a, b, what, n=None):
    for i, (x, y) in enumerate(zip(a["raw"][:n], b["raw"][:n])):
        assert bits_equal(x, y), "%s: output %d differs" % (what, i)


def _pattern_case(pattern):
    return [c for c in gr.guided_cases() if c["pattern"] == pattern and c["base"]["name"] == "guided-pattern"][0]


# ---------------------------------------------------------------------------------------------------------------------
# 1. no guided row
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nets", [1, 2, 3])
def test_no_guided_row_gives_the_plain_calls_bits(eng, nets):
    """A mask of zeros, and mask bytes 2, 4, 6 under mask_bits 1, with NaN in every target: gradients and stats[0:8] == pgd_ppo_grad
    (without and with a critic) and pgd_ppo_grad_cost; n_g and bc_loss are zero."""
    for pattern in ("none", "bytes246_bits1"):
        case, _ = gr.case_and_reference(_pattern_case(pattern))
        assert not case["guided"].any() and np.isnan(case["target"]).all()
        P = Problem(case)
        guided, plain = run(eng, P, nets=nets), run(eng, P, "plain", nets=nets)
        assert np.array_equal(guided["stats"][:8].view(np.uint32), plain["stats"].view(np.uint32)) and (guided["stats"][8:] == 0).all()
        assert guided["stats"][0] == 33 and (nets < 3) == (guided["stats"][7] == 0)
        for x, y in zip(guided["raw"][1:], plain["raw"][1:]):
            assert bits_equal(x, y), "%s, %d networks: a gradient differs from the plain call's" % (pattern, nets)


# ---------------------------------------------------------------------------------------------------------------------
# 2. guided patterns against float64
# ---------------------------------------------------------------------------------------------------------------------
WHOLE_CASES = [c for c in gr.guided_cases() if "split" not in c]


@pytest.mark.parametrize("c", WHOLE_CASES, ids=lambda c: "%s-%d-%d-%s" % (c["base"]["name"], c["base"]["in_dim"], c["base"]["rows"], c["pattern"]))
def test_guided_cases_against_float64(eng, c):
    case, ref = gr.case_and_reference(c)
    got = run(eng, Problem(case))
    check(got, ref, str(c))
    u = case["guided"]
    assert got["stats"][8] == u.sum() and (got["stats"][9] != 0) == bool(u.any())
    if not (~u | case["keep"]).any():
        assert (got["stats"][[1, 4, 5, 6]] == 0).all(), "no row carries the surrogate, but its statistics are not zero"
    same_bits(got, run(eng, Problem(case)), "the same bytes twice")


def test_a_mask_of_ones_is_the_null_mask(eng):
    case, _ = gr.case_and_reference(_pattern_case("null"))
    assert case["mask"] is None
    same_bits(run(eng, Problem(case)), run(eng, Problem(case, mask=np.ones(33, np.uint8))), "mask of ones against the null mask")
    case, _ = gr.case_and_reference(_pattern_case("ones"))
    same_bits(run(eng, Problem(case)), run(eng, Problem(case, mask=None)), "null mask against the mask of ones")


def test_a_bad_guide_is_refused_and_nothing_is_written(eng):
    """The guide's own checks, in the library (PGD_ERR_ARG before any launch: every output keeps its sentinel) and in the Engine."""
    import ctypes as C
    import torch
    from pgdrive_amd import _abi
    from pgdrive_amd.engine import PgdArgError
    case, _ = gr.case_and_reference(_pattern_case("alternating"))
    P = Problem(case)
    k, oc, t = case["in_dim"], case["policy"][4].shape[1], P.t
    pg, vg = [[torch.full(s, SENT, device="cuda") for s in _shapes(k, oc, critic)] for critic in (False, True)]
    stats = torch.full((12, ), SENT, device="cuda")
    work = torch.empty(eng.ppo_work_bytes(k, 33) // 4 + 1, device="cuda")
    nets, _, b, grads, _ = eng._ppo_batch("test", (P.pw, P.vw, None), (pg, vg, None), t["x"], t["action"], t["logp_old"], t["adv"], t["ret"], None,
                                          stats, work, 0, 1, None, None, None, None, P.stats_in, k, n_stats=12)
    hp = _abi.PPOHyper(rf.CLIP, rf.VF_COEF, rf.ENT_COEF)
    good = dict(target=t["target"].data_ptr(), mask=P.mask.data_ptr(), target_stride=4, mask_bits=1, bc_coef=1.0, mode=0)

    def call(gd):
        return eng.L.pgd_ppo_grad_guided(eng.h, C.byref(nets), None, C.byref(b), None, None if gd is None else C.byref(_abi.PPOGuide(**gd)),
                                         C.byref(hp), C.byref(grads), None, C.c_void_p(stats.data_ptr()), C.c_void_p(work.data_ptr()),
                                         work.numel() * 4)

    bad = [None, dict(good, target=None), dict(good, target_stride=1), dict(good, mode=2), dict(good, mode=3), dict(good, bc_coef=-1.0),
           dict(good, bc_coef=float("nan")), dict(good, bc_coef=float("inf")), dict(good, mask_bits=0)]
    for gd in bad:
        assert call(gd) == 1, gd
    cost = _abi.PPOCost(t["cost_ret"].data_ptr(), 0.5)   # a cost without its network
    assert eng.L.pgd_ppo_grad_guided(eng.h, C.byref(nets), None, C.byref(b), C.byref(cost), C.byref(_abi.PPOGuide(**good)), C.byref(hp),
                                     C.byref(grads), None, C.c_void_p(stats.data_ptr()), C.c_void_p(work.data_ptr()), work.numel() * 4) == 1
    eng.sync()
    assert all(bool((q == SENT).all()) for q in [stats] + pg + vg), "a refused call wrote"
    assert call(dict(good, mask=None, mask_bits=0)) == 0 and call(good) == 0   # (mask_bits is not looked at without a mask)
    eng.sync()
    assert float(stats[0]) == 33 and float(stats[8]) == case["guided"].sum()
    args = (P.pw, P.vw, pg, vg, t["x"], t["action"], t["logp_old"], t["adv"], t["ret"], stats, work)
    for kw in (dict(target=t["target"][:, :3].contiguous()), dict(target=t["target"][:16]), dict(target=t["target"].double()),
               dict(target=t["target"], mask=P.mask[:32]), dict(target=t["target"], mask=P.mask.int()), dict(target=t["target"], bc_coef=-0.5),
               dict(target=t["target"], mask=P.mask, mask_bits=0), dict(target=t["target"], mask=P.mask, mask_bits=256),
               dict(target=t["target"], cost_weights=P.cw)):
        with pytest.raises(PgdArgError):
            eng.ppo_grad_guided(*args, in_dim=k, **kw)
    with pytest.raises(PgdArgError):
        eng.ppo_grad_guided(*args[:9], torch.zeros(8, device="cuda"), work, t["target"], in_dim=k)   # eight statistics are the plain calls'


# ---------------------------------------------------------------------------------------------------------------------
# 3. by row, not by position
# ---------------------------------------------------------------------------------------------------------------------
def test_mask_and_target_are_followed_by_row(eng):
    """The 33 rows scattered over 71 behind a permuted index whose count is smaller than the list (garbage behind it): the float64
    reference of the rows in minibatch order, and the bits of the plain layout.  Every row that is not listed -- those the garbage
    entries name among them -- holds a set guided bit and a NaN target in one run, a clear bit and a finite target in the other: ==."""
    c = _pattern_case("bytes246_bits3")
    case, ref = gr.case_and_reference(c)
    assert case["guided"].any() and not case["guided"].all()
    rows, n_rows = 33, 71
    where = np.random.default_rng(11).permutation(n_rows)[:rows]
    index = np.concatenate([where, [0x7fffffff, -5, n_rows, 1 << 20, -(1 << 30), 3, 0, 1, 2]])
    a = run(eng, Problem(case, n_rows, where, index, rows, junk_mask=0xff, junk_target=np.nan), rows=len(index))
    b = run(eng, Problem(case, n_rows, where, index, rows, junk_mask=0, junk_target=0.25), rows=len(index))
    check(a, ref, "behind a permuted index")
    same_bits(a, b, "guided bits and NaN targets on rows beyond the count")
    same_bits(a, run(eng, Problem(case)), "the same rows in the same order, wherever they lie")
    # read by list POSITION the mask would be another one
    scattered = np.full(n_rows, 0xff, np.uint8)
    scattered[where] = case["mask"]
    assert not np.array_equal((scattered[:rows] & 3) != 0, case["guided"])


def test_a_row_without_the_surrogate_takes_nothing_from_its_action_advantage_or_logp_old(eng):
    """keep_surrogate off: NaN in the action, the advantage and the old log-probability of every guided row changes no bit of any output
    (u and s select; nothing is multiplied by zero).  The advantage statistics are the call's argument, so they are the same in both."""
    case, ref = gr.case_and_reference(_pattern_case("alternating"))
    u = case["guided"]
    assert not case["keep"] and u.any() and not u.all()
    poisoned = dict(case)
    for key in ("action", "logp_old", "adv"):
        poisoned[key] = case[key].copy()
        poisoned[key][u] = np.nan
    got = run(eng, Problem(poisoned))
    check(got, ref, "NaN in what a masked row does not read")
    same_bits(got, run(eng, Problem(case)), "NaN in the action, advantage and logp_old of the rows without the surrogate")


# ---------------------------------------------------------------------------------------------------------------------
# 4. strided splits
# ---------------------------------------------------------------------------------------------------------------------
def test_strided_splits_sum_to_the_whole(eng):
    """The 1027 rows with three networks, every other row guided, the surrogate kept: its two strided halves, each against float64 over
    its own rows, and sum_j n_j g_j / n against the device's gradient of the whole -- 1 / n is over all live rows, a guided row does not
    renormalise.  Every g_j is within its tolerance times norm_j of float64 and sum_j n_j norm_j = n norm, so the weighted sum is within
    the largest of the parts' tolerances times norm of float64; the whole is within its own."""
    whole_c = gr.split_whole()
    case, ref = gr.case_and_reference(whole_c)
    P = Problem(case)
    whole = run(eng, P)
    check(whole, ref, "the 1027 rows")
    parts = []
    for j in range(gr.SPLIT_MB):
        sub, sub_ref = gr.case_and_reference(dict(whole_c, split=(j, gr.SPLIT_MB)))
        g = run(eng, P, start=j, stride=gr.SPLIT_MB, rows=-(-(P.n_list - j) // gr.SPLIT_MB))
        check(g, sub_ref, "half %d of the 1027 rows" % j)
        parts.append((sub["x"].shape[0], g))
    n = sum(n_j for n_j, _ in parts)
    assert n == 1027 and sum(g["stats"][8] for _, g in parts) == whole["stats"][8]
    tol = max(gr.tolerances(n_j)[0] for n_j, _ in parts) + gr.tolerances(n)[0]
    worst = 0.0
    for net in ("policy", "value", "cost"):
        for i, (w, nrm) in enumerate(zip(whole[net], ref[net + "_norm"])):
            acc = sum(n_j * g[net][i].astype(np.float64) for n_j, g in parts) / n
            err = np.abs(acc - w).reshape(nrm.shape)
            assert (err <= tol * nrm).all(), (net, i, float((err / (nrm + 1e-300)).max()), tol)
            worst = max(worst, float((err / (nrm + 1e-300)).max()))
    print("weighted sum of the halves against the whole: %.3f of %.2e" % (worst / tol, tol))


# ---------------------------------------------------------------------------------------------------------------------
# 5. the observation binding
# ---------------------------------------------------------------------------------------------------------------------
def test_a_bound_table_equals_the_unbound_call_on_normalised_rows(eng):
    c = [c for c in gr.guided_cases() if c["base"]["in_dim"] == 416][0]
    case, _ = gr.case_and_reference(c)
    k = 416
    rng = np.random.default_rng(5)
    table = np.zeros((2, k), dtype=np.float32)
    table[0], table[1] = rng.normal(0.5, 0.2, size=k), rng.uniform(0.5, 2.0, size=k)
    clip = np.float32(1.5)
    pre = case["x"].copy()
    pre[:, :k] = np.clip((case["x"][:, :k] - table[0]) * table[1], -clip, clip)   # one fp32 subtraction, one fp32 multiplication
    want = run(eng, Problem(dict(case, x=pre)))
    tab = dev(table)
    eng.obs_norm_bind(tab, k, float(clip))
    try:
        got = run(eng, Problem(case))
    finally:
        eng.obs_norm_bind(None)
    same_bits(got, want, "bound table against pre-normalised rows")
    assert not np.array_equal(got["policy"][0], run(eng, Problem(case))["policy"][0])


# ---------------------------------------------------------------------------------------------------------------------
# 6. capture
# ---------------------------------------------------------------------------------------------------------------------
def test_the_first_call_of_a_fresh_engine_is_capturable(descs):
    """Nothing is allocated inside pgd_ppo_grad_guided: its very first call on an engine, three networks at a width whose LDS lies above
    the default limit (274 inputs), is made inside a graph capture; three replays give the same bytes, those of an eager call."""
    import torch
    c = [c for c in gr.guided_cases_rows() if c["base"]["rows"] == 17][0]
    case, ref = gr.case_and_reference(c)
    assert c["nets"] == 3 and rf.ar.lds_bytes(274) + 1024 > 49152
    fresh = ego_engine(descs, 1)
    try:
        P = Problem(case)
        k, oc, t = 274, case["policy"][4].shape[1], P.t
        g = {name: [torch.full(s, SENT, device="cuda") for s in _shapes(k, oc, name != "policy")] for name in ("policy", "value", "cost")}
        stats = torch.full((12, ), SENT, device="cuda")
        work = torch.empty(fresh.ppo_cost_work_bytes(k, 17) // 4 + 1, device="cuda")
        outputs = [stats] + g["policy"] + g["value"] + g["cost"]
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()   # (its own capture: nothing runs eagerly in front)
        with torch.cuda.graph(graph, stream=s):
            fresh.ppo_grad_guided(P.pw, P.vw, g["policy"], g["value"], t["x"], t["action"], t["logp_old"], t["adv"], t["ret"], stats, work,
                                  t["target"], mask=P.mask, mask_bits=case["mask_bits"], bc_coef=case["bc_coef"], keep_surrogate=case["keep"],
                                  cost_weights=P.cw, cost_grads=g["cost"], cost_ret=t["cost_ret"], cvf_coef=gr.CVF_COEF, adv_stats=P.stats_in,
                                  clip=rf.CLIP, vf_coef=rf.VF_COEF, ent_coef=rf.ENT_COEF, in_dim=k)
        torch.cuda.synchronize()
        assert all(bool((q == SENT).all()) for q in outputs), "the capture itself ran the kernels"
        seen = []
        with torch.cuda.stream(s):
            for _ in range(3):
                graph.replay()
                torch.cuda.synchronize()
                seen.append([q.clone() for q in outputs])
                for q in outputs:
                    q.fill_(SENT)
                torch.cuda.synchronize()
        for again in seen[1:]:
            assert all(bits_equal(a, b) for a, b in zip(seen[0], again)), "a replay gave other bytes"
        got = dict(stats=seen[0][0].cpu().numpy(), policy=[q.cpu().numpy() for q in seen[0][1:7]], value=[q.cpu().numpy() for q in seen[0][7:13]],
                   cost=[q.cpu().numpy() for q in seen[0][13:]])
        check(got, ref, "first call, captured")
        eager = run(fresh, P)
        assert all(bits_equal(a, b) for a, b in zip(eager["raw"], seen[0])), "the replay of the captured first call differs from the eager call"
        del graph
    finally:
        fresh.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. the collector's bits
# ---------------------------------------------------------------------------------------------------------------------
COL_N, COL_T, COL_SEED = 16, 8, 3
CL_KW = dict(lr=3e-4, epochs=2, minibatches=2)


def _Col(descs, safe=False):
    """16 envs with traffic, the policy steering to one side (the guardian has something to do), the expert of the fixture at save_level 0.5."""
    return Traffic(descs, COL_N, COL_T, COL_SEED, safe=safe, steer_bias=0.5, expert=FIXTURE)


@pytest.mark.parametrize("immediate", [False, True])
def test_the_takeover_bits_are_the_rows_whose_applied_action_differs(descs, immediate):
    import torch
    from pgdrive_amd.learner import guide_options
    S = _Col(descs)
    try:
        col = make_collector("single", S, guardian=dict(S.guardian, immediate=immediate))
        bits = guide_options("test", "takeover", 1.0, False, col.guardian)["mask_bits"]
        assert bits == (3 if immediate else 1)
        guided_rows = free_rows = 0
        with torch.no_grad():
            for _ in range(2):
                batch = col.collect()
                torch.cuda.synchronize()
                differs = (batch["applied_actions"] != batch["actions"]).any(dim=-1).cpu().numpy()
                guided = (batch["takeover"].cpu().numpy() & bits) != 0
                assert np.array_equal(guided, differs), "immediate=%r: (takeover & %d) != 0 is not the rows whose applied action differs" % (immediate, bits)
                guided_rows, free_rows = guided_rows + int(guided.sum()), free_rows + int((~guided).sum())
        print("immediate=%r: %d guided and %d free env-steps" % (immediate, guided_rows, free_rows))
        assert guided_rows >= 1 and free_rows >= 1
    finally:
        S.eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8. update() by hand
# ---------------------------------------------------------------------------------------------------------------------
def _by_hand(e, L, batch, guide, lagrange, epochs, minibatches, lr):
    """update() of a guided learner restated in Engine calls on L's buffers."""
    n_list = L.n_list
    adv, norm = batch["advantages"], None
    if lagrange:
        e.lagrange(batch["ep_cost_sum"], batch["ep_cost_count"], L.lagrange_state, 1.0, 0.05, 100.0)
        norm = e.adv_stats(adv, out=L.adv_stats)
        cnorm = e.adv_stats(batch["cost_advantages"], out=L.cadv_stats)
        adv, norm = e.adv_mix(adv, batch["cost_advantages"], L.lagrange_state, out=L.mixed, adv_stats=norm, cadv_stats=cnorm), None
    else:
        norm = e.adv_stats(adv, out=L.adv_stats)
    target, mask = (batch["applied_actions"], batch["takeover"]) if guide == "takeover" else (batch["guardian_trace"], None)
    cost = dict(cost_weights=L.cost_weights, cost_grads=L.cost_grads, cost_ret=batch["cost_returns"], cvf_coef=0.5) if lagrange else {}
    k = 0
    for _ in range(epochs):
        for j in range(minibatches):
            e.ppo_grad_guided(L.policy_weights, L.value_weights, L.policy_grads, L.value_grads, batch["obs"], batch["actions"], batch["logp"], adv,
                              batch["returns"], L.stats[k], L.work, target, mask=mask, mask_bits=1, bc_coef=0.5, keep_surrogate=False,
                              start=j, stride=minibatches, rows=-(-(n_list - j) // minibatches), n_list=n_list, adv_stats=norm, **cost)
            e.adam(L.params, L.grads, L.m, L.v, L.step, lr, eps=1e-5, max_grad_norm=0.5)
            k += 1


@pytest.mark.parametrize("kind,guide", [("single", "takeover"), ("single", "all"), ("safe", "takeover")])
def test_guided_update_is_the_engine_calls_made_by_hand(descs, kind, guide):
    import torch
    from pgdrive_amd.learner import PPOLagLearner, PPOLearner
    lag = kind == "safe"

    def make():
        S = _Col(descs, safe=lag)
        S.col = make_collector(kind, S, guardian=S.guardian)
        kw = dict(CL_KW, guide=guide, bc_coef=0.5)
        return S, (PPOLagLearner(S.col, cost_limit=1.0, **kw) if lag else PPOLearner(S.col, **kw))

    need = LAGRANGIAN if lag else EVERY_LEARNER
    (A, LA), (B, LB) = make(), make()
    assert LA.stats.shape == (4, 12)
    want = []
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        for it in range(3):
            stats = LA.update(A.col.collect())
            want.append(learner_state(LA))
            _by_hand(B.eng, LB, B.col.collect(), guide, lag, **CL_KW)
            assert_same(want[-1], learner_state(LB), "iteration %d, against the calls made by hand" % it, need=need)
            st = stats.cpu().numpy()
            assert np.isfinite(st).all() and (st[:, 0] == COL_T * COL_N // 2).all() and int(LA.step[0]) == 4 * (it + 1)
            assert (st[:, 8] == st[:, 0]).all() if guide == "all" else (st[:, 8] <= st[:, 0]).all()
            assert ((st[:, 9] != 0) == (st[:, 8] > 0)).all() and (st[:, 10:] == 0).all()
    A.eng.close()
    B.eng.close()
    G, LG = make()
    eager_then_graph(lambda: LG.update(G.col.collect()), lambda: learner_state(LG), want, need=need)
    G.eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 9. the closed loop
# ---------------------------------------------------------------------------------------------------------------------
def test_ten_guided_steps_lower_bc_loss(eng):
    """guided_ref.loop_case(): ten ppo_grad_guided (every row guided, no surrogate) + adam steps lower bc_loss, evaluated in float64 from
    the downloaded weights, by at least half of what ten float64 steps do (tests/test_guided_cpu.py measures GUIDED_LOOP_D)."""
    import torch
    from pgdrive_amd import learner
    case = gr.loop_case()
    k, n = case["in_dim"], case["x"].shape[0]
    layout, total = learner.flat_layout(k, 4)
    params, grads = torch.zeros(total, device="cuda"), torch.zeros(total, device="cuda")
    views = [params[o:o + int(np.prod(sh))].view(sh) for _, sh, o in layout]
    gviews = [grads[o:o + int(np.prod(sh))].view(sh) for _, sh, o in layout]
    for dst, src in zip(views, list(case["policy"]) + list(case["value"])):
        dst.copy_(dev(src))
    m, v, step = torch.zeros(total, device="cuda"), torch.zeros(total, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
    stats = torch.zeros(12, device="cuda")
    work = torch.empty(eng.ppo_work_bytes(k, n) // 4 + 1, device="cuda")
    arrays = [dev(case[q]) for q in ("x", "action", "logp_old", "adv", "ret", "target")]

    def bc_loss():
        torch.cuda.synchronize()
        w = [t.cpu().numpy() for t in views]
        return gr.loss_and_grads_guided_f64(case["x"][:, :k], case["action"], case["logp_old"], case["adv"], case["ret"], w[:6], w[6:],
                                            case["target"], None, ent_coef=0.0)["stats"][9]

    first = bc_loss()
    seen = []
    for _ in range(10):
        eng.ppo_grad_guided(views[:6], views[6:], gviews[:6], gviews[6:], arrays[0], arrays[1], arrays[2], arrays[3], arrays[4], stats, work,
                            arrays[5], in_dim=k, ent_coef=0.0)
        eng.adam(params, grads, m, v, step, 3e-4, eps=1e-5, max_grad_norm=0.5)
        seen.append(float(stats[9]))
    last = bc_loss()
    print("ten guided updates: bc_loss %.6f -> %.6f (float64 reference: -%.6f); the device's own: %s" % (first, last, gr.GUIDED_LOOP_D, seen))
    assert abs(seen[0] - first) <= 1e-5 * abs(first) and float(stats[8]) == n and float(stats[1]) == 0.0
    assert first - last >= 0.5 * gr.GUIDED_LOOP_D
