"""tests/categorical_ref.py on the CPU: the float64 reference against torch.distributions.Categorical and autograd, the measured tolerances
and the half-tolerance rule, the near-tie cap of every seeded case of the GPU module on the reference alone, what the case builder
promises, and the refusals of the collectors, the learner and the work-bytes function that need no device."""
import ctypes
import types
import warnings

import numpy as np
import pytest

from tests import categorical_ref as cf
from tests import ppo_ref as pp


def _autograd(c, has_critic):
    """The formulas of include/pgdrive_hip.h as torch ops in float64, the heads as torch.distributions.Categorical -> (loss terms, logp,
    entropy per row, gradients by autograd)."""
    import torch
    from torch.distributions import Categorical
    k, (ks, kt) = c["in_dim"], c["bins"]
    t64 = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
    x, lpo, adv, ret = [t64(c[q]) for q in ("x", "logp_old", "adv", "ret")]
    idx = torch.tensor(np.asarray(c["index"], dtype=np.int64))
    x = x[:, :k]
    pw = [t64(np.nan_to_num(w)).requires_grad_(True) for w in c["policy"]]   # (the unused head columns hold NaN: zero them, they are sliced away)
    vw = [t64(w).requires_grad_(True) for w in c["value"]]

    def hidden(w):
        return torch.tanh(torch.tanh(x @ w[0] + w[1]) @ w[2] + w[3])

    o = hidden(pw) @ pw[4][:, :ks + kt] + pw[5][:ks + kt]
    ds, dt = Categorical(logits=o[:, :ks]), Categorical(logits=o[:, ks:])
    logp = ds.log_prob(idx[:, 0]) + dt.log_prob(idx[:, 1])
    ent_rows = ds.entropy() + dt.entropy()
    s = c["adv_stats"]
    A = adv if s is None else (adv - float(s[0])) * float(s[1])
    r = torch.exp(logp - lpo)
    clip, vf, ce = [float(np.float32(q)) for q in (cf.CLIP, cf.VF_COEF, cf.ENT_COEF)]
    l_pi = -torch.minimum(r * A, torch.clamp(r, 1 - clip, 1 + clip) * A).mean()
    loss = l_pi - ce * ent_rows.mean()
    l_v = torch.zeros((), dtype=torch.float64)
    if has_critic:
        v = (hidden(vw) @ vw[4] + vw[5])[:, 0]
        l_v = (0.5 * (v - ret) ** 2).mean()
        loss = loss + vf * l_v
    loss.backward()
    grads = [w.grad.numpy() for w in pw], ([w.grad.numpy() for w in vw] if has_critic else None)
    return (float(loss.detach()), float(l_pi.detach()), float(l_v.detach()), float(ent_rows.mean().detach()),
            float((lpo - logp).mean().detach())), logp.detach().numpy(), grads


@pytest.mark.parametrize("has_critic", [True, False])
def test_the_reference_equals_torch_categorical_and_autograd(has_critic):
    """logp, entropy, approx_kl, the loss and every gradient of both networks, with the entropy bonus and the clipping active."""
    assert cf.ENT_COEF > 0
    worst = 0.0
    for c in (cf.GRAD_CASES[2], cf.LIST_CASE, cf.NOCRITIC_CASE):
        case = cf.grad_case(c)
        ref = cf.reference_of(case, has_critic)
        assert 0.0 < ref["stats"][5] < 1.0   # rows on both sides of the clip
        (loss, l_pi, l_v, ent, kl), logp, (pg, vg) = _autograd(case, has_critic)
        for a, b in ((ref["loss"], loss), (ref["stats"][1], l_pi), (ref["stats"][2], l_v), (ref["stats"][3], ent), (ref["stats"][4], kl)):
            assert abs(a - b) <= 1e-10 * max(1.0, abs(b)), (a, b)
        _, _, l = cf.logits_f64(case["x"], case["policy"], case["bins"])
        mine = cf.row_terms_f64(l, case["index"], case["logp_old"], case["adv"], case["adv_stats"], cf.CLIP, case["bins"])[1]
        assert np.abs(mine - logp).max() <= 1e-12
        for mine, theirs in ((ref["policy"], pg), (ref["value"], vg)):
            if theirs is None:
                assert mine is None
                continue
            for g, w in zip(mine, theirs):
                scale = np.abs(w).max()
                assert scale > 0
                worst = max(worst, float(np.abs(g - w).max() / scale))
        K = sum(case["bins"])
        assert (np.asarray(ref["policy"][4])[:, K:] == 0).all() and (np.asarray(ref["policy"][5])[K:] == 0).all()
    print("hand-derived backward against autograd: %.2e relative" % worst)
    assert worst <= 1e-10


def test_the_sampling_rule_of_the_reference():
    """index = #{j < K - 1 : c_j <= u}: u below p_0 gives 0, u above every partial sum gives K - 1, never beyond; the argmax takes the
    lowest index among equal logits (numpy's rule)."""
    c = cf.FORWARD_CASES[2]
    case = cf.forward_case(c)
    n = c["rows"]
    lo = cf.forward_f64(case["x"], case["policy"], None, c["bins"], np.full((n, 2), 2.0 ** -24))
    hi = cf.forward_f64(case["x"], case["policy"], None, c["bins"], np.full((n, 2), 1.0 - 2.0 ** -24))
    assert (lo["index"] == 0).all() and (hi["index"] == np.array(c["bins"]) - 1).all()
    assert (cf.grid_value(np.arange(5), 5) == np.array([-1.0, -0.5, 0.0, 0.5, 1.0], dtype=np.float32)).all()
    assert cf.grid_value(np.arange(13), 13)[[0, 12]].tolist() == [-1.0, 1.0]


def measure_forward():
    worst = 0.0
    for c in cf.FORWARD_CASES:
        case = cf.forward_case(c)
        for u, ref in ((case["u"], case["sampled"]), (None, case["argmax"])):
            index, logp = cf.emulate_forward(case["x"], case["policy"], c["bins"], u)
            skip = cf.admitted_differences(ref, index)
            e = cf.logp_error(logp, ref, skip)
            print("%s %s: logp %.3e (normalised), %d rows differ" % (c, "sampled" if u is not None else "argmax", e, int(skip.sum())))
            worst = max(worst, e)
    return worst


def measure_grad():
    worst = {name: [0.0, 0.0] for name, _, _ in pp.ROW_CLASSES}
    for label, case, ref, critic in cf.compared_grad_cases():
        g, s = cf.grad_errors(cf.emulation_of(case, critic), ref)
        cls = pp.row_class(case["x"].shape[0])
        print("%s [%s]: gradients %.3e, statistics %.3e (normalised); per slot 1 .. 6: %s" % (
            label, cls, g, s, " ".join("%.2e" % e for e in cf.stat_errors(cf.emulation_of(case, critic), ref))))
        worst[cls] = [max(worst[cls][0], g), max(worst[cls][1], s)]
    return worst


def test_the_emulation_keeps_half_of_every_tolerance():
    ef, by_class = measure_forward(), measure_grad()
    print("measured: logp %.3e, %s" % (ef, by_class))
    pairs = [(ef, cf.TOL_CAT_LOGP_MEASURED, cf.TOL_CAT_LOGP)]
    for (name, lo, _), (eg, es) in zip(pp.ROW_CLASSES, by_class.values()):
        tol_g, tol_s = cf.tolerances(lo)
        pairs += [(eg, cf.TOL_GRAD_MEASURED[name], tol_g), (es, cf.TOL_STAT_MEASURED[name], tol_s)]
    for measured, recorded, tol in pairs:
        assert 0.0 < measured <= 0.5 * tol, (measured, tol)
        assert recorded <= 1.02 * measured, (measured, recorded)   # the constants are the measurements, not something looser


def test_every_seeded_case_stays_under_the_near_tie_cap():
    """On the reference alone: at most 1 % of a case's rows lie near a tie, sampled and argmax."""
    for c in cf.FORWARD_CASES:
        case = cf.forward_case(c)
        for ref in (case["sampled"], case["argmax"]):
            near = int(cf.near_tie_rows(ref).sum())
            assert near <= int(cf.NEAR_TIE_CAP * c["rows"]), (c, near)
            assert np.abs(ref["logits"]).max() <= 8.0   # what MARGIN's derivation assumes of |lse|
    assert cf.margin(16) < 1e-4


def test_every_grad_case_holds_what_the_builder_promises():
    """All four cut / uncut branches (cases of 16 rows and more), no row within 1e-3 of a discontinuity; indices inside their heads."""
    for label, case, ref, critic in cf.compared_grad_cases():
        k, bins = case["in_dim"], case["bins"]
        _, _, l = cf.logits_f64(case["x"][:, :k], case["policy"], bins)
        A, logp, r, flows, rc = cf.row_terms_f64(l, case["index"], case["logp_old"], case["adv"], case["adv_stats"], cf.CLIP, bins)[:5]
        assert (np.abs(r - (1 - cf.CLIP)) > 1e-3).all() and (np.abs(r - (1 + cf.CLIP)) > 1e-3).all() and (np.abs(A) > 1e-3).all()
        b = case["branch"]
        assert (~flows[b < 2]).all() and flows[b >= 2].all(), label
        assert (case["index"] >= 0).all() and (case["index"] < np.array(bins)).all()
        if len(b) >= 16:
            assert set(b.tolist()) == {0, 1, 2, 3}


def test_collector_head_refusals_need_no_device():
    from pgdrive_amd import rollout
    opt = rollout.action_head_options
    assert opt("c", "gaussian", None, 4) == ("gaussian", None, False)
    assert opt("c", "categorical", (5, 5), 10) == ("categorical", (5, 5), False)
    assert opt("c", "categorical", (5, 5), 16, True, (5, 5)) == ("categorical", (5, 5), True)
    for bins in ((1, 5), (5, 1), (8, 9), (16, 2), None, (5, ), (2.5, 3), "ab"):
        with pytest.raises(ValueError):
            opt("c", "categorical", bins, 32)
    with pytest.raises(ValueError):
        opt("c", "categorical", (5, 5), 9)               # w3 too narrow
    with pytest.raises(ValueError):
        opt("c", "categorical", (5, 5), 16, True, (3, 3))  # bins that mismatch the engine's discrete dims
    with pytest.raises(ValueError):
        opt("c", "gaussian", (5, 5), 16)
    with pytest.raises(ValueError):
        opt("c", "softmax", None, 16)
    with pytest.raises(NotImplementedError):
        opt("c", "categorical", (5, 5), 16, guardian=dict(weights=()))
    with pytest.raises(NotImplementedError):
        opt("c", "categorical", (5, 5), 16, safe=True)
    with warnings.catch_warnings(record=True) as seen:   # the Gaussian head on a discrete engine: today's behaviour and ONE warning
        warnings.simplefilter("always")
        assert opt("c", "gaussian", None, 4, True, (5, 5)) == ("gaussian", None, False)
    assert len(seen) == 1 and 'action_head="categorical"' in str(seen[0].message)
    assert rollout.SafeRolloutCollector._SAFE and not rollout.RolloutCollector._SAFE


def test_learner_head_and_layout_need_no_device():
    from pgdrive_amd import learner
    cat = types.SimpleNamespace(action_head="categorical", bins=(5, 5))
    assert learner.collector_head("PPOLearner", cat) == ("categorical", (5, 5))
    assert learner.collector_head("PPOLearner", types.SimpleNamespace()) == ("gaussian", None)
    with pytest.raises(NotImplementedError):
        learner.collector_head("PPOLagLearner", cat, cost=True)
    layout, total = learner.flat_layout(274, 10)
    shapes = {name: shape for name, shape, _ in layout}
    assert shapes["w3"] == (256, 10) and shapes["b3"] == (10, ) and all(o % 4 == 0 for _, _, o in layout) and total % 4 == 0


def test_cat_work_bytes_without_a_device():
    from pgdrive_amd import _abi, engine
    assert _abi.AC_EMIT_INDEX == 2 and _abi.cat_bins((3, 13), "t") == (3, 13)
    lib = engine.load_library()
    cat, plain = lib.pgd_ppo_cat_work_bytes, lib.pgd_ppo_work_bytes
    for f in (cat, plain):
        f.restype, f.argtypes = ctypes.c_size_t, [ctypes.c_int] * 3
    for in_dim, rows, critic in ((3, 16, 1), (417, 16, 1), (4097, 16, 0), (274, 0, 1), (274, 16777217, 1)):
        assert cat(in_dim, rows, critic) == 0 and plain(in_dim, rows, critic) == 0
    for in_dim in (4, 19, 274, 416):
        for rows in (1, 16, 17, 1025):
            for critic in (0, 1):
                a, b = cat(in_dim, rows, critic), plain(in_dim, rows, critic)
                r16 = (rows + 15) & ~15
                assert a >= b > 0 and a - b == 4 * ((critic + 1) * r16 * 12 + (r16 // 16) * 8)   # dOut [R16][16] for [R16][4], 24 tile sums for 16
