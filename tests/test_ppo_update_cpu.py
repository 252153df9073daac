"""tests/ppo_ref.py on the CPU: the hand-derived float64 backward pass against torch autograd, the measured tolerances and the
half-tolerance rule, the conditions the case builders promise, PPOLearner's minibatch partition and flat-buffer layout, and the loss
decrease the closed-loop GPU test asks for."""
import numpy as np
import pytest

from tests import ppo_ref as rf


def _autograd(c, n_rows, has_critic, adv_stats):
    """The formulas of include/pgdrive_hip.h as torch ops in float64 -> (stats terms, gradients) by autograd."""
    import torch
    k = c["in_dim"]
    t64 = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
    x, act, lpo, adv, ret = [t64(c[q][:n_rows]) for q in ("x", "action", "logp_old", "adv", "ret")]
    x = x[:, :k]
    pw = [t64(np.nan_to_num(w)).requires_grad_(True) for w in c["policy"]]   # (the unused head columns hold NaN: zero them, they are sliced away)
    vw = [t64(w).requires_grad_(True) for w in c["value"]]

    def hidden(w):
        return torch.tanh(torch.tanh(x @ w[0] + w[1]) @ w[2] + w[3])

    o = hidden(pw) @ pw[4][:, :4] + pw[5][:4]
    mean, ls = o[:, :2], o[:, 2:4]
    A = adv if adv_stats is None else (adv - float(adv_stats[0])) * float(adv_stats[1])
    z = (act - mean) * torch.exp(-ls)
    logp = -0.5 * (z ** 2).sum(dim=1) - ls.sum(dim=1) - rf.LOG_2PI
    r = torch.exp(logp - lpo)
    clip, vf, ce = [float(np.float32(q)) for q in (rf.CLIP, rf.VF_COEF, rf.ENT_COEF)]
    l_pi = -torch.minimum(r * A, torch.clamp(r, 1 - clip, 1 + clip) * A).mean()
    ent = (ls.sum(dim=1) + rf.LOG_2PIE).mean()
    loss = l_pi - ce * ent
    l_v = torch.zeros((), dtype=torch.float64)
    if has_critic:
        v = (hidden(vw) @ vw[4] + vw[5])[:, 0]
        l_v = (0.5 * (v - ret) ** 2).mean()
        loss = loss + vf * l_v
    loss.backward()
    grads = [w.grad.numpy() for w in pw], ([w.grad.numpy() for w in vw] if has_critic else None)
    return float(loss.detach()), float(l_pi.detach()), float(l_v.detach()), float(ent.detach()), grads


@pytest.mark.parametrize("has_critic", [True, False])
def test_the_hand_derived_backward_pass_equals_autograd(has_critic):
    worst = 0.0
    for c in (dict(name="sweep", in_dim=35, rows=33, scaling="unit", out_cols=6, seed=2, normalise=True),
              dict(name="sweep", in_dim=5, rows=17, scaling="normalised", out_cols=4, seed=1, normalise=False)):
        case = rf.build_case(**c)
        k = c["in_dim"]
        ref = rf.loss_and_grads_f64(case["x"][:, :k], case["action"], case["logp_old"], case["adv"], case["ret"], case["policy"],
                                    case["value"] if has_critic else None, adv_stats=case["adv_stats"])
        loss, l_pi, l_v, ent, (pg, vg) = _autograd(case, c["rows"], has_critic, case["adv_stats"])
        for a, b in ((ref["loss"], loss), (ref["stats"][1], l_pi), (ref["stats"][2], l_v), (ref["stats"][3], ent)):
            assert abs(a - b) <= 1e-10 * max(1.0, abs(b))
        for mine, theirs in ((ref["policy"], pg), (ref["value"], vg)):
            if theirs is None:
                assert mine is None
                continue
            for g, w in zip(mine, theirs):
                scale = np.abs(w).max()
                assert scale > 0
                worst = max(worst, float(np.abs(g - w).max() / scale))
        assert (np.asarray(ref["policy"][4])[:, 4:] == 0).all() and (np.asarray(ref["policy"][5])[4:] == 0).all()
    print("hand-derived backward against autograd: %.2e relative" % worst)
    assert worst <= 1e-10


def measure_grad():
    """{row class: (largest gradient error, largest statistics error)} of the emulation over compared_cases()."""
    worst = {name: [0.0, 0.0] for name, _, _ in rf.ROW_CLASSES}
    for label, case, ref, critic in rf.compared_cases():
        g, s = rf.grad_errors(rf.emulation_of(case, critic), ref)
        cls = rf.row_class(case["x"].shape[0])
        print("%s [%s]: gradients %.3e, statistics %.3e (normalised)" % (label, cls, g, s))
        worst[cls] = [max(worst[cls][0], g), max(worst[cls][1], s)]
    return worst


def measure_adv():
    worst = 0.0
    for n in rf.ADV_COUNTS:
        for with_index in (False, True):
            adv, index, _ = rf.build_adv(n, with_index)
            live = adv[:n] if index is None else adv[index[:n]]
            want, got = rf.adv_stats_f64(live), rf.emulate_adv_stats(live)
            scale = np.array([np.abs(live.astype(np.float64)).mean() if n else 1.0, want[1]])
            worst = max(worst, float((np.abs(got - want) / np.where(scale > 0, scale, 1.0)).max()))
    return worst


def measure_adam():
    return rf.adam_errors(lambda p, g, m, v, t, mx: rf.emulate_adam(p, g, m, v, t, max_grad_norm=mx, **rf.ADAM_HYPER))


def test_the_emulation_keeps_half_of_every_tolerance():
    by_class = measure_grad()
    ea, em = measure_adv(), measure_adam()
    print("measured: %s, adv_stats %.3e, adam %.3e" % (by_class, ea, em))
    pairs = [(ea, rf.TOL_ADV_MEASURED, rf.TOL_ADV), (em, rf.TOL_ADAM_MEASURED, rf.TOL_ADAM)]
    for (name, lo, _), (eg, es) in zip(rf.ROW_CLASSES, by_class.values()):
        tol_g, tol_s = rf.tolerances(lo)
        pairs += [(eg, rf.TOL_GRAD_MEASURED[name], tol_g), (es, rf.TOL_STAT_MEASURED[name], tol_s)]
    for measured, recorded, tol in pairs:
        assert 0.0 < measured <= 0.5 * tol, (measured, tol)
        assert recorded <= 1.02 * measured, (measured, recorded)   # the constants are the measurements, not something looser


def test_every_case_holds_what_the_builder_promises():
    """All four cut / uncut branches with at least 10 % of the rows each (cases of 15 rows and more), no row within 1e-3 of a
    discontinuity of the gradient; on the float64 reference."""
    for c in list(rf.grad_cases()) + [rf.closed_loop_case(), rf.LIST_CASE, rf.NOCRITIC_CASE, rf.PART_CASE, rf.SPLIT_CASE]:
        case, _ = rf.case_and_reference(c)
        k = c["in_dim"]
        mean, ls, _ = rf.ar.heads_f64(case["x"][:, :k], case["policy"], None)
        A, logp, r, flows, z, e, rc = rf.row_terms_f64(mean, ls, case["action"], case["logp_old"], case["adv"], case["adv_stats"], rf.CLIP)
        clip = float(np.float32(rf.CLIP))
        assert np.abs(r - (1 + clip)).min() >= 1e-3 and np.abs(r - (1 - clip)).min() >= 1e-3 and np.abs(A).min() >= 1e-3, c
        kinds = [(A > 0) & (r > 1 + clip), (A < 0) & (r < 1 - clip), (A > 0) & (np.abs(r - 1) < clip), (A < 0) & (np.abs(r - 1) < clip)]
        for b, kind in enumerate(kinds):
            assert (kind == (case["branch"] == b)).all(), (c, rf.BRANCHES[b])
            if c["rows"] >= 15:
                assert kind.mean() >= 0.1, (c, rf.BRANCHES[b], kind.mean())
        assert (~flows == (kinds[0] | kinds[1])).all()
        assert not np.isfinite(case["x"][:, k:]).any() and case["x"].shape[1] > k   # NaN in the observation columns at and beyond in_dim


def test_strided_minibatches_partition_the_list():
    from pgdrive_amd import learner
    T, N, A = 8, 2, 5
    n_list = T * N * A
    for n_mb in (1, 2, 4, 7):
        plan = learner.minibatch_plan(n_list, n_mb)
        assert len(plan) == n_mb
        for count in sorted({0, 1, max(n_mb - 1, 0), n_mb, n_mb + 1, n_list}):
            seen = sorted(q for start, stride, rows in plan for q in learner.live_positions(start, stride, rows, count))
            assert seen == list(range(count)), (n_mb, count)
            for start, stride, rows in plan:
                assert rows >= 1 and start + (rows - 1) * stride < n_list + stride


def test_flat_buffer_offsets_are_multiples_of_four():
    from pgdrive_amd import learner
    for in_dim in (4, 5, 35, 274, 275, 416):
        for out_cols in (4, 5, 6, 7):
            layout, total = learner.flat_layout(in_dim, out_cols)
            assert [n for n, _, _ in layout] == ["w1", "b1", "w2", "b2", "w3", "b3", "vw1", "vb1", "vw2", "vb2", "vw3", "vb3"]
            end = 0
            for _, shape, off in layout:
                assert off % 4 == 0 and off >= end
                end = off + int(np.prod(shape))
            assert total % 4 == 0 and total >= end
            assert layout[4][1] == (256, out_cols) and layout[10][1] == (256, 1)


def closed_loop_decrease():
    """Ten adam_f64 steps (lr 3e-4, the learner's defaults otherwise) on the fixed minibatch of closed_loop_case(), gradients from
    loss_and_grads_f64: L before - L after."""
    c = rf.build_case(**rf.closed_loop_case())
    k = c["in_dim"]
    nets = [np.nan_to_num(np.asarray(w, dtype=np.float64)) for w in list(c["policy"]) + list(c["value"])]
    m, v = [np.zeros_like(w) for w in nets], [np.zeros_like(w) for w in nets]

    def evaluate():
        return rf.loss_and_grads_f64(c["x"][:, :k], c["action"], c["logp_old"], c["adv"], c["ret"], nets[:6], nets[6:], ent_coef=0.0)

    first = evaluate()["loss"]
    for t in range(1, 11):
        ref = evaluate()
        g = [np.asarray(q) for q in ref["policy"] + ref["value"]]
        flat = np.concatenate([q.reshape(-1) for q in g])
        scale = min(1.0, 0.5 / (np.sqrt((flat * flat).sum()) + 1e-6))
        for i in range(12):
            nets[i], m[i], v[i] = rf.adam_f64(nets[i], g[i] * scale, m[i], v[i], t, 3e-4)
    return first - evaluate()["loss"]


def test_ten_reference_steps_lower_the_loss():
    d = closed_loop_decrease()
    print("ten float64 Adam steps lower L by %.6e" % d)
    assert d > 0 and abs(d - rf.CLOSED_LOOP_D) <= 1e-6 * abs(d)
