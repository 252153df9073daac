"""tests/safe_ppo_ref.py on the CPU: the three-network loss against torch autograd, the flat layout with a cost critic, the multiplier
and the bookkeeping references, the ctypes mirrors of the new structs, and the measured tolerance with its half-tolerance rule."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from tests import ppo_ref as rf
from tests import safe_ppo_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_three_network_loss_equals_autograd():
    """in_dim 35, rows 17: L = L_pi + vf L_v - ent mean(H) + cvf L_c as torch ops in float64; the gradients of all eighteen tensors."""
    import torch
    c = dict(name="safe", in_dim=35, rows=17, scaling="unit", out_cols=6, seed=3, normalise=True)
    case = rf.build_case(**c)
    cw, cost_ret = sr.cost_side(c)
    k = c["in_dim"]
    main, cost = sr.loss_and_grads3_f64(case["x"][:, :k], case["action"], case["logp_old"], case["adv"], case["ret"], cost_ret, case["policy"],
                                        case["value"], cw, adv_stats=case["adv_stats"])
    t64 = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
    x, act, lpo, adv, ret, cret = [t64(q) for q in (case["x"][:, :k], case["action"], case["logp_old"], case["adv"], case["ret"], cost_ret)]
    pw = [t64(np.nan_to_num(w)).requires_grad_(True) for w in case["policy"]]
    vw = [t64(w).requires_grad_(True) for w in case["value"]]
    cwt = [t64(w).requires_grad_(True) for w in cw]

    def hidden(w):
        return torch.tanh(torch.tanh(x @ w[0] + w[1]) @ w[2] + w[3])

    o = hidden(pw) @ pw[4][:, :4] + pw[5][:4]
    mean, ls = o[:, :2], o[:, 2:4]
    A = (adv - float(case["adv_stats"][0])) * float(case["adv_stats"][1])
    z = (act - mean) * torch.exp(-ls)
    logp = -0.5 * (z ** 2).sum(dim=1) - ls.sum(dim=1) - rf.LOG_2PI
    r = torch.exp(logp - lpo)
    clip, vf, ce, cvf = [float(np.float32(q)) for q in (rf.CLIP, rf.VF_COEF, rf.ENT_COEF, sr.CVF_COEF)]
    l_pi = -torch.minimum(r * A, torch.clamp(r, 1 - clip, 1 + clip) * A).mean()
    ent = (ls.sum(dim=1) + rf.LOG_2PIE).mean()
    l_v = (0.5 * ((hidden(vw) @ vw[4] + vw[5])[:, 0] - ret) ** 2).mean()
    l_c = (0.5 * ((hidden(cwt) @ cwt[4] + cwt[5])[:, 0] - cret) ** 2).mean()
    (l_pi - ce * ent + vf * l_v + cvf * l_c).backward()
    for a, b in ((main["stats"][1], l_pi), (main["stats"][2], l_v), (main["stats"][3], ent), (cost["stats"][2], l_c)):
        assert abs(a - float(b.detach())) <= 1e-10 * max(1.0, abs(float(b.detach())))
    worst = 0.0
    for mine, theirs in ((main["policy"], pw), (main["value"], vw), (cost["value"], cwt)):
        for g, w in zip(mine, theirs):
            scale = float(w.grad.abs().max())
            assert scale > 0
            worst = max(worst, float(np.abs(g - w.grad.numpy()).max() / scale))
    print("three-network backward against autograd: %.2e relative" % worst)
    assert worst <= 1e-10


def test_flat_layout_with_a_cost_critic():
    from pgdrive_amd import learner
    for in_dim, out_cols in ((4, 4), (35, 6), (274, 4), (275, 5), (416, 4)):
        two, n2 = learner.flat_layout(in_dim, out_cols)
        three, n3 = learner.flat_layout(in_dim, out_cols, has_cost_critic=True)
        assert learner.flat_layout(in_dim, out_cols, True, False) == (two, n2), "the default output changed"
        assert len(two) == 12 and len(three) == 18 and three[:12] == two
        assert [n for n, _, _ in three[12:]] == ["cw1", "cb1", "cw2", "cb2", "cw3", "cb3"]
        assert [s for _, s, _ in three[12:]] == [s for _, s, _ in two[6:]], "the cost critic has the value network's shapes"
        assert all(o % 4 == 0 for _, _, o in three) and n3 % 4 == 0
        ends = [o + int(np.prod(s)) for _, s, o in three]
        assert all(e <= o for e, (_, _, o) in zip(ends, three[1:])) and ends[-1] <= n3, "tensors overlap"
        assert three[12][2] >= n2 - 3


def test_lagrange_reference_leaves_the_state_without_episodes_and_clamps():
    state = np.array([0.7, np.nan, 3.0, 0.0], dtype=np.float32)
    out = sr.lagrange_f64(np.array([5.0, 1.0], dtype=np.float32), np.zeros(2, dtype=np.int32), state, 1.0, 0.05, 5.0)
    assert out[0] == np.float64(np.float32(0.7)) and np.isnan(out[1]) and out[2] == 3.0
    for rows in sr.LAG_ROWS:
        seen = {}
        for move in sr.LAG_MOVES:
            ep_sum, count, st, limit, lr = sr.build_lagrange(rows, move)
            new = sr.lagrange_f64(ep_sum, count, st, limit, lr, sr.LAG_MAX)
            E = int(count.sum())
            assert E > 0 and new[2] == E and abs(new[1] - ep_sum.astype(np.float64).sum() / E) < 1e-12
            assert (ep_sum[count == 0] == 0).all()
            seen[move] = (float(st[0]), new[0])
        assert seen["up"][1] > seen["up"][0] and 0.0 < seen["down"][1] < seen["down"][0]
        assert seen["clamp_zero"][1] == 0.0 and seen["clamp_max"][1] == sr.LAG_MAX


def test_bookkeeping_one_scan_equals_two_with_the_carry():
    """2 T steps in one scan against two scans of T with the running cost carried: the same run, and the finished episodes add up."""
    for T, rows, mode in sr.cost_gae_cases():
        flags, done, cv, run = sr.build_cost_rollout(2 * T, rows, mode, True)
        whole = sr.cost_gae_f64(flags, done, cv, sr.DYADIC, 0.99, 0.95, run)
        a = sr.cost_gae_f64(flags[:T], done[:T], cv[:T + 1], sr.DYADIC, 0.99, 0.95, run)
        b = sr.cost_gae_f64(flags[T:], done[T:], cv[T:], sr.DYADIC, 0.99, 0.95, a["run"])
        assert np.array_equal(whole["run"], b["run"]) and np.array_equal(whole["ep_sum"], a["ep_sum"] + b["ep_sum"])
        assert np.array_equal(whole["ep_count"], a["ep_count"] + b["ep_count"])
        assert np.array_equal(whole["cost"], np.concatenate([a["cost"], b["cost"]]))
        # dyadic costs: the float32 emulation is exact
        rn, es, ec = sr.emulate_bookkeeping(whole["cost"], done, run)
        assert np.array_equal(rn.astype(np.float64), whole["run"]) and np.array_equal(es.astype(np.float64), whole["ep_sum"])
        assert np.array_equal(ec, whole["ep_count"])
        if mode == "every":
            assert (whole["ep_count"] == 2 * T).all() and (whole["run"] == 0).all()
        if mode == "none":
            assert (whole["ep_count"] == 0).all() and (whole["ep_sum"] == 0).all()


def test_cost_cases_cover_every_combination_of_the_cost_bits():
    seen = set()
    for T, rows, mode in sr.cost_gae_cases():
        flags, done, cv, run = sr.build_cost_rollout(T, rows, mode, True)
        cost = sr.costs_of_flags(flags, sr.DYADIC)
        f = flags.astype(np.int64)
        want = np.where(f & 2, 1.0, np.where(f & 4, 0.5, np.where(f & 8, 0.25, 0.0)))
        assert np.array_equal(cost, want.astype(np.float32))
        seen |= set(((f >> 1) & 7).reshape(-1).tolist())
        if T * rows >= 64:
            assert set(((f >> 1) & 7).reshape(-1).tolist()) == set(range(8))
            assert all((f & bit).any() and not (f & bit).all() for bit in sr.OTHER_FLAG_BITS)
    assert seen == set(range(8))


def measure_bookkeeping():
    worst = 0.0
    for T, rows, mode in sr.cost_gae_cases():
        flags, done, cv, run = sr.build_cost_rollout(T, rows, mode, False)
        ref = sr.cost_gae_f64(flags, done, cv, sr.NONDYADIC, 0.99, 0.95, run)
        rn, es, ec = sr.emulate_bookkeeping(ref["cost"], done, run)
        assert np.array_equal(ec, ref["ep_count"])
        worst = max(worst, sr.bookkeeping_error(rn, es, ref))
    return worst


def test_the_bookkeeping_emulation_keeps_half_of_the_tolerance():
    worst = measure_bookkeeping()
    print("bookkeeping emulation against float64: %.3e (TOL_EP_MEASURED %.3e)" % (worst, sr.TOL_EP_MEASURED))
    assert 0.0 < worst <= sr.TOL_EP / 2.0
    assert worst >= 0.5 * sr.TOL_EP_MEASURED, "the recorded measurement is stale"


def test_the_cost_critic_emulation_keeps_half_of_ppo_refs_tolerances():
    """The cost side of the cases that the GPU test holds against float64 at ppo_ref.tolerances: the float32 emulation of the kernels'
    summation order, with the cost network as "the critic", keeps within half of them, as ppo_ref's own cases do."""
    worst = [0.0, 0.0]
    for c in sr.f64_cases():
        case, _ = rf.case_and_reference(c)
        cw, cost_ret = sr.cost_side(c)
        k = c["in_dim"]
        args = (case["x"][:, :k], case["action"], case["logp_old"], case["adv"], cost_ret, case["policy"], cw)
        ref = rf.loss_and_grads_f64(*args, vf_coef=sr.CVF_COEF, adv_stats=case["adv_stats"])
        emu = rf.emulate_grads(*args, vf_coef=sr.CVF_COEF, adv_stats=case["adv_stats"])
        eg, es = rf.grad_errors(emu, ref)
        tol_g, tol_s = rf.tolerances(c["rows"])
        worst = [max(worst[0], eg / tol_g), max(worst[1], es / tol_s)]
        assert eg <= tol_g / 2.0 and es <= tol_s / 2.0, (c, eg, tol_g, es, tol_s)
    print("cost critic emulation: gradients %.3f, statistics %.3f of ppo_ref's tolerances" % tuple(worst))


def test_adv_mix_reference():
    adv, cadv, s, cs = sr.build_mix(65)
    out, bound = sr.adv_mix_f64(adv, cadv, s, None, 0.0)
    assert np.array_equal(out, (adv.astype(np.float64) - float(s[0])) * float(s[1]))
    out, bound = sr.adv_mix_f64(adv, cadv, None, cs, 100.0)
    want = (adv.astype(np.float64) - float(np.float32(100.0)) * (cadv.astype(np.float64) - float(cs[0]))) / 101.0
    assert np.allclose(out, want, rtol=1e-14, atol=0) and (bound > 0).all()


def test_new_struct_mirrors_have_the_c_sizes_and_offsets():
    from pgdrive_amd import _abi
    mirrors = {"pgd_value_net": _abi.ValueNet, "pgd_ppo_cost": _abi.PPOCost, "pgd_value_grads": _abi.ValueGrads}
    lines = []
    for st, m in mirrors.items():
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (st, st))
        for n, _ in m._fields_:
            lines.append('  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (st, n, st, n))
    prog = "#include <stdio.h>\n#include <stddef.h>\n#include \"pgdrive_hip.h\"\nint main(void) {\n" + "\n".join(lines) + "\n  return 0;\n}\n"
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "s.c")
        open(c, "w").write(prog)
        exe = os.path.join(td, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        out = dict(line.split() for line in subprocess.check_output([exe]).decode().strip().splitlines())
    for st, m in mirrors.items():
        assert int(out[st]) == C.sizeof(m), (st, out[st], C.sizeof(m))
        for n, _ in m._fields_:
            assert int(out["%s.%s" % (st, n)]) == getattr(m, n).offset, (st, n)
    assert _abi.PPO_COST_STATS[7] == "cost_value_loss" and _abi.PPO_COST_STATS[:7] == _abi.PPO_STATS[:7]


def test_the_library_exports_the_safe_entry_points_and_refuses_null_handles():
    from pgdrive_amd import build, engine
    build.build()
    L = engine.load_library()
    for fn in ("pgd_mlp_actor_critic_cost", "pgd_cost_gae", "pgd_lagrange", "pgd_adv_mix", "pgd_ppo_cost_work_bytes", "pgd_ppo_grad_cost"):
        assert hasattr(L, fn) and fn in engine.EXPORTS
    assert L.pgd_cost_gae(None, None, None, None, 1, 1, None, 0.99, 0.95, None, None, None, None, None, None) == 1
    assert L.pgd_lagrange(None, None, None, 1, 1.0, 0.05, 100.0, None) == 1
    assert L.pgd_adv_mix(None, None, None, 1, None, None, None, None) == 1
    assert L.pgd_ppo_cost_work_bytes(417, 16) == 0 and L.pgd_ppo_cost_work_bytes(3, 16) == 0 and L.pgd_ppo_cost_work_bytes(35, 0) == 0
    # three networks' scratch: the two-network one plus one more W2^T, four activation planes, dOut and the partials -- the tile sums do
    # not grow (the cost critic's two take free slots of the record)
    two, one = L.pgd_ppo_work_bytes(35, 33, 1), L.pgd_ppo_work_bytes(35, 33, 0)
    assert L.pgd_ppo_cost_work_bytes(35, 33) == two + (two - one)


def test_lazy_imports_know_the_new_names():
    import pgdrive_amd
    from pgdrive_amd import learner, rollout
    assert pgdrive_amd.SafeRolloutCollector is rollout.SafeRolloutCollector and pgdrive_amd.PPOLagLearner is learner.PPOLagLearner
