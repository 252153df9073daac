"""tests/guided_ref.py and the host side of the guided update on the CPU: the float64 formulas against torch autograd and, with no guided
row, against ppo_ref.loss_and_grads_f64 for equality; the measured tolerances and the half-tolerance rule; NaN targets on free rows;
guide_options' refusals; pgd_ppo_guide's layout against the header; and the bc_loss decrease the closed-loop GPU test asks for."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import guided_ref as gr
from tests import ppo_ref as rf
from tests import recording_engine as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _autograd(c):
    """The guided loss of include/pgdrive_hip.h as torch ops in float64 -> (loss, gradients of the case's networks) by autograd."""
    import torch
    k, n = c["in_dim"], c["x"].shape[0]
    t64 = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
    x, act, lpo, adv, ret, cret = [t64(c[q]) for q in ("x", "action", "logp_old", "adv", "ret", "cost_ret")]
    x = x[:, :k]
    u = torch.tensor(c["guided"])
    s = ~u | bool(c["keep"])
    tgt = t64(np.where(c["guided"][:, None], c["target"][:, :2], 0.0))
    nets = dict(policy=[t64(np.nan_to_num(w)).requires_grad_(True) for w in c["policy"]])
    if c["nets"] >= 2:
        nets["value"] = [t64(w).requires_grad_(True) for w in c["value"]]
    if c["nets"] == 3:
        nets["cost"] = [t64(w).requires_grad_(True) for w in c["cost"]]

    def hidden(w):
        return torch.tanh(torch.tanh(x @ w[0] + w[1]) @ w[2] + w[3])

    pw = nets["policy"]
    o = hidden(pw) @ pw[4][:, :4] + pw[5][:4]
    mean, ls = o[:, :2], o[:, 2:4]
    A = adv if c["adv_stats"] is None else (adv - float(c["adv_stats"][0])) * float(c["adv_stats"][1])

    def logp_of(a):
        z = (a - mean) * torch.exp(-ls)
        return -0.5 * (z ** 2).sum(dim=1) - ls.sum(dim=1) - rf.LOG_2PI

    r = torch.exp(logp_of(act) - lpo)
    clip, vf, ce, cvf, bc = [float(np.float32(q)) for q in (rf.CLIP, rf.VF_COEF, rf.ENT_COEF, gr.CVF_COEF, c["bc_coef"])]
    surrogate = -torch.minimum(r * A, torch.clamp(r, 1 - clip, 1 + clip) * A)
    zero = torch.zeros(n, dtype=torch.float64)
    loss = (torch.where(s, surrogate, zero).sum() + bc * torch.where(u, -logp_of(tgt), zero).sum()) / n - ce * (ls.sum(dim=1) + rf.LOG_2PIE).mean()
    for name, targets, coef in (("value", ret, vf), ("cost", cret, cvf)):
        if name in nets:
            w = nets[name]
            loss = loss + coef * (0.5 * ((hidden(w) @ w[4] + w[5])[:, 0] - targets) ** 2).mean()
    loss.backward()
    return float(loss.detach()), {name: [w.grad.numpy() for w in ws] for name, ws in nets.items()}


AUTOGRAD_CASES = [dict(base=dict(name="guided-auto", in_dim=35, rows=33, scaling="unit", out_cols=6, seed=2, normalise=True), pattern="alternating",
                       stride=4, keep=False, bc_coef=0.7, nets=3),
                  dict(base=dict(name="guided-auto", in_dim=5, rows=17, scaling="normalised", out_cols=4, seed=1, normalise=False),
                       pattern="bytes246_bits3", stride=2, keep=True, bc_coef=1.0, nets=2),
                  dict(base=dict(name="guided-auto", in_dim=5, rows=17, scaling="unit", out_cols=5, seed=3, normalise=False), pattern="null",
                       stride=2, keep=False, bc_coef=2.0, nets=1)]


@pytest.mark.parametrize("c", AUTOGRAD_CASES, ids=lambda c: "%s-nets%d" % (c["pattern"], c["nets"]))
def test_the_guided_formulas_equal_autograd(c):
    case = gr.build_guided(**c)
    ref = gr.reference_of(case)
    loss, grads = _autograd(case)
    assert abs(ref["loss"] - loss) <= 1e-10 * max(1.0, abs(loss))
    worst = 0.0
    for name in ("policy", "value", "cost"):
        assert (ref[name] is None) == (name not in grads)
        for g, w in zip(ref[name] or (), grads.get(name, ())):
            assert np.abs(w).max() > 0
            worst = max(worst, float(np.abs(g - w).max() / np.abs(w).max()))
    print("guided backward against autograd: %.2e relative" % worst)
    assert worst <= 1e-10
    u, s = case["guided"], ~case["guided"] | case["keep"]
    assert ref["stats"][0] == len(u) and ref["stats"][8] == u.sum() and (ref["stats"][10:] == 0).all()
    assert (ref["stats"][[1, 4, 5, 6]] != 0).any() == bool(s.any())


def test_no_guided_row_is_the_plain_reference_exactly():
    """Every output the two share, ==: the guided formulas are the plain ones with the selections made, not a restatement beside them."""
    for pattern in ("none", "bytes246_bits1"):
        for nets in (1, 2):
            c = gr.build_guided(base=dict(name="guided-free", in_dim=35, rows=33, scaling="unit", out_cols=5, seed=4, normalise=True), pattern=pattern,
                                stride=4, keep=False, bc_coef=1.0, nets=nets)
            assert not c["guided"].any() and np.isnan(c["target"]).all()
            got, want = gr.reference_of(c), rf.reference_of(c, critic=nets == 2)
            assert np.array_equal(got["stats"][:8], want["stats"]) and np.array_equal(got["stat_norm"][:8], want["stat_norm"])
            assert (got["stats"][8:] == 0).all() and got["loss"] == want["loss"]
            for net in ("policy", "value"):
                assert (got[net] is None) == (want[net] is None)
                for a, b, na, nb in zip(got[net] or (), want[net] or (), got[net + "_norm"] or (), want[net + "_norm"] or ()):
                    assert np.array_equal(a, b) and np.array_equal(na, nb)


def test_nan_targets_of_free_rows_and_unread_columns_reach_nothing():
    for c in gr.guided_cases():
        case, ref = gr.case_and_reference(c)
        free = ~case["guided"]
        assert np.isnan(case["target"][free]).all() and (c["stride"] == 2 or np.isnan(case["target"][:, 2:]).all())
        assert np.isfinite(case["target"][case["guided"], :2]).all()
        for net in ("policy", "value", "cost"):
            assert ref[net] is None or all(np.isfinite(g).all() for g in ref[net])
        assert np.isfinite(ref["stats"]).all() and np.isfinite(ref["loss"])
    patterns = {c["pattern"] for c in gr.guided_cases()}
    assert patterns == set(gr.PATTERNS)


def measure():
    """{row class: [largest gradient error, largest statistics error]} of the emulation over guided_cases()."""
    worst = {name: [0.0, 0.0] for name, _, _ in rf.ROW_CLASSES}
    for c in gr.guided_cases():
        case, ref = gr.case_and_reference(c)
        g, s = gr.grad_errors(gr.emulation_of(case), ref)
        cls = rf.row_class(case["x"].shape[0])
        print("%s [%s]: gradients %.3e, statistics %.3e (normalised)" % (c, cls, g, s))
        worst[cls] = [max(worst[cls][0], g), max(worst[cls][1], s)]
    return worst


def test_the_emulation_keeps_half_of_every_tolerance():
    by_class = measure()
    print("measured: %s" % by_class)
    for (name, lo, _), (eg, es) in zip(rf.ROW_CLASSES, by_class.values()):
        tol_g, tol_s = gr.tolerances(lo)
        for measured, recorded, tol in ((eg, gr.TOL_GRAD_MEASURED[name], tol_g), (es, gr.TOL_STAT_MEASURED[name], tol_s)):
            assert 0.0 < measured <= 0.5 * tol, (name, measured, tol)
            assert recorded <= 1.02 * measured, (name, measured, recorded)   # the constants are the measurements, not something looser


def test_guide_options_refuses_without_a_device():
    from pgdrive_amd.learner import guide_options
    guardian = dict(weights=None, save_level=0.5, deterministic=False, immediate=False)
    assert guide_options("L", None, 1.0, False, None) is None and guide_options("L", None, 1.0, False, guardian) is None
    g = guide_options("L", "takeover", 0.5, True, guardian)
    assert g == dict(target="applied_actions", mask="takeover", mask_bits=1, bc_coef=0.5, keep_surrogate=True)
    assert guide_options("L", "takeover", 1, False, dict(guardian, immediate=True))["mask_bits"] == 3
    assert guide_options("L", "all", 0.0, False, guardian) == dict(target="guardian_trace", mask=None, mask_bits=1, bc_coef=0.0, keep_surrogate=False)
    with pytest.raises(ValueError, match="guide = 'expert'"):
        guide_options("L", "expert", 1.0, False, guardian)
    with pytest.raises(ValueError, match="guardian="):
        guide_options("L", "takeover", 1.0, False, None)
    for bad in (-1.0, float("nan"), float("inf"), "much", None, True):
        with pytest.raises(ValueError, match="bc_coef"):
            guide_options("L", "all", bad, False, guardian)
    with pytest.raises(ValueError, match="keep_surrogate=True without guide="):
        guide_options("L", None, 1.0, True, guardian)
    with pytest.raises(ValueError, match="keep_surrogate"):
        guide_options("L", "all", 1.0, "yes", guardian)


def test_the_learners_refuse_a_guide_without_a_guardian():
    """The refusal comes before the learner touches the engine: a collector built without guardian= (its attribute is None)."""
    import types
    from pgdrive_amd.learner import PPOLagLearner, PPOLearner
    col = types.SimpleNamespace(guardian=None)
    with pytest.raises(ValueError, match="guardian="):
        PPOLearner(col, guide="takeover")
    with pytest.raises(ValueError, match="guardian="):
        PPOLagLearner(col, cost_limit=1.0, guide="all")
    with pytest.raises(ValueError, match="keep_surrogate"):
        PPOLearner(col, keep_surrogate=True)


class LearnerEngine(rc.AllSwitchesEngine):
    """recording_engine's engine with the learners' calls, recorded by name (the gradient calls with what they were handed) and doing
    nothing: what update() asks of an Engine, without a device."""
    def ppo_work_bytes(self, in_dim, rows, has_critic=True):
        return 16

    ppo_cost_work_bytes = ppo_work_bytes

    def _note(self, name, out=None, **kw):
        self.calls.append(name)
        if kw:   # (a gradient call: what it was handed)
            self.handed = kw
        return out

    def adv_stats(self, adv, out=None, **kw):
        return self._note("adv_stats", out)

    def lagrange(self, *a, **kw):
        self._note("lagrange")

    def adv_mix(self, adv, cadv, state, out=None, **kw):
        return self._note("adv_mix", out)

    def adam(self, *a, **kw):
        self._note("adam")

    def ppo_grad(self, *a, **kw):
        self._note("ppo_grad", stats=a[9])

    def ppo_grad_cost(self, *a, **kw):
        self._note("ppo_grad_cost", stats=a[12])

    def ppo_grad_guided(self, *a, **kw):
        self._note("ppo_grad_guided", stats=a[9], target=a[11], **kw)


def _learner(kind, immediate=False, **kw):
    """A learner on recording_engine's collector of `kind` with a guardian; the networks are real tensors of the expert's shape (the
    collector of recording_engine hands its weights through unseen, the learner copies them into its flat buffer)."""
    import torch
    from pgdrive_amd.learner import PPOLagLearner, PPOLearner
    eng, col = rc.collector(kind, engine=LearnerEngine, guardian=dict(weights=tuple(torch.zeros((rc.D, 1)) for _ in range(6)), immediate=immediate))
    net = lambda heads: tuple(torch.zeros(sh) for sh in ((rc.D, 256), (256, ), (256, 256), (256, ), (256, heads), (heads, )))  # noqa: E731
    col.policy_weights, col.value_weights, col.cost_weights = net(4), net(1), net(1)
    L = PPOLagLearner(col, cost_limit=1.0, epochs=2, minibatches=2, **kw) if kind == "safe" else PPOLearner(col, epochs=2, minibatches=2, **kw)
    batch = col.collect()
    del eng.calls[:]
    return eng, col, L, batch


@pytest.mark.parametrize("kind", ["single", "safe"])
def test_guide_none_makes_the_parents_calls_and_a_guide_the_guided_ones(kind):
    """On a collector WITH a guardian.  guide=None: update() makes the calls of before and no others, into eight statistics.  A guide:
    the same list with ppo_grad_guided in the gradient call's place, handed the batch's own tensors, into twelve."""
    lag = kind == "safe"
    head = ["lagrange", "adv_stats", "adv_stats", "adv_mix"] if lag else ["adv_stats"]
    eng, col, L, batch = _learner(kind)
    assert L.guide is None and L.stats.shape == (4, 8)
    assert L.update(batch) is L.stats
    assert eng.calls == head + ["ppo_grad_cost" if lag else "ppo_grad", "adam"] * 4, eng.calls
    for immediate in (False, True):
        eng, col, L, batch = _learner(kind, immediate, guide="takeover", bc_coef=0.25)
        assert L.stats.shape == (4, 12)
        L.update(batch)
        assert eng.calls == head + ["ppo_grad_guided", "adam"] * 4, eng.calls
        h = eng.handed
        assert h["target"] is batch["applied_actions"] and h["mask"] is batch["takeover"] and h["mask_bits"] == (3 if immediate else 1)
        assert h["bc_coef"] == 0.25 and h["keep_surrogate"] is False and h["stats"].shape == (12, )
        assert ("cost_weights" in h) == lag and (not lag or (h["cost_ret"] is batch["cost_returns"] and h["cost_grads"] is L.cost_grads))
    eng, col, L, batch = _learner(kind, guide="all", keep_surrogate=True)
    L.update(batch)
    assert eng.calls == head + ["ppo_grad_guided", "adam"] * 4
    assert eng.handed["target"] is batch["guardian_trace"] and eng.handed["mask"] is None and eng.handed["keep_surrogate"] is True


def test_ppo_guide_layout_matches_c():
    """sizeof and offsetof of pgd_ppo_guide from a C program compiled against the header == the ctypes mirror; the mode bit and the names."""
    from pgdrive_amd import _abi
    fields = [n for n, _ in _abi.PPOGuide._fields_]
    assert fields == ["target", "mask", "target_stride", "mask_bits", "bc_coef", "mode"]
    lines = ['  printf("%%zu\\n", offsetof(pgd_ppo_guide, %s));' % n for n in fields]
    prog = "#include <stdio.h>\n#include <stddef.h>\n#include \"pgdrive_hip.h\"\nint main(void) {\n" + "\n".join(lines) + \
        '\n  printf("%zu %u\\n", sizeof(pgd_ppo_guide), PGD_GUIDE_KEEP_SURROGATE);\n  return 0;\n}\n'
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "g.c"), os.path.join(td, "g")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = subprocess.check_output([exe]).decode().split()
    assert [int(x) for x in out[:6]] == [getattr(_abi.PPOGuide, n).offset for n in fields]
    assert int(out[6]) == C.sizeof(_abi.PPOGuide) == 32 and int(out[7]) == _abi.GUIDE_KEEP_SURROGATE == 1
    assert len(_abi.PPO_GUIDED_STATS) == gr.N_STATS == 12 and _abi.PPO_GUIDED_STATS[:8] == _abi.PPO_COST_STATS
    assert _abi.PPO_GUIDED_STATS[8:10] == ("guided_rows", "bc_loss")


def loop_decrease():
    """Ten adam_f64 steps (lr 3e-4, the learner's defaults otherwise) on loop_case() with every row guided and no surrogate, gradients from
    loss_and_grads_guided_f64: bc_loss before - bc_loss after."""
    c = gr.loop_case()
    k = c["in_dim"]
    nets = [np.nan_to_num(np.asarray(w, dtype=np.float64)) for w in list(c["policy"]) + list(c["value"])]
    m, v = [np.zeros_like(w) for w in nets], [np.zeros_like(w) for w in nets]

    def evaluate():
        return gr.loss_and_grads_guided_f64(c["x"][:, :k], c["action"], c["logp_old"], c["adv"], c["ret"], nets[:6], nets[6:], c["target"], None,
                                            ent_coef=0.0)

    first = evaluate()["stats"][9]
    for t in range(1, 11):
        ref = evaluate()
        g = [np.asarray(q) for q in ref["policy"] + ref["value"]]
        flat = np.concatenate([q.reshape(-1) for q in g])
        scale = min(1.0, 0.5 / (np.sqrt((flat * flat).sum()) + 1e-6))
        for i in range(12):
            nets[i], m[i], v[i] = rf.adam_f64(nets[i], g[i] * scale, m[i], v[i], t, 3e-4)
    return first - evaluate()["stats"][9]


def test_ten_reference_steps_lower_bc_loss():
    d = loop_decrease()
    print("ten float64 Adam steps lower bc_loss by %.8e" % d)
    assert d > 0 and abs(d - gr.GUIDED_LOOP_D) <= 1e-6 * abs(d)
