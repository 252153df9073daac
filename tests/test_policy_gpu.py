"""The kernels that close the loop around the step, against plain float64 restatements (tests/policy_ref.py):

* k_mlp_policy / k_mlp_prepare + k_mlp_policy_bf (pgdrive_amd/csrc/pgd_policy.h) at every input width of WIDTHS (both forms of the row
  prologue, less than one round, odd / even round counts, every residue mod 4 and mod 32), at the acceptance boundary that follows
  from the LDS formulas, at row counts around the 16-row tile, with rows permuted and NaN rows beside finite ones, on multi-agent
  engines per env group, with out_cols 3 and 4, with prepared weights re-prepared in place;
* k_lane_keep against the formula stated in include/pgdrive_hip.h;
* the closed loop policy -> step -> policy ... in the forms the benchmark times (no host synchronisation, a HIP graph of four
  iterations, two env groups on their own streams, eager and as one graph per group) against the loop run one synchronised call at a
  time: bit-identical.

Tolerances (tests/policy_ref.py): 2e-5 exact kernel, 1e-4 split-bf16 kernel, 1e-5 lane keeping; every element of every case is
compared, nothing is excluded.  tests/test_policy_ref_cpu.py shows on the CPU that the arithmetic alone keeps half of them.

Measured on an MI355X (max |action - float64|; the device adds __expf and reciprocal division to what the CPU emulation shows):
    width sweep     exact kernel  6.6e-7 unit, 8.0e-7 normalised, 2.3e-6 saturating      (emulation 5.5e-7 / 7.7e-7 / 2.1e-6; tolerance 2e-5)
                    split bf16    8.4e-6 unit, 1.7e-5 normalised, 4.0e-5 saturating      (emulation 9.0e-6 / 1.6e-5 / 4.0e-5; tolerance 1e-4)
    in_dim 448      exact 3.9e-7 / 8.5e-7, split bf16 5.6e-6 / 1.4e-5 (unit / normalised)
    4099 rows       split bf16 1.1e-5;  prepared weights re-prepared in place 5.7e-6
    lane keeping    6.4e-7 (tolerance 1e-5)
    closed loop     768 episode ends in 38,400 env-steps, mean ego speed 3.3 m/s; sampled actions within 2.9e-7 (exact) / 6.4e-6 (split bf16);
                    all four timed forms bit-identical to the synchronised loop, for both kernels
Wall time of the module: 5 s (20 tests; 7 s with the interpreter's start).

That the tests can fail -- each line changed alone in a scratch copy, library rebuilt, module run once (first test that caught it; error):
    1  mlp_layer: padded activations not zeroed (a[j] = av)            test_width_sweep[exact], in_dim 4: 0.73       (12 tests fail)
    2  mlp_store_hidden: two of the four interleaved columns swapped   test_acceptance_boundary, in_dim 448: 0.65    (13)
    3  mlp_layer_bf: the aL * bH product left out                      test_acceptance_boundary, split bf16: 2.1e-3  (14)
    4  k_mlp_prepare: head column 1 read as W3[id * 2 + 1]             test_acceptance_boundary, out_cols 3: 1.8     (4: every out_cols > 2)
    5  k_mlp_policy, second prologue: k < in_dim - 1                   test_acceptance_boundary: 1.3e-2; sweep from in_dim 321 on (12)
    6  lane_keep_action: n2 from the low half-word                     test_lane_keep_actions_match_the_stated_formula: 9.7e-2 (1)
    7  pgd_mlp_policy: row0 = g.first (without * A)                    test_multi_agent_rows_and_env_groups, group 1: rows of other groups written (2)
"""
import ctypes as C

import numpy as np
import pytest

from tests import policy_ref as pr
from tests.train_util import dev as _dev, ego_engine as _ego_engine

pytestmark = pytest.mark.gpu

SENT = 7.0  # what every output buffer holds before a launch
ERR_ARG, ERR_STATE = 1, 3
KINDS = ("exact", "bf16")
TOL = dict(exact=pr.TOL_EXACT, bf16=pr.TOL_BF16)


def _launch(eng, kind, obs, wt, out, ft, in_dim, group=-1, prep=None):
    if kind == "exact":
        eng.mlp_policy(wt, out, obs=obs, group=group, final_tanh=ft, in_dim=in_dim)
    else:
        eng.mlp_policy(None, out, obs=obs, group=group, final_tanh=ft, in_dim=in_dim, prepared=prep if prep is not None else eng.mlp_prepare(wt))


def _evaluate(eng, kind, x, w, ft, in_dim, tail=8):
    """One launch over all rows of `x` (NaN padding columns) into a sentinel-filled buffer with `tail` rows behind the last one.
    Returns the actions [rows, 2]; asserts that the tail kept the sentinel."""
    import torch
    rows = x.shape[0]
    big = torch.full((rows + tail, 2), SENT, dtype=torch.float32, device="cuda")
    _launch(eng, kind, _dev(x), tuple(_dev(v) for v in w), big[:rows], ft, in_dim)
    eng.sync()
    got = big.cpu().numpy()
    assert (got[rows:] == SENT).all(), "rows past the end were written"
    return got[:rows]


def _check(got, x, w, ft, in_dim, kind, what):
    want = pr.mlp_f64(x[:, :in_dim], w, ft)
    assert np.isfinite(got).all(), what
    err = float(np.abs(got - want).max())
    assert err < TOL[kind], (what, kind, err)
    assert np.abs(want).max() > 0.02, what  # (not a trivially small output)
    return err


# ---------------------------------------------------------------------------------------------------------------------
# 2. shapes and edges of the MLP kernels
# ---------------------------------------------------------------------------------------------------------------------
def test_acceptance_boundary_and_refused_arguments(descs):
    """The largest in_dim both kernels take follows from the LDS formulas (448, not the 4096 of the argument check): it computes
    correctly -- on a fresh engine whose first launches need the raised LDS limit --, the next width and every other bad argument is
    refused with PGD_ERR_ARG by every entry point, and nothing is written."""
    import torch
    kmax = pr.max_in_dim()
    assert kmax == 448 and pr.lds_bytes_exact(kmax) > pr.LDS_DEFAULT and pr.lds_bytes_bf16(kmax) > pr.LDS_DEFAULT
    eng = _ego_engine(descs, 20)
    try:
        for case in pr.other_cases():
            if case["name"] != "boundary":
                continue
            x, w = pr.build_case(**case)
            for kind in KINDS:
                for ft in (True, False):
                    err = _check(_evaluate(eng, kind, x, w, ft, kmax), x, w, ft, kmax, kind, case)
                    print("in_dim %d (the largest accepted), %s, %s kernel, final tanh %d: max |action - float64| = %.2e" % (
                        kmax, case["scaling"], kind, ft, err))
        # one width more: weights, prepared buffer and rows are really that large, so the refusal is the only thing tested
        k1 = kmax + 1
        L, h = eng.L, eng.h
        rng = np.random.default_rng(5)
        w = pr.make_weights(rng, k1, nan_unused=False)
        wt = [_dev(v) for v in w]
        wide = torch.zeros((20, 4100), dtype=torch.float32, device="cuda")
        out = torch.full((20, 2), SENT, dtype=torch.float32, device="cuda")
        prep = eng.mlp_prepare(tuple(wt))  # (preparing is not bound by the kernel's LDS)
        assert prep.numel() == L.pgd_mlp_prepared_bytes(k1)
        shifted = [torch.zeros(v.numel() + 4, dtype=torch.float32, device="cuda")[1:] for v in wt[:4]]  # 4 bytes off a 16-byte boundary
        prep_off = torch.zeros(prep.numel() + 16, dtype=torch.uint8, device="cuda")[4:]
        eng.sync()
        p = [C.c_void_p(t.data_ptr()) for t in wt]
        po, pa, pp = C.c_void_p(wide.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(prep.data_ptr())

        def exact(in_dim, stride=4100, hidden=256, out_cols=2, ptrs=p):
            return L.pgd_mlp_policy(h, -1, po, stride, in_dim, hidden, *ptrs, out_cols, 0, pa)

        def prepared(in_dim, stride=4100, buf=pp):
            return L.pgd_mlp_policy_prepared(h, -1, po, stride, in_dim, buf, 0, pa)

        def prepare(in_dim, hidden=256, out_cols=2, buf=pp):
            return L.pgd_mlp_prepare(h, in_dim, hidden, *p, out_cols, buf)

        assert exact(k1) == ERR_ARG and prepared(k1) == ERR_ARG
        for bad in (3, 4097):
            assert exact(bad) == ERR_ARG and prepared(bad) == ERR_ARG and prepare(bad) == ERR_ARG and L.pgd_mlp_prepared_bytes(bad) == 0
        assert exact(kmax, hidden=128) == ERR_ARG and prepare(kmax, hidden=128) == ERR_ARG
        assert exact(kmax, out_cols=1) == ERR_ARG and prepare(kmax, out_cols=1) == ERR_ARG
        assert exact(kmax, stride=kmax - 1) == ERR_ARG and prepared(kmax, stride=kmax - 1) == ERR_ARG
        for i in range(4):  # w1, b1, w2, b2 are read 16 bytes at a time
            assert shifted[i].data_ptr() % 16 == 4
            q = list(p)
            q[i] = C.c_void_p(shifted[i].data_ptr())
            assert exact(kmax, ptrs=q) == ERR_ARG, i
        off = C.c_void_p(prep_off.data_ptr())
        assert prep_off.data_ptr() % 16 == 4 and prepared(kmax, buf=off) == ERR_ARG and prepare(kmax, buf=off) == ERR_ARG
        eng.sync()
        assert bool((out == SENT).all()), "a refused call wrote actions"
        assert exact(kmax, stride=kmax) == 0 and prepared(kmax) == 0  # (the same calls with good arguments are taken)
        eng.sync()
        assert not bool((out == SENT).any())
    finally:
        eng.close()


@pytest.mark.parametrize("kind", KINDS)
def test_width_sweep(descs, kind):
    """Every width of the sweep in three scalings, final tanh off and on, against float64 per element; one engine, widths ascending --
    the launches cross the line above which the kernel's LDS limit is raised on the way up, and the first widths run again afterwards
    (down across the line) must give the same bits as before."""
    eng = _ego_engine(descs, pr.SWEEP_ROWS)
    try:
        worst, first = {}, {}
        for case in pr.sweep_cases():
            x, w = pr.build_case(**case)
            k = case["in_dim"]
            if case["scaling"] == "saturating":
                p = np.abs(pr.hidden_preact_f64(x[:, :k], w))
                assert (p > 5.0).mean() > 0.1 and (p > pr.CLAMP).any()
            for ft in (False, True):
                got = _evaluate(eng, kind, x, w, ft, k)
                err = _check(got, x, w, ft, k, kind, case)
                worst[case["scaling"]] = max(worst.get(case["scaling"], 0.0), err)
                first[(k, case["scaling"], ft)] = got
        for case in pr.sweep_cases():
            if case["in_dim"] in (4, 33, 128, 274, 448):
                x, w = pr.build_case(**case)
                for ft in (False, True):
                    again = _evaluate(eng, kind, x, w, ft, case["in_dim"])
                    assert np.array_equal(again.view(np.int32), first[(case["in_dim"], case["scaling"], ft)].view(np.int32)), case
        for sc in pr.SCALINGS:
            print("width sweep, %s kernel, %-10s: max |action - float64| = %.2e (tolerance %.0e)" % (kind, sc, worst[sc], TOL[kind]))
    finally:
        eng.close()


@pytest.mark.parametrize("rows", pr.ROW_COUNTS)
def test_row_counts(descs, rows):
    """Engines of 1, 15, 16, 17, 33 and 4099 rows: the last tile partly empty, rows past the end never written."""
    eng = _ego_engine(descs, rows)
    try:
        for case in pr.row_cases():
            if case["rows"] != rows:
                continue
            x, w = pr.build_case(**case)
            for kind in KINDS:
                for ft in (False, True):
                    err = _check(_evaluate(eng, kind, x, w, ft, case["in_dim"], tail=40), x, w, ft, case["in_dim"], kind, case)
            print("%d rows, in_dim %d: ok (split bf16, final tanh: %.2e)" % (rows, case["in_dim"], err))
    finally:
        eng.close()


@pytest.mark.parametrize("kind", KINDS)
def test_row_position_invariance(descs, kind):
    """A row's result depends on nothing but the row: permuted rows give the permuted actions bit for bit, and NaN rows next to finite
    ones leave the finite rows' bits alone."""
    eng = _ego_engine(descs, 40)
    try:
        for case in pr.other_cases():
            if case["name"] != "permute":
                continue
            x, w = pr.build_case(**case)
            k = case["in_dim"]
            base = _evaluate(eng, kind, x, w, True, k)
            _check(base, x, w, True, k, kind, case)
            rng = np.random.default_rng(k)
            for _ in range(3):
                perm = rng.permutation(x.shape[0])
                got = _evaluate(eng, kind, x[perm], w, True, k)
                assert np.array_equal(got.view(np.int32), base[perm].view(np.int32)), (case, "permutation")
            bad = np.array([0, 3, 17, 18, 39])
            x2 = x.copy()
            x2[bad] = np.nan
            got = _evaluate(eng, kind, x2, w, True, k)
            keep = np.setdiff1d(np.arange(x.shape[0]), bad)
            assert np.array_equal(got[keep].view(np.int32), base[keep].view(np.int32)), (case, "NaN rows")
    finally:
        eng.close()


@pytest.mark.parametrize("agents,n_envs,n_groups", [(8, 8, 4), (5, 6, 2)])
def test_multi_agent_rows_and_env_groups(agents, n_envs, n_groups):
    """rows = envs x agents; group g covers rows [first * A, (first + count) * A): 16 rows per group with 8 seats, 15 with 5.  While
    group g runs, the observation rows of the other groups hold NaN and their action rows the sentinel."""
    import torch
    from pgdrive_amd.engine import Engine
    from tests import util
    _, mb, sb = util.make_marl_banks(num_agents=agents)
    eng = Engine(util.marl_config(n_envs, sb), mb, sb)
    try:
        assert eng.A == agents
        rows, per = n_envs * agents, n_envs // n_groups * agents
        cases = [c for c in pr.other_cases() if c["name"] == "marl" and c["rows"] == rows]
        assert len(cases) == 2
        for case in cases:
            x, w = pr.build_case(**case)
            k = case["in_dim"]
            for kind in KINDS:
                _check(_evaluate(eng, kind, x, w, False, k), x, w, False, k, kind, case)  # the whole batch
        eng.set_groups(n_groups)
        for case in cases:
            x, w = pr.build_case(**case)
            k = case["in_dim"]
            wt = tuple(_dev(v) for v in w)
            prep = eng.mlp_prepare(wt)
            eng.sync()
            want = pr.mlp_f64(x[:, :k], w, True)
            for kind in KINDS:
                for g in range(n_groups):
                    mine = slice(g * per, (g + 1) * per)
                    xg = np.full_like(x, np.nan)
                    xg[mine] = x[mine]
                    obs = _dev(xg)
                    out = torch.full((n_envs, agents, 2), SENT, dtype=torch.float32, device="cuda")
                    torch.cuda.synchronize()
                    _launch(eng, kind, obs, wt, out, True, k, group=g, prep=prep)
                    eng.group_sync(g)
                    got = out.view(rows, 2).cpu().numpy()
                    other = np.ones(rows, dtype=bool)
                    other[mine] = False
                    assert (got[other] == SENT).all(), (case, kind, g, "rows of other groups written")
                    assert np.isfinite(got[mine]).all() and np.abs(got[mine] - want[mine]).max() < TOL[kind], (case, kind, g)
    finally:
        eng.close()


@pytest.mark.parametrize("kind", KINDS)
def test_out_cols_3_and_4_with_nan_in_the_unused_columns(descs, kind):
    eng = _ego_engine(descs, 24)
    try:
        for case in pr.other_cases():
            if case["name"] != "out_cols":
                continue
            x, w = pr.build_case(**case)
            assert w[4].shape[1] == case["out_cols"] and np.isnan(w[4][:, 2:]).all() and np.isnan(w[5][2:]).all()
            for ft in (False, True):
                _check(_evaluate(eng, kind, x, w, ft, case["in_dim"]), x, w, ft, case["in_dim"], kind, case)
    finally:
        eng.close()


def test_prepared_weights_are_a_pure_function_and_updates_are_seen(descs):
    """pgd_mlp_prepare into NaN-filled buffers: two buffers come out byte for byte alike, the kernel reads no NaN from them (checked
    through the result), and preparing other weights into the same buffer on the same stream is seen by the next launch."""
    import torch
    eng = _ego_engine(descs, 24)
    try:
        for k in (33, 275, 352):
            (xa, wa), (xb, wb) = [pr.build_case(**c) for c in pr.other_cases() if c["name"] == "prepared" and c["in_dim"] == k]
            nbytes = int(eng.L.pgd_mlp_prepared_bytes(k))
            bufs = [torch.full((nbytes, ), 0xff, dtype=torch.uint8, device="cuda") for _ in range(2)]

            def prepare(wt, buf):
                assert eng.L.pgd_mlp_prepare(eng.h, k, 256, *[C.c_void_p(t.data_ptr()) for t in wt], int(wt[4].shape[1]),
                                             C.c_void_p(buf.data_ptr())) == 0
            wta, wtb = tuple(_dev(v) for v in wa), tuple(_dev(v) for v in wb)
            oa, ob = _dev(xa), _dev(xb)
            outa = torch.full((24, 1, 2), SENT, dtype=torch.float32, device="cuda")
            outb = torch.full((24, 1, 2), SENT, dtype=torch.float32, device="cuda")
            prepare(wta, bufs[0])
            prepare(wta, bufs[1])
            eng.sync()
            assert torch.equal(bufs[0], bufs[1])
            untouched = int((bufs[0].view(torch.int32) == -1).sum())
            assert untouched <= 2  # (the buffer's size is rounded up behind b3; 0xffffffff is no value a split produces elsewhere)
            # no synchronisation from here on: launch, re-prepare in place, launch
            eng.mlp_policy(None, outa, obs=oa, in_dim=k, prepared=bufs[0])
            prepare(wtb, bufs[0])
            eng.mlp_policy(None, outb, obs=ob, in_dim=k, prepared=bufs[0])
            eng.sync()
            assert not torch.equal(bufs[0], bufs[1])
            ea = _check(outa.view(24, 2).cpu().numpy(), xa, wa, False, k, "bf16", ("prepared", k, "first weights"))
            eb = _check(outb.view(24, 2).cpu().numpy(), xb, wb, False, k, "bf16", ("prepared", k, "weights prepared in place"))
            print("prepared weights, in_dim %d: %.2e, after the update %.2e" % (k, ea, eb))
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. pgd_lane_keep_actions against the formula of include/pgdrive_hip.h
# ---------------------------------------------------------------------------------------------------------------------
GAINS = (dict(k_lat=1.0, k_head=2.0, v_target_kmh=30.0), dict(k_lat=1.5, k_head=1.25, v_target_kmh=45.0))
TICKS = (0, 1, 2 ** 31, 2 ** 32 - 1)


def test_lane_keep_actions_match_the_stated_formula(descs):
    """Synthetic rows (columns 0 .. 3 set, the rest NaN) on an engine with seed and env_base non-zero and N no multiple of 256.
    Tolerance 1e-5, derived: the throttle term is 0.3 * (v_target - (81 o3 - 1)) -- two roundings near 81 .. 128 (half an ulp each,
    3.8e-6) times 0.3, plus ulps of O(1) terms: about 2.4e-6; the steering term is O(1) throughout."""
    import torch
    n, seed, base = 300, 11, 1000
    eng = _ego_engine(descs, n, seed=seed, env_base=base)
    try:
        assert eng.A == 1 and eng.D >= 4
        rng = np.random.default_rng(4)
        out = torch.full((n + 8, 2), SENT, dtype=torch.float32, device="cuda")
        worst = 0.0
        for gains in GAINS:
            o = np.full((n, eng.D), np.nan, dtype=np.float32)
            o[:, 0:2] = rng.uniform(0, 1, size=(n, 2))
            o[:, 2] = rng.uniform(0.2, 0.8, size=n)
            o[:, 3] = (gains["v_target_kmh"] + 1.0) / 81.0 + rng.uniform(-0.1, 0.1, size=n)
            obs = _dev(o)
            for noise in (0.0, 0.05):
                for tick in TICKS:
                    out.fill_(SENT)
                    eng.lane_keep_actions(out[:n], tick, obs=obs, noise=noise, **gains)
                    eng.sync()
                    got = out.cpu().numpy()
                    assert (got[n:] == SENT).all()
                    want, raw = pr.lane_keep_f64(o, seed, base, tick, noise=noise, **gains)
                    for c in range(2):  # both outputs land below, inside and above the clip
                        assert min((raw[:, c] < -1.05).mean(), (np.abs(raw[:, c]) < 0.95).mean(), (raw[:, c] > 1.05).mean()) > 0.08, (gains, c)
                    err = float(np.abs(got[:n] - want).max())
                    worst = max(worst, err)
                    assert err < pr.TOL_LANE_KEEP, (gains, noise, tick, err)
        print("lane keeping: max |action - float64| = %.2e (tolerance %.0e)" % (worst, pr.TOL_LANE_KEEP))
        # the noise alone: every row centred, aligned and at the target speed, so that the action IS noise * (n1, n2)
        o = np.full((n, eng.D), np.nan, dtype=np.float32)
        o[:, 0:3] = 0.5
        o[:, 3] = 31.0 / 81.0
        obs = _dev(o)
        acts = []
        for tick in TICKS:
            eng.lane_keep_actions(out[:n], tick, obs=obs, noise=0.05)
            eng.sync()
            acts.append(out[:n].cpu().numpy().copy())
            want, _ = pr.lane_keep_f64(o, seed, base, tick, noise=0.05)
            assert np.abs(acts[-1] - want).max() < pr.TOL_LANE_KEEP
            assert (np.abs(acts[-1][:, 0] - acts[-1][:, 1]) > 1e-4).mean() > 0.98, "the two noise values of an env are the same"
            assert np.abs(acts[-1]).max() <= 0.05 + 1e-5 and acts[-1].std() > 0.025  # (U(-0.05, 0.05): 0.0289)
        for i in range(len(TICKS)):
            for j in range(i):
                assert (np.abs(acts[i] - acts[j]) > 1e-4).all(axis=1).mean() > 0.95, "the noise does not change with the tick"
    finally:
        eng.close()


def test_lane_keep_actions_refuses_other_row_layouts(descs):
    import torch
    from pgdrive_amd.engine import Engine
    from tests import util
    _, mb, sb = util.make_marl_banks(num_agents=8)
    engs = [Engine(util.marl_config(4, sb), mb, sb), _ego_engine(descs, 4, side_lasers=120)]
    try:
        for eng in engs:
            out = torch.full((eng.N * eng.A, 2), SENT, dtype=torch.float32, device="cuda")
            rc = eng.L.pgd_lane_keep_actions(eng.h, C.c_void_p(eng.obs.data_ptr()), C.c_void_p(out.data_ptr()), 1.0, 2.0, 30.0, 0.05, 0)
            eng.sync()
            assert rc == ERR_STATE and bool((out == SENT).all())
    finally:
        for eng in engs:
            eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the closed loop in its timed forms equals the synchronised loop
# ---------------------------------------------------------------------------------------------------------------------
LOOP_N, LOOP_ITERS, WARM, UNROLL = 128, 300, 20, 4
SAMPLED = (0, 1, 50, 150, 299)


def _bits_equal(a, b):
    import torch
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


class _Loop:
    """An engine of the default configuration and what its loop needs; every instance starts from the same state."""
    def __init__(self, descs, kind, groups=1):
        import torch
        from pgdrive_amd import _abi
        from pgdrive_amd.engine import Engine
        from tests import util
        mb, sb = util.make_banks(descs, n_maps=8)
        self.eng = eng = Engine(_abi.make_config(LOOP_N, auto_reset=1, seed=5), mb, sb)
        eng.reset(np.arange(LOOP_N) % 8)
        rng = np.random.default_rng(0)  # (examples/fused_policy_rollout.py: random weights, a bias towards the throttle -- the cars drive)
        D = eng.D
        self.w = [np.ascontiguousarray(v, dtype=np.float32) for v in (
            rng.normal(0, D ** -0.5, (D, 256)), np.zeros(256), rng.normal(0, 1 / 16, (256, 256)), np.zeros(256),
            rng.normal(0, 1 / 16, (256, 2)), np.array([0.0, 0.5]))]
        # the steering column of the head scaled down: with the example's weights the steering is tanh of an N(0, 1) value and every car
        # leaves the road within 17 steps of its reset, still below 2 m/s; with 0.05 the episodes last about 50 steps and the cars get
        # up to speed (chosen on the fp64 oracle under mlp_f64 as policy: 768 episode ends, 3.3 m/s)
        self.w[4][:, 0] *= 0.05
        self.wt = tuple(_dev(v) for v in self.w)
        self.act = torch.zeros((LOOP_N, 1, 2), dtype=torch.float32, device="cuda")
        if groups > 1:
            eng.set_groups(groups)
        self.prep = eng.mlp_prepare(self.wt) if kind == "bf16" else None
        eng.sync()
        torch.cuda.synchronize()

    def iteration(self, group=-1):
        self.eng.mlp_policy(self.wt, self.act, group=group, final_tanh=True, prepared=self.prep)
        if group < 0:
            return self.eng.step(self.act)
        return self.eng.step_group(group, self.act)

    def outputs(self):
        return self.eng.obs, self.eng.reward, self.eng.done, self.eng.flags


def _history():
    import torch
    return [torch.zeros((LOOP_ITERS, ) + tuple(t.shape), dtype=t.dtype, device="cuda") for t in (
        torch.empty((LOOP_N, 1, 274)), torch.empty((LOOP_N, 1)), torch.empty((LOOP_N, 1), dtype=torch.uint8),
        torch.empty((LOOP_N, 1), dtype=torch.int32))]


def _same_integer_state(a, b, what):
    (_, ia, eia), (_, ib, eib) = a, b
    assert (ia == ib).all() and (eia == eib).all(), what


@pytest.mark.parametrize("kind", KINDS)
def test_closed_loop_forms_equal_the_synchronised_loop(descs, kind):
    import torch
    # S: every call followed by a full device synchronisation
    S = _Loop(descs, kind)
    assert S.eng.D == 274
    hist = _history()
    worst = 0.0
    for t in range(LOOP_ITERS):
        before = S.eng.obs.view(LOOP_N, -1).cpu().numpy() if t in SAMPLED else None
        S.eng.mlp_policy(S.wt, S.act, final_tanh=True, prepared=S.prep)
        torch.cuda.synchronize()
        if t in SAMPLED:  # the action against float64 of the observation it was computed from
            got = S.act.view(LOOP_N, 2).cpu().numpy()
            err = float(np.abs(got - pr.mlp_f64(before, S.w, True)).max())
            worst = max(worst, err)
            assert np.isfinite(got).all() and err < TOL[kind], (t, err)
        out = S.eng.step(S.act)
        torch.cuda.synchronize()
        for h, o in zip(hist, out):
            h[t].copy_(o)
    torch.cuda.synchronize()
    state_s = S.eng.get_state()
    n_done = int(hist[2].sum())
    speed = float((81.0 * hist[0][:, :, 0, 3].double().mean().item() - 1.0) / 3.6)  # state_obs.py:82, over all env-steps [m/s]
    print("closed loop, %s kernel: %d episode ends in %d env-steps, mean ego speed %.1f m/s, sampled actions within %.2e of float64" % (
        kind, n_done, LOOP_N * LOOP_ITERS, speed, worst))
    assert n_done >= 20 and speed > 2.0  # the cars drive, leave the road, and reset rows pass through the policy
    S.eng.close()

    # (a) the same calls with no synchronisation inside the loop, on a non-default stream
    A = _Loop(descs, kind)
    mine = _history()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        for t in range(LOOP_ITERS):
            out = A.iteration()
            for h, o in zip(mine, out):
                h[t].copy_(o)
    torch.cuda.synchronize()
    for name, h, m in zip(("obs", "reward", "done", "flags"), hist, mine):
        assert _bits_equal(h, m), "no synchronisation: %s differs" % name
    _same_integer_state(state_s, A.eng.get_state(), "no synchronisation")
    A.eng.close()
    del mine

    # (b) four iterations captured in one HIP graph and replayed, as examples/fused_policy_rollout.py does it
    B = _Loop(descs, kind)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        for _ in range(WARM):
            B.iteration()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(g, stream=s):
        for _ in range(UNROLL):
            B.iteration()
    torch.cuda.synchronize()
    t = WARM
    with torch.cuda.stream(s), torch.no_grad():
        while t + UNROLL <= LOOP_ITERS:
            g.replay()
            torch.cuda.synchronize()
            t += UNROLL
            for name, h, o in zip(("obs", "reward", "done", "flags"), hist, B.outputs()):
                assert _bits_equal(h[t - 1], o), "graph: %s differs after iteration %d" % (name, t)
    assert t == LOOP_ITERS
    _same_integer_state(state_s, B.eng.get_state(), "graph")
    del g
    B.eng.close()

    # (c) two env groups, each its own policy(group) -> step_group loop on its stream, nothing between the groups
    G = _Loop(descs, kind, groups=2)
    gs = G.eng.group_streams
    mine = _history()
    cur = torch.cuda.current_stream()
    for k in range(2):
        gs[k].wait_stream(cur)
    with torch.no_grad():
        for t in range(LOOP_ITERS):
            for k in range(2):
                sl = G.eng.group_slice(k)
                with torch.cuda.stream(gs[k]):
                    out = G.iteration(group=k)
                    for h, o in zip(mine, out):
                        h[t, sl].copy_(o)
    torch.cuda.synchronize()
    for name, h, m in zip(("obs", "reward", "done", "flags"), hist, mine):
        assert _bits_equal(h, m), "env groups: %s differs" % name
    _same_integer_state(state_s, G.eng.get_state(), "env groups")
    G.eng.close()
    del mine

    # (d) the same as one single-stream graph per group, replayed on the group's stream (bench.py's groups_graph)
    G = _Loop(descs, kind, groups=2)
    gs = G.eng.group_streams
    cur = torch.cuda.current_stream()
    graphs = []
    with torch.no_grad():
        for k in range(2):
            gs[k].wait_stream(cur)
            with torch.cuda.stream(gs[k]):
                for _ in range(WARM):
                    G.iteration(group=k)
        torch.cuda.synchronize()
        for k in range(2):
            gk = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gk, stream=gs[k]):
                for _ in range(UNROLL):
                    G.iteration(group=k)
            graphs.append(gk)
        torch.cuda.synchronize()
        t = WARM
        while t + UNROLL <= LOOP_ITERS:
            for k in range(2):
                with torch.cuda.stream(gs[k]):
                    graphs[k].replay()
            torch.cuda.synchronize()
            t += UNROLL
            for name, h, o in zip(("obs", "reward", "done", "flags"), hist, G.outputs()):
                assert _bits_equal(h[t - 1], o), "one graph per env group: %s differs after iteration %d" % (name, t)
    assert t == LOOP_ITERS
    _same_integer_state(state_s, G.eng.get_state(), "one graph per env group")
    del graphs
    G.eng.close()
