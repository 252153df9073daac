"""k_mlp_actor_critic, k_gae (pgdrive_amd/csrc/pgd_actor_critic.h) and pgdrive_amd.rollout.RolloutCollector on the device, against the
float64 restatement of tests/actor_critic_ref.py:

* means, log_stds, sampled actions, log-probabilities and values at every width of the sweep (both forms of the row prologue, the
  derived limit), at row counts around the 16-row tile, with out_cols 4, 5, 6 (NaN beyond column 3) and NaN in the row padding;
* the noise itself (a head of zeros returns z), its dependence on seed, tick and the GLOBAL row, bit-identical repeats;
* rows permuted; env groups and a multi-agent engine (only the group's rows are written); no critic; refused arguments;
* GAE at every shape and done pattern of the checker;
* the collector against the same calls made one at a time with a synchronisation behind each, eagerly and from a HIP graph: every
  tensor bit-identical.

Tolerances (tests/actor_critic_ref.py): heads 2e-5; z 2.74e-6; action and logp propagated per element; GAE 9.74e-6.
tests/test_actor_critic_cpu.py shows on the CPU that the arithmetic alone keeps half of each.
"""
import ctypes as C

import numpy as np
import pytest

from tests import actor_critic_ref as ar
from tests import policy_ref as pr
from tests.train_util import ERR_ARG, KEYS, SENT, Traffic, ac_nets as _nets, bits_equal as _bits_equal, dev as _dev, eager_then_graph, \
    ego_engine as _ego_engine, make_collector, snapshot as _snapshot, synchronised_rollouts

pytestmark = pytest.mark.gpu


def _run(eng, x, policy, value, seed, tick, in_dim, det=False, group=-1, tail=8):
    """One launch over the rows of `x` into sentinel-filled buffers with `tail` rows behind the last one -> (act, logp, value) as numpy;
    value is None without a critic."""
    import torch
    rows = x.shape[0]
    act = torch.full((rows + tail, 2), SENT, dtype=torch.float32, device="cuda")
    logp = torch.full((rows + tail, ), SENT, dtype=torch.float32, device="cuda")
    val = torch.full((rows + tail, ), SENT, dtype=torch.float32, device="cuda")
    pw = tuple(_dev(w) for w in policy)
    vw = tuple(_dev(w) for w in value) if value is not None else None
    torch.cuda.synchronize()
    eng.mlp_actor_critic(pw, vw, act[:rows], logp[:rows], val[:rows] if vw is not None else None, seed, tick, obs=_dev(x), group=group,
                         deterministic=det, in_dim=in_dim)
    if group >= 0:
        eng.group_sync(group)
    eng.sync()
    a, lp, v = act.cpu().numpy(), logp.cpu().numpy(), val.cpu().numpy()
    assert (a[rows:] == SENT).all() and (lp[rows:] == SENT).all() and (v[rows:] == SENT).all(), "rows past the end were written"
    if vw is None:
        assert (v == SENT).all(), "no critic, but the value buffer was written"
    return a[:rows], lp[:rows], (v[:rows] if vw is not None else None)


def _check_case(eng, c, rows_global=None, tail=8):
    """The deterministic and the sampled launch of one case against float64.  Returns the case's arrays and the sampled outputs."""
    x, p, v = ar.build_case(**c)
    k = c["in_dim"]
    mean, ls, val = ar.heads_f64(x[:, :k], p, v)
    g = np.arange(c["rows"]) if rows_global is None else rows_global
    z = ar.noise_f64(c["seed"], g, c["tick"])
    a64, l64 = ar.sample_f64(mean, ls, z)
    # deterministic: the action is the mean, logp the density at the mean (-log_std0 - log_std1 - log 2 pi)
    a, lp, vv = _run(eng, x, p, v, c["seed"], c["tick"], k, det=True, tail=tail)
    assert np.isfinite(a).all() and np.isfinite(lp).all() and np.isfinite(vv).all(), c
    e_mean, e_val = float(np.abs(a - mean).max()), float(np.abs(vv - val).max())
    e_ls = float(np.abs(lp - (-ls.sum(axis=1) - ar.LOG_2PI)).max())
    print("%s: |mean - f64| %.2e, |value - f64| %.2e, |log_std0 + log_std1 - f64| %.2e" % (c, e_mean, e_val, e_ls))
    assert e_mean < pr.TOL_EXACT and e_val < pr.TOL_EXACT and e_ls < 2 * pr.TOL_EXACT + 4 * ar.EPS * 8.0, c
    det_val = vv
    # sampled
    a, lp, vv = _run(eng, x, p, v, c["seed"], c["tick"], k, tail=tail)
    assert np.isfinite(a).all() and np.isfinite(lp).all(), c
    fa = float((np.abs(a - a64) / ar.tol_action(mean, ls, z)).max())
    fl = float((np.abs(lp - l64) / ar.tol_logp(ls, z)).max())
    print("    sampled: action %.3f, logp %.3f of their tolerances (max |action - f64| %.2e, |logp - f64| %.2e)" % (
        fa, fl, np.abs(a - a64).max(), np.abs(lp - l64).max()))
    assert fa < 1.0 and fl < 1.0, (c, fa, fl)
    assert np.array_equal(vv.view(np.int32), det_val.view(np.int32)), (c, "the value depends on the sampling")
    assert c["rows"] < 15 or np.abs(a - mean).max() > 0.05, (c, "no noise in the sampled action")
    return x, p, v, (a, lp, vv)


def _one_log_std(p, which):
    """The policy with the OTHER log_std column zeroed: the deterministic logp is then -log_std[which] - log 2 pi."""
    q = [w.copy() for w in p]
    q[4][:, 3 - which] = 0.0   # column 2 or 3
    q[5][3 - which] = 0.0
    return q


# ---------------------------------------------------------------------------------------------------------------------
# shapes and edges of the network kernel
# ---------------------------------------------------------------------------------------------------------------------
def test_width_sweep(descs):
    """Every width in two scalings, out_cols cycling through 4, 5, 6, ticks 0, 1, 2^31, 2^32 - 1; one engine, widths ascending across
    the line above which the LDS limit is raised; each log_std recovered alone; the first widths again afterwards: the same bits."""
    eng = _ego_engine(descs, ar.SWEEP_ROWS)
    try:
        first = {}
        for c in ar.sweep_cases():
            x, p, v, got = _check_case(eng, c)
            first[(c["in_dim"], c["scaling"])] = got
            k = c["in_dim"]
            _, ls, _ = ar.heads_f64(x[:, :k], p, None)
            for which in (0, 1):
                _, lp, _ = _run(eng, x, _one_log_std(p, which), None, 0, 0, k, det=True)
                err = float(np.abs(-lp - ar.LOG_2PI - ls[:, which]).max())
                assert err < pr.TOL_EXACT + 4 * ar.EPS * 8.0, (c, "log_std", which, err)
        assert ar.max_in_dim() in [k for k, _ in first]
        for c in ar.sweep_cases():
            if c["in_dim"] in (4, 274, ar.max_in_dim()):
                x, p, v = ar.build_case(**c)
                again = _run(eng, x, p, v, c["seed"], c["tick"], c["in_dim"])
                for a, b in zip(again, first[(c["in_dim"], c["scaling"])]):
                    assert np.array_equal(a.view(np.int32), b.view(np.int32)), (c, "not the same bits twice")
    finally:
        eng.close()


@pytest.mark.parametrize("rows", ar.ROW_COUNTS)
def test_row_counts(descs, rows):
    """Engines of 1, 15, 16, 17, 33 and 4099 rows: the last tile partly empty, rows past the end never written."""
    eng = _ego_engine(descs, rows)
    try:
        for c in ar.row_cases():
            if c["rows"] == rows:
                _check_case(eng, c, tail=40)
    finally:
        eng.close()


def _zero_head(in_dim=4, out_cols=4):
    p = pr.make_weights(np.random.default_rng(1), in_dim, 1.0, out_cols, nan_unused=False)
    p[4][:] = 0.0
    p[5][:] = 0.0
    return p


def test_the_noise_itself(descs):
    """w3 = 0, b3 = 0: the action is z, logp = -0.5 |z|^2 - log 2 pi.  Against the restated generator at every run of NOISE_RUNS (4099
    rows; engines whose env_base is not zero: the noise is a function of the GLOBAL row); other seeds and ticks give other noise."""
    p = _zero_head()
    seen = {}
    for n, base in sorted(set((n, base) for n, base, _, _ in ar.NOISE_RUNS)):
        eng = _ego_engine(descs, n, env_base=base)
        try:
            x = np.zeros((n, 4), dtype=np.float32)
            for n2, base2, seed, tick in ar.NOISE_RUNS:
                if (n2, base2) != (n, base):
                    continue
                a, lp, _ = _run(eng, x, p, None, seed, tick, 4)
                z = ar.noise_f64(seed, base + np.arange(n), tick)
                err = float(np.abs(a - z).max())
                print("noise, %d rows from global row %d, seed %#x, tick %#x: max |z - f64| = %.2e (TOL_Z %.2e), max |z| %.2f" % (
                    n, base, seed, tick, err, ar.TOL_Z, np.abs(z).max()))
                assert np.isfinite(a).all() and err < ar.TOL_Z, (n, base, seed, tick, err)
                zero = np.zeros_like(z)
                assert (np.abs(lp - ar.sample_f64(zero, zero, z)[1]) < ar.tol_logp(zero, z)).all()
                a2, lp2, _ = _run(eng, x, p, None, seed, tick, 4)
                assert np.array_equal(a.view(np.int32), a2.view(np.int32)) and np.array_equal(lp.view(np.int32), lp2.view(np.int32))
                seen[(n, base, seed, tick)] = a
        finally:
            eng.close()
    big = [v for (n, _, _, _), v in seen.items() if n == ar.NOISE_ROWS]
    assert len(big) == 5
    for i in range(len(big)):
        for j in range(i):  # another seed or tick: other noise in (nearly) every row
            assert (big[i] == big[j]).mean() < 0.001
    small = [v for (n, _, _, _), v in seen.items() if n == 33]
    assert len(small) == 2 and not np.array_equal(small[0], small[1])


def test_row_position_invariance(descs):
    """Permuted observation rows: means and values are the permuted ones bit for bit, while the noise stays with the row index."""
    eng = _ego_engine(descs, 40)
    try:
        for c in ar.other_cases():
            if c["name"] != "permute":
                continue
            x, p, v, _ = _check_case(eng, c)
            k = c["in_dim"]
            mean0, _, val0 = _run(eng, x, p, v, c["seed"], c["tick"], k, det=True)
            m64, ls64, _ = ar.heads_f64(x[:, :k], p, v)
            z = ar.noise_f64(c["seed"], np.arange(40), c["tick"])
            rng = np.random.default_rng(k)
            for _ in range(3):
                perm = rng.permutation(40)
                mean1, lpd, val1 = _run(eng, x[perm], p, v, c["seed"], c["tick"], k, det=True)
                assert np.array_equal(mean1.view(np.int32), mean0[perm].view(np.int32)), (c, "means")
                assert np.array_equal(val1.view(np.int32), val0[perm].view(np.int32)), (c, "values")
                a, lp, _ = _run(eng, x[perm], p, v, c["seed"], c["tick"], k)
                a64, l64 = ar.sample_f64(m64[perm], ls64[perm], z)  # row i: the network's output for x[perm[i]], the noise of row i
                assert (np.abs(a - a64) < ar.tol_action(m64[perm], ls64[perm], z)).all(), (c, "actions")
                assert (np.abs(lp - l64) < ar.tol_logp(ls64[perm], z)).all(), (c, "logp")
    finally:
        eng.close()


def _check_groups(eng, c, n_groups, per):
    """Group g alone: its rows against float64 (noise of the global row), the sentinel everywhere else in actions, logp and value."""
    import torch
    x, p, v = ar.build_case(**c)
    k, rows = c["in_dim"], c["rows"]
    assert rows == eng.N * eng.A and per * n_groups == rows
    mean, ls, val = ar.heads_f64(x[:, :k], p, v)
    z = ar.noise_f64(c["seed"], np.arange(rows), c["tick"])
    a64, l64 = ar.sample_f64(mean, ls, z)
    pw, vw = tuple(_dev(w) for w in p), tuple(_dev(w) for w in v)
    for g in range(n_groups):
        mine = slice(g * per, (g + 1) * per)
        xg = np.full_like(x, np.nan)
        xg[mine] = x[mine]
        act = torch.full((eng.N, eng.A, 2), SENT, dtype=torch.float32, device="cuda")
        logp = torch.full((eng.N, eng.A), SENT, dtype=torch.float32, device="cuda")
        value = torch.full((eng.N, eng.A), SENT, dtype=torch.float32, device="cuda")
        obs = _dev(xg)
        torch.cuda.synchronize()
        eng.mlp_actor_critic(pw, vw, act, logp, value, c["seed"], c["tick"], obs=obs, group=g, in_dim=k)
        eng.group_sync(g)
        a, lp, vv = act.view(rows, 2).cpu().numpy(), logp.view(rows).cpu().numpy(), value.view(rows).cpu().numpy()
        other = np.ones(rows, dtype=bool)
        other[mine] = False
        assert (a[other] == SENT).all() and (lp[other] == SENT).all() and (vv[other] == SENT).all(), (c, g, "rows of other groups written")
        assert np.isfinite(a[mine]).all() and np.isfinite(lp[mine]).all() and np.isfinite(vv[mine]).all(), (c, g)
        assert (np.abs(a[mine] - a64[mine]) < ar.tol_action(mean, ls, z)[mine]).all(), (c, g)
        assert (np.abs(lp[mine] - l64[mine]) < ar.tol_logp(ls, z)[mine]).all(), (c, g)
        assert np.abs(vv[mine] - val[mine]).max() < pr.TOL_EXACT, (c, g)


def test_env_groups(descs):
    """16 single-agent envs in 2 groups of 8, each on its group's stream."""
    eng = _ego_engine(descs, 16)
    try:
        c = [c for c in ar.other_cases() if c["name"] == "groups"][0]
        _check_case(eng, c)
        eng.set_groups(2)
        _check_groups(eng, c, 2, 8)
    finally:
        eng.close()


def test_multi_agent_rows_and_env_groups():
    """rows = envs x agents (6 x 5); group g covers rows [first * A, (first + count) * A): 15 rows per group."""
    from pgdrive_amd.engine import Engine
    from tests import util
    _, mb, sb = util.make_marl_banks(num_agents=5)
    eng = Engine(util.marl_config(6, sb), mb, sb)
    try:
        assert eng.A == 5
        c = [c for c in ar.other_cases() if c["name"] == "marl"][0]
        _check_case(eng, c)
        eng.set_groups(2)
        _check_groups(eng, c, 2, 15)
    finally:
        eng.close()


def test_no_critic_leaves_the_value_buffer_alone(descs):
    """All six value pointers null: one row of workgroups; d_value is not touched even when it is given."""
    import torch
    eng = _ego_engine(descs, 24)
    try:
        c = [c for c in ar.other_cases() if c["name"] == "nocritic"][0]
        x, p, v, (a_with, lp_with, _) = _check_case(eng, c)
        k = c["in_dim"]
        a, lp, none = _run(eng, x, p, None, c["seed"], c["tick"], k)  # (asserts the sentinel in the value buffer it did not pass)
        assert none is None
        assert np.array_equal(a.view(np.int32), a_with.view(np.int32)) and np.array_equal(lp.view(np.int32), lp_with.view(np.int32))
        pw = tuple(_dev(w) for w in p)
        act = torch.full((24, 2), SENT, dtype=torch.float32, device="cuda")
        logp = torch.full((24, ), SENT, dtype=torch.float32, device="cuda")
        value = torch.full((24, ), SENT, dtype=torch.float32, device="cuda")
        obs = _dev(x)
        torch.cuda.synchronize()
        rc = eng.L.pgd_mlp_actor_critic(eng.h, -1, C.c_void_p(obs.data_ptr()), x.shape[1], k, C.byref(_nets(pw, None)), c["seed"], c["tick"], 0,
                                        C.c_void_p(act.data_ptr()), C.c_void_p(logp.data_ptr()), C.c_void_p(value.data_ptr()))
        assert rc == 0
        eng.sync()
        assert bool((value == SENT).all()) and np.array_equal(act.cpu().numpy().view(np.int32), a.view(np.int32))
    finally:
        eng.close()


def test_refused_arguments_and_the_accepted_boundary(descs):
    """PGD_ERR_ARG and no launch: one width beyond the derived limit, out_cols 3, a misaligned w1 (either network), unknown flags, a critic
    with only some pointers set, a critic without a value buffer, T = 0.  The same call with good arguments at the limit -- the first
    launch of a fresh engine, which needs the raised LDS limit -- computes correctly."""
    import torch
    kmax = ar.max_in_dim()
    eng = _ego_engine(descs, 20)
    try:
        L, h = eng.L, eng.h
        k1 = kmax + 1
        rng = np.random.default_rng(5)
        p, v = ar.make_networks(rng, k1, 4)
        pw, vw = [_dev(w) for w in p], [_dev(w) for w in v]
        wide = torch.zeros((20, 512), dtype=torch.float32, device="cuda")
        act = torch.full((20, 2), SENT, dtype=torch.float32, device="cuda")
        logp = torch.full((20, ), SENT, dtype=torch.float32, device="cuda")
        value = torch.full((20, ), SENT, dtype=torch.float32, device="cuda")
        shifted = torch.zeros(pw[0].numel() + 4, dtype=torch.float32, device="cuda")[1:]
        assert shifted.data_ptr() % 16 == 4
        eng.sync()

        def call(in_dim=kmax, nets=None, flags=0, stride=512, val=value):
            nets = _nets(pw, vw) if nets is None else nets
            return L.pgd_mlp_actor_critic(h, -1, C.c_void_p(wide.data_ptr()), stride, in_dim, C.byref(nets), 0, 0, flags,
                                          C.c_void_p(act.data_ptr()), C.c_void_p(logp.data_ptr()), C.c_void_p(val.data_ptr()) if val is not None else None)

        assert call(in_dim=k1) == ERR_ARG and call(in_dim=3) == ERR_ARG and call(in_dim=4097) == ERR_ARG
        assert call(nets=_nets(pw, vw, out_cols=3)) == ERR_ARG
        assert call(stride=kmax - 1) == ERR_ARG
        assert call(flags=2) == ERR_ARG
        for net in (0, 1):
            q = [list(pw), list(vw)]
            q[net][0] = shifted
            assert call(nets=_nets(q[0], q[1])) == ERR_ARG, net
        for missing in range(6):
            n = _nets(pw, vw)
            setattr(n, ("vw1", "vb1", "vw2", "vb2", "vw3", "vb3")[missing], None)
            assert call(nets=n) == ERR_ARG, missing
        n = _nets(pw, vw)
        n.w3 = None
        assert call(nets=n) == ERR_ARG
        assert call(val=None) == ERR_ARG
        z1 = torch.zeros(4, dtype=torch.float32, device="cuda")
        d1 = torch.zeros(4, dtype=torch.uint8, device="cuda")
        gae = lambda T, rows: L.pgd_gae(h, C.c_void_p(z1.data_ptr()), C.c_void_p(z1.data_ptr()), C.c_void_p(d1.data_ptr()), T, rows, 0.99, 0.95,  # noqa: E731
                                        C.c_void_p(act.data_ptr()), C.c_void_p(logp.data_ptr()))
        assert gae(0, 1) == ERR_ARG and gae(-1, 1) == ERR_ARG and gae(1, 0) == ERR_ARG
        eng.sync()
        assert bool((act == SENT).all()) and bool((logp == SENT).all()) and bool((value == SENT).all()), "a refused call wrote"
        # the accepted boundary on this fresh engine
        c = [c for c in ar.other_cases() if c["name"] == "boundary"][0]
        assert c["in_dim"] == kmax
        _check_case(eng, c)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# GAE
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", ar.GAE_T)
def test_gae(descs, T):
    """T x rows x done patterns x lambda against float64; the arrays sit inside sentinel-filled buffers that stay untouched."""
    import torch
    eng = _ego_engine(descs, 1)
    try:
        worst = 0.0
        for c in ar.gae_cases():
            if c["T"] != T:
                continue
            r, v, d = ar.build_gae(**c)
            rows = c["rows"]
            tr, tv, td = _dev(r), _dev(v), _dev(d)
            for lam in ar.GAE_LAM:
                buf = torch.full((2, T + 1, rows), SENT, dtype=torch.float32, device="cuda")
                adv, ret = eng.gae(tr, tv, td, ar.GAE_GAMMA, lam, adv=buf[0, :T], ret=buf[1, :T])
                eng.sync()
                got = buf.cpu().numpy()
                assert (got[:, T] == SENT).all(), (c, "written past the end")
                a64, r64 = ar.gae_f64(r, v, d, ar.GAE_GAMMA, lam)
                err = max(float(np.abs(got[0, :T] - a64).max()), float(np.abs(got[1, :T] - r64).max()))
                worst = max(worst, err)
                assert np.isfinite(got).all() and err < ar.TOL_GAE, (c, lam, err)
            a2, r2 = eng.gae(tr, tv, td, ar.GAE_GAMMA, ar.GAE_LAM[-1])  # (buffers of its own)
            eng.sync()
            assert np.array_equal(a2.cpu().numpy(), got[0, :T]) and np.array_equal(r2.cpu().numpy(), got[1, :T])
        print("GAE, T = %d: max |device - f64| = %.2e (tolerance %.2e)" % (T, worst, ar.TOL_GAE))
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# the collector
# ---------------------------------------------------------------------------------------------------------------------
COL_N, COL_T, COL_HORIZON, COL_SEED = 64, 16, 12, 3


def _Col(descs):
    """64 envs of the default configuration with traffic and a short horizon, freshly reset; random networks of the expert's shape."""
    return Traffic(descs, COL_N, COL_T, COL_SEED, horizon=COL_HORIZON)


def test_collector_equals_the_synchronised_loop_eagerly_and_from_a_graph(descs):
    import torch
    S = _Col(descs)
    want = synchronised_rollouts(S, 3)
    first_obs = S.first.cpu().numpy()
    S.eng.close()

    # what the rollouts hold
    ends = 0
    for k, r in enumerate(want):
        d = r["dones"].cpu().numpy() != 0
        obs, val, rew = r["obs"].cpu().numpy(), r["values"].cpu().numpy().astype(np.float64), r["rewards"].cpu().numpy().astype(np.float64)
        adv = r["advantages"].cpu().numpy()
        ends += int(d.sum())
        for t, e in zip(*np.nonzero(d)):
            if t + 1 < COL_T:  # the row behind a done is the first observation of a new episode (the env restarts its scenario)
                assert np.abs(obs[t + 1, e, :18] - first_obs[e, :18]).max() < 1e-5, (k, t, e)
            # and the advantage is cut there: nothing behind the done reaches it
            assert abs(adv[t, e] - (rew[t, e] - val[t, e])) < ar.TOL_GAE, (k, t, e)
        a64, r64 = ar.gae_f64(rew, val, d, 0.99, 0.95)
        assert np.abs(adv - a64).max() < ar.TOL_GAE  # (values of a tenth, rewards up to the penalty of 5: smaller than what TOL_GAE was measured on)
        if k:
            assert _bits_equal(want[k - 1]["values"][COL_T], r["values"][0])
    print("collector: %d episode ends in 3 rollouts of %d x %d steps" % (ends, COL_N, COL_T))
    assert ends >= COL_N  # (horizon 12 < T = 16: every env ends at least one episode per rollout)

    # (a) the collector, eagerly, nothing synchronised inside collect()
    A = _Col(descs)
    col = make_collector("single", A, gamma=0.99, lam=0.95)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        for k in range(3):
            batch = col.collect()
            got = _snapshot(batch, KEYS)
            assert tuple(batch["obs"].shape) == (COL_T, COL_N, A.eng.D) and tuple(batch["values"].shape) == (COL_T + 1, COL_N)
            for key in KEYS:
                assert _bits_equal(got[key], want[k][key]), "eager collect %d: %s differs from the synchronised loop" % (k, key)
            if k == 0:
                col.set_weights(A.pw, A.vw)
    A.eng.close()

    # (b) collect() captured in a HIP graph behind one eager rollout, replayed twice: the device counter advances the tick
    B = _Col(descs)
    col = make_collector("single", B)
    eager_then_graph(col.collect, lambda: _snapshot(col.batch, KEYS), want)
    B.eng.close()
