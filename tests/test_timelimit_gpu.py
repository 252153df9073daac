"""GAE that bootstraps through a time limit, on the device (pgdrive_amd/csrc/pgd_timelimit.h; include/pgdrive_hip.h states `truncated` and
the formulas): pgd_mlp_terminal_value, pgd_gae_bootstrap, pgd_cost_gae_bootstrap and the bootstrap_truncations switch of RolloutCollector
and SafeRolloutCollector.

* the terminal-value launch: truncated rows bit for bit the `value` of pgd_mlp_actor_critic on the same rows and weights, every other
  row exactly 0, rows past the end untouched; rows around the tile, widths on both sides of the prologue switch and at the limit,
  truncation patterns, NaN in every row that is not truncated, NaN in every weight when nothing is truncated, with and without the cost
  critic, env groups, refusals; and the predicate from the flags of real engines against twins that have no time limit;
* both GAE kernels at every shape, done pattern and truncation mode of tests/timelimit_ref.py against float64 within TOL_GAE_BOOTSTRAP,
  equal to their parents with term_value = 0, NaN behind every done, the cost form's books bit for bit its parent's;
* the collectors against the same calls made one at a time, eagerly and from a HIP graph, and the property the feature exists for.
"""
import ctypes as C

import numpy as np
import pytest

from tests import actor_critic_ref as ar
from tests import policy_ref as pr
from tests import timelimit_ref as tl
from tests import train_util
from tests.train_util import ERR_ARG, SENT, Traffic, bits_equal as _bits_equal, dev as _dev, eager_then_graph, ego_engine as _ego_engine, make_collector, \
    np_bits, six as _six, snapshot as _snapshot, synchronised_rollouts

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------------
# pgd_mlp_terminal_value
# ---------------------------------------------------------------------------------------------------------------------
def _values(eng, x, p, v, in_dim):
    """value [rows] of pgd_mlp_actor_critic on the rows of `x`: what a truncated row has to receive."""
    import torch
    rows = x.shape[0]
    act = torch.zeros((rows, 2), device="cuda")
    logp, val = torch.zeros(rows, device="cuda"), torch.zeros(rows, device="cuda")
    eng.mlp_actor_critic(tuple(_dev(w) for w in p), tuple(_dev(w) for w in v), act, logp, val, 0, 0, obs=_dev(x), deterministic=True, in_dim=in_dim)
    eng.sync()
    return val.cpu().numpy()


def _term(eng, x, v, cost, flags, done, in_dim, group=-1, tail=8, rows=None):
    """One launch into sentinel-filled buffers with `tail` entries behind the last row -> (term_value, term_cost_value or None), the
    tails checked."""
    import torch
    rows = x.shape[0] if rows is None else rows
    tv = torch.full((rows + tail, ), SENT, dtype=torch.float32, device="cuda")
    tcv = torch.full((rows + tail, ), SENT, dtype=torch.float32, device="cuda")
    vw = tuple(_dev(w) for w in v)
    cw = tuple(_dev(w) for w in cost) if cost is not None else None
    torch.cuda.synchronize()
    eng.mlp_terminal_value(vw, cw, _dev(x), _dev(flags), _dev(done), tv[:rows], tcv[:rows] if cw is not None else None, group=group, in_dim=in_dim)
    if group >= 0:
        eng.group_sync(group)
    eng.sync()
    a, b = tv.cpu().numpy(), tcv.cpu().numpy()
    assert (a[rows:] == SENT).all() and (b[rows:] == SENT).all(), "rows past the end were written"
    if cw is None:
        assert (b == SENT).all(), "no cost critic, but its buffer was written"
    return a[:rows], (b[:rows] if cw is not None else None)


def _check_launch(eng, x, p, v, cw, in_dim, trunc, seed, safe=False, f64=False):
    """The contracts of one launch with the truncated rows `trunc`: NaN in every other observation row."""
    flags, done = tl.flags_of(trunc, np.random.default_rng(seed), safe)
    want, want_c = _values(eng, x, p, v, in_dim), _values(eng, x, p, cw, in_dim)
    xn = x.copy()
    xn[~trunc] = np.nan
    tv, none = _term(eng, xn, v, None, flags, done, in_dim)
    assert none is None
    assert np.array_equal(np_bits(tv[trunc]), np_bits(want[trunc])), "truncated rows are not pgd_mlp_actor_critic's value bits"
    assert np.array_equal(np_bits(tv[~trunc]), np.zeros(int((~trunc).sum()), dtype=np.int32)), "a row that is not truncated is not exactly +0.0"
    tv2, tcv = _term(eng, xn, v, cw, flags, done, in_dim)
    assert np.array_equal(np_bits(tv2), np_bits(tv)), "the critic's output depends on the cost critic's presence"
    as_critic, _ = _term(eng, xn, cw, None, flags, done, in_dim)
    assert np.array_equal(np_bits(tcv), np_bits(as_critic)), "y = 1 is not a call that is handed the cost network as critic"
    assert np.array_equal(np_bits(tcv[trunc]), np_bits(want_c[trunc])) and np.array_equal(np_bits(tcv[~trunc]), np.zeros(int((~trunc).sum()), dtype=np.int32))
    if f64 and trunc.any():
        _, _, v64 = ar.heads_f64(x[trunc][:, :in_dim], p, v)
        err = float(np.abs(tv[trunc] - v64).max())
        print("terminal values, in_dim %d: max |device - f64| = %.2e (tolerance %.0e)" % (in_dim, err, pr.TOL_EXACT))
        assert err < pr.TOL_EXACT
    return tv


def _nets(name, in_dim, rows, seed=0):
    x, p, v = ar.build_case(name, in_dim, rows, seed=seed)
    _, cw = ar.make_networks(np.random.default_rng([in_dim, rows, seed, 99]), in_dim, 4)
    return x, p, v, cw


@pytest.mark.parametrize("rows", tl.TV_ROWS)
def test_rows_around_the_tile_and_every_truncation_pattern(descs, rows):
    """Engines of 1, 15, 16, 17 and 33 rows at width 274; patterns none, all, one row per tile, only the last row and -- 33 rows, three
    tiles -- a tile with none between two tiles with some.  One pattern also against float64; safe_rl_env engines read a crash as a cost."""
    for safe in (False, True):
        eng = _ego_engine(descs, rows, safe_rl_env=safe)
        try:
            x, p, v, cw = _nets("timelimit_rows", 274, rows, seed=rows)
            for j, pattern in enumerate(tl.TV_PATTERNS):
                if pattern == "gap" and rows < 33:
                    continue
                trunc = tl.trunc_pattern(rows, pattern)
                tv = _check_launch(eng, x, p, v, cw, 274, trunc, seed=rows * 10 + j, safe=safe, f64=(pattern == "all" and not safe))
                assert (tv != 0).sum() == trunc.sum()
        finally:
            eng.close()


def test_width_sweep(descs):
    """Widths 4, 35, 274, 319, 320, 321, 324 and 416 on one engine, ascending across the prologue switch and across the line above which
    the LDS limit is raised; 48 rows: one row per tile, and the tile with none between two with some."""
    assert tl.TV_WIDTHS[-1] == ar.max_in_dim() and ar.PROLOGUE_SWITCH in tl.TV_WIDTHS
    eng = _ego_engine(descs, tl.TV_GAP_ROWS)
    try:
        for i, k in enumerate(tl.TV_WIDTHS):
            x, p, v, cw = _nets("timelimit_sweep", k, tl.TV_GAP_ROWS, seed=i)
            for pattern in ("one_per_tile", "gap", "all"):
                _check_launch(eng, x, p, v, cw, k, tl.trunc_pattern(tl.TV_GAP_ROWS, pattern), seed=k, f64=(k == 274 and pattern == "all"))
    finally:
        eng.close()


def test_no_truncation_reads_no_weight_and_no_observation(descs):
    """Nothing truncated in the whole launch -- running rows, terminations, terminations on the time limit's step --: NaN in every
    weight of both networks and in every observation row, and the outputs are all +0.0: the early exit reads neither."""
    eng = _ego_engine(descs, 33)
    try:
        x, p, v, cw = _nets("timelimit_nan", 274, 33)
        nan = [np.full_like(w, np.nan) for w in v]
        flags, done = tl.flags_of(np.zeros(33, dtype=bool), np.random.default_rng(4))
        assert done.any() and (flags & tl.F_MAX_STEP).any()
        tv, tcv = _term(eng, np.full_like(x, np.nan), nan, nan, flags, done, 274)
        assert np.array_equal(np_bits(tv), np.zeros(33, dtype=np.int32)) and np.array_equal(np_bits(tcv), np.zeros(33, dtype=np.int32))
        # one truncated row: its tile runs (and NaN weights show), the other two tiles still exit early
        trunc = tl.trunc_pattern(33, "last_row")
        flags, done = tl.flags_of(trunc, np.random.default_rng(5))
        tv, _ = _term(eng, x, nan, None, flags, done, 274)
        assert np.isnan(tv[32]) and np.array_equal(np_bits(tv[:32]), np.zeros(32, dtype=np.int32))
    finally:
        eng.close()


def test_env_groups(descs):
    """16 envs in 2 groups of 8, each on its group's stream: only the group's rows are written (0 or the value), NaN in the other
    group's observations."""
    import torch
    eng = _ego_engine(descs, 16)
    try:
        x, p, v, cw = _nets("timelimit_groups", 274, 16)
        trunc = np.zeros(16, dtype=bool)
        trunc[[1, 7, 8, 13]] = True
        flags, done = tl.flags_of(trunc, np.random.default_rng(6))
        want, want_c = _values(eng, x, p, v, 274), _values(eng, x, p, cw, 274)
        eng.set_groups(2)
        vw, cww = tuple(_dev(w) for w in v), tuple(_dev(w) for w in cw)
        for g in range(2):
            mine = np.zeros(16, dtype=bool)
            mine[g * 8:(g + 1) * 8] = True
            xg = np.full_like(x, np.nan)
            xg[mine & trunc] = x[mine & trunc]
            tv = torch.full((16, ), SENT, dtype=torch.float32, device="cuda")
            tcv = torch.full((16, ), SENT, dtype=torch.float32, device="cuda")
            obs, fl, dn = _dev(xg), _dev(flags), _dev(done)
            torch.cuda.synchronize()
            eng.mlp_terminal_value(vw, cww, obs, fl, dn, tv, tcv, group=g, in_dim=274)
            eng.group_sync(g)
            for got, ref in ((tv.cpu().numpy(), want), (tcv.cpu().numpy(), want_c)):
                assert (got[~mine] == SENT).all(), (g, "rows of the other group written")
                assert np.array_equal(np_bits(got[mine & trunc]), np_bits(ref[mine & trunc])), g
                assert np.array_equal(np_bits(got[mine & ~trunc]), np.zeros(6, dtype=np.int32)), g
    finally:
        eng.close()


def test_refused_arguments(descs):
    """PGD_ERR_ARG and no launch: in_dim 3 and 417, a null critic, a critic with only some pointers set, a misaligned w1, obs_stride <
    in_dim, a cost critic without its output, null flags / done / output; a multi-agent engine."""
    import torch
    from pgdrive_amd import _abi
    from pgdrive_amd.engine import Engine
    from tests import util
    eng = _ego_engine(descs, 20)
    try:
        L, h = eng.L, eng.h
        x, p, v, cw = _nets("timelimit_refuse", 416, 20)
        obs, vw, cww = _dev(x), [_dev(w) for w in v], [_dev(w) for w in cw]
        stride = x.shape[1]
        trunc = np.ones(20, dtype=bool)
        flags, done = tl.flags_of(trunc, np.random.default_rng(7))
        fl, dn = _dev(flags), _dev(done)
        tv = torch.full((20, ), SENT, dtype=torch.float32, device="cuda")
        tcv = torch.full((20, ), SENT, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
        net = lambda ws: C.byref(_six(_abi.ValueNet(), ws)) if ws is not None else None   # noqa: E731

        def call(in_dim=416, stride=stride, critic=vw, cost=cww, fl=fl, dn=dn, tv=tv, tcv=tcv, obs=obs, handle=h):
            return L.pgd_mlp_terminal_value(handle, -1, P(obs), stride, in_dim, net(critic), net(cost), P(fl), P(dn), P(tv), P(tcv))

        assert call(in_dim=3) == ERR_ARG and call(in_dim=417, stride=512) == ERR_ARG
        assert call(critic=None) == ERR_ARG
        some = _six(_abi.ValueNet(), vw)
        some.w3 = None
        assert L.pgd_mlp_terminal_value(h, -1, P(obs), stride, 416, C.byref(some), None, P(fl), P(dn), P(tv), None) == ERR_ARG
        big = torch.zeros(416 * 256 + 1, device="cuda")
        off = [big[1:].view(416, 256)] + vw[1:]
        assert off[0].data_ptr() % 16 == 4
        assert call(critic=off) == ERR_ARG and call(cost=off) == ERR_ARG
        assert call(stride=415) == ERR_ARG
        assert call(tcv=None) == ERR_ARG
        assert call(fl=None) == ERR_ARG and call(dn=None) == ERR_ARG and call(tv=None) == ERR_ARG and call(obs=None) == ERR_ARG
        assert call(handle=None) == ERR_ARG
        eng.sync()
        torch.cuda.synchronize()
        assert bool((tv == SENT).all()) and bool((tcv == SENT).all()), "a refused call wrote"
        # the same call with good arguments at the limit: the first launch of this engine, which needs the raised LDS limit
        assert call() == 0
        eng.sync()
        assert np.array_equal(np_bits(tv.cpu().numpy()), np_bits(_values(eng, x, p, v, 416)))
        # T = 0, rows = 0 of the GAE forms
        z = torch.zeros(4, device="cuda")
        zb, zi = torch.zeros(4, dtype=torch.uint8, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
        c3 = (C.c_float * 3)(1.0, 1.0, 1.0)
        for T, rows in ((0, 1), (1, 0)):
            assert L.pgd_gae_bootstrap(h, P(z), P(z), P(zb), P(z), T, rows, 0.99, 0.95, P(z), P(z)) == ERR_ARG
            assert L.pgd_cost_gae_bootstrap(h, P(zi), P(zb), P(z), P(z), T, rows, c3, 0.99, 0.95, P(z), P(z), P(z), P(z), P(z), P(zi)) == ERR_ARG
        assert L.pgd_gae_bootstrap(h, P(z), P(z), P(zb), None, 1, 1, 0.99, 0.95, P(z), P(z)) == ERR_ARG
        assert L.pgd_cost_gae_bootstrap(h, P(zi), P(zb), P(z), None, 1, 1, c3, 0.99, 0.95, P(z), P(z), P(z), P(z), P(z), P(zi)) == ERR_ARG
    finally:
        eng.close()
    _, mb, sb = util.make_marl_banks(num_agents=5)
    marl = Engine(util.marl_config(4, sb), mb, sb)
    try:
        x, p, v, cw = _nets("timelimit_refuse", 274, 20)
        vw = [_dev(w) for w in v]
        obs, fl, dn = _dev(x), torch.zeros(20, dtype=torch.int32, device="cuda"), torch.zeros(20, dtype=torch.uint8, device="cuda")
        tv = torch.full((20, ), SENT, dtype=torch.float32, device="cuda")
        rc = marl.L.pgd_mlp_terminal_value(marl.h, -1, C.c_void_p(obs.data_ptr()), x.shape[1], 274, C.byref(_six(_abi.ValueNet(), vw)), None,
                                           C.c_void_p(fl.data_ptr()), C.c_void_p(dn.data_ptr()), C.c_void_p(tv.data_ptr()), None)
        assert rc == ERR_ARG and bool((tv == SENT).all())
    finally:
        marl.close()


# seed of the actions below: with it both kinds of first end occur often enough on both engines (the assertion says how often)
TWIN_N, TWIN_HORIZON, TWIN_STEPS, TWIN_ACTION_SEED = 64, 25, 60, 8


@pytest.mark.parametrize("safe", [False, True], ids=["pgdrive", "safe"])
def test_the_predicate_from_the_flags_of_a_real_engine(descs, safe):
    """64 envs with traffic, horizon 25, random driving for 60 steps; beside them a twin with horizon 0 and the same actions.  Up to an
    env's first done the two states are identical, so at that step the done is a truncation exactly when the twin is not done there.
    The launch (a critic that says 1 everywhere) must mark those envs and no others -- at every step up to each env's first done."""
    import torch
    from pgdrive_amd import _abi
    from pgdrive_amd.engine import Engine
    from pgdrive_amd.rollout import truncated
    from tests import parity, util
    kw = dict(auto_reset=1, seed=2, safe_rl_env=safe)
    mb, sb = util.make_banks(descs, n_maps=8)
    a = Engine(_abi.make_config(TWIN_N, horizon=TWIN_HORIZON, **kw), mb, sb)
    b = Engine(_abi.make_config(TWIN_N, horizon=0, **kw), mb, sb)
    try:
        ids = np.arange(TWIN_N) % 8
        a.reset(ids); b.reset(ids)
        one = [np.zeros(s, dtype=np.float32) for s in ((a.D, 256), (256, ), (256, 256), (256, ), (256, 1), (1, ))]
        one[5][0] = 1.0
        vw = tuple(_dev(w) for w in one)
        tv = torch.zeros(TWIN_N, device="cuda")
        actions = parity.driving_with_bursts(np.random.default_rng(TWIN_ACTION_SEED), TWIN_N)
        running = np.ones(TWIN_N, dtype=bool)
        n_trunc = n_term = 0
        for t in range(TWIN_STEPS):
            at = torch.from_numpy(actions(t)).to(a.device)
            obs, _, done, flags = a.step(at)
            _, _, done_b, _ = b.step(at)
            a.mlp_terminal_value(vw, None, obs.view(TWIN_N, -1), flags.view(-1), done.view(-1), tv)
            a.sync(); b.sync()
            torch.cuda.synchronize()
            got = tv.cpu().numpy()
            da, db, fl = done.view(-1).cpu().numpy() != 0, done_b.view(-1).cpu().numpy() != 0, flags.view(-1).cpu().numpy()
            assert set(np.unique(got)) <= {0.0, 1.0}
            assert np.array_equal(got != 0, truncated(fl, da, safe)), "the device's predicate is not pgdrive_amd.rollout.truncated"
            assert not (db & ~da & running).any(), "the twin without a time limit ended an episode the engine did not"
            want = da & ~db
            assert np.array_equal((got != 0)[running], want[running]), (t, "truncated != done here and not done in the twin")
            first = running & da
            n_trunc += int((first & want).sum())
            n_term += int((first & ~want).sum())
            running &= ~da
        print("first ends (%s): %d truncations, %d terminations, %d envs still running" % ("safe" if safe else "pgdrive", n_trunc, n_term, running.sum()))
        assert n_trunc >= 8 and n_term >= 8
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------------------------------------------------------------
# pgd_gae_bootstrap, pgd_cost_gae_bootstrap
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", ar.GAE_ROWS)
@pytest.mark.parametrize("T", ar.GAE_T)
def test_both_gae_forms(descs, T, rows):
    """Every done pattern x truncated = none / all / Bernoulli of the dones, both lambdas: against float64 within TOL_GAE_BOOTSTRAP; with
    term_value = 0 the parents' float values; the cost form's books its parent's bytes.  NaN in value[t + 1] behind every done:
    value[t + 1] is also step t + 1's own baseline, so adv[t + 1] cannot be finite where t + 1 < T; every OTHER output keeps the bits of
    the clean run, and where the dones sit in the last step only (value[T] is nobody's baseline) every output is finite."""
    import torch
    eng = _ego_engine(descs, 1)
    try:
        worst = 0.0
        for pattern in ar.GAE_DONES:
            for mode in tl.TRUNC_MODES:
                r, v, d, trunc, term = tl.build_bootstrap(T, rows, pattern, mode)
                fl, _, _, cv, cterm, run = tl.build_cost_bootstrap(T, rows, pattern, mode)
                tr, tv, td, tt = _dev(r), _dev(v), _dev(d), _dev(term)
                tfl, tcv, tct = _dev(fl), _dev(cv), _dev(cterm)
                for lam in ar.GAE_LAM:
                    buf = torch.full((2, T + 1, rows), SENT, dtype=torch.float32, device="cuda")
                    eng.gae_bootstrap(tr, tv, td, tt, ar.GAE_GAMMA, lam, adv=buf[0, :T], ret=buf[1, :T])
                    eng.sync()
                    got = buf.cpu().numpy()
                    assert (got[:, T] == SENT).all(), "written past the end"
                    a64, r64 = tl.gae_bootstrap_f64(r, v, d, term, ar.GAE_GAMMA, lam)
                    err = max(float(np.abs(got[0, :T] - a64).max()), float(np.abs(got[1, :T] - r64).max()))
                    worst = max(worst, err)
                    assert np.isfinite(got).all() and err < tl.TOL_GAE_BOOTSTRAP, (T, rows, pattern, mode, lam, err)
                    # the cost form
                    run_d = _dev(run)
                    cost, cadv, cret, es, ec = eng.cost_gae_bootstrap(tfl, td, tcv, tct, tl.COSTS, ar.GAE_GAMMA, lam, run_d)
                    run_p = _dev(run)
                    cost_p, cadv_p, cret_p, es_p, ec_p = eng.cost_gae(tfl, td, tcv, tl.COSTS, ar.GAE_GAMMA, lam, run_p)
                    eng.sync()
                    ref = tl.cost_gae_bootstrap_f64(fl, d, cv, cterm, tl.COSTS, ar.GAE_GAMMA, lam, run)
                    err = max(float(np.abs(cadv.cpu().numpy() - ref["cadv"]).max()), float(np.abs(cret.cpu().numpy() - ref["cret"]).max()))
                    worst = max(worst, err)
                    assert err < tl.TOL_GAE_BOOTSTRAP, (T, rows, pattern, mode, lam, "cost", err)
                    for x, y, name in ((cost, cost_p, "cost"), (run_d, run_p, "run"), (es, es_p, "ep_sum"), (ec, ec_p, "ep_count")):
                        assert _bits_equal(x, y), (name, "the books are not pgd_cost_gae's")
                    if mode == "none":   # term_value is zero everywhere: the parents' results as float values
                        a0, r0 = eng.gae(tr, tv, td, ar.GAE_GAMMA, lam)
                        eng.sync()
                        assert np.array_equal(got[0, :T], a0.cpu().numpy()) and np.array_equal(got[1, :T], r0.cpu().numpy())
                        assert torch.equal(cadv, cadv_p) and torch.equal(cret, cret_p)
                # NaN in value[t + 1] behind every done.  value[t + 1] is also step t + 1's own baseline, so adv[t + 1] = ... - NaN
                # cannot be finite there; every OTHER output must keep its bits -- no NaN travels across a done --, and where the
                # dones sit in the last step only (value[T] is nobody's baseline) every output is finite.
                lam = ar.GAE_LAM[-1]
                clean_a, clean_r = eng.gae_bootstrap(tr, tv, td, tt, ar.GAE_GAMMA, lam)
                clean_c = eng.cost_gae_bootstrap(tfl, td, tcv, tct, tl.COSTS, ar.GAE_GAMMA, lam, _dev(run))
                vn, cvn = v.copy(), cv.copy()
                vn[1:][d != 0] = np.nan
                cvn[1:][d != 0] = np.nan
                own = torch.from_numpy(np.isfinite(vn[:-1])).cuda()
                nan_a, nan_r = eng.gae_bootstrap(tr, _dev(vn), td, tt, ar.GAE_GAMMA, lam)
                nan_c = eng.cost_gae_bootstrap(tfl, td, _dev(cvn), tct, tl.COSTS, ar.GAE_GAMMA, lam, _dev(run))
                eng.sync()
                for x, y in ((clean_a, nan_a), (clean_r, nan_r), (clean_c[1], nan_c[1]), (clean_c[2], nan_c[2])):
                    assert _bits_equal(x[own], y[own]), (T, rows, pattern, mode, "a NaN behind a done reached another output")
                if pattern == "last" or T == 1:
                    assert bool(own.all())
                    for y in (nan_a, nan_r, nan_c[1], nan_c[2]):
                        assert bool(torch.isfinite(y).all()), (T, rows, pattern, mode)
        print("bootstrap GAE, T = %d, rows = %d: max |device - f64| = %.2e (tolerance %.2e)" % (T, rows, worst, tl.TOL_GAE_BOOTSTRAP))
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# the collectors
# ---------------------------------------------------------------------------------------------------------------------
COL_N, COL_T, COL_HORIZON, COL_SEED = 64, 16, 12, 3
KEYS = train_util.KEYS + ("term_values", )
SAFE_KEYS = KEYS + ("cost_values", "term_cost_values", "costs", "cost_advantages", "cost_returns", "ep_cost_sum", "ep_cost_count")
COSTS = (1.0, 0.5, 0.25)


def _Col(descs, safe):
    """64 envs of the default configuration with traffic and horizon 12 < T = 16, freshly reset, the step info on; random networks of
    the expert's shape (a third one as cost critic)."""
    return Traffic(descs, COL_N, COL_T, COL_SEED, horizon=COL_HORIZON, safe=safe, step_info_costs=COSTS)


def _collector(S, on=True):
    return make_collector("safe", S, costs=COSTS, bootstrap_truncations=on) if S.safe else make_collector("single", S, bootstrap_truncations=on)


@pytest.mark.parametrize("safe", [False, True], ids=["RolloutCollector", "SafeRolloutCollector"])
def test_collectors_with_the_switch_on(descs, safe):
    import torch
    from pgdrive_amd.rollout import truncated
    keys = SAFE_KEYS if safe else KEYS
    S = _Col(descs, safe)
    want = synchronised_rollouts(S, 3, cost_critic=safe, bootstrap=True, costs=COSTS)
    S.eng.close()

    # what the rollouts hold
    n_trunc = n_carried = 0
    for k, r in enumerate(want):
        d, fl = r["dones"].cpu().numpy(), r["flags"].cpu().numpy()
        tr = truncated(fl, d, safe)
        n_trunc += int(tr.sum())
        assert tr.any(axis=0).sum() >= COL_N // 2, "few envs reach the time limit in rollout %d" % k   # (horizon 12 < T = 16)
        if k:   # an episode that began in the rollout before: its time limit falls on one of this rollout's first steps
            n_carried += int(tr[:COL_T - COL_HORIZON].sum())
        fo = r["final_obs"].cpu().numpy()
        for name, net in (("term_values", S.v), ("term_cost_values", S.c))[:2 if safe else 1]:
            tv = r[name].cpu().numpy()
            assert np.array_equal(tv != 0, tr) and np.array_equal(np_bits(tv[~tr]), np.zeros(int((~tr).sum()), dtype=np.uint32))
            _, _, v64 = ar.heads_f64(fo[tr], S.p, net)
            err = float(np.abs(tv[tr] - v64).max())
            assert err < pr.TOL_EXACT, (k, name, err)
        rew, val, term = [r[x].cpu().numpy() for x in ("rewards", "values", "term_values")]
        a64, r64 = tl.gae_bootstrap_f64(rew, val, d, term, 0.99, 0.95)
        err = max(float(np.abs(r["advantages"].cpu().numpy() - a64).max()), float(np.abs(r["returns"].cpu().numpy() - r64).max()))
        print("rollout %d: %d truncations, %d other ends; |adv - f64| %.2e (tolerance %.2e)" % (k, tr.sum(), (d != 0).sum() - tr.sum(), err, tl.TOL_GAE_BOOTSTRAP))
        assert err < tl.TOL_GAE_BOOTSTRAP
        if safe:
            ref = tl.cost_gae_bootstrap_f64(fl, d, r["cost_values"].cpu().numpy(), r["term_cost_values"].cpu().numpy(), COSTS, 0.99, 0.95,
                                            np.zeros(COL_N))
            assert np.abs(r["cost_advantages"].cpu().numpy() - ref["cadv"]).max() < tl.TOL_GAE_BOOTSTRAP
            assert np.array_equal(r["ep_cost_count"].cpu().numpy(), (d != 0).sum(axis=0))   # a truncated episode finishes for the books
        if k:
            assert _bits_equal(want[k - 1]["values"][COL_T], r["values"][0])
    assert n_trunc >= 2 * COL_N and n_carried >= 8

    # (a) the collector, eagerly, nothing synchronised inside collect()
    A = _Col(descs, safe)
    col = _collector(A)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    on = []
    with torch.cuda.stream(s), torch.no_grad():
        for k in range(3):
            batch = col.collect()
            got = _snapshot(batch, keys)
            on.append(got)
            assert tuple(batch["term_values"].shape) == (COL_T, COL_N)
            for key in keys:
                assert _bits_equal(got[key], want[k][key]), "eager collect %d: %s differs from the synchronised loop" % (k, key)
    A.eng.close()

    # (b) collect() captured in a HIP graph behind one eager rollout, replayed twice, against the eager collects
    B = _Col(descs, safe)
    col = _collector(B)
    eager_then_graph(col.collect, lambda: _snapshot(col.batch, keys), on)
    B.eng.close()

    # (c) the switch off, same engine configuration (step info on) and seeds: the same trajectory, today's pgd_gae bit for bit -- which
    # differs from the switched-on advantages at every truncated step
    Cc = _Col(descs, safe)
    col = _collector(Cc, on=False)
    with torch.no_grad():
        for k in range(3):
            batch = col.collect()
            off = _snapshot(batch, [x for x in keys if x not in ("term_values", "term_cost_values")])
            assert "term_values" not in batch
            for key in ("obs", "actions", "values", "rewards", "dones", "flags"):
                assert _bits_equal(off[key], on[k][key]), (k, key, "the switch changed the trajectory")
            adv, ret = Cc.eng.gae(off["rewards"], off["values"], off["dones"], 0.99, 0.95)
            torch.cuda.synchronize()
            assert _bits_equal(adv, off["advantages"]) and _bits_equal(ret, off["returns"])
            tr = truncated(off["flags"], off["dones"], safe)
            assert bool(tr.any()) and bool((off["advantages"][tr] != on[k]["advantages"][tr]).all())
            if safe:
                assert bool((off["cost_advantages"][tr] != on[k]["cost_advantages"][tr]).all())
                for key in ("costs", "ep_cost_sum", "ep_cost_count"):
                    assert _bits_equal(off[key], on[k][key]), (k, key)
    Cc.eng.close()


def test_a_time_limit_is_invisible_to_a_correct_critic_on_the_device(descs):
    """A critic whose weights are zero except vb3 = r / (1 - gamma) -- it says V everywhere, the terminal observations included -- and
    rewards overwritten with r: with the switch on |adv| stays below TOL_GAE_BOOTSTRAP / (1 - gamma lam), the bound of a geometric sum
    of per-step errors; with it off adv = r - V at every truncated step.  A termination still cuts the value (its one-step target is 0
    with either switch), so the bound is asserted over the envs without a termination in the rollout."""
    import torch
    from pgdrive_amd.rollout import truncated
    r, gamma, lam = 0.05, 0.99, 0.95
    V = np.float32(r / (1.0 - float(np.float32(gamma))))
    for on in (True, False):
        S = _Col(descs, False)
        for w in S.v:
            w[:] = 0.0
        S.v[5][0] = V
        S.vw = tuple(_dev(w) for w in S.v)
        col = _collector(S, on=on)
        eng = S.eng
        try:
            with torch.no_grad():
                for k in range(2):
                    batch = col.collect()
                    torch.cuda.synchronize()
                    assert bool((batch["values"] == float(V)).all())
                    rew = torch.full_like(batch["rewards"], r)
                    tr = truncated(batch["flags"], batch["dones"])
                    assert int(tr.sum()) >= COL_N // 2
                    if on:
                        assert torch.equal(batch["term_values"], tr.float() * float(V))
                        adv, _ = eng.gae_bootstrap(rew, batch["values"], batch["dones"], batch["term_values"], gamma, lam)
                    else:
                        adv, _ = eng.gae(rew, batch["values"], batch["dones"], gamma, lam)
                    torch.cuda.synchronize()
                    a = adv.cpu().numpy().astype(np.float64)
                    trn = tr.cpu().numpy()
                    if on:
                        # (terminations still cut the value: the property speaks of the steps whose episode ends at a time limit or
                        # runs on, i.e. every step of an env without a termination in this rollout)
                        clean = ~((batch["dones"].cpu().numpy() != 0) & ~trn).any(axis=0)
                        assert clean.sum() >= 8
                        worst = float(np.abs(a[:, clean]).max())
                        print("switch on: max |adv| %.2e (bound %.2e)" % (worst, tl.TOL_GAE_BOOTSTRAP / (1.0 - gamma * lam)))
                        assert worst < tl.TOL_GAE_BOOTSTRAP / (1.0 - gamma * lam)
                    else:
                        assert np.abs(a[trn] - (r - float(V))).max() < tl.TOL_GAE_BOOTSTRAP
        finally:
            eng.close()
