"""pgd_live_rows, pgd_rollout_index, pgd_mlp_actor_critic_rows, pgd_gae_masked (pgdrive_amd/csrc/pgd_marl_rollout.h) and
pgdrive_amd.rollout.MultiAgentRolloutCollector on the device, against tests/marl_rollout_ref.py:

* the two index lists at every flag pattern of the checker, exactly, with the count, sentinels behind the count and behind the buffers,
  the same bytes twice, and env groups.  Sizes: 1, 15, 16, 17, 63, 64, 65, 4099 and one below, at and one above the boundaries of the
  compaction -- a chunk of 256 indices (255 .. 257), a workgroup's block of 1024 (1023 .. 1025), two blocks (2047 .. 2049) -- and, for
  the scan workgroup, which takes 256 block counts per pass, 255, 256, 257 and 261 blocks (261,120 / 262,144 / 262,145 / 266,435 entries);
* the network launch over a row list: listed rows bit-identical to pgd_mlp_actor_critic (sampled, deterministic, with the device tick
  counter), unlisted rows exactly zero with their observations NaN, the tail untouched, no critic, the refusal of in_dim 417, list
  entries that are no row of the range;
* masked GAE on the histories of the checker against float64 (tolerance 8.68e-6, measured by the emulation and doubled), zero where no
  agent acted, the mask exact, and pgd_gae's bits when every flag is PGD_F_REPORT;
* the collector on a roundabout engine: see test_collector_on_the_roundabout.
"""
import ctypes as C

import numpy as np
import pytest

from tests import actor_critic_ref as ar
from tests import marl_rollout_ref as mr
from tests import train_util
from tests.train_util import ERR_ARG, SENT, Roundabout, ac_nets as _nets, bits_equal as _bits_equal, dev as _dev, eager_then_graph, \
    ego_engine as _ego_engine, make_collector, np_bits as _bits, snapshot as _snapshot, synchronised_rollouts

pytestmark = pytest.mark.gpu

ISENT = -7


def _flags_dev(f):
    return _dev(np.ascontiguousarray(f).view(np.int32))


def _check_list(call, want, cap, where):
    """`call(list_buffer, count_buffer)` twice into sentinel-filled buffers (8 entries behind the list, one on either side of the count):
    the list and the count exact, everything else untouched, the same bytes both times."""
    import torch
    got = []
    for _ in range(2):
        buf = torch.full((cap + 8, ), ISENT, dtype=torch.int32, device="cuda")
        cnt = torch.full((3, ), ISENT, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        call(buf[:cap], cnt[1:2])
        torch.cuda.synchronize()
        b, c = buf.cpu().numpy(), cnt.cpu().numpy()
        assert c[0] == ISENT and c[2] == ISENT and c[1] == len(want), (where, c, len(want))
        assert np.array_equal(b[:len(want)], want), (where, "the list differs")
        assert (b[len(want):] == ISENT).all(), (where, "written behind the count")
        got.append(b)
    assert np.array_equal(got[0], got[1])


# ---------------------------------------------------------------------------------------------------------------------
# live rows and the rollout index
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", mr.LIVE_ROW_COUNTS)
def test_live_rows(descs, rows):
    eng = _ego_engine(descs, rows)
    try:
        for pattern in mr.PATTERNS:
            f, d = mr.build_flags(rows, pattern, "live")
            tf, td = _flags_dev(f), _dev(d)
            _check_list(lambda buf, cnt: eng.live_rows(tf, td, rows=buf, count=cnt), mr.live_list(f, d), rows, (rows, pattern))
    finally:
        eng.close()


def test_live_rows_of_env_groups(descs):
    """2056 envs in 2 groups of 1028 rows (two blocks each, the second group's first row inside a block of the whole range): each group
    lists its own rows only, by their engine-wide numbers, on its own stream and in its own scratch, beside a call over the whole engine."""
    import torch
    n = 2056
    eng = _ego_engine(descs, n)
    try:
        eng.set_groups(2)
        for pattern in ("half", "combos", "all"):
            f, d = mr.build_flags(n, pattern, "live")
            tf, td = _flags_dev(f), _dev(d)
            want = mr.live_list(f, d)
            bufs = [torch.full((n // 2 + 8, ), ISENT, dtype=torch.int32, device="cuda") for _ in range(2)]
            cnts = [torch.full((1, ), ISENT, dtype=torch.int32, device="cuda") for _ in range(2)]
            torch.cuda.synchronize()
            whole = torch.full((n + 8, ), ISENT, dtype=torch.int32, device="cuda")
            cw = torch.full((1, ), ISENT, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            eng.live_rows(tf, td, rows=whole[:n], count=cw)  # (the whole engine on the engine's stream and both groups in flight together)
            for g in range(2):
                eng.live_rows(tf, td, rows=bufs[g][:n // 2], count=cnts[g], group=g)
            for g in range(2):
                eng.group_sync(g)
                mine = want[(want >= g * (n // 2)) & (want < (g + 1) * (n // 2))]
                b = bufs[g].cpu().numpy()
                assert int(cnts[g].item()) == len(mine), (pattern, g)
                assert np.array_equal(b[:len(mine)], mine) and (b[len(mine):] == ISENT).all(), (pattern, g)
            eng.sync()
            torch.cuda.synchronize()
            b = whole.cpu().numpy()
            assert int(cw.item()) == len(want) and np.array_equal(b[:len(want)], want) and (b[len(want):] == ISENT).all(), pattern
    finally:
        eng.close()


@pytest.mark.parametrize("shape", mr.INDEX_SHAPES)
def test_rollout_index(descs, shape):
    T, rows = shape
    eng = _ego_engine(descs, 1)
    try:
        for pattern in mr.PATTERNS:
            f, _ = mr.build_flags(T * rows, pattern, "acted")
            tf = _flags_dev(f.reshape(T, rows))
            _check_list(lambda buf, cnt: eng.rollout_index(tf, index=buf, count=cnt), mr.acted_index(f), T * rows, (shape, pattern))
    finally:
        eng.close()


def test_refused_arguments(descs):
    """Null pointers with a good handle, T or rows below 1, more than 2^31 - 1 entries: PGD_ERR_ARG, nothing launched."""
    import torch
    eng = _ego_engine(descs, 4)
    try:
        L, h = eng.L, eng.h
        i4 = torch.full((8, ), ISENT, dtype=torch.int32, device="cuda")
        f4 = torch.full((8, ), SENT, dtype=torch.float32, device="cuda")
        u4 = torch.zeros((8, ), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        pi, pf, pu = C.c_void_p(i4.data_ptr()), C.c_void_p(f4.data_ptr()), C.c_void_p(u4.data_ptr())
        for k in range(4):
            args = [pi, pu, pi, pi]
            args[k] = None
            assert L.pgd_live_rows(h, -1, *args) == ERR_ARG, k
        assert L.pgd_live_rows(h, 0, pi, pu, pi, pi) == ERR_ARG  # (no env groups)
        assert L.pgd_rollout_index(h, None, 1, 4, pi, pi) == ERR_ARG and L.pgd_rollout_index(h, pi, 1, 4, None, pi) == ERR_ARG
        assert L.pgd_rollout_index(h, pi, 1, 4, pi, None) == ERR_ARG
        assert L.pgd_rollout_index(h, pi, 0, 4, pi, pi) == ERR_ARG and L.pgd_rollout_index(h, pi, 1, 0, pi, pi) == ERR_ARG
        assert L.pgd_rollout_index(h, pi, 65536, 32768, pi, pi) == ERR_ARG and L.pgd_rollout_index(h, pi, 1, 2 ** 31 - 1024, pi, pi) == ERR_ARG
        for k in range(7):
            args = [pf, pf, pu, pi, pf, pf, pu]
            args[k] = None
            assert L.pgd_gae_masked(h, *args[:4], 1, 4, 0.99, 0.95, *args[4:]) == ERR_ARG, k
        assert L.pgd_gae_masked(h, pf, pf, pu, pi, 0, 4, 0.99, 0.95, pf, pf, pu) == ERR_ARG
        assert L.pgd_gae_masked(h, pf, pf, pu, pi, 1, 0, 0.99, 0.95, pf, pf, pu) == ERR_ARG
        eng.sync()
        torch.cuda.synchronize()
        assert bool((i4 == ISENT).all()) and bool((f4 == SENT).all()) and bool((u4 == 0).all()), "a refused call wrote"
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# the network launch over a row list
# ---------------------------------------------------------------------------------------------------------------------
TAIL = 8


def _buffers(rows, a=1):
    import torch
    return (torch.full((rows + TAIL, 2), SENT, dtype=torch.float32, device="cuda"), torch.full((rows + TAIL, ), SENT, dtype=torch.float32, device="cuda"),
            torch.full((rows + TAIL, ), SENT, dtype=torch.float32, device="cuda"))


def _plain(eng, x, pw, vw, seed, tick, k, det=False):
    import torch
    rows = x.shape[0]
    act, logp, val = _buffers(rows)
    torch.cuda.synchronize()
    eng.mlp_actor_critic(pw, vw, act[:rows], logp[:rows], val[:rows] if vw is not None else None, seed, tick, obs=_dev(x), deterministic=det, in_dim=k)
    eng.sync()
    return act.cpu().numpy()[:rows], logp.cpu().numpy()[:rows], val.cpu().numpy()[:rows]


def _listed(eng, x, pw, vw, seed, tick, k, listed, det=False, group=-1, lo=0, hi=None, foreign=()):
    """The launch over `listed` (ascending row numbers) -> (act, logp, value) of all rows.  Every unlisted row's observation is NaN; the
    list buffer holds unlisted rows of the range behind the count (a kernel that read them would compute NaN into a row that must be
    zero); the tail behind the rows stays the sentinel; rows outside [lo, hi) (another env group's) stay the sentinel too."""
    import torch
    rows = x.shape[0]
    hi = rows if hi is None else hi
    xn = np.full_like(x, np.nan)
    xn[listed] = x[listed]
    unlisted = np.setdiff1d(np.arange(lo, hi), listed)
    entries = [int(r) for r in listed]
    for j, bad in enumerate(foreign):  # entries that are no row of the range, spread through the counted part of the list
        entries.insert((j * (len(entries) + 1)) // len(foreign), int(bad))
    assert len(entries) <= hi - lo
    lst = np.full(hi - lo, ISENT, dtype=np.int32)
    lst[:len(entries)] = entries
    if len(unlisted):
        lst[len(entries):] = np.resize(unlisted, hi - lo - len(entries))
    act, logp, val = _buffers(rows)
    tl, tc = _dev(lst), _dev(np.array([len(entries)], dtype=np.int32))
    torch.cuda.synchronize()
    eng.mlp_actor_critic_rows(pw, vw, tl, tc, act[:rows], logp[:rows], val[:rows] if vw is not None else None, seed, tick, obs=_dev(xn),
                              group=group, deterministic=det, in_dim=k)
    if group >= 0:
        eng.group_sync(group)
    eng.sync()
    a, lp, v = act.cpu().numpy(), logp.cpu().numpy(), val.cpu().numpy()
    assert (a[rows:] == SENT).all() and (lp[rows:] == SENT).all() and (v[rows:] == SENT).all(), "rows past the end were written"
    out = np.ones(rows, dtype=bool)
    out[lo:hi] = False
    assert (a[:rows][out] == SENT).all() and (lp[:rows][out] == SENT).all() and (v[:rows][out] == SENT).all(), "rows of another group were written"
    if vw is None:
        assert (v == SENT).all(), "no critic, but the value buffer was written"
    return a[:rows], lp[:rows], v[:rows]


def _compare(got, want, listed, lo, hi, critic, where):
    on = np.zeros(len(want[0]), dtype=bool)
    on[listed] = True
    off = ~on
    off[:lo] = False
    off[hi:] = False
    for name, g, w in zip(("action", "logp", "value"), got, want):
        if name == "value" and not critic:
            continue
        assert np.array_equal(_bits(g[on]), _bits(w[on])), (where, name, "listed rows differ from the plain launch")
        assert np.array_equal(_bits(g[off]), np.zeros_like(_bits(g[off]))), (where, name, "unlisted rows are not zero")
        assert np.isfinite(w[on]).all()


def _lists(rows, rng, lo=0, hi=None):
    hi = rows if hi is None else hi
    n = hi - lo
    return dict(empty=np.zeros(0, dtype=np.int64), full=np.arange(lo, hi), random=lo + np.flatnonzero(rng.uniform(size=n) < 0.5),
                single=np.array([lo + n // 2]))


@pytest.mark.parametrize("rows", ar.ROW_COUNTS)
def test_listed_rows_get_the_plain_launchs_bits(descs, rows):
    """Widths 35 and 324 (either form of the row prologue), 1 .. 4099 rows, lists empty / full / random / a single row; sampled and
    deterministic; the random list also with the device tick counter set (counter 5 + argument 3 == argument 8)."""
    import torch
    eng = _ego_engine(descs, rows)
    try:
        for k in (35, 324):
            c = dict(name="listed", in_dim=k, rows=rows, scaling="unit", out_cols=5, seed=rows + k, tick=9)
            x, p, v = ar.build_case(**c)
            pw, vw = tuple(_dev(w) for w in p), tuple(_dev(w) for w in v)
            want = {det: _plain(eng, x, pw, vw, c["seed"], c["tick"], k, det=det) for det in (False, True)}
            assert not np.array_equal(want[False][0], want[True][0])
            for name, listed in _lists(rows, np.random.default_rng([rows, k])).items():
                for det in (False, True):
                    got = _listed(eng, x, pw, vw, c["seed"], c["tick"], k, listed, det=det)
                    _compare(got, want[det], listed, 0, rows, True, (rows, k, name, det))
                if name == "random":
                    counter = torch.full((1, ), 5, dtype=torch.int32, device="cuda")
                    eng.actor_critic_tick(counter)
                    got = _listed(eng, x, pw, vw, c["seed"], 3, k, listed)
                    plain5 = _plain(eng, x, pw, vw, c["seed"], 3, k)
                    eng.actor_critic_tick(None)
                    plain8 = _plain(eng, x, pw, vw, c["seed"], 8, k)
                    assert np.array_equal(_bits(plain5[0]), _bits(plain8[0])) and not np.array_equal(plain8[0], want[False][0])
                    _compare(got, plain8, listed, 0, rows, True, (rows, k, "device tick"))
                    got = _listed(eng, x, pw, None, c["seed"], c["tick"], k, listed)  # no critic: the value buffer keeps its bytes
                    _compare(got, want[False], listed, 0, rows, False, (rows, k, "no critic"))
    finally:
        eng.close()


def test_entries_that_are_no_row_of_the_range_are_skipped(descs):
    """Negative numbers, the first row behind the range (the tail's first row), far beyond it, INT_MIN and INT_MAX inside the counted
    part of the list: nothing but the listed rows of the range is written, and those keep the plain launch's bits."""
    rows = 33
    eng = _ego_engine(descs, rows)
    try:
        for k in (35, 324):
            c = dict(name="foreign", in_dim=k, rows=rows, scaling="unit", out_cols=4, seed=k, tick=4)
            x, p, v = ar.build_case(**c)
            pw, vw = tuple(_dev(w) for w in p), tuple(_dev(w) for w in v)
            want = _plain(eng, x, pw, vw, c["seed"], c["tick"], k)
            listed = np.array([0, 2, 3, 7, 15, 16, 17, 20, 21, 30, 32])
            foreign = (-1, ISENT, rows, rows + 5, 2 ** 30, -2 ** 31, 2 ** 31 - 1)
            got = _listed(eng, x, pw, vw, c["seed"], c["tick"], k, listed, foreign=foreign)  # (asserts the tail's sentinels)
            _compare(got, want, listed, 0, rows, True, ("foreign entries", k))
    finally:
        eng.close()


def test_the_multi_agent_row_width_env_groups_and_the_in_dim_limit():
    """6 envs x 5 seats of the roundabout (rows of eng.D floats): the whole engine, then env group 1 alone (rows 15 .. 29; group 0's
    outputs keep their bytes).  in_dim 417, a null list and a null count are refused before any launch."""
    import torch
    from pgdrive_amd.engine import Engine
    from tests import util
    _, mb, sb = util.make_marl_banks(num_agents=5)
    eng = Engine(util.marl_config(6, sb), mb, sb)
    try:
        rows, k = 30, eng.D
        assert eng.A == 5 and k > 64
        c = dict(name="listed-marl", in_dim=k, rows=rows, scaling="unit", out_cols=4, seed=6, tick=12)
        x, p, v = ar.build_case(**c)
        pw, vw = tuple(_dev(w) for w in p), tuple(_dev(w) for w in v)
        want = _plain(eng, x, pw, vw, c["seed"], c["tick"], k)
        rng = np.random.default_rng(30)
        for name, listed in _lists(rows, rng).items():
            _compare(_listed(eng, x, pw, vw, c["seed"], c["tick"], k, listed), want, listed, 0, rows, True, ("marl", name))
        # refused: nothing is written, the clearing launch included
        act, logp, val = _buffers(rows)
        lst, cnt = _dev(np.arange(rows, dtype=np.int32)), _dev(np.array([rows], dtype=np.int32))
        wide = torch.zeros((rows, 512), dtype=torch.float32, device="cuda")
        p417, v417 = ar.make_networks(np.random.default_rng(1), 417, 4)
        pw417, vw417 = tuple(_dev(w) for w in p417), tuple(_dev(w) for w in v417)
        torch.cuda.synchronize()

        def call(nets, in_dim, pl, pc):
            return eng.L.pgd_mlp_actor_critic_rows(eng.h, -1, C.c_void_p(wide.data_ptr()), 512, in_dim, C.byref(nets), 0, 0, 0, pl, pc,
                                                   C.c_void_p(act.data_ptr()), C.c_void_p(logp.data_ptr()), C.c_void_p(val.data_ptr()))

        pl, pc = C.c_void_p(lst.data_ptr()), C.c_void_p(cnt.data_ptr())
        assert call(_nets(pw417, vw417), 417, pl, pc) == ERR_ARG
        assert call(_nets(pw, vw), k, None, pc) == ERR_ARG and call(_nets(pw, vw), k, pl, None) == ERR_ARG
        eng.sync()
        torch.cuda.synchronize()
        assert bool((act == SENT).all()) and bool((logp == SENT).all()) and bool((val == SENT).all()), "a refused call wrote"
        eng.set_groups(2)
        for name, listed in _lists(rows, rng, lo=15, hi=30).items():
            got = _listed(eng, x, pw, vw, c["seed"], c["tick"], k, listed, group=1, lo=15, hi=30)
            _compare(got, want, listed, 15, 30, True, ("marl group 1", name))
        listed = np.array([15, 18, 29])  # rows of group 0 and of no group in group 1's list: skipped, group 0's outputs keep their bytes
        got = _listed(eng, x, pw, vw, c["seed"], c["tick"], k, listed, group=1, lo=15, hi=30, foreign=(3, 14, 30, -1))
        _compare(got, want, listed, 15, 30, True, ("marl group 1", "foreign entries"))
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# masked GAE
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", mr.GAE_T)
def test_gae_masked(descs, T):
    """T x rows x lambda on the checker's seat histories (NaN wherever no agent acted) against float64; exactly zero where the mask is
    0; the mask exact; nothing written past the end; the all-PGD_F_REPORT history: pgd_gae's bits."""
    import torch
    eng = _ego_engine(descs, 1)
    try:
        worst = 0.0
        for c in mr.gae_cases():
            if c["T"] != T:
                continue
            rows = c["rows"]
            for all_report in (False, True):
                r, v, d, f, _ = mr.build_history(all_report=all_report, **c)
                tr, tv, td, tf = _dev(r), _dev(v), _dev(d), _flags_dev(f)
                for lam in mr.GAE_LAM:
                    buf = torch.full((2, T + 1, rows), SENT, dtype=torch.float32, device="cuda")
                    mbuf = torch.full((T + 1, rows), 9, dtype=torch.uint8, device="cuda")
                    eng.gae_masked(tr, tv, td, tf, mr.GAE_GAMMA, lam, adv=buf[0, :T], ret=buf[1, :T], mask=mbuf[:T])
                    eng.sync()
                    got, m = buf.cpu().numpy(), mbuf.cpu().numpy()
                    assert (got[:, T] == SENT).all() and (m[T] == 9).all(), (c, "written past the end")
                    a64, r64, m64 = mr.gae_masked_f64(r, v, d, f, mr.GAE_GAMMA, lam)
                    assert np.array_equal(m[:T], m64), (c, lam, "mask")
                    assert np.isfinite(got).all(), (c, lam)
                    assert (got[0, :T][m64 == 0] == 0).all() and (got[1, :T][m64 == 0] == 0).all(), (c, lam, "not zero where no agent acted")
                    err = max(float(np.abs(got[0, :T] - a64).max()), float(np.abs(got[1, :T] - r64).max()))
                    worst = max(worst, err)
                    assert err < mr.TOL_GAE_MASKED, (c, all_report, lam, err)
                    if all_report:
                        a2, r2 = eng.gae(tr, tv, td, mr.GAE_GAMMA, lam)
                        eng.sync()
                        assert np.array_equal(_bits(a2.cpu().numpy()), _bits(got[0, :T])) and np.array_equal(_bits(r2.cpu().numpy()), _bits(got[1, :T])), \
                            (c, lam, "not pgd_gae's bits")
        print("masked GAE, T = %d: max |device - f64| = %.2e (tolerance %.2e)" % (T, worst, mr.TOL_GAE_MASKED))
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# the collector
# ---------------------------------------------------------------------------------------------------------------------
COL_N, COL_A, COL_T, COL_SEED, COL_ROLLOUTS = Roundabout.N, Roundabout.A, 32, 3, 3
KEYS = train_util.KEYS + ("mask", "index", "count")


def _batch_equal(got, want, where):
    n = int(want["count"].item())
    assert int(got["count"].item()) == n, (where, "count")
    for key in KEYS:
        if key == "index":  # (entries at and behind the count are not written: they hold whatever an earlier rollout left)
            assert _bits_equal(got[key][:n], want[key][:n]), "%s: index differs from the synchronised loop" % where
        else:
            assert _bits_equal(got[key], want[key]), "%s: %s differs from the synchronised loop" % (where, key)


def test_collector_on_the_roundabout():
    """Three rollouts of T = 32 on 6 envs x 5 seats (horizon 40, delay_done 3; see train_util.Roundabout for the two envs that start near 5 x horizon).
    They hold -- asserted, so that nothing below passes vacuously -- agents ending by done, respawns (PGD_F_NEW without PGD_F_RESET), env
    resets, and resets that cut an agent that was not done.  Then:
    acted(t + 1) == live(t) for every t within and across the rollouts, and acted(0) is the state's ACTIVE seats; every tensor of the
    batch bit-identical to the same calls made one at a time with a synchronisation behind each, eagerly and replayed from a HIP graph;
    rows with mask 1 hold what mlp_actor_critic over ALL rows gives them; adv / ret within tolerance of the float64 checker on the
    collector's own arrays; index[:count] == flatnonzero(mask); actions, logp and values of seats that are not live are zero."""
    import torch
    T, N, A = COL_T, COL_N, COL_A
    S = Roundabout(COL_T, COL_SEED)
    want = synchronised_rollouts(S, COL_ROLLOUTS)

    # what the rollouts hold
    fl = np.concatenate([r["flags"].cpu().numpy() for r in want]).view(np.uint32)      # [3 T, N, A]
    dn = np.concatenate([r["dones"].cpu().numpy() for r in want])
    ac, lv = mr.acted(fl), mr.live(fl, dn)
    reset, new = (fl & mr.F_RESET) != 0, (fl & mr.F_NEW) != 0
    n_done, n_respawn = int((ac & (dn != 0)).sum()), int((new & ~reset).sum())
    n_reset, n_cut = int(reset.any(axis=2).sum()), int((reset & ac & (dn == 0)).sum())
    print("collector: %d agent-steps of %d seat-steps; %d ends by done, %d respawns, %d env resets, %d agents cut by a reset" % (
        ac.sum(), ac.size, n_done, n_respawn, n_reset, n_cut))
    assert n_done > 0 and n_respawn > 0 and n_reset > 0 and n_cut > 0
    assert np.array_equal(ac[0], S.active0), "acted(0) is not the state's ACTIVE seats"
    assert np.array_equal(ac[1:], lv[:-1]), "acted(t + 1) != live(t)"
    assert 0.1 < ac.mean() < 0.95
    for k, r in enumerate(want):
        m = r["mask"].cpu().numpy()
        f, d = r["flags"].cpu().numpy().view(np.uint32), r["dones"].cpu().numpy()
        assert np.array_equal(m != 0, mr.acted(f))
        n = int(r["count"].item())
        assert np.array_equal(r["index"].cpu().numpy()[:n], np.flatnonzero(m.reshape(-1)))
        rew, val = r["rewards"].cpu().numpy(), r["values"].cpu().numpy()
        a64, r64, _ = mr.gae_masked_f64(rew, val, d, f, 0.99, 0.95)
        adv, ret = r["advantages"].cpu().numpy(), r["returns"].cpu().numpy()
        err = max(float(np.abs(adv - a64).max()), float(np.abs(ret - r64).max()))
        assert err < mr.TOL_GAE_MASKED, (k, err)  # (values of a tenth, rewards up to the penalty of 10 once per agent)
        # seats that are not live: zeros in every row of actions, logp, values (row T: not live behind the last step)
        seat_live = np.concatenate([m != 0, mr.live(f[-1:], d[-1:])])                   # [T + 1, N, A]
        assert (val[~seat_live] == 0).all() and (r["logp"].cpu().numpy()[m == 0] == 0).all() and (r["actions"].cpu().numpy()[m == 0] == 0).all()
        assert (val[seat_live] != 0).all()
        # rows with mask 1: what the plain launch over all rows gives them
        for t in range(T):
            a_all = torch.zeros((N, A, 2), dtype=torch.float32, device="cuda")
            lp_all = torch.zeros((N, A), dtype=torch.float32, device="cuda")
            v_all = torch.zeros((N, A), dtype=torch.float32, device="cuda")
            S.eng.mlp_actor_critic(S.pw, S.vw, a_all, lp_all, v_all, COL_SEED, k * T + t, obs=r["obs"][t].contiguous())
            S.eng.sync()
            on = torch.from_numpy(m[t] != 0).cuda()
            assert _bits_equal(a_all[on], r["actions"][t][on]) and _bits_equal(lp_all[on], r["logp"][t][on]) and _bits_equal(v_all[on], r["values"][t][on]), (k, t)
        if k:
            assert _bits_equal(want[k - 1]["values"][T], r["values"][0])
    S.eng.close()

    # (a) the collector, eagerly, nothing synchronised inside collect()
    E = Roundabout(COL_T, COL_SEED)
    col = make_collector("marl", E, gamma=0.99, lam=0.95)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        for k in range(COL_ROLLOUTS):
            batch = col.collect()
            got = _snapshot(batch, KEYS)
            assert tuple(batch["obs"].shape) == (T, N, A, E.eng.D) and tuple(batch["values"].shape) == (T + 1, N, A)
            assert tuple(batch["mask"].shape) == (T, N, A) and tuple(batch["index"].shape) == (T * N * A, ) and tuple(batch["count"].shape) == (1, )
            _batch_equal(got, want[k], "eager collect %d" % k)
            if k == 0:
                col.set_weights(E.pw, E.vw)
    E.eng.close()

    # (b) collect() captured in a HIP graph behind one eager rollout (which primes the collector), replayed twice
    B = Roundabout(COL_T, COL_SEED)
    col = make_collector("marl", B)
    eager_then_graph(col.collect, lambda: _snapshot(col.batch, KEYS), want, compare=_batch_equal)
    B.eng.close()
