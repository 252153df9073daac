"""Observation normalisation on the device (pgdrive_amd/csrc/pgd_obs_norm.h and the NORM instantiations of the training kernels) against
the checker tests/obs_norm_ref.py:

* the moments (pgd_obs_norm_update / pgd_obs_norm_publish): exact inputs equal the checker with ==, general inputs within the bound
  derived from the sum lengths, the table within 1 fp32 ulp; every list form, NaN wherever it may stand, split calls, the same bytes
  twice, the first call of a fresh engine from a HIP graph, the refusals;
* the fused loads: each of the six entry points bound on raw observations against the unbound call on an array normalised beforehand
  with torch, bit for bit;
* the three collectors and the two learners with normalise_obs=True.
"""
import ctypes as C

import numpy as np
import pytest

from tests import actor_critic_ref as ar
from tests import obs_norm_ref as on
from tests.train_util import ERR_ARG, EVERY_LEARNER, KEYS, SENT, bits_equal, dev, eager_then_graph, ego_engine, learner_state, make, np_bits as _u64, restore, snapshot

pytestmark = pytest.mark.gpu

P = on.PART
WIDTHS = (4, 19, 274, 416)
LISTS = (1, P - 1, P, P + 1, 2 * P + 3)
EPS = 1e-8


@pytest.fixture(scope="module")
def eng(descs):
    """One env, ego only, no lidar: the moments need the engine for its device and stream only."""
    e = ego_engine(descs, 1)
    yield e
    e.close()


def _fold(eng, obs, D, record=None, index=None, count=None, n_list=None):
    """One pgd_obs_norm_update on numpy inputs, the scratch filled with NaN -> the record (numpy)."""
    import torch
    obs_d = dev(np.asarray(obs, np.float32))
    rec = dev(on.empty_record(D) if record is None else np.asarray(record, np.float64))
    idx = None if index is None else dev(np.asarray(index, np.int32))
    cnt = None if count is None else dev(np.array([count], np.int32))
    n = int(n_list if n_list is not None else (len(index) if index is not None else len(obs)))
    work = torch.full(((eng.obs_norm_work_bytes(D, n) + 7) // 8, ), float("nan"), dtype=torch.float64, device="cuda")
    eng.obs_norm_update(obs_d, rec, index=idx, count=cnt, n_list=n, in_dim=D, work=work)
    eng.sync()
    return rec.cpu().numpy()


def _publish(eng, record, eps=EPS):
    import torch
    D = (len(record) - 1) // 2
    tab = torch.full((2, on.padded(D)), float("nan"), dtype=torch.float32, device="cuda")
    eng.obs_norm_publish(dev(np.asarray(record, np.float64)), tab, eps=eps)
    eng.sync()
    return tab.cpu().numpy()


def _held(record, x, calls=1):
    """The record against two passes in extended precision within the derived bounds."""
    D = x.shape[1]
    n, mean, m2 = on.two_pass(x)
    bm, bq = on.bounds(x, calls)
    assert record[0] == n
    em, eq = np.abs(record[1:1 + D] - mean), np.abs(record[1 + D:] - m2)
    assert (em <= bm).all() and (eq <= bq).all(), (float((em / np.maximum(bm, 1e-300)).max()), float((eq / np.maximum(bq, 1e-300)).max()))
    return float(max((em / np.maximum(bm, 1e-300)).max(), (eq / np.maximum(bq, 1e-300)).max()))


def _general(rng, n, stride, D):
    x = (rng.normal(size=(n, stride)) * rng.uniform(0.01, 30.0, size=stride) + rng.normal(size=stride) * 5.0).astype(np.float32)
    x[:, D // 2] = 0.625
    x[:, D:] = np.nan
    return x


# ---------------------------------------------------------------------------------------------------------------------
# the moments
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", WIDTHS)
def test_exact_inputs_equal_the_checker(eng, D):
    stride = D + 3
    for n in LISTS:
        rng = np.random.default_rng([D, n])
        x = on.exact_rows(rng, n, stride)
        x[:, D:] = np.nan
        got = _fold(eng, x, D)
        want = on.update(on.empty_record(D), x[:, :D])
        assert np.array_equal(_u64(got), _u64(want)), (D, n, int((_u64(got) != _u64(want)).sum()))
        assert on.within_one_ulp(_publish(eng, got), on.table(want, EPS)), (D, n)
        # a second call of other rows on top of the first
        y = on.exact_rows(rng, n, stride)
        got2, want2 = _fold(eng, y, D, record=got), on.update(want, y[:, :D])
        assert np.array_equal(_u64(got2), _u64(want2)), (D, n, "second call")


@pytest.mark.parametrize("D", WIDTHS)
def test_general_inputs_are_within_the_derived_bound(eng, D):
    stride = D + 5
    worst = 0.0
    for n in LISTS:
        x = _general(np.random.default_rng([D, n, 1]), n, stride, D)
        got = _fold(eng, x, D)
        worst = max(worst, _held(got, x[:, :D]))
        want = on.update(on.empty_record(D), x[:, :D])
        _held(want, x[:, :D])
        tab = _publish(eng, got)
        assert on.within_one_ulp(tab, on.table(got, EPS)), (D, n)
        assert (tab[0, D:] == 0).all() and (tab[1, D:] == 1).all()
        if n > 1:
            assert tab[1, D // 2] == np.float32(1.0 / np.sqrt(EPS))   # (the constant column)
    print("in_dim %d: the largest share of the derived bound used %.4f" % (D, worst))


def test_the_empty_record_publishes_the_identity(eng):
    for D in WIDTHS:
        tab = _publish(eng, on.empty_record(D))
        assert (tab[0] == 0).all() and (tab[1] == 1).all()


@pytest.mark.parametrize("D", (4, 19, 274))
def test_list_forms_and_nan_in_every_row_that_is_not_listed(eng, D):
    rng = np.random.default_rng(D)
    stride, n_rows = D + 2, 2 * P + 40
    x = on.exact_rows(rng, n_rows, stride)
    x[:, D:] = np.nan
    perm = rng.permutation(n_rows).astype(np.int32)
    for n_list in (1, P + 1, 2 * P + 3):
        for count in (None, 0, n_list // 2 if n_list > 1 else 1):
            live = n_list if count is None else count
            # a shuffled index: the rows behind the count are in the index and hold NaN, as every row that is not in it
            y = x.copy()
            y[perm[live:]] = np.nan
            rec0 = on.update(on.empty_record(D), on.exact_rows(rng, 7, D))
            got = _fold(eng, y, D, record=rec0, index=perm[:n_list], count=count)
            want = on.update(rec0, x[perm[:live], :D])
            assert np.array_equal(_u64(got), _u64(want)), (D, n_list, count, "index")
            # no index: position = row
            y = x.copy()
            y[live:] = np.nan
            got = _fold(eng, y, D, record=rec0, count=count, n_list=n_list)
            want = on.update(rec0, x[:live, :D])
            assert np.array_equal(_u64(got), _u64(want)), (D, n_list, count, "plain")
            if live == 0:
                assert np.array_equal(_u64(got), _u64(rec0)), "a call with no live position moved the record"


def test_two_calls_of_half_a_list_are_one_call(eng):
    D, n = 19, 2 * P + 3
    rng = np.random.default_rng(7)
    for exact in (True, False):
        x = on.exact_rows(rng, n, D + 1) if exact else _general(rng, n, D + 1, D)
        first = _fold(eng, x[:n // 2], D)
        both = _fold(eng, x[n // 2:], D, record=first)
        _held(both, x[:, :D], calls=2)
        _held(_fold(eng, x, D), x[:, :D])
        if exact:
            want = on.update(on.update(on.empty_record(D), x[:n // 2, :D]), x[n // 2:, :D])
            assert np.array_equal(_u64(both), _u64(want))


def test_identical_bytes_from_two_runs(eng):
    D, n = 274, 2 * P + 3
    rng = np.random.default_rng(8)
    x = _general(rng, n, D + 2, D)
    idx = rng.permutation(n).astype(np.int32)
    a, b = _fold(eng, x, D, index=idx, count=n - 5), _fold(eng, x, D, index=idx, count=n - 5)
    assert np.array_equal(_u64(a), _u64(b))
    assert np.array_equal(_publish(eng, a).view(np.uint32), _publish(eng, b).view(np.uint32))


def test_the_first_call_of_a_fresh_engine_is_capturable(descs):
    """Nothing is allocated inside the calls: update and publish are captured as the very first calls of an engine; replay k folds the
    rows once more and publishes, as k eager calls do."""
    import torch
    D, n = 19, P + 1
    x = dev(_general(np.random.default_rng(9), n, D + 1, D))
    fresh = ego_engine(descs, 1)
    try:
        (rec_g, tab_g), (rec_e, tab_e) = fresh.obs_norm_state(D), fresh.obs_norm_state(D)
        work = torch.empty(((fresh.obs_norm_work_bytes(D, n) + 7) // 8, ), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()   # (its own capture: the first call on a fresh engine is made inside the capture, nothing runs eagerly in front)
        with torch.cuda.graph(graph, stream=s):
            fresh.obs_norm_update(x, rec_g, in_dim=D, work=work)
            fresh.obs_norm_publish(rec_g, tab_g, eps=EPS)
        torch.cuda.synchronize()
        assert bool((rec_g == 0).all()), "the capture itself ran the kernels"
        for k in range(3):
            with torch.cuda.stream(s):
                graph.replay()
            torch.cuda.synchronize()
            fresh.obs_norm_update(x, rec_e, in_dim=D)
            fresh.obs_norm_publish(rec_e, tab_e, eps=EPS)
            fresh.sync()
            assert bits_equal(rec_g, rec_e) and bits_equal(tab_g, tab_e), "replay %d" % (k + 1)
            assert float(rec_g[0]) == (k + 1) * n
        del graph
    finally:
        fresh.close()


def test_refused_arguments(eng):
    import torch
    D, stride, n = 19, 21, 40
    x = dev(on.exact_rows(np.random.default_rng(10), n, stride))
    rec, tab = eng.obs_norm_state(D)
    idx, cnt = dev(np.arange(n, dtype=np.int32)), dev(np.array([n], np.int32))
    work = torch.zeros((eng.obs_norm_work_bytes(D, n) // 8 + 1, ), dtype=torch.float64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    good = dict(obs=p(x), stride=stride, D=D, n_rows=n, index=p(idx), count=p(cnt), n_list=n, record=p(rec), work=p(work),
                work_bytes=eng.obs_norm_work_bytes(D, n))
    order = ("obs", "stride", "D", "n_rows", "index", "count", "n_list", "record", "work", "work_bytes")
    call = lambda **kw: eng.L.pgd_obs_norm_update(eng.h, *[dict(good, **kw)[k] for k in order])
    assert eng.obs_norm_work_bytes(D, n) == 8 * (2 + 2 * D) and eng.obs_norm_work_bytes(D, P + 1) == 8 * (2 + 4 * D)
    assert eng.obs_norm_work_bytes(3, n) == 0 and eng.obs_norm_work_bytes(417, n) == 0 and eng.obs_norm_work_bytes(D, 0) == 0
    bad = [dict(D=3), dict(D=417), dict(stride=D - 1), dict(n_list=0), dict(n_list=-1), dict(n_rows=0), dict(work_bytes=good["work_bytes"] - 1),
           dict(obs=None), dict(record=None), dict(work=None), dict(record=C.c_void_p(rec.data_ptr() + 4)),
           dict(work=C.c_void_p(work.data_ptr() + 4)), dict(index=None, n_list=n + 1, work_bytes=1 << 20)]
    for kw in bad:
        assert call(**kw) == ERR_ARG, kw
    assert eng.L.pgd_obs_norm_update(None, *[good[k] for k in order]) == ERR_ARG
    pub = lambda **kw: eng.L.pgd_obs_norm_publish(eng.h, *[dict(dict(record=p(rec), D=D, eps=EPS, table=p(tab)), **kw)[k]
                                                          for k in ("record", "D", "eps", "table")])
    for kw in (dict(D=3), dict(D=417), dict(eps=-1e-9), dict(eps=float("nan")), dict(record=None), dict(table=None),
               dict(table=C.c_void_p(tab.data_ptr() + 4))):
        assert pub(**kw) == ERR_ARG, kw
    bind = lambda table, D_, clip: eng.L.pgd_obs_norm_bind(eng.h, table, D_, clip)
    for args in ((p(tab), 3, 1.0), (p(tab), 417, 1.0), (p(tab), D, 0.0), (p(tab), D, -1.0), (p(tab), D, float("nan")),
                 (C.c_void_p(tab.data_ptr() + 4), D, 1.0)):
        assert bind(*args) == ERR_ARG, args
    assert eng.L.pgd_obs_norm_bind(None, p(tab), D, 1.0) == ERR_ARG
    eng.sync()
    assert bool((rec == 0).all()) and bool((tab[0] == 0).all()), "a refused call launched"
    for kw in (dict(), dict(index=None), dict(count=None), dict(index=None, count=None)):
        assert call(**kw) == 0, kw
    assert pub() == 0 and pub(eps=0.0) == 0
    assert bind(p(tab), D, float("inf")) == 0 and bind(None, 0, 0.0) == 0
    eng.sync()


# ---------------------------------------------------------------------------------------------------------------------
# the fused loads
# ---------------------------------------------------------------------------------------------------------------------
F_WIDTHS = (4, 19, 274, 330, 416)   # 330: the loader's slow path (more than 320 padded columns)
F_ROWS = (1, 15, 16, 17, 33)
CLIP = 1.5
F_MAX_STEP = 32


@pytest.fixture(scope="module")
def engines(descs):
    es = {n: ego_engine(descs, n) for n in F_ROWS}
    yield es
    for e in es.values():
        e.close()


class _Case:
    """Raw rows [rows, D + 3] (NaN beyond D), a table with a nonzero shift in every column (the last real one included) that drives
    entries into the clamp on both sides, the same rows normalised beforehand with torch's separate fp32 ops (columns at and beyond D:
    0), and three random networks."""
    def __init__(self, rows, D, seed=0, clip=CLIP):
        import torch
        rng = np.random.default_rng([rows, D, seed])
        self.D, self.clip = D, clip
        raw = (rng.normal(size=(rows, D + 3)) * 2.0 + 0.5).astype(np.float32)
        raw[:, D:] = np.nan
        tab = np.zeros((2, on.padded(D)), np.float32)
        tab[1] = 1.0
        tab[0, :D] = rng.normal(size=D) + 0.75
        tab[1, :D] = rng.uniform(0.3, 2.5, size=D)
        self.raw, self.table = dev(raw), dev(tab)
        x = self.raw[:, :D]
        pre = torch.zeros_like(self.raw)
        pre[:, :D] = ((x - self.table[0, :D]) * self.table[1, :D]).clamp(-clip, clip)
        self.pre = pre
        assert np.array_equal(pre.cpu().numpy().view(np.uint32), on.normalise(raw, tab, clip, D).view(np.uint32)), "torch is not the checker"
        assert bool((pre == clip).any()) and bool((pre == -clip).any()) or rows * D < 40
        p, v = ar.make_networks(rng, D, 4)
        _, c = ar.make_networks(rng, D, 4)
        self.pw, self.vw, self.cw = [tuple(dev(w) for w in n) for n in (p, v, c)]
        self.ident = dev(on.table(on.empty_record(D), EPS))


def _outputs(rows, n):
    import torch
    return [torch.full((rows, 1, 2) if i == 0 else (rows, 1), SENT, dtype=torch.float32, device="cuda") for i in range(n)]


def _both(eng, case, run):
    """run(obs) bound on the raw rows, unbound on the normalised ones, and bound to the identity with clip = inf on the normalised ones
    -> the three results (lists of tensors)."""
    import torch
    eng.obs_norm_bind(case.table, case.D, case.clip)
    fused = run(case.raw)
    eng.obs_norm_bind(None)
    plain = run(case.pre)
    eng.obs_norm_bind(case.ident, case.D, float("inf"))
    ident = run(case.pre)
    eng.obs_norm_bind(None)
    torch.cuda.synchronize()
    return fused, plain, ident


def _same(fused, plain, ident, where):
    for i, (f, q, d) in enumerate(zip(fused, plain, ident)):
        assert bool(torch_isfinite(q)), (where, i)
        assert bits_equal(f, q), (where, i, "the bound call on raw rows is not the unbound call on normalised rows")
        assert bits_equal(d, q), (where, i, "the identity table with clip = inf is not the unbound call")


def torch_isfinite(t):
    import torch
    return torch.isfinite(t).all()


@pytest.mark.parametrize("D", F_WIDTHS)
def test_fused_forward_entry_points(engines, D):
    import torch
    for rows in F_ROWS:
        eng, case = engines[rows], _Case(rows, D)
        seed, tick = 11, 3

        def ac(obs):
            out = _outputs(rows, 3)
            eng.mlp_actor_critic(case.pw, case.vw, *out, seed, tick, obs=obs, in_dim=D)
            return out

        def ac_cost(obs):
            out = _outputs(rows, 4)
            eng.mlp_actor_critic_cost(case.pw, case.vw, case.cw, *out, seed, tick, obs=obs, in_dim=D)
            return out

        _same(*_both(eng, case, ac), ("mlp_actor_critic", D, rows))
        _same(*_both(eng, case, ac_cost), ("mlp_actor_critic_cost", D, rows))

        # the row-list form: every row that is not listed holds NaN
        rng = np.random.default_rng([D, rows])
        listed = np.sort(rng.permutation(rows)[:max(1, (2 * rows) // 3)]).astype(np.int32)
        keep = np.zeros(rows, bool)
        keep[listed] = True
        holes = dev(~keep)
        rows_t = torch.zeros((rows, ), dtype=torch.int32, device="cuda")
        rows_t[:len(listed)] = dev(listed)
        count = dev(np.array([len(listed)], np.int32))

        def ac_rows(obs):
            o = obs.clone()
            o[holes] = float("nan")
            out = _outputs(rows, 3)
            eng.mlp_actor_critic_rows(case.pw, case.vw, rows_t, count, *out, seed, tick, obs=o, in_dim=D)
            return out

        _same(*_both(eng, case, ac_rows), ("mlp_actor_critic_rows", D, rows))

        # the mask form: the truncated rows alone are read
        flags = dev(np.where(keep, F_MAX_STEP, 0).astype(np.int32))
        done = dev(keep.astype(np.uint8))

        def term(obs):
            o = obs.clone()
            o[holes] = float("nan")
            tv, tcv = [torch.full((rows, ), SENT, dtype=torch.float32, device="cuda") for _ in range(2)]
            eng.mlp_terminal_value(case.vw, case.cw, o, flags, done, tv, tcv, in_dim=D)
            return [tv, tcv]

        f, q, d = _both(eng, case, term)
        _same(f, q, d, ("mlp_terminal_value", D, rows))
        assert bool((q[0][holes] == 0).all()) and bool((q[0][~holes] != 0).all())


@pytest.mark.parametrize("D", F_WIDTHS)
def test_fused_ppo_grad(engines, D):
    """A strided minibatch whose live positions cross a 1024-row partition of the weight gradients, through an index: every gradient of
    the two (pgd_ppo_grad) and three (pgd_ppo_grad_cost) networks and all 8 statistics, bit for bit."""
    import torch
    from pgdrive_amd.learner import flat_layout
    eng = engines[1]
    n_rows, start, stride, rows = 2200, 1, 2, 1060
    case = _Case(n_rows, D, seed=1)
    rng = np.random.default_rng(D)
    index = dev(rng.permutation(n_rows).astype(np.int32))
    count = dev(np.array([n_rows - 20], np.int32))   # live positions 1, 3, .. < 2180: 1090 > rows -> all 1060 live, 1024 crossed
    actions = dev(rng.normal(size=(n_rows, 2)).astype(np.float32))
    logp, adv, ret, cret = [dev(rng.normal(size=n_rows).astype(np.float32)) for _ in range(4)]
    f32 = dict(dtype=torch.float32, device="cuda")

    for cost in (False, True):
        layout, total = flat_layout(D, 4, has_cost_critic=cost)
        work = torch.empty(((eng.ppo_cost_work_bytes(D, rows) if cost else eng.ppo_work_bytes(D, rows, True)) // 4 + 4, ), **f32)

        def run(obs):
            grads = torch.full((total, ), SENT, **f32)
            gv = tuple(grads[o:o + int(np.prod(shape))].view(shape) for _, shape, o in layout)
            stats = torch.full((8, ), SENT, **f32)
            kw = dict(start=start, stride=stride, rows=rows, index=index, count=count, n_list=n_rows, in_dim=D)
            if cost:
                eng.ppo_grad_cost(case.pw, case.vw, case.cw, gv[:6], gv[6:12], gv[12:], obs, actions, logp, adv, ret, cret, stats, work, **kw)
            else:
                eng.ppo_grad(case.pw, case.vw, gv[:6], gv[6:], obs, actions, logp, adv, ret, stats, work, **kw)
            return [grads, stats]

        f, q, d = _both(eng, case, run)
        _same(f, q, d, ("ppo_grad_cost" if cost else "ppo_grad", D))
        assert float(q[1][0]) == rows and bool((q[0] != SENT).any())


def test_a_width_mismatch_between_the_binding_and_the_call_is_refused(engines):
    import torch
    from pgdrive_amd.engine import PgdError
    from pgdrive_amd.learner import flat_layout
    eng, rows = engines[16], 16
    case, other = _Case(rows, 19), _Case(rows, 274)
    eng.obs_norm_bind(other.table, 274, CLIP)
    try:
        out = _outputs(rows, 4)
        flags, done = dev(np.full(rows, F_MAX_STEP, np.int32)), dev(np.ones(rows, np.uint8))
        rows_t, count = dev(np.arange(rows, dtype=np.int32)), dev(np.array([rows], np.int32))
        layout, total = flat_layout(19, 4, has_cost_critic=True)
        grads = torch.zeros((total, ), dtype=torch.float32, device="cuda")
        gv = tuple(grads[o:o + int(np.prod(shape))].view(shape) for _, shape, o in layout)
        stats = torch.full((8, ), SENT, dtype=torch.float32, device="cuda")
        work = torch.empty((eng.ppo_cost_work_bytes(19, rows) // 4 + 4, ), dtype=torch.float32, device="cuda")
        act, vec = dev(np.zeros((rows, 2), np.float32)), dev(np.zeros(rows, np.float32))
        calls = [lambda: eng.mlp_actor_critic(case.pw, case.vw, *out[:3], 0, 0, obs=case.raw, in_dim=19),
                 lambda: eng.mlp_actor_critic_cost(case.pw, case.vw, case.cw, *out, 0, 0, obs=case.raw, in_dim=19),
                 lambda: eng.mlp_actor_critic_rows(case.pw, case.vw, rows_t, count, *out[:3], 0, 0, obs=case.raw, in_dim=19),
                 lambda: eng.mlp_terminal_value(case.vw, None, case.raw, flags, done, out[1].view(-1), in_dim=19),
                 lambda: eng.ppo_grad(case.pw, case.vw, gv[:6], gv[6:12], case.raw, act, vec, vec, vec, stats, work, in_dim=19),
                 lambda: eng.ppo_grad_cost(case.pw, case.vw, case.cw, gv[:6], gv[6:12], gv[12:], case.raw, act, vec, vec, vec, vec, stats, work,
                                           in_dim=19)]
        for i, c in enumerate(calls):
            with pytest.raises(PgdError):
                c()
        torch.cuda.synchronize()
        assert all(bool((o == SENT).all()) for o in out) and bool((stats == SENT).all()), "a refused call launched"
        # the policy-only kernel ignores the binding
        a = torch.zeros((rows, 1, 2), dtype=torch.float32, device="cuda")
        eng.mlp_policy(case.pw, out=a, obs=case.pre, in_dim=19)
        eng.obs_norm_bind(None)
        b = torch.zeros((rows, 1, 2), dtype=torch.float32, device="cuda")
        eng.mlp_policy(case.pw, out=b, obs=case.pre, in_dim=19)
        torch.cuda.synchronize()
        assert bits_equal(a, b)
    finally:
        eng.obs_norm_bind(None)


# ---------------------------------------------------------------------------------------------------------------------
# the collectors and the learners
# ---------------------------------------------------------------------------------------------------------------------
C_CLIP, C_EPS = 2.0, 1e-6
ON_KEYS = ("obs_norm", "obs_norm_record")
KINDS = [("single", False), ("single", True), ("safe", False), ("safe", True), ("marl", False)]
IDS = ["RolloutCollector", "RolloutCollector-bootstrap", "SafeRolloutCollector", "SafeRolloutCollector-bootstrap", "MultiAgentRolloutCollector"]


def _make(kind, descs, bootstrap, **kw):
    extra = dict(bootstrap_truncations=True) if bootstrap else {}
    return make(kind, descs, **extra, **kw)


def _hand_rows(kind, S, col, table, clip, t, tick, live):
    """The network call of observation row t made by hand, unbound, on rows normalised with torch -> (actions, logp, values)."""
    import torch
    eng, D = S.eng, S.eng.D
    raw = col._obs[t].reshape(-1, D)
    pre = ((raw - table[0, :D]) * table[1, :D]).clamp(-clip, clip)
    n = raw.shape[0]
    a = torch.full(col._actions[t].shape, SENT, dtype=torch.float32, device="cuda")
    lp, v, cv = [torch.full(col._logp[t].shape, SENT, dtype=torch.float32, device="cuda") for _ in range(3)]
    if kind == "marl":
        pre = torch.where(torch.isfinite(pre), pre, torch.zeros_like(pre))
        eng.mlp_actor_critic_rows(col.policy_weights, col.value_weights, live[0], live[1], a, lp, v, col.seed, tick, obs=pre.view(col._obs[t].shape))
    elif kind == "safe":
        eng.mlp_actor_critic_cost(col.policy_weights, col.value_weights, col.cost_weights, a, lp, v, cv, col.seed, tick, obs=pre)
    else:
        eng.mlp_actor_critic(col.policy_weights, col.value_weights, a, lp, v, col.seed, tick, obs=pre)
    torch.cuda.synchronize()
    return a, lp, v


@pytest.mark.parametrize("kind,bootstrap", KINDS, ids=IDS)
def test_collectors_and_learners(descs, kind, bootstrap):
    """Three `collect(); update()` iterations with normalise_obs=True: the table and the record from the rollout's raw obs by the checker
    (publish, T steps, fold), the first table the identity, rows 1 .. T of actions / logp / values the unbound network call on
    torch-normalised rows with the rollout's table and row 0 the carried row T of the rollout before, the multi-agent fold counting
    batch["count"] samples, update() the same calls made by hand with the table bound; then the frozen mode and a state_dict round trip."""
    import torch
    marl = kind == "marl"
    S, col, L = _make(kind, descs, bootstrap, normalise_obs=True, clip_obs=C_CLIP, obs_eps=C_EPS)
    eng, D, T = S.eng, S.eng.D, col.T
    record = on.empty_record(D)
    last_row = None
    with torch.no_grad():
        for it in range(3):
            batch = col.collect()
            torch.cuda.synchronize()
            assert all(k in batch for k in ON_KEYS) and batch["obs_norm"].shape == (2, on.padded(D)) and batch["obs_norm_record"].dtype == torch.float64
            tab = batch["obs_norm"].cpu().numpy()
            want_tab = on.table(record, C_EPS)
            if it == 0:
                assert np.array_equal(tab, want_tab) and (tab[0] == 0).all() and (tab[1] == 1).all(), "the first rollout's table is not the identity"
            assert on.within_one_ulp(tab, want_tab), (kind, it, "table")
            obs = batch["obs"].cpu().numpy().reshape(-1, D)
            if marl:
                n = int(batch["count"].item())
                listed = obs[batch["index"][:n].cpu().numpy()]
            else:
                n, listed = len(obs), obs
            assert np.isfinite(listed).all()
            got = batch["obs_norm_record"].cpu().numpy()
            assert got[0] == record[0] + n, (kind, it, "the fold did not count the listed rows")
            record = on.update(record, listed)
            err_m = np.abs(got[1:1 + D] - record[1:1 + D]).max()
            # the device against the checker on the same samples: both within the derived bound of the exact moments of everything folded
            seen = listed if it == 0 else np.concatenate([seen, listed])
            _held(got, seen, calls=it + 1)
            _held(record, seen, calls=it + 1)
            print("%s, rollout %d: %d samples, |mean - checker| %.1e" % (kind, it, n, err_m))
            assert bits_equal(batch["obs"], col._obs[:T])   # raw
            # rows 1 .. T: the unbound call on normalised rows, with this rollout's table and weights
            for t in range(1, T + 1):
                live = None
                if marl:
                    live = eng.live_rows(col.flags[t - 1], col.dones[t - 1])
                a, lp, v = _hand_rows(kind, S, col, batch["obs_norm"], C_CLIP, t, it * T + t, live)
                assert bits_equal(a, col._actions[t]) and bits_equal(lp, col._logp[t]) and bits_equal(v, col.values[t]), (kind, it, t)
            if last_row is not None:   # row 0: evaluated under the table and the weights of the rollout before
                for x, y in zip(last_row, (col._actions[0], col._logp[0], col.values[0])):
                    assert bits_equal(x, y), (kind, it, "row 0 is not the carried row T")
            last_row = [x[T].clone() for x in (col._actions, col._logp, col.values)]
            # update(): the same calls by hand with the table bound
            before = learner_state(L)
            L.update(batch)
            torch.cuda.synchronize()
            after = learner_state(L)
            restore(L, before)
            index, count = batch.get("index"), batch.get("count")
            adv, norm = L._advantages(batch, index, count)
            eng.obs_norm_bind(batch["obs_norm"], D, C_CLIP)
            k = 0
            for _ in range(L.epochs):
                for start, stride, rows in L.plan:
                    L._grad(batch, adv, L.stats[k], start=start, stride=stride, rows=rows, index=index, count=count, n_list=L.n_list,
                            adv_stats=norm, clip=L.clip, ent_coef=L.ent_coef, in_dim=L.in_dim)
                    eng.adam(L.params, L.grads, L.m, L.v, L.step, L.lr, betas=L.betas, eps=L.eps, max_grad_norm=L.max_grad_norm)
                    k += 1
            eng.obs_norm_bind(None)
            torch.cuda.synchronize()
            hand = learner_state(L)
            for key in after:
                assert bits_equal(after[key], hand[key]), (kind, it, key, "update() is not the calls by hand with the table bound")
            if it == 1:   # and without the table the gradients are others
                restore(L, before)
                adv, norm = L._advantages(batch, index, count)
                start, stride, rows = L.plan[0]
                L._grad(batch, adv, L.stats[0], start=start, stride=stride, rows=rows, index=index, count=count, n_list=L.n_list, adv_stats=norm,
                        clip=L.clip, ent_coef=L.ent_coef, in_dim=L.in_dim)
                torch.cuda.synchronize()
                unbound = L.grads.clone()
                restore(L, after)
                assert not bits_equal(unbound, after["grads"])
        # the frozen mode
        state = col.state_dict()
        assert np.array_equal(_u64(state["obs_norm_record"]), _u64(col.obs_norm_record.cpu().numpy()))
        col.freeze_obs_norm(True)
        batch = col.collect()
        torch.cuda.synchronize()
        assert np.array_equal(_u64(col.state_dict()["obs_norm_record"]), _u64(state["obs_norm_record"])), "the frozen mode moved the record"
        assert on.within_one_ulp(batch["obs_norm"].cpu().numpy(), on.table(state["obs_norm_record"], C_EPS))
        col.freeze_obs_norm(False)
        table_next = on.table(state["obs_norm_record"], C_EPS)
    S.eng.close()

    # a state_dict round trip into a fresh collector: it continues from the record -- its next table and its next fold
    S2, col2, _ = _make(kind, descs, bootstrap, learn=False, normalise_obs=True, clip_obs=C_CLIP, obs_eps=C_EPS)
    col2.load_state_dict(state)
    with torch.no_grad():
        b2 = col2.collect()
    torch.cuda.synchronize()
    assert np.array_equal(b2["obs_norm"].cpu().numpy().view(np.uint32), batch["obs_norm"].cpu().numpy().view(np.uint32)), "another table"
    assert on.within_one_ulp(b2["obs_norm"].cpu().numpy(), table_next)
    o2 = b2["obs"].cpu().numpy().reshape(-1, D)
    if marl:
        o2 = o2[b2["index"][:int(b2["count"].item())].cpu().numpy()]
    got, want = b2["obs_norm_record"].cpu().numpy(), on.update(state["obs_norm_record"], o2)
    assert got[0] == want[0] == state["obs_norm_record"][0] + len(o2)
    _held(got, np.concatenate([seen, o2]), calls=4)
    S2.eng.close()

    # a state for a collector built without the switch is refused; the switch off: the batch of before, none of the new calls
    S3, col3, L3 = _make(kind, descs, bootstrap)
    with pytest.raises(ValueError):
        col3.load_state_dict(state)

    def boom(*a, **kw):
        raise AssertionError("an observation normalisation call with normalise_obs=False")

    S3.eng.obs_norm_update = S3.eng.obs_norm_publish = S3.eng.obs_norm_bind = boom
    S4, col4, _ = _make(kind, descs, bootstrap, learn=False, normalise_obs=True, clip_obs=C_CLIP, obs_eps=C_EPS)
    with torch.no_grad():
        off, first = col3.collect(), col4.collect()
        L3.update(off)
    torch.cuda.synchronize()
    assert not any(k in off for k in ON_KEYS) and "obs_norm_record" not in col3.state_dict()
    assert sorted(off) == sorted(k for k in first if k not in ON_KEYS)
    for key in ("obs", "actions", "logp", "values", "rewards", "dones", "advantages"):   # (the identity table: the first rollout is raw)
        assert bits_equal(off[key], first[key]), (key, "the first rollout under the identity table is not the rollout without the switch")
    S3.eng.close()
    S4.eng.close()


@pytest.mark.parametrize("kind,bootstrap", KINDS, ids=IDS)
def test_prime_collect_update_in_one_graph(descs, kind, bootstrap):
    """Behind one eager iteration: prime(), collect() and update() captured in ONE graph (the multi-agent prime() reads the engine's state
    on the host and stays outside, as its docstring says) and replayed three times, against the same calls made eagerly, bit for bit."""
    import torch
    marl = kind == "marl"
    keys = KEYS + ON_KEYS + (("mask", "count") if marl else ()) + (("term_values", ) if bootstrap else ())

    def iteration(col, L):
        if not marl:
            col.prime()
        L.update(col.collect())

    def state(col, L):
        return dict(snapshot(col.batch, keys), **learner_state(L))

    kw = dict(normalise_obs=True, clip_obs=C_CLIP, obs_eps=C_EPS)
    E, col, L = _make(kind, descs, bootstrap, **kw)
    want = []
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        for it in range(4):
            iteration(col, L)
            want.append(state(col, L))
    E.eng.close()
    assert not bits_equal(want[1]["obs_norm"], want[2]["obs_norm"])

    G, col, L = _make(kind, descs, bootstrap, **kw)
    eager_then_graph(lambda: iteration(col, L), lambda: state(col, L), want, replays=3, need=keys + EVERY_LEARNER)
    G.eng.close()
