"""pgd_shuffle_index and pgd_adam_gated (pgdrive_amd/csrc/pgd_minibatch.h) and the learners' switches shuffle / target_kl / lr_scale on the
device:

* the permutation kernel against the integer restatement of tests/minibatch_ref.py with `==`: counts around every power of two and the
  workgroup size, with and without an index, a device count below n_list (the tail keeps its sentinel), zero, negative, above n_list,
  the epoch rule, the refusals;
* pgd_ppo_grad over a shuffled list against the float64 checker of tests/ppo_ref.py on the same permuted rows (that file's tolerances);
* pgd_adam_gated byte for byte against pgd_adam when it applies, against the untouched buffers when it skips; the gate's counters;
* PPOLearner: shuffle=True against the calls made by hand, collect + update from one graph whose replays draw new permutations, the
  switches off against today's calls, an update that stops inside; PPOLagLearner with both switches; a multi-agent rollout whose shuffled
  minibatches the host recomputes from the mask.
"""
import ctypes as C

import numpy as np
import pytest

from tests import actor_critic_ref as ar
from tests import minibatch_ref as mr
from tests import ppo_ref as rf
from tests.ppo_util import Problem as _Problem, check as _check, grad as _grad
from tests.train_util import ERR_ARG, EVERY_LEARNER, Traffic, assert_same, dev as _dev, ego_engine, learner_state, make_collector, update_by_hand

pytestmark = pytest.mark.gpu

SHUF_COUNTS = (1, 2, 3, 5, 16, 17, 255, 256, 257, 1025, 4099)
ISENT = -77   # what an int32 output holds before a launch


@pytest.fixture(scope="module")
def eng(descs):
    e = ego_engine(descs, 1)
    yield e
    e.close()


def _i32(a):
    return _dev(np.asarray(a, dtype=np.int32))


def _shuffle(eng, index, count, n_list, seed, epoch, epoch_dev=None):
    """One Engine.shuffle_index into a sentinel-filled buffer of n_list + 3 entries -> numpy (the three behind n_list must survive)."""
    import torch
    out = torch.full((n_list + 3, ), ISENT, dtype=torch.int32, device="cuda")
    eng.shuffle_index(None if index is None else _i32(index), None if count is None else _i32([count]), n_list, seed, epoch,
                      epoch_dev=None if epoch_dev is None else _i32([epoch_dev]), out=out)
    eng.sync()
    got = out.cpu().numpy()
    assert (got[n_list:] == ISENT).all(), "written beyond n_list"
    return got[:n_list]


# ---------------------------------------------------------------------------------------------------------------------
# pgd_shuffle_index
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_index", [False, True])
def test_shuffle_index_equals_the_restatement(eng, with_index):
    for c in SHUF_COUNTS:
        index = (np.random.default_rng(c).permutation(3 * c + 7)[:c] - 5).astype(np.int32) if with_index else None   # (entries are data: any int32)
        for seed, epoch in ((0, 0), (0xdeadbeef, 0xfffffffe)):
            got = _shuffle(eng, index, None, c, seed, epoch)
            want = mr.shuffle_index(index, None, c, seed, epoch)
            assert (got == want).all(), (c, with_index, seed, epoch)
            assert sorted(got) == sorted(index if with_index else range(c))


def test_shuffle_index_reads_the_count_and_the_epoch_on_the_device(eng):
    n_list = 300
    index = np.concatenate([np.arange(1000, 1037), np.full(n_list - 37, 0x7fffffff)]).astype(np.int32)   # garbage behind the count
    sent = np.full(n_list, ISENT, dtype=np.int32)
    for idx in (None, index):
        got = _shuffle(eng, idx, 37, n_list, 5, 2)
        assert (got == mr.shuffle_index(idx, 37, n_list, 5, 2, out=sent)).all()
        assert (got[37:] == ISENT).all() and (got[:37] != ISENT).all(), "the tail behind the count was written"
        for count in (0, -4):   # nothing is written
            assert (_shuffle(eng, idx, count, n_list, 5, 2) == ISENT).all()
    for count in (n_list + 1, 0x7fffffff):   # a count above n_list clamps
        assert (_shuffle(eng, None, count, n_list, 5, 2) == mr.permutation(n_list, 5, 2)).all()
    assert (_shuffle(eng, None, None, 0, 5, 2) == ISENT).all()   # an empty list: no launch
    # e = epoch + *d_epoch
    a, b = _shuffle(eng, index, 37, n_list, 5, 3, epoch_dev=4), _shuffle(eng, index, 37, n_list, 5, 7)
    assert (a == b).all() and (a == mr.shuffle_index(index, 37, n_list, 5, 7, out=sent)).all()
    assert (_shuffle(eng, None, None, 257, 5, 0, epoch_dev=-1) == mr.permutation(257, 5, 0xffffffff)).all()
    assert not (_shuffle(eng, None, None, 257, 5, 0) == _shuffle(eng, None, None, 257, 5, 1)).all()


def test_shuffle_index_refusals(eng):
    import torch
    from pgdrive_amd import _abi
    out = torch.full((8, ), ISENT, dtype=torch.int32, device="cuda")
    idx = torch.arange(8, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    eng._follow_stream()
    f, po, pi = eng.L.pgd_shuffle_index, C.c_void_p(out.data_ptr()), C.c_void_p(idx.data_ptr())
    assert f(None, pi, None, 8, 0, 0, None, po) == ERR_ARG
    assert f(eng.h, pi, None, 8, 0, 0, None, None) == ERR_ARG
    assert f(eng.h, pi, None, -1, 0, 0, None, po) == ERR_ARG
    assert f(eng.h, None, None, _abi.PPO_ROWS_MAX + 1, 0, 0, None, po) == ERR_ARG
    assert f(eng.h, po, None, 8, 0, 0, None, po) == ERR_ARG   # d_out must not be d_index
    eng.sync()
    assert bool((out == ISENT).all()), "a refused call wrote"
    base = torch.arange(16, dtype=torch.int32, device="cuda")
    with pytest.raises(AssertionError, match="overlaps"):
        eng.shuffle_index(base[:8], None, 8, 0, 0, out=base[4:12])
    assert f(eng.h, pi, None, 8, 0, 0, None, po) == 0
    eng.sync()
    assert sorted(out.cpu().numpy()) == list(range(8))


# ---------------------------------------------------------------------------------------------------------------------
# pgd_ppo_grad over a shuffled list
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_dim", [20, 274])
def test_ppo_grad_on_a_shuffled_list(eng, in_dim):
    """64 rows in 4 strided minibatches over the device's permutation: each against float64 over the rows the HOST reads out of `shuffled`;
    together they cover the list exactly once."""
    import torch
    n, n_mb = 64, 4
    case = rf.build_case("shuffled", in_dim, n, scaling="normalised", out_cols=4, seed=in_dim, normalise=True)
    P = _Problem(case)
    shuffled = torch.full((n, ), ISENT, dtype=torch.int32, device="cuda")
    eng.shuffle_index(None, None, n, 21, 1, out=shuffled)
    eng.sync()
    host = shuffled.cpu().numpy()
    assert (host == mr.permutation(n, 21, 1)).all()
    P.index, P.n_list = shuffled, n
    seen = []
    for j in range(n_mb):
        sel = host[j::n_mb]
        seen.append(sel)
        got = _grad(eng, P, start=j, stride=n_mb, rows=n // n_mb)
        assert got["stats"][0] == len(sel)
        _check(got, rf.reference_of(rf.subset_case(case, sel)), "in_dim %d, shuffled minibatch %d of %d" % (in_dim, j, n_mb))
    assert np.array_equal(np.sort(np.concatenate(seen)), np.arange(n))
    assert len(set(seen[0] % n_mb)) > 1, "minibatch 0 is the strided one"


# ---------------------------------------------------------------------------------------------------------------------
# pgd_adam_gated
# ---------------------------------------------------------------------------------------------------------------------
def _adam_state(p0, n):
    import torch
    return dict(p=_dev(p0), m=torch.zeros(n, device="cuda"), v=torch.zeros(n, device="cuda"), step=torch.zeros(4, dtype=torch.int32, device="cuda"))


def _same(a, b, what):
    import torch
    torch.cuda.synchronize()
    assert_same(a, b, what)


@pytest.mark.parametrize("n_elem", [1, 1000])
def test_adam_gated_applies_as_adam_and_skips_without_a_trace(eng, n_elem):
    import torch
    for mode in rf.ADAM_NORMS:
        p0, g, mx = rf.build_adam(n_elem, mode)
        gs = [_dev(x) for x in g]
        # three ungated calls: pgd_adam's bytes
        plain, gated = _adam_state(p0, n_elem), _adam_state(p0, n_elem)
        gate = torch.zeros(4, dtype=torch.int32, device="cuda")
        for t in range(3):
            eng.adam(plain["p"], gs[t], plain["m"], plain["v"], plain["step"], max_grad_norm=mx, **rf.ADAM_HYPER)
            eng.adam_gated(gated["p"], gs[t], gated["m"], gated["v"], gated["step"], gate=gate, max_grad_norm=mx, **rf.ADAM_HYPER)
        _same(plain, gated, "ungated, %s" % mode)
        assert gate.tolist() == [0, 3, 0, 0] and int(gated["step"][0]) == 3
        # a kl below the limit applies as well, and leaves the count alone
        kl, cg = _dev(np.array([0.0149], dtype=np.float32)), _i32([55])
        eng.adam(plain["p"], gs[0], plain["m"], plain["v"], plain["step"], max_grad_norm=mx, **rf.ADAM_HYPER)
        eng.adam_gated(gated["p"], gs[0], gated["m"], gated["v"], gated["step"], gate=gate, max_grad_norm=mx, kl=kl, kl_limit=0.015, count_gate=cg,
                       **rf.ADAM_HYPER)
        _same(plain, gated, "kl below the limit, %s" % mode)
        assert gate.tolist() == [0, 4, 0, 0] and int(cg[0]) == 55
        # the skips: gate[0] preset, kl above the limit, kl NaN -- every buffer keeps its bytes, the counters move, the count is zeroed
        before = {k: x.clone() for k, x in gated.items()}
        for what, preset, klv in (("preset", 1, 0.0), ("above", 0, 0.0151), ("nan", 0, float("nan"))):
            gate = _i32([preset, 4, 2, 0])
            kl, cg = _dev(np.array([klv], dtype=np.float32)), _i32([55])
            eng.adam_gated(gated["p"], gs[1], gated["m"], gated["v"], gated["step"], gate=gate, max_grad_norm=mx, kl=kl, kl_limit=0.015,
                           count_gate=cg, **rf.ADAM_HYPER)
            _same(before, gated, "skip (%s), %s" % (what, mode))
            assert gate.tolist() == [1, 4, 3, 1] and int(cg[0]) == 0, (what, gate.tolist())
            eng.adam_gated(gated["p"], gs[2], gated["m"], gated["v"], gated["step"], gate=gate, max_grad_norm=mx, **rf.ADAM_HYPER)   # shut stays shut, no kl, no count
            _same(before, gated, "second skip (%s), %s" % (what, mode))
            assert gate.tolist() == [1, 4, 4, 1]
        # lr_scale 0.5: pgd_adam with the fp32 product as its lr
        a, b = _adam_state(p0, n_elem), _adam_state(p0, n_elem)
        gate = torch.zeros(4, dtype=torch.int32, device="cuda")
        scale = _dev(np.array([0.5], dtype=np.float32))
        hyper = dict(rf.ADAM_HYPER)
        lr = hyper.pop("lr")
        for t in range(2):
            eng.adam(a["p"], gs[t], a["m"], a["v"], a["step"], float(np.float32(lr) * np.float32(0.5)), max_grad_norm=mx, **hyper)
            eng.adam_gated(b["p"], gs[t], b["m"], b["v"], b["step"], lr, gate, max_grad_norm=mx, lr_scale=scale, **hyper)
        _same(a, b, "lr_scale 0.5, %s" % mode)
        scale.fill_(0.3)   # not a power of two: the product is rounded to fp32 once, on the device as on the host
        eng.adam(a["p"], gs[2], a["m"], a["v"], a["step"], float(np.float32(lr) * np.float32(0.3)), max_grad_norm=mx, **hyper)
        eng.adam_gated(b["p"], gs[2], b["m"], b["v"], b["step"], lr, gate, max_grad_norm=mx, lr_scale=scale, **hyper)
        _same(a, b, "lr_scale 0.3, %s" % mode)
    # against float64 once, through the restatement (ppo_ref's tolerance of pgd_adam)
    p0, g, mx = rf.build_adam(n_elem, "above")
    st = _adam_state(p0, n_elem)
    gate = torch.zeros(4, dtype=torch.int32, device="cuda")
    eng.adam_gated(st["p"], _dev(g[0]), st["m"], st["v"], st["step"], gate=gate, max_grad_norm=mx, lr_scale=_dev(np.array([0.5], dtype=np.float32)),
                   **rf.ADAM_HYPER)
    eng.sync()
    zero = np.zeros_like(p0)
    p64, _, _, t, g64, _ = mr.adam_gated_f64(p0, g[0], zero, zero, 0, rf.ADAM_HYPER["lr"], (0, 0, 0, 0), lr_scale=0.5, max_grad_norm=mx,
                                            betas=rf.ADAM_HYPER["betas"], eps=rf.ADAM_HYPER["eps"])
    err = rf.normalised_error(st["p"].cpu().numpy(), p64, np.abs(p0.astype(np.float64)) + np.abs(p64 - p0))
    assert err < rf.TOL_ADAM and t == 1 and g64 == gate.tolist(), (err, gate.tolist())


def test_adam_gated_refusals(eng):
    import torch
    st = _adam_state(np.ones(8, dtype=np.float32), 8)
    g = torch.ones(8, device="cuda")
    gate = torch.zeros(5, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    eng._follow_stream()
    p = lambda x: C.c_void_p(x.data_ptr())   # noqa: E731

    def call(h=eng.h, gate_ptr=p(gate), n=8, b1=0.9, step_ptr=p(st["step"])):
        return eng.L.pgd_adam_gated(h, p(st["p"]), p(g), p(st["m"]), p(st["v"]), n, step_ptr, 3e-4, b1, 0.999, 1e-5, 0.5, None, None, 0.0, gate_ptr, None)

    assert call(h=None) == ERR_ARG and call(gate_ptr=None) == ERR_ARG and call(n=0) == ERR_ARG and call(b1=1.0) == ERR_ARG
    assert call(step_ptr=None) == ERR_ARG and call(gate_ptr=C.c_void_p(gate.data_ptr() + 2)) == ERR_ARG
    eng.sync()
    assert int(st["step"][0]) == 0 and gate.tolist() == [0] * 5 and bool((st["p"] == 1).all()), "a refused call wrote"
    with pytest.raises(AssertionError):
        eng.adam_gated(st["p"], g, st["m"], st["v"], st["step"], 3e-4, gate[:3])


# ---------------------------------------------------------------------------------------------------------------------
# the learners
# ---------------------------------------------------------------------------------------------------------------------
CL_N, CL_T, CL_SEED = 16, 8, 3
CL_ROWS = CL_N * CL_T
CL_KW = dict(lr=3e-4, epochs=2, minibatches=4)
SHUF_SEED = 9
# the stopping case, chosen on the device.  These random networks move far: at lr 3e-4 the estimator mean(logp_old - logp) of the rollout
# below reads 9.7e-8, 3.78, 17.6, 24.1, 32.0, 36.2, 44.9, 46.1 before the eight steps (at 3e-3: 366 before the second), so the learning
# rate needs no raising; 1.5 * STOP_KL = 28.5 lies between the fourth and the fifth: four steps are applied, the stop falls on the first
# minibatch of the second epoch
STOP_LR, STOP_KL = 3e-4, 19.0


def _Single(descs):
    S = Traffic(descs, CL_N, CL_T, CL_SEED)
    S.col = make_collector("single", S)
    return S


def _equal_states(a, b, what):
    assert set(a) == set(b)
    assert_same(a, b, what, need=EVERY_LEARNER)


def test_switches_off_and_a_shuffled_update_by_hand(descs):
    """One engine, one rollout per iteration, several learners over it (each owns its parameters; update() leaves the batch alone).
    (a) every switch off: today's calls, and none of the switches' tensors exist.  (b) shuffle=True over two iterations against
    shuffle_index + ppo_grad + adam made by hand; `shuffled` is the restatement's permutation of the last epoch, with the epochs of the
    earlier iteration counted on the device.  (c) state_dict() / load_state_dict()."""
    import torch
    from pgdrive_amd.learner import PPOLearner
    S = _Single(descs)
    eng = S.eng
    try:
        off, off_hand = PPOLearner(S.col, shuffle=False, shuffle_seed=0, target_kl=None, lr_scale=False, **CL_KW), PPOLearner(S.col, **CL_KW)
        hand = PPOLearner(S.col, **CL_KW)   # (its buffers only)
        LS = PPOLearner(S.col, shuffle=True, shuffle_seed=SHUF_SEED, **CL_KW)
        assert all(getattr(off, q) is None for q in ("shuffled", "live_count", "gate", "_epoch", "lr_scale"))
        assert LS.gate is None and LS.lr_scale is None and LS.shuffled.shape == (CL_ROWS, )
        shuffled = torch.full((CL_ROWS, ), ISENT, dtype=torch.int32, device="cuda")
        live, epoch = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s), torch.no_grad():
            for it in range(2):
                batch = S.col.collect()
                if it == 0:
                    off.update(batch)
                    update_by_hand(eng, off_hand, batch, **CL_KW)
                    _equal_states(learner_state(off), learner_state(off_hand), "switches off")
                stats = LS.update(batch)
                got = learner_state(LS)
                update_by_hand(eng, hand, batch, shuffle=dict(seed=SHUF_SEED, shuffled=shuffled, live=live, epoch=epoch), **CL_KW)
                want = learner_state(hand)
                want.update(shuffled=shuffled.clone(), live_count=live.clone(), _epoch=epoch.clone())
                _equal_states(got, want, "iteration %d, shuffle=True" % it)
                st = stats.cpu().numpy()
                assert np.isfinite(st).all() and (st[:, 0] == CL_ROWS // 4).all() and int(LS.step[0]) == 8 * (it + 1)
                assert (LS.shuffled.cpu().numpy() == mr.permutation(CL_ROWS, SHUF_SEED, 1, epoch_dev=2 * it)).all()
                assert int(LS._epoch[0]) == 2 * (it + 1)
            assert not torch.equal(LS.params, off.params)
            # (c) a checkpoint: into a fresh learner of the same switches; a learner without the epoch counter refuses it
            sd = LS.state_dict()
            assert set(sd) == {"params", "m", "v", "step", "_epoch", "lr_scale"} and sd["lr_scale"] is None and int(sd["_epoch"][0]) == 4
            L2 = PPOLearner(S.col, shuffle=True, shuffle_seed=SHUF_SEED, **CL_KW)
            ptr = L2.params.data_ptr()
            L2.load_state_dict(sd)
            torch.cuda.synchronize()
            assert L2.params.data_ptr() == ptr and all(torch.equal(getattr(L2, q), getattr(LS, q)) for q in ("params", "m", "v", "step", "_epoch"))
            batch = S.col.collect()
            LS.update(batch)
            L2.update(batch)
            _equal_states(learner_state(LS), learner_state(L2), "after load_state_dict")
            with pytest.raises(ValueError, match="_epoch"):
                off.load_state_dict(sd)
            L3 = PPOLearner(S.col, lr_scale=True, **CL_KW)
            assert L3.lr_scale.tolist() == [1.0] and L3.gate is not None and L3.live_count is None and L3.state_dict()["lr_scale"].tolist() == [1.0]
    finally:
        eng.close()


def test_collect_and_update_from_one_graph_draws_new_permutations(descs):
    """shuffle, target_kl (never reached) and lr_scale on: one eager iteration, then `collect(); update()` captured once and replayed
    twice, against an eager twin's three iterations bit for bit; lr_scale is written between the replays as between the twin's
    iterations.  The replays' permutations are those of the epochs 2, 3 and 4, 5: different ones."""
    import torch
    from pgdrive_amd.learner import PPOLearner
    kw = dict(shuffle=True, shuffle_seed=SHUF_SEED, target_kl=1e6, lr_scale=True, **CL_KW)
    scales = (1.0, 0.75, 0.5)
    A, G = _Single(descs), _Single(descs)
    try:
        LA, LG = PPOLearner(A.col, **kw), PPOLearner(G.col, **kw)
        want = []
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s), torch.no_grad():
            for it in range(3):
                LA.lr_scale.fill_(scales[it])
                LA.update(A.col.collect())
                want.append(learner_state(LA))
                assert LA.gate.tolist() == [0, 8, 0, 0] and int(LA.live_count[0]) == CL_ROWS
                assert (LA.shuffled.cpu().numpy() == mr.permutation(CL_ROWS, SHUF_SEED, 2 * it + 1)).all()
            assert not torch.equal(want[1]["shuffled"], want[2]["shuffled"])
            LG.update(G.col.collect())
            _equal_states(learner_state(LG), want[0], "the eager iteration of the graph's engine")
            graph = torch.cuda.CUDAGraph()   # (its own capture: the host writes lr_scale between the replays)
        with torch.no_grad(), torch.cuda.graph(graph, stream=s):
            LG.update(G.col.collect())
        torch.cuda.synchronize()
        with torch.cuda.stream(s), torch.no_grad():
            for it in (1, 2):
                LG.lr_scale.fill_(scales[it])
                graph.replay()
                _equal_states(learner_state(LG), want[it], "graph replay %d" % it)
        del graph
    finally:
        A.eng.close()
        G.eng.close()


def test_an_update_that_stops_inside(descs):
    """lr = STOP_LR, target_kl = STOP_KL, the list as it lies (shuffle off): the device stops the update where stats[k, 4] first exceeds
    1.5 * STOP_KL.  On the MI355X: gate (1, 4, 4, 1), the figures beside STOP_LR."""
    import torch
    from pgdrive_amd.learner import PPOLearner
    S = _Single(descs)
    eng = S.eng
    try:
        twin = PPOLearner(S.col, **dict(CL_KW, lr=STOP_LR))
        L = PPOLearner(S.col, target_kl=STOP_KL, **dict(CL_KW, lr=STOP_LR))
        assert L.kl_limit == 1.5 * STOP_KL and L.shuffled is None and L.live_count is not None
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s), torch.no_grad():
            batch = S.col.collect()
            st = L.update(batch).cpu().numpy()
            gate = L.gate.tolist()
            print("stopping case: lr %g, target_kl %g: gate %s, n %s, kl %s" % (STOP_LR, STOP_KL, gate, st[:, 0].tolist(), st[:, 4].tolist()))
            total = CL_KW["epochs"] * CL_KW["minibatches"]
            applied, skipped = gate[1], gate[2]
            assert gate[0] == 1 and gate[3] == 1
            assert 1 <= applied < total
            assert applied + skipped == total
            assert (st[:applied, 4] <= np.float32(1.5 * STOP_KL)).all() and st[applied, 4] > np.float32(1.5 * STOP_KL)
            assert (st[:applied + 1, 0] == CL_ROWS // 4).all(), "the minibatches up to the stop are whole"
            assert (st[applied + 1:, 0] == 0).all() and (st[applied + 1:] == 0).all(), "rows behind the stop are not empty"
            assert int(L.live_count[0]) == 0 and int(L.step[0]) == applied
            assert bool((L.grads == 0).all()) or applied + 1 == total, "a gradient call behind the stop found live rows"
            update_by_hand(eng, twin, batch, n_steps=applied, **dict(CL_KW, lr=STOP_LR))
            torch.cuda.synchronize()
            for q in ("params", "m", "v", "step"):
                assert torch.equal(getattr(L, q).view(torch.int32), getattr(twin, q).view(torch.int32)), "%s: not the %d steps made by hand" % (q, applied)
            # the next update opens the gate and restores the count.  (Its carry row was evaluated with the weights of four steps ago, so
            # its very first minibatch may read a KL above the limit and stop: steps applied + skipped are counted from zero either way.)
            L.update(S.col.collect())
            torch.cuda.synchronize()
            assert int(L.gate[1]) + int(L.gate[2]) == total and float(L.stats[0, 0]) == CL_ROWS // 4 and int(L.step[0]) == applied + int(L.gate[1])
    finally:
        eng.close()


def test_ppo_lag_learner_with_both_switches():
    """SafeRolloutCollector, 16 envs, T = 8: PPOLagLearner(shuffle=True, target_kl=...) against lagrange, adv_stats, adv_mix, then
    shuffle_index + ppo_grad_cost + adam_gated made by hand."""
    import torch
    from pgdrive_amd import PPOLagLearner, SafeRolloutCollector
    from pgdrive_amd.vec_env import PGDriveVecEnv
    N, T, kl = 16, 8, 6.0   # (on the MI355X the estimator reads 5e-8, 3.65, 4.14, 13.9 before the first four steps: the fourth is refused)
    env = PGDriveVecEnv(dict(num_envs=N, start_seed=1000, environment_num=N, accident_prob=1.0, traffic_density=0.05, safe_rl_env=True, horizon=20))
    try:
        env.reset(force_seed=np.arange(1000, 1000 + N))
        eng = env.engine
        p, v = ar.make_networks(np.random.default_rng(0), eng.D, 4)
        _, cw = ar.make_networks(np.random.default_rng(1), eng.D, 4)
        p[4][:, 0] *= 0.05
        p[5][1] = 0.5
        pw, vw, cw = [tuple(_dev(w) for w in net) for net in (p, v, cw)]
        col = SafeRolloutCollector(env, pw, vw, cw, T, seed=3)
        kw = dict(cost_limit=-1.0, lambda_lr=0.05, lr=3e-4, epochs=2, minibatches=4)
        LB = PPOLagLearner(col, **kw)
        LA = PPOLagLearner(col, shuffle=True, shuffle_seed=SHUF_SEED, target_kl=kl, **kw)
        n_list = N * T
        shuffled = torch.full((n_list, ), ISENT, dtype=torch.int32, device="cuda")
        live, epoch, gate = [torch.zeros(n, dtype=torch.int32, device="cuda") for n in (1, 1, 4)]
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s), torch.no_grad():
            batch = col.collect()
            stats = LA.update(batch)
            update_by_hand(eng, LB, batch, 2, 4, lagrange=dict(cost_limit=-1.0, lambda_lr=0.05), gate=gate, kl_limit=1.5 * kl,
                           shuffle=dict(seed=SHUF_SEED, shuffled=shuffled, live=live, epoch=epoch))
            torch.cuda.synchronize()
            for q in ("params", "m", "v", "step", "stats", "grads", "lagrange_state", "mixed"):
                assert torch.equal(getattr(LA, q), getattr(LB, q)), "%s differs from the calls made by hand" % q
            assert torch.equal(LA.gate, gate) and torch.equal(LA.live_count, live) and int(LA._epoch[0]) == 2
            g, st = gate.tolist(), stats.cpu().numpy()
            print("PPOLagLearner, both switches: gate %s, n %s, kl %s" % (g, st[:, 0].tolist(), st[:, 4].tolist()))
            assert g[1] + g[2] == 8 and g[1] >= 1 and int(LA.step[0]) == g[1]
            if g[0]:
                assert (st[g[1] + 1:, 0] == 0).all()
            # a stop in epoch 0 (step g[1] < 4) zeroes the count, and epoch 1 writes no permutation
            assert (LA.shuffled.cpu().numpy() == mr.permutation(n_list, SHUF_SEED, 0 if g[0] and g[1] < 4 else 1)).all()
    finally:
        env.close()


def test_multi_agent_shuffled_minibatches_recomputed_on_the_host():
    """Roundabout, 2 envs, T = 8, one epoch of two minibatches, shuffle=True: `shuffled` is the restatement's permutation of the listed
    transitions (recomputed from the mask), each minibatch's statistics row counts the entries the host finds in it, and the update equals
    the launches made by hand over the HOST's shuffled list."""
    import torch
    from pgdrive_amd import learner as lm
    from pgdrive_amd.engine import Engine
    from pgdrive_amd.learner import PPOLearner
    from pgdrive_amd.rollout import MultiAgentRolloutCollector
    from tests import util
    N, T, A = 2, 8, 5
    _, mb, sb = util.make_marl_banks(num_agents=A)
    eng = Engine(util.marl_config(N, sb, horizon=40, seed=5), mb, sb)
    try:
        eng.reset(np.arange(N) % len(sb.scenarios))
        p, v = ar.make_networks(np.random.default_rng(0), eng.D, 4)
        p[5][1] = 0.5
        p[5][2:4] += 1.0
        col = MultiAgentRolloutCollector(eng, tuple(_dev(w) for w in p), tuple(_dev(w) for w in v), T, seed=CL_SEED)
        L = PPOLearner(col, lr=3e-4, epochs=1, minibatches=2, ent_coef=0.01, shuffle=True, shuffle_seed=SHUF_SEED)
        L.shuffled.fill_(ISENT)
        batch = col.collect()
        torch.cuda.synchronize()
        layout, total = lm.flat_layout(eng.D, 4)
        flat = {q: torch.zeros(total, device="cuda") for q in ("p", "g", "m", "v")}
        flat["p"].copy_(L.params)
        views = {q: [flat[q][o:o + int(np.prod(sh))].view(sh) for _, sh, o in layout] for q in ("p", "g")}
        step = torch.zeros(4, dtype=torch.int32, device="cuda")
        stats_update = L.update(batch).clone()
        torch.cuda.synchronize()
        listed = np.flatnonzero(batch["mask"].cpu().numpy().reshape(-1) != 0)
        count = int(batch["count"][0])
        assert count == len(listed) and 4 <= count <= L.n_list and int(L.live_count[0]) == count
        host = np.full(L.n_list, ISENT, dtype=np.int32)
        host[:count] = listed[mr.permutation(count, SHUF_SEED, 0)]
        assert (L.shuffled.cpu().numpy() == host).all(), "`shuffled` is not the permutation of the listed transitions"
        assert not np.array_equal(host[:count], listed)
        hidx = _dev(host)
        seen = []
        for j in range(2):
            sel = host[:count][j::2]
            seen.append(sel)
            st = torch.zeros(8, device="cuda")
            eng.ppo_grad(views["p"][:6], views["p"][6:], views["g"][:6], views["g"][6:], batch["obs"], batch["actions"], batch["logp"],
                         batch["advantages"], batch["returns"], st, L.work, start=j, stride=2, rows=L.plan[j][2], index=hidx,
                         count=batch["count"], n_list=L.n_list, adv_stats=L.adv_stats, ent_coef=0.01)
            eng.sync()
            assert float(st[0]) == len(sel) and torch.equal(st, stats_update[j]), "minibatch %d: update() saw other rows" % j
            eng.adam(flat["p"], flat["g"], flat["m"], flat["v"], step, 3e-4, eps=1e-5, max_grad_norm=0.5)
        eng.sync()
        assert np.array_equal(np.sort(np.concatenate(seen)), listed)
        assert torch.equal(flat["p"], L.params) and torch.equal(flat["g"], L.grads) and torch.equal(flat["m"], L.m) and torch.equal(step, L.step), \
            "update() is not the launches made by hand"
    finally:
        eng.close()
