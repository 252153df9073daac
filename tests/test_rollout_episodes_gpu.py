"""pgd_rollout_episodes (pgdrive_amd/csrc/pgd_rollout_episodes.h) and the collectors' episode_stats switch on the device, against the
checker tests/rollout_episodes_ref.py (by definition: every row cut into episodes, float32 returns by sequential adds, numpy statistics):

* exact inputs (integer rewards) at T in {1, 2, 16} x rows in {1, 63, 64, 65, 257, 1000} and 1 x 16449 (258 partials: a second pass of the
  merge's threads), dones at rate 0.2, everywhere and nowhere; general inputs (normal rewards, 33 x 257); seats that change hands with NaN
  wherever nobody acted: the carries and the dense outputs bit for bit, every integer slot of both records with ==, return_min /
  return_max bit for bit, mean and m2 within 1e-12 (return_norm_ref's criterion);
* two calls of T against one of 2 T, a call in which nothing ends, each optional output left out, the refusals, the same bytes twice, the
  first call of a fresh engine from a HIP graph;
* the three collectors with the switch off and on, and the single-agent engine's step info as a second witness of the integer counts.
"""
import ctypes as C

import numpy as np
import pytest

from tests import rollout_episodes_ref as er
from tests import recording_engine as rc
from tests.train_util import ERR_ARG, SENT, Ego, bits_equal as _bits_equal, dev as _dev, eager_then_graph, ego_engine as _ego_engine, make, make_collector, \
    snapshot as _snapshot

pytestmark = pytest.mark.gpu

TAIL, ISENT = 8, -77
OUT = ("ret_carry", "len_carry", "record", "call", "ep_return", "ep_length")


@pytest.fixture(scope="module")
def eng(descs):
    """One env, ego only, no lidar: pgd_rollout_episodes needs the engine for its device and stream only."""
    e = _ego_engine(descs, 1)
    yield e
    e.close()


class _Buffers:
    """The tensors of one call: reward / done / flags and the carries from numpy (a case of the checker), `record` as given, `call`, the
    dense outputs and the scratch filled with NaN (ep_length: ISENT); every output carries a sentinel tail, the scratch one behind
    work_bytes."""
    def __init__(self, eng, case, record=er.INIT):
        import torch
        reward, done, flags, ret, length = case
        self.T, self.rows = reward.shape[0], int(np.prod(reward.shape[1:]))
        n, rows = self.T * self.rows, self.rows
        self.reward, self.done = _dev(np.asarray(reward, np.float32)), _dev(np.asarray(done, np.uint8))
        self.flags = _dev(np.asarray(flags).astype(np.int32))
        f32, i32, f64 = (dict(dtype=d, device="cuda") for d in (torch.float32, torch.int32, torch.float64))
        self._ret, self._len = torch.full((rows + TAIL, ), SENT, **f32), torch.full((rows + TAIL, ), ISENT, **i32)
        self.ret, self.len = self._ret[:rows], self._len[:rows]
        self.ret.copy_(_dev(np.asarray(ret, np.float32).reshape(-1)))
        self.len.copy_(_dev(np.asarray(length, np.int32).reshape(-1)))
        self._records = torch.full((32 + TAIL, ), float("nan"), **f64)
        self._records[32:] = SENT
        self.record, self.call_record = self._records[:16], self._records[16:32]
        self.record.copy_(_dev(np.asarray(record, np.float64)))
        self._epr, self._epl = torch.full((n + TAIL, ), float("nan"), **f32), torch.full((n + TAIL, ), ISENT, **i32)
        self._epr[n:] = SENT
        self.ep_return, self.ep_length = self._epr[:n].view(self.reward.shape), self._epl[:n].view(self.reward.shape)
        need = eng.rollout_episodes_work_bytes(rows) // 8
        assert need == 16 * ((rows + 63) // 64)
        self._work = torch.full((need + TAIL, ), float("nan"), **f64)
        self._work[need:] = SENT
        self.work = self._work[:need]

    def tails_intact(self):
        n, rows = self.T * self.rows, self.rows
        return bool((self._ret[rows:] == SENT).all()) and bool((self._len[rows:] == ISENT).all()) and bool((self._records[32:] == SENT).all()) and \
            bool((self._epr[n:] == SENT).all()) and bool((self._epl[n:] == ISENT).all()) and bool((self._work[self.work.numel():] == SENT).all())

    def read(self):
        return dict(ret_carry=self.ret.cpu().numpy(), len_carry=self.len.cpu().numpy(), record=self.record.cpu().numpy(),
                    call=self.call_record.cpu().numpy(), ep_return=self.ep_return.cpu().numpy(), ep_length=self.ep_length.cpu().numpy())

    def call(self, eng, seats=False, record=True, call=True, ep_return=True, ep_length=True):
        eng.rollout_episodes(self.reward, self.done, self.flags, self.ret, self.len, record=self.record if record else None,
                             call=self.call_record if call else None, seats=seats, ep_return=self.ep_return if ep_return else None,
                             ep_length=self.ep_length if ep_length else None, work=self.work)
        eng.sync()
        assert self.tails_intact(), "written past the end"
        return self.read()


def _same(a, b, keys=OUT, where=None):
    for key in keys:
        assert np.array_equal(er.bits(a[key]), er.bits(b[key])), (where, key)


def _check(got, ref, record0, where):
    """A call's outputs against the checker's by_definition: carries and dense outputs bit for bit; both records by er.check_record."""
    shape = got["ep_return"].shape
    assert np.array_equal(er.bits(got["ret_carry"]), er.bits(ref["ret_carry"])), (where, "ret_carry")
    assert np.array_equal(got["len_carry"], ref["len_carry"]), (where, "len_carry")
    assert np.array_equal(er.bits(got["ep_return"]), er.bits(ref["ep_return"].reshape(shape))), (where, "ep_return")
    assert np.array_equal(got["ep_length"], ref["ep_length"].reshape(shape)), (where, "ep_length")
    err = er.check_record(got["call"], ref["call"], (where, "call"))
    return max(err, er.check_record(got["record"], er.merge_record(record0, ref["call"]), (where, "record")))


RECORD0 = np.array([3.0, 1.5, 0.25, -1.0, 4.0, 17.0, 9.0, 1.0, 2.0, 0.0, 0.0, 0.0, 1.0, 0.0, 40.0, 2.0])   # a record that holds something


# ---------------------------------------------------------------------------------------------------------------------
# the call against the checker
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,rows", er.EXACT_SHAPES)
def test_exact_inputs(eng, T, rows):
    worst = 0.0
    for dones in ("some", "all", "none"):
        case = er.exact_case(T, rows, dones)
        ref = er.by_definition(*case)
        for record0 in (er.INIT, RECORD0):
            worst = max(worst, _check(_Buffers(eng, case, record0).call(eng), ref, record0, (T, rows, dones)))
        assert ref["call"][0] == dict(some=ref["call"][0], all=T * rows, none=0)[dones]
    print("exact inputs, T = %d, rows = %d: records against the checker %.1e (bound %.0e)" % (T, rows, worst, er.TOL_STATS))


def test_general_inputs(eng):
    """Normal rewards: the samples are still bit-exact (a return is a chain of plain float32 adds in the order of t), so the dense outputs,
    the carries and min / max are compared bit for bit and the statistics with the checker's own samples."""
    case = er.general_case(33, 257)
    ref = er.by_definition(*case)
    assert ref["call"][0] > 257
    err = max(_check(_Buffers(eng, case, r0).call(eng), ref, r0, "general") for r0 in (er.INIT, RECORD0))
    print("general inputs: records against the checker %.1e (bound %.0e)" % (err, er.TOL_STATS))


@pytest.mark.parametrize("T,rows", [(16, 37), (33, 257), (2, 1000)])
def test_seats_that_change_hands(eng, T, rows):
    """Agents that start mid-rollout, end by done, are cut by PGD_F_RESET without a done and follow each other in a seat; every reward of
    an entry at which nobody acted is NaN, and so are the outputs in front of the call: all outputs are finite."""
    case = er.seat_case(T, rows)
    reward, done, flags = case[:3]
    acted, ends = er.predicates(done, flags, True)
    assert np.isnan(reward[~acted]).all() and np.isfinite(reward[acted]).all()
    combos = {(bool(f & er.F_REPORT), bool(f & er.F_NEW), bool(f & er.F_RESET), bool(d)) for f, d in zip(flags.reshape(-1).tolist(), done.reshape(-1).tolist())}
    if T * rows > 2000:
        assert len(combos) == 16, "not every combination of REPORT / NEW / RESET and done"
    ref = er.by_definition(*case, seats=True)
    assert ref["call"][13] > 0, "no agent cut by an env-wide restart"
    assert (ends.sum(axis=0) >= 2).any() or T < 3, "no seat with two episodes"
    assert (~acted[0]).any() and (acted[1:] & ~acted[:-1]).any(), "no agent starts mid-rollout"
    got = _Buffers(eng, case, RECORD0).call(eng, seats=True)
    for key in OUT:
        assert np.isfinite(got[key]).all(), key
    err = _check(got, ref, RECORD0, (T, rows))
    assert got["call"][14] == acted.sum() and got["call"][0] == ends.sum()
    print("seats, %d x %d: %d episodes, %d cut, records against the checker %.1e" % (T, rows, ref["call"][0], ref["call"][13], err))


def test_seats_mode_with_every_flag_report_is_mode_0(eng):
    for T, rows in ((1, 1), (16, 65), (33, 257)):
        reward, done, flags, ret, length = er.general_case(T, rows, p_done=0.2)
        flags = (flags | er.F_REPORT | np.where(np.random.default_rng(T).uniform(size=flags.shape) < 0.3, er.F_NEW, 0)).astype(np.int32)
        case = (reward, done, flags, ret, length)
        _same(_Buffers(eng, case).call(eng), _Buffers(eng, case).call(eng, seats=True), where=(T, rows))


# ---------------------------------------------------------------------------------------------------------------------
# carries and records
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seats", [False, True])
def test_two_calls_of_t_are_one_call_of_2t(eng, seats):
    T, rows = 16, 257
    reward, done, flags, ret, length = er.seat_case(2 * T, rows) if seats else er.general_case(2 * T, rows)
    whole = _Buffers(eng, (reward, done, flags, ret, length)).call(eng, seats=seats)
    first = _Buffers(eng, (reward[:T], done[:T], flags[:T], ret, length)).call(eng, seats=seats)
    second = _Buffers(eng, (reward[T:], done[T:], flags[T:], first["ret_carry"], first["len_carry"]), first["record"]).call(eng, seats=seats)
    _same(second, whole, ("ret_carry", "len_carry"))
    assert np.array_equal(er.bits(np.concatenate([first["ep_return"], second["ep_return"]])), er.bits(whole["ep_return"]))   # (the samples)
    assert np.array_equal(np.concatenate([first["ep_length"], second["ep_length"]]), whole["ep_length"])
    want = whole["record"].copy()
    want[15] = 2.0
    er.check_record(second["record"], want, "two calls")   # (the same samples merged in another order)
    assert first["call"][0] + second["call"][0] == whole["call"][0] > 0


def test_a_call_in_which_no_episode_ends(eng):
    case = er.exact_case(4, 70, "none")
    got = _Buffers(eng, case, RECORD0).call(eng)
    assert np.array_equal(er.bits(got["record"][:14]), er.bits(RECORD0[:14])), "slots 0 .. 13 moved"
    assert got["record"][14] == RECORD0[14] + 280 and got["record"][15] == RECORD0[15] + 1
    assert np.array_equal(er.bits(got["call"]), er.bits(np.concatenate([er.INIT[:14], [280.0, 1.0]])))
    assert not got["ep_return"].any() and not got["ep_length"].any()
    assert np.array_equal(got["len_carry"], case[4] + 4)
    # seats at which nobody ever acts: nothing moves but `calls`
    flags = (case[2] & ~er.F_REPORT) | er.F_RESET
    got = _Buffers(eng, (np.full((4, 70), np.nan, np.float32), case[1], flags, case[3], case[4]), RECORD0).call(eng, seats=True)
    assert np.array_equal(er.bits(got["record"][:15]), er.bits(RECORD0[:15])) and got["record"][15] == RECORD0[15] + 1
    assert np.array_equal(er.bits(got["ret_carry"]), er.bits(case[3])) and np.array_equal(got["len_carry"], case[4])


@pytest.mark.parametrize("seats", [False, True])
def test_every_optional_output_left_out(eng, seats):
    """d_record null, d_call null, each dense output null, all four: what is left out keeps its fill, what is named equals the full call,
    and nothing else is written (the sentinel tails of every buffer and of the scratch behind work_bytes, checked by _Buffers.call)."""
    case = er.seat_case(16, 257) if seats else er.general_case(16, 257)
    full = _Buffers(eng, case, RECORD0).call(eng, seats=seats)
    for left_out in (("record", ), ("call", ), ("ep_return", ), ("ep_length", ), ("ep_return", "ep_length"), ("record", "call", "ep_return", "ep_length")):
        b = _Buffers(eng, case, RECORD0)
        fill = b.read()
        got = b.call(eng, seats=seats, **{k: False for k in left_out})
        for key in OUT:
            _same(got, fill if key in left_out else full, (key, ), where=left_out)


def test_refused_arguments(eng):
    import torch
    case = er.general_case(4, 70)
    b = _Buffers(eng, case, RECORD0)
    fill = b.read()
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    good = dict(reward=p(b.reward), done=p(b.done), flags=p(b.flags), T=4, rows=70, mode=0, ret=p(b.ret), len=p(b.len), record=p(b.record),
                call=p(b.call_record), epr=p(b.ep_return), epl=p(b.ep_length), work=p(b.work), work_bytes=b.work.numel() * 8)
    order = ("reward", "done", "flags", "T", "rows", "mode", "ret", "len", "record", "call", "epr", "epl", "work", "work_bytes")

    def call(**kw):
        a = dict(good, **kw)
        return eng.L.pgd_rollout_episodes(eng.h, *[a[k] for k in order])

    assert eng.rollout_episodes_work_bytes(70) == 256 and eng.rollout_episodes_work_bytes(0) == 0
    bad = [dict(T=0), dict(T=-1), dict(rows=0), dict(rows=-3), dict(mode=2), dict(mode=3), dict(mode=1 << 31), dict(work_bytes=255), dict(work_bytes=0),
           dict(record=p(b.record, 4)), dict(call=p(b.call_record, 4)), dict(work=p(b.work, 4))]
    bad += [{k: None} for k in ("reward", "done", "flags", "ret", "len", "work")]
    for kw in bad:
        assert call(**kw) == ERR_ARG, kw
    assert eng.L.pgd_rollout_episodes(None, *[good[k] for k in order]) == ERR_ARG
    eng.sync()
    _same(b.read(), fill, where="a refused call launched")
    assert bool(torch.isnan(b.work).all()) and b.tails_intact()
    for kw in (dict(), dict(mode=1), dict(record=None), dict(call=None), dict(epr=None, epl=None)):
        assert call(**kw) == 0, kw
    eng.sync()
    assert bool(torch.isfinite(b.ep_return).all()) and b.tails_intact()


@pytest.mark.parametrize("seats", [False, True])
def test_identical_bytes_from_two_runs(eng, seats):
    case = er.seat_case(16, 1000) if seats else er.general_case(16, 1000)
    _same(_Buffers(eng, case, RECORD0).call(eng, seats=seats), _Buffers(eng, case, RECORD0).call(eng, seats=seats))


def test_the_first_call_of_a_fresh_engine_is_capturable(descs):
    """Nothing is allocated inside the call and the scratch is the caller's: the very first call on an engine is made inside a graph
    capture (which runs nothing).  Replay k continues from the carries and the record that replay k - 1 left: behind each of four replays
    every output holds the bytes of k eager calls on the same inputs."""
    import torch
    case = er.seat_case(33, 257)
    fresh = _ego_engine(descs, 1)
    try:
        G, E = _Buffers(fresh, case), _Buffers(fresh, case)
        fill = G.read()
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()   # (its own capture: the first call on a fresh engine is made inside the capture, nothing runs eagerly in front)
        with torch.cuda.graph(graph, stream=s):
            fresh.rollout_episodes(G.reward, G.done, G.flags, G.ret, G.len, record=G.record, call=G.call_record, seats=True, ep_return=G.ep_return,
                                   ep_length=G.ep_length, work=G.work)
        torch.cuda.synchronize()
        _same(G.read(), fill, where="the capture itself ran the kernels")
        for k in range(4):
            with torch.cuda.stream(s):
                graph.replay()
            torch.cuda.synchronize()
            want = E.call(fresh, seats=True)
            _same(G.read(), want, where="replay %d differs from %d eager calls" % (k + 1, k + 1))
            assert want["record"][15] == k + 1 and G.tails_intact()
        del graph
    finally:
        fresh.close()


# ---------------------------------------------------------------------------------------------------------------------
# the collectors
# ---------------------------------------------------------------------------------------------------------------------
KINDS = [("single", "RolloutCollector"), ("safe", "SafeRolloutCollector"), ("marl", "MultiAgentRolloutCollector")]
EP_KEYS = ("episode_stats", "episode_stats_rollout", "ep_returns", "ep_lengths")
TRAJECTORY = ("rewards", "dones", "flags")


@pytest.mark.parametrize("kind", [k for k, _ in KINDS], ids=[i for _, i in KINDS])
def test_collectors_switch_off(descs, kind, monkeypatch):
    """episode_stats=False: Engine.rollout_episodes is never called and the batch has exactly the keys it has today."""
    import torch
    from pgdrive_amd.engine import Engine

    def refuse(*a, **kw):
        raise AssertionError("Engine.rollout_episodes called with the switch off")

    monkeypatch.setattr(Engine, "rollout_episodes", refuse)
    S, col, _ = make(kind, descs, learn=False, episode_stats=False)
    try:
        with torch.no_grad():
            batch = col.collect()
            batch = col.collect()
        torch.cuda.synchronize()
        assert set(batch) == dict(single=rc.TODAY, safe=rc.TODAY_SAFE, marl=rc.TODAY_MARL)[kind]
        assert col.state_dict() == {} and not any(hasattr(col, a) for a in ("ep_returns", "ep_lengths", "episode_record"))
    finally:
        S.eng.close()


def _episode_state(col):
    return dict(_snapshot(col.batch, EP_KEYS + TRAJECTORY), ret_carry=col._ep_ret_carry.clone(), len_carry=col._ep_len_carry.clone())


@pytest.mark.parametrize("kind", [k for k, _ in KINDS], ids=[i for _, i in KINDS])
def test_collectors_switch_on(descs, kind):
    """Over three rollouts the host recomputes everything from the batches' own rewards / dones / flags with the checker: the integer
    slots exactly, the samples (ep_returns, min, max, the carries) bit for bit, mean and m2 within 1e-12, ep_lengths exactly.  collect()
    captured in a HIP graph behind one eager rollout and replayed twice equals the eager rollouts bit for bit; clear_episode_stats() keeps
    the carries; state_dict() round-trips; normalise_rewards=True changes no episode statistic."""
    import torch
    marl = kind == "marl"
    # (a) eagerly
    A, col, _ = make(kind, descs, learn=False, episode_stats=True)
    rows = col.rewards[0].numel()
    ret, length, record = np.zeros(rows, np.float32), np.zeros(rows, np.int32), er.INIT
    want = []
    with torch.no_grad():
        for it in range(3):
            batch = col.collect()
            torch.cuda.synchronize()
            assert batch["episode_stats"].dtype == torch.float64 and batch["ep_lengths"].dtype == torch.int32
            assert batch["ep_returns"].shape == batch["rewards"].shape == batch["ep_lengths"].shape
            rew, dn, fl = [batch[k].cpu().numpy() for k in TRAJECTORY]
            ref = er.by_definition(rew, dn, fl, ret, length, seats=marl)
            got = dict(ret_carry=col._ep_ret_carry.cpu().numpy(), len_carry=col._ep_len_carry.cpu().numpy(), record=batch["episode_stats"].cpu().numpy(),
                       call=batch["episode_stats_rollout"].cpu().numpy(), ep_return=batch["ep_returns"].cpu().numpy(),
                       ep_length=batch["ep_lengths"].cpu().numpy())
            err = _check(got, ref, record, (kind, it))
            ret, length, record = ref["ret_carry"], ref["len_carry"], er.merge_record(record, ref["call"])
            print("%s, rollout %d: %d episodes ended, %d steps, records against the checker %.1e" % (kind, it, ref["call"][0], ref["steps"], err))
            want.append(_episode_state(col))
    assert record[0] > 0, "no episode ended in three rollouts"
    summary = col.episode_summary()
    assert summary["episodes"] == record[0] and summary["steps"] == record[14] and abs(summary["mean_return"] - record[1]) <= 1e-12 * max(1.0, abs(record[1]))
    assert summary["mean_length"] == record[5] / record[0] and all(0.0 <= summary[k] <= 1.0 for k in summary if k.endswith("_rate"))
    assert col.episode_summary(rollout=True)["episodes"] == ref["call"][0]
    A.eng.close()

    # (b) one collect() captured behind one eager rollout, replayed twice
    G, col, _ = make(kind, descs, learn=False, episode_stats=True)
    eager_then_graph(col.collect, lambda: _episode_state(col), want)
    # a checkpoint of what the replays left; clearing keeps the carries
    state = col.state_dict()
    assert set(state) == {"episode_return_carry", "episode_length_carry", "episode_stats"}
    assert np.array_equal(er.bits(state["episode_stats"]), er.bits(want[2]["episode_stats"].cpu().numpy()))
    assert np.array_equal(er.bits(state["episode_return_carry"]), er.bits(want[2]["ret_carry"].cpu().numpy()))
    assert np.array_equal(state["episode_length_carry"], want[2]["len_carry"].cpu().numpy())
    col.clear_episode_stats()
    cleared = col.state_dict()
    assert np.array_equal(er.bits(cleared["episode_stats"]), er.bits(er.INIT))
    assert np.array_equal(er.bits(cleared["episode_return_carry"]), er.bits(state["episode_return_carry"]))
    assert np.array_equal(cleared["episode_length_carry"], state["episode_length_carry"])
    none = col.episode_summary()
    assert none["episodes"] == 0 and none["mean_return"] is None and none["arrive_rate"] is None
    col._ep_ret_carry.zero_()
    col._ep_len_carry.zero_()
    col.load_state_dict(state)
    back = col.state_dict()
    for key in state:
        assert np.array_equal(er.bits(back[key]), er.bits(state[key])), key
    G.eng.close()

    # (c) with reward normalisation: GAE reads scaled rewards, the episode statistics read the raw ones
    N, col, _ = make(kind, descs, learn=False, episode_stats=True, normalise_rewards=True)
    with torch.no_grad():
        for it in range(3):
            batch = col.collect()
            got = _episode_state(col)
            assert "scaled_rewards" in batch and not _bits_equal(batch["scaled_rewards"], batch["rewards"])
            for key in got:
                assert _bits_equal(got[key], want[it][key]), "normalise_rewards changed %s in rollout %d" % (key, it)
    N.eng.close()


def test_the_step_info_counts_the_same_episodes(descs):
    """The single-agent engine with step info: the episode count, the length sum and the arrive / out-of-road / max-step counts of
    Engine.episode_stats(clear=False) equal the record's, exactly, over the same steps.  Only these integer quantities are compared: the
    step info sums the returns in another order (the float64 checker holds the returns, above)."""
    import torch
    S = Ego(descs, False)
    try:
        S.eng.enable_step_info()
        col = make_collector("single", S, episode_stats=True)
        with torch.no_grad():
            for it in range(3):
                col.collect()
        torch.cuda.synchronize()
        info = S.eng.episode_stats(clear=False)
        rec = dict(zip(er.FIELDS, col.episode_record.cpu().numpy()))
        n = int(rec["episodes"])
        assert n == info["episodes"] > 0
        assert info["mean_length"] == rec["length_sum"] / n and info["arrive_rate"] == rec["arrive"] / n
        assert info["out_of_road_rate"] == rec["out_of_road"] / n and info["max_step_rate"] == rec["max_step"] / n
        si = S.eng.step_info
        for key, field in (("ep_count", "episodes"), ("ep_length_sum", "length_sum"), ("ep_arrive", "arrive"), ("ep_out_of_road", "out_of_road"),
                           ("ep_max_step", "max_step")):
            assert float(si[key].sum(dtype=torch.float64)) == rec[field], (key, field)
        assert rec["steps"] == 3 * S.T * S.N and rec["cut"] == 0
    finally:
        S.eng.close()
