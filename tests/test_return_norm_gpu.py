"""pgd_return_norm (pgdrive_amd/csrc/pgd_return_norm.h) and the collectors' normalise_rewards switch on the device, against the float64
checker tests/return_norm_ref.py:

* exact inputs (gamma = 0.5, integer rewards: every running return is exact in float32, tests/test_return_norm_cpu.py holds that): the
  carry bit for bit, the record's count exactly, mean and m2 within 1e-12, the scaled rewards within 1 ulp, at T in {1, 2, 16} x rows in
  {1, 63, 64, 65, 257, 1000} x dones at rate 0.2, everywhere and nowhere;
* general inputs (gamma = 0.99, normal rewards, 33 x 257): the carry within the rounding bound of an fma chain, the statistics against the
  checker run on the DEVICE'S OWN samples, reconstructed by T = 1 calls;
* two calls of T against one of 2 T, the flag form with every flag PGD_F_REPORT against the plain form, NaN wherever one may stand, the
  frozen mode, a call without a sample, the refusals, the same bytes twice, the first call of a fresh engine from a HIP graph;
* the three collectors with the switch on and off.
"""
import ctypes as C

import numpy as np
import pytest

from tests import return_norm_ref as rn
from tests.train_util import ERR_ARG, EVERY_LEARNER, KEYS, SENT, Ego, Roundabout, bits_equal as _bits_equal, dev as _dev, eager_then_graph, ego_engine as _ego_engine, \
    hand_gae, learner_state, make, np_bits as _bits, snapshot as _snapshot, synchronised_rollouts

pytestmark = pytest.mark.gpu

TAIL = 8


@pytest.fixture(scope="module")
def eng(descs):
    """One env, ego only, no lidar: pgd_return_norm needs the engine for its device and stream only."""
    e = _ego_engine(descs, 1)
    yield e
    e.close()


class _Buffers:
    """The tensors of one call: reward / done / flags from numpy, carry and record as given, `scaled` and the scratch filled with NaN;
    carry and scaled carry a sentinel tail.  misalign: `scaled` starts 4 bytes behind a 16-byte boundary, with a sentinel in front (the
    arrays are only asked to be 4-byte aligned)."""
    def __init__(self, eng, reward, done, carry, record, flags=None, misalign=False):
        import torch
        self.T, self.rows = reward.shape[0], int(np.prod(reward.shape[1:]))
        self.reward, self.done = _dev(np.asarray(reward, np.float32)), _dev(np.asarray(done, np.uint8))
        self.flags = None if flags is None else _dev(np.asarray(flags).astype(np.int32))
        self._carry = torch.full((self.rows + TAIL, ), SENT, dtype=torch.float32, device="cuda")
        self.carry = self._carry[:self.rows]
        self.carry.copy_(_dev(np.asarray(carry, np.float32).reshape(-1)))
        self.record = _dev(np.asarray(record, np.float64))
        lo = 1 if misalign else 0
        self._scaled = torch.full((lo + self.T * self.rows + TAIL, ), float("nan"), dtype=torch.float32, device="cuda")
        self._scaled[:lo] = SENT
        self._scaled[lo + self.T * self.rows:] = SENT
        self.scaled = self._scaled[lo:lo + self.T * self.rows].view(self.reward.shape)
        assert self.scaled.data_ptr() % 16 == 4 * lo
        self._ends = (lo, lo + self.T * self.rows)
        self.work = torch.full(((eng.return_norm_work_bytes(self.rows) + 7) // 8, ), float("nan"), dtype=torch.float64, device="cuda")

    def call(self, eng, gamma, **kw):
        eng.return_norm(self.reward, self.done, gamma, self.carry, self.record, flags=self.flags, out=self.scaled, work=self.work, **kw)
        eng.sync()
        lo, hi = self._ends
        assert bool((self._carry[self.rows:] == SENT).all()) and bool((self._scaled[:lo] == SENT).all()) and bool((self._scaled[hi:] == SENT).all()), \
            "written past the end"
        return dict(carry=self.carry.cpu().numpy(), record=self.record.cpu().numpy(), scaled=self.scaled.cpu().numpy())


def _check_record(got, want, where, same_merges=True):
    """count exactly; mean within 1e-12 of sqrt(m2 / count); m2 and the scale within 1e-12, relative.  same_merges False: `want` went
    through other calls than `got` ((1e-4 + n) + n is not the double 1e-4 + 2 n): the count within two roundings of a double."""
    assert got[0] == want[0] or (not same_merges and abs(got[0] - want[0]) <= 2.0 * np.spacing(want[0])), (where, "count", got[0], want[0])
    sd = np.sqrt(want[2] / want[0])
    err = max(abs(got[1] - want[1]) / sd, abs(got[2] - want[2]) / want[2], abs(got[3] - want[3]) / want[3])
    assert err < rn.TOL_STATS, (where, err, got, want)
    return err


def _check_scaled(got, want, where):
    """Within 1 ulp of float32: the scale may round the other way once."""
    assert np.isfinite(got).all(), where
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    ok = d <= np.spacing(np.maximum(np.abs(got), np.abs(want)))
    assert ok.all(), (where, int((~ok).sum()), float(d.max()))


# ---------------------------------------------------------------------------------------------------------------------
# exact inputs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", rn.EXACT_ROWS)
@pytest.mark.parametrize("T", rn.EXACT_T)
def test_exact_inputs(eng, T, rows):
    worst = 0.0
    for dones in ("some", "all", "none"):
        reward, done = rn.exact_case(T, rows, dones)
        carry = np.random.default_rng(rows).integers(-4, 5, size=rows).astype(np.float32)
        for clip in (10.0, 0.0):
            got = _Buffers(eng, reward, done, carry, rn.RECORD_INIT, misalign=clip == 0.0).call(eng, rn.EXACT_GAMMA, eps=1e-8, clip=clip)
            want = rn.return_norm_f64(reward, done, rn.EXACT_GAMMA, carry, rn.RECORD_INIT, eps=1e-8, clip=clip)
            where = (T, rows, dones, clip)
            assert np.array_equal(_bits(got["carry"]), _bits(want["carry"].astype(np.float32))), (where, "carry")
            assert got["record"][0] == 1e-4 + T * rows
            worst = max(worst, _check_record(got["record"], want["record"], where))
            _check_scaled(got["scaled"], want["scaled"], where)
            if clip > 0:
                assert np.abs(got["scaled"]).max() <= clip
    print("exact inputs, T = %d, rows = %d: record against the checker %.1e (bound %.0e)" % (T, rows, worst, rn.TOL_STATS))


# ---------------------------------------------------------------------------------------------------------------------
# general inputs
# ---------------------------------------------------------------------------------------------------------------------
GEN_T, GEN_ROWS, GEN_GAMMA = 33, 257, 0.99


def _general(seed=0):
    rng = np.random.default_rng(seed)
    reward = rng.normal(size=(GEN_T, GEN_ROWS)).astype(np.float32)
    done = (rng.uniform(size=(GEN_T, GEN_ROWS)) < 0.1).astype(np.uint8)
    return reward, done


def test_general_inputs(eng):
    """The carry against the float64 recursion within 2^-24 max|R| / (1 - gamma), the accumulated rounding of an fma chain with ratio
    gamma.  The statistics against the checker run on the device's own samples: RECONSTRUCTED by running the call with T = 1, step
    after step, on a carry of its own -- the carry behind step t is the sample where the row is not done, and one float32 fma of the
    carry in front of the step where it is (the other option, a tolerance implied by the sample bound, was not taken)."""
    reward, done = _general()
    zeros = np.zeros(GEN_ROWS, np.float32)
    got = _Buffers(eng, reward, done, zeros, rn.RECORD_INIT).call(eng, GEN_GAMMA)
    g32 = float(np.float32(GEN_GAMMA))
    want = rn.return_norm_f64(reward, done, g32, zeros, rn.RECORD_INIT)
    R64, _, _ = rn.running_returns(reward, done, g32, zeros)
    bound = 2.0 ** -24 * np.abs(R64).max() / (1.0 - g32)
    err = np.abs(got["carry"] - want["carry"]).max()
    print("general inputs: |carry - f64| %.2e (bound %.2e)" % (err, bound))
    assert err <= bound
    # the device's samples, one step per call
    samples = np.zeros((GEN_T, GEN_ROWS), np.float32)
    c = zeros
    for t in range(GEN_T):
        one = _Buffers(eng, reward[t:t + 1], done[t:t + 1], c, rn.RECORD_INIT).call(eng, GEN_GAMMA)
        samples[t] = np.where(done[t] != 0, rn.fma32(np.float32(GEN_GAMMA), c, reward[t]), one["carry"])
        c = one["carry"]
    assert np.array_equal(_bits(c), _bits(got["carry"])), "T calls of one step do not end in the carry of one call of T steps"
    assert np.abs(samples - R64).max() <= bound
    on_device = rn.return_norm_f64(reward, done, g32, zeros, rn.RECORD_INIT, samples=samples)
    err = _check_record(got["record"], on_device["record"], "general")
    print("general inputs: record against the checker on the device's samples %.1e (bound %.0e)" % (err, rn.TOL_STATS))
    _check_scaled(got["scaled"], on_device["scaled"], "general")


def test_two_calls_of_t_are_one_call_of_2t(eng):
    reward, done = _general(1)
    reward, done = reward[:32], done[:32]
    zeros = np.zeros(GEN_ROWS, np.float32)
    whole = _Buffers(eng, reward, done, zeros, rn.RECORD_INIT).call(eng, GEN_GAMMA)
    first = _Buffers(eng, reward[:16], done[:16], zeros, rn.RECORD_INIT).call(eng, GEN_GAMMA)
    second = _Buffers(eng, reward[16:], done[16:], first["carry"], first["record"]).call(eng, GEN_GAMMA)
    assert np.array_equal(_bits(second["carry"]), _bits(whole["carry"]))
    _check_record(second["record"], whole["record"], "two calls", same_merges=False)   # (the same samples merged in another order)
    assert first["record"][0] == 1e-4 + 16 * GEN_ROWS and not np.array_equal(first["scaled"], whole["scaled"][:16])   # (another scale)


def test_the_flag_form_with_every_flag_report_is_the_plain_form(eng):
    rng = np.random.default_rng(2)
    for T, rows in ((1, 1), (16, 65), (33, 257), (8, 1000)):
        reward = rng.normal(size=(T, rows)).astype(np.float32)
        done = (rng.uniform(size=(T, rows)) < 0.2).astype(np.uint8)
        flags = (rng.integers(0, 1 << 14, size=(T, rows)) | rn.F_REPORT | np.where(rng.uniform(size=(T, rows)) < 0.3, 1 << 18, 0)).astype(np.int32)
        carry = rng.normal(size=rows).astype(np.float32)
        plain = _Buffers(eng, reward, done, carry, rn.RECORD_INIT).call(eng, GEN_GAMMA)
        flagged = _Buffers(eng, reward, done, carry, rn.RECORD_INIT, flags=flags, misalign=True).call(eng, GEN_GAMMA)
        for key in plain:
            assert np.array_equal(_bits(plain[key]), _bits(flagged[key])), (T, rows, key)


@pytest.mark.parametrize("shape", [(16, 37), (33, 257), (2, 1000)])
def test_nan_at_every_place_that_may_hold_one(eng, shape):
    """The rewards of rows that did not act are NaN, and so are `scaled` and the scratch in front of the call (_Buffers): every output is
    finite, rows that did not act are scaled to exactly 0, the carry equals the float32 recursion bit for bit and the record the checker
    on those samples."""
    T, rows = shape
    rng = np.random.default_rng(T)
    flags, done = rn.seat_history(rng, T, rows)
    reward = rng.normal(size=(T, rows)).astype(np.float32) * 3.0
    reward[~rn.acted(flags)] = np.nan
    carry = rng.normal(size=rows).astype(np.float32)
    got = _Buffers(eng, reward, done, carry, rn.RECORD_INIT, flags=flags).call(eng, GEN_GAMMA, clip=5.0)
    want = rn.return_norm_f64(reward, done, GEN_GAMMA, carry, rn.RECORD_INIT, flags=flags, clip=5.0, fp32=True)
    for key in got:
        assert np.isfinite(got[key]).all(), key
    assert np.array_equal(_bits(got["carry"]), _bits(want["carry"]))
    assert got["record"][0] == 1e-4 + rn.acted(flags).sum()
    _check_record(got["record"], want["record"], shape)
    _check_scaled(got["scaled"], want["scaled"], shape)
    assert np.array_equal(_bits(got["scaled"][~rn.acted(flags)]), np.zeros(int((~rn.acted(flags)).sum()), np.uint32))


def test_the_frozen_mode_leaves_carry_and_record_their_bytes(eng):
    reward, done = _general(3)
    rng = np.random.default_rng(3)
    carry, record = rng.normal(size=GEN_ROWS).astype(np.float32), np.array([1234.0001, 0.75, 9876.5, 0.3125])
    for flags in (None, rn.seat_history(rng, GEN_T, GEN_ROWS)[0]):
        b = _Buffers(eng, reward, done, carry, record, flags=flags)
        b.work.fill_(SENT)
        got = b.call(eng, GEN_GAMMA, clip=0.5, freeze=True)
        assert np.array_equal(_bits(got["carry"]), _bits(carry)) and np.array_equal(_bits(got["record"]), _bits(record))
        assert bool((b.work == SENT).all()), "the frozen mode wrote the scratch"
        assert np.array_equal(_bits(got["scaled"]), _bits(rn.scaled_rewards(reward, 0.3125, 0.5, flags)))


def test_a_call_without_a_sample_leaves_count_mean_and_m2(eng):
    T, rows = 5, 130
    flags = np.random.default_rng(4).integers(0, 1 << 14, size=(T, rows)).astype(np.int32) | rn.F_RESET   # (never PGD_F_REPORT)
    record = np.array([12.5, -3.0, 77.0, 123.0])
    got = _Buffers(eng, np.full((T, rows), np.nan, np.float32), np.zeros((T, rows), np.uint8), np.ones(rows, np.float32), record,
                   flags=flags).call(eng, GEN_GAMMA, eps=1e-8)
    assert np.array_equal(_bits(got["record"][:3]), _bits(record[:3]))
    assert abs(got["record"][3] - 1.0 / np.sqrt(77.0 / 12.5 + 1e-8)) <= 1e-12 * got["record"][3]
    assert (got["carry"] == 0).all() and np.array_equal(_bits(got["scaled"]), np.zeros((T, rows), np.uint32))


def test_refused_arguments(eng):
    import torch
    T, rows = 4, 70
    reward, done = _general(5)
    b = _Buffers(eng, reward[:T, :rows], done[:T, :rows], np.zeros(rows, np.float32), rn.RECORD_INIT, flags=np.full((T, rows), rn.F_REPORT))
    odd = torch.zeros((6, ), dtype=torch.float32, device="cuda")   # 4 floats behind the first: a record that is not 8-byte aligned
    assert odd.data_ptr() % 8 == 0
    p = lambda t: C.c_void_p(t.data_ptr())
    good = dict(reward=p(b.reward), done=p(b.done), flags=p(b.flags), T=T, rows=rows, gamma=0.99, eps=1e-8, clip=10.0, mode=0, carry=p(b.carry),
                record=p(b.record), scaled=p(b.scaled), work=p(b.work), work_bytes=b.work.numel() * 8)
    order = ("reward", "done", "flags", "T", "rows", "gamma", "eps", "clip", "mode", "carry", "record", "scaled", "work", "work_bytes")

    def call(**kw):
        a = dict(good, **kw)
        return eng.L.pgd_return_norm(eng.h, *[a[k] for k in order])

    assert eng.return_norm_work_bytes(rows) == 48
    bad = [dict(T=0), dict(rows=0), dict(T=-1), dict(gamma=-0.01), dict(gamma=1.01), dict(gamma=float("nan")), dict(eps=-1e-9),
           dict(eps=float("nan")), dict(mode=2), dict(work_bytes=47), dict(record=C.c_void_p(odd.data_ptr() + 4)),
           dict(work=C.c_void_p(b.work.data_ptr() + 4))]
    bad += [{k: None} for k in ("reward", "done", "carry", "record", "scaled", "work")]
    for kw in bad:
        assert call(**kw) == ERR_ARG, kw
    assert eng.L.pgd_return_norm(None, *[good[k] for k in order]) == ERR_ARG
    eng.sync()
    assert bool(torch.isnan(b.scaled).all()) and bool((b.carry == 0).all()), "a refused call launched"
    assert np.array_equal(b.record.cpu().numpy(), np.array(rn.RECORD_INIT))
    for kw in (dict(), dict(flags=None), dict(gamma=0.0), dict(gamma=1.0), dict(eps=0.0), dict(mode=1), dict(clip=-1.0)):
        assert call(**kw) == 0, kw
    eng.sync()
    assert bool(torch.isfinite(b.scaled).all())


def test_identical_bytes_from_two_runs(eng):
    rng = np.random.default_rng(6)
    T, rows = 16, 1000
    flags, done = rn.seat_history(rng, T, rows)
    reward = rng.normal(size=(T, rows)).astype(np.float32)
    carry = rng.normal(size=rows).astype(np.float32)
    for fl in (None, flags):
        a = _Buffers(eng, reward, done, carry, rn.RECORD_INIT, flags=fl).call(eng, GEN_GAMMA)
        b = _Buffers(eng, reward, done, carry, rn.RECORD_INIT, flags=fl).call(eng, GEN_GAMMA)
        for key in a:
            assert np.array_equal(_bits(a[key]), _bits(b[key])), key


def test_the_first_call_of_a_fresh_engine_is_capturable(descs):
    """Nothing is allocated inside the call and the scratch is the caller's: the very first call on an engine is made inside a graph
    capture (which runs nothing).  Replay k continues from the carry and the record that replay k - 1 left: behind each of four replays
    carry, record and scaled hold the bytes of k eager calls on the same inputs."""
    import torch
    reward, done = _general(7)
    zeros = np.zeros(GEN_ROWS, np.float32)
    fresh = _ego_engine(descs, 1)
    try:
        G, E = _Buffers(fresh, reward, done, zeros, rn.RECORD_INIT), _Buffers(fresh, reward, done, zeros, rn.RECORD_INIT)
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()   # (its own capture: the first call on a fresh engine is made inside the capture, nothing runs eagerly in front)
        with torch.cuda.graph(graph, stream=s):
            fresh.return_norm(G.reward, G.done, GEN_GAMMA, G.carry, G.record, out=G.scaled, work=G.work)
        torch.cuda.synchronize()
        assert bool(torch.isnan(G.scaled).all()) and bool((G.carry == 0).all()), "the capture itself ran the kernels"
        count = 1e-4
        for k in range(4):
            with torch.cuda.stream(s):
                graph.replay()
            torch.cuda.synchronize()
            want = E.call(fresh, GEN_GAMMA)
            got = dict(carry=G.carry.cpu().numpy(), record=G.record.cpu().numpy(), scaled=G.scaled.cpu().numpy())
            for key in want:
                assert np.array_equal(_bits(got[key]), _bits(want[key])), "replay %d: %s differs from %d eager calls" % (k + 1, key, k + 1)
            count += GEN_T * GEN_ROWS   # (one addition per call, as the record takes them)
            assert got["record"][0] == count
        del graph
    finally:
        fresh.close()


# ---------------------------------------------------------------------------------------------------------------------
# the collectors
# ---------------------------------------------------------------------------------------------------------------------
COL_ITER = 3
NORM_KEYS = ("scaled_rewards", "return_norm")
CLIP, EPS = 2.0, 1e-6


@pytest.mark.parametrize("kind,bootstrap", [("single", False), ("single", True), ("safe", False), ("safe", True), ("marl", False)],
                         ids=["RolloutCollector", "RolloutCollector-bootstrap", "SafeRolloutCollector", "SafeRolloutCollector-bootstrap",
                              "MultiAgentRolloutCollector"])
def test_collectors(descs, kind, bootstrap):
    """With the switch on, over three `collect(); update()` iterations: advantages and returns are the GAE call made by hand on
    batch["scaled_rewards"], bit for bit; scaled_rewards and the record equal the checker fed the rollout's own rewards, dones and flags
    (its recursion in float32, as the device forms the samples: the carry bit for bit, the count exactly, mean and m2 within 1e-12, the
    scaled rewards within 1 ulp); `rewards` stays raw; the safe collector's cost side is what it is with the switch off.  One
    `collect(); update()` captured in a HIP graph behind one eager iteration and replayed twice equals the eager sequence.  With the
    switch off the batch equals train_util.synchronised_rollouts, as today's tests hold it."""
    import torch
    marl = kind == "marl"
    extra = dict(bootstrap_truncations=True) if bootstrap else {}
    on_kw = dict(normalise_rewards=True, clip_reward=CLIP, reward_eps=EPS, **extra)
    keys = KEYS + NORM_KEYS + (("mask", "count") if marl else ()) + (("term_values", ) if bootstrap else ()) + \
        (("costs", "cost_advantages", "cost_returns", "ep_cost_sum", "ep_cost_count") if kind == "safe" else ())

    # (a) eagerly
    def snap(col, L):
        return dict(_snapshot(col.batch, keys), carry=col._rn_carry.clone(), **learner_state(L))

    A, col, L = make(kind, descs, **on_kw)
    shape = tuple(col.rewards.shape[1:])
    carry, record = np.zeros(shape, np.float32), np.array(rn.RECORD_INIT)
    want = []
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        for it in range(COL_ITER):
            batch = col.collect()
            torch.cuda.synchronize()
            assert batch["scaled_rewards"].shape == batch["rewards"].shape and batch["return_norm"].dtype == torch.float64
            adv, ret = hand_gae(A.eng, batch, marl, bootstrap)
            torch.cuda.synchronize()
            assert _bits_equal(adv, batch["advantages"]) and _bits_equal(ret, batch["returns"]), (it, "not the GAE call on the scaled rewards")
            rew, dn, fl = [batch[k].cpu().numpy() for k in ("rewards", "dones", "flags")]
            assert (dn != 0).any(), "no episode ends in rollout %d" % it
            ref = rn.return_norm_f64(rew, dn, 0.99, carry, record, flags=fl if marl else None, eps=EPS, clip=CLIP, fp32=True)
            carry, record = ref["carry"], ref["record"]
            assert np.array_equal(_bits(col._rn_carry.cpu().numpy().reshape(shape)), _bits(carry)), (it, "carry")
            err = _check_record(batch["return_norm"].cpu().numpy(), record, (kind, it))
            _check_scaled(batch["scaled_rewards"].cpu().numpy(), ref["scaled"], (kind, it))
            print("%s, rollout %d: %d samples, scale %.4f, record against the checker %.1e" % (kind, it, ref["samples"].size, record[3], err))
            assert not _bits_equal(batch["scaled_rewards"], batch["rewards"])
            L.update(batch)
            want.append(snap(col, L))
    A.eng.close()

    # (b) one collect() + update() captured behind one eager iteration, replayed twice
    G, col, L = make(kind, descs, **on_kw)
    eager_then_graph(lambda: L.update(col.collect()), lambda: snap(col, L), want, need=keys + ("carry", ) + EVERY_LEARNER)
    # a checkpoint of what the replays left, and the frozen mode
    state = col.state_dict()
    assert np.array_equal(_bits(state["return_norm"]), _bits(want[2]["return_norm"].cpu().numpy()))
    assert np.array_equal(_bits(state["return_norm_carry"]), _bits(want[2]["carry"].cpu().numpy()))
    col.load_state_dict(state)
    col.freeze_return_norm(True)
    with torch.no_grad():
        batch = col.collect()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(col.state_dict()["return_norm"]), _bits(state["return_norm"])), "the frozen mode moved the record"
    assert np.array_equal(_bits(col.state_dict()["return_norm_carry"]), _bits(state["return_norm_carry"]))
    fl = batch["flags"].cpu().numpy() if marl else None
    assert np.array_equal(_bits(batch["scaled_rewards"].cpu().numpy()), _bits(rn.scaled_rewards(batch["rewards"].cpu().numpy(), state["return_norm"][3], CLIP, fl)))
    G.eng.close()

    # (c) the switch off: today's batch, against the calls made one at a time (no update: the weights stay the first ones)
    off_keys = KEYS + (("mask", "index", "count") if marl else ())
    O, col, _ = make(kind, descs, learn=False, normalise_rewards=False, **extra)
    off = []
    with torch.no_grad():
        for it in range(2):
            batch = col.collect()
            assert "scaled_rewards" not in batch and "return_norm" not in batch
            off.append(_snapshot(batch, keys=[k for k in batch if k not in NORM_KEYS]))
    O.eng.close()
    for key in ("obs", "actions", "rewards", "dones", "flags"):   # (rollout 0 ran with the same weights: the switch changes no trajectory)
        assert _bits_equal(off[0][key], want[0][key]), (key, "the switch changed the trajectory")
    assert not _bits_equal(off[0]["advantages"], want[0]["advantages"])
    if kind == "safe":
        for key in ("costs", "cost_advantages", "cost_returns", "ep_cost_sum", "ep_cost_count"):
            assert _bits_equal(off[0][key], want[0][key]), (key, "the switch changed the cost side")
    if not bootstrap:
        S = Roundabout() if marl else Ego(descs, kind == "safe")
        sync = synchronised_rollouts(S, 2)
        S.eng.close()
        for it in range(2):
            if marl:
                n = int(sync[it]["count"].item())
                assert int(off[it]["count"].item()) == n and _bits_equal(off[it]["index"][:n], sync[it]["index"][:n])
            for key in off_keys:
                if key != "index":
                    assert _bits_equal(off[it][key], sync[it][key]), "switch off, rollout %d: %s differs from the synchronised loop" % (it, key)
