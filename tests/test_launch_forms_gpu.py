"""The launch forms of a step on the GPU -- pgd_step_n, pgd_step_packed, pgd_step_group and a step captured in a HIP graph -- in every
engine mode of tests/modes.py.  step_impl hands one set of kernels a different output addressing per form (no observation pointer,
a row stride and the packed tail, a first block unit, state blocks written by k_step, the zero-row marks keyed by address and
stride, a memset node in front of k_observe under capture), and every kernel path reads those fields in its own place.

Every protocol runs twin engines of one mode on the same seed, scenarios and action stream: twin A is stepped with plain
Engine.step, twin B through the form under test, and everything is compared as bits (torch.equal, assert_same_state) -- the kernels
and their inputs are the same, only the addressing differs, so there is no tolerance.

  protocol N   step_n: a ring of 7 actions, 5 steps per call, 30 calls with `first` walking through the ring; one call without the
               observation, then a plain step;
  protocol P   packed rows in four layouts carved out of one allocation: the exact stride A*(D+2), that + 1, that + 2, and the exact
               stride from a base that is 4-byte aligned only; 40 steps each, sentinels around and between the rows;
  protocol G   env groups: 2 groups, and 3 or 4 where the envs divide into whole waves, stepped in an order that changes from step to
               step for 150 steps, then one group two steps ahead on its own;
  protocol H   one Engine.step captured in a HIP graph on one stream and replayed against the eager twin; multi-agent modes also a
               captured step_packed into layout 1 replayed in turns with eager calls into layout 2.

The `odd_*` modes give every layout an odd row width D (the 4-byte side of the observation code's store-width guards), the others
an even one; tests/test_parity_gpu.py holds the odd widths to the oracle.  48 - 66 envs, horizon 60, at least 130 steps per case:
every env ends at least once (n_done >= n is asserted), and the multi-agent cases count the rows that are not due.  Their floor is
half of what the fp64 oracle alone shows for the mode's configuration, seed and action stream (Setup.actions(), seed 17; every
protocol feeds that stream) in the first 130 steps -- tests/test_launch_forms_cpu.py holds the oracle to twice the floor:

  mode                          oracle   floor          mode                  oracle   floor
  marl8, odd_marl8, marl8_rows   17064    8532          parking                18184    9092
  marl40, odd_marl40            122296   61148          tollgate               15049    7524

Two contracts are stated at the end: Engine.step_packed forgets the zero-row marks for a rows tensor it has not seen alive (a fresh
tensor at a recycled address with the same stride would inherit them), and the action pointer of every step call is 8-byte aligned
(PGD_ERR_ARG otherwise, before anything is launched).  Run-time kernels, step info, images and the gather have tests of their own."""
import ctypes as C

import numpy as np
import pytest

from pgdrive_amd import _abi
from tests import parity
from tests.modes import MODES, Setup, assert_same_state, state_of, step_all
from tests.parity import closed_engines  # noqa: F401 (the fixture closes every engine a test made)

pytestmark = pytest.mark.gpu

PGD_ERR_ARG = 1  # include/pgdrive_hip.h
SENTINEL = -7.0  # no observation value, reward of these configurations or done flag
ALL_MODES = tuple(MODES)
MARL_MODES = tuple(m for m in MODES if "marl" in MODES[m])
# rows that are not due in the first 130 steps: half of the oracle's count (module docstring)
NOT_DUE_FLOOR = dict(marl8=8532, odd_marl8=8532, marl8_rows=8532, parking=9092, tollgate=7524, marl40=61148, odd_marl40=61148)
assert set(NOT_DUE_FLOOR) == set(MARL_MODES)
# env groups are launched as whole waves: three envs per wave in throughput mode, four in the ego-only kernel
GROUP_N = dict(pack=66, odd_pack=66, ego_only=64)
GROUP_CASES = [(m, 2) for m in ALL_MODES] + [(m, 4 if GROUP_N.get(m, MODES[m]["n"]) == 64 else 3) for m in ALL_MODES
                                             if GROUP_N.get(m, MODES[m]["n"]) in (48, 64)]


class Twins:
    """Twin engines A and B of a mode after the same reset, the mode's action stream, and the tally of what A's steps showed."""
    def __init__(self, descs, mode, n=None, env_b=None):
        s = self.s = Setup(descs, mode)
        if n is not None:
            s.n = n  # (the banks do not depend on it; configurations and actions read it when they are made)
        self.n, self.A = s.n, s.A
        self.a, self.b = s.engine(), s.engine(env=env_b)
        ids0 = np.arange(s.n) % s.n_scen
        import torch
        assert torch.equal(self.a.reset(ids0), self.b.reset(ids0))
        s.stagger(self.a, self.b)
        self.actions = s.actions()
        self.D, self.dev = self.a.D, self.a.device
        self.n_done = self.not_due = self.steps = 0
        self.all_envs = np.ones(s.n, dtype=bool)

    def step_a(self, act):
        """One plain step of A: its four outputs, cloned; counted."""
        outs, = step_all((self.a, ), act)
        self.count(outs[2], outs[3])
        return outs

    def count(self, done, flags):
        self.steps += 1
        self.n_done += int(done.sum())
        if self.A > 1:
            self.not_due += int(((flags & (_abi.F_REPORT | _abi.F_NEW)) == 0).sum())

    def same_state(self, what, envs=None):
        assert_same_state(state_of(self.a, skip=()), state_of(self.b, skip=()), self.all_envs if envs is None else envs, what)

    def finish(self, protocol, check_names=True):
        """the kernel the mode is about has run in both twins, and the case was no idle run"""
        if check_names:
            self.s.check_name(self.a)
            self.s.check_name(self.b)
        print("launch forms, %s:" % protocol, self.s.mode, "envs", self.n, "D", self.D, "steps", self.steps, "dones", self.n_done, "rows not due", self.not_due,
              "| A:", self.a.describe_step(), "| B:", self.b.describe_step())
        assert self.steps >= 130 and self.n_done >= self.n
        if self.A > 1:
            assert self.not_due >= NOT_DUE_FLOOR[self.s.mode]


def same_outputs(outs_a, outs_b, what):
    import torch
    for xa, xb, name in zip(outs_a, outs_b, parity.OUTPUTS):
        assert torch.equal(xa, xb), "%s differs, %s" % (name, what)


# ---------------------------------------------------------------------------------------------------------------------
# Protocol N
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ALL_MODES)
def test_step_n_equals_single_steps(descs, mode):
    """B: 30 calls of step_n, 5 steps each out of a ring of 7 whose first entry walks through the ring (the entries a call does not
    use hold other valid actions).  A: the same actions by plain steps.  Reward, done and flags of every slice, the observation
    after the last step -- the whole buffer: in multi-agent modes a row that is not due at the last step reads zero although the
    last observed step lies 5 steps back -- and the full state after every call.  Then one call without the observation, and a
    plain step on both twins: the same bits again."""
    import torch
    tw = Twins(descs, mode)
    a, b, L, K = tw.a, tw.b, 7, 5
    unused = tw.s.actions(99)
    t = 0

    def call(rep, want_obs):
        nonlocal t
        first = rep % L
        ring = np.stack([unused(k) for k in range(L)])
        for k in range(K):
            ring[(first + k) % L] = tw.actions(t + k)
        ring_d = torch.from_numpy(ring).to(tw.dev)
        obs_n, rew_n, done_n, fl_n = b.step_n(ring_d, first, K, want_obs=want_obs)
        for k in range(K):
            o, r, dn, fl = tw.step_a(ring[(first + k) % L])
            b.sync()
            assert torch.equal(rew_n[k], r) and torch.equal(done_n[k], dn) and torch.equal(fl_n[k], fl), "call %d, slice %d" % (rep, k)
        t += K
        assert (obs_n is None) if not want_obs else torch.equal(obs_n, o), "observation after call %d" % rep
        tw.same_state("after call %d" % rep)

    for rep in range(30):
        call(rep, True)
    rows_before = b.obs.clone()
    call(30, False)
    assert torch.equal(b.obs, rows_before), "a call without the observation wrote rows"
    act = tw.actions(t)
    outs_a = tw.step_a(act)
    outs_b, = step_all((b, ), act)
    same_outputs(outs_a, outs_b, "plain step after a call without the observation")
    tw.same_state("plain step after a call without the observation")
    tw.finish("step_n")


# ---------------------------------------------------------------------------------------------------------------------
# Protocol P
# ---------------------------------------------------------------------------------------------------------------------
def packed_layouts(tw, flat_extra=4):
    """One flat fp32 allocation and the four row layouts inside it: (first float, row stride).  The allocation is 8-byte aligned, so
    layouts 1 - 3 (from float 2) are too and layout 4 (from float 3) is 4-byte aligned only."""
    import torch
    W = tw.A * (tw.D + 2)
    layouts = [(2, W), (2, W + 1), (2, W + 2), (3, W)]
    flat = torch.full((3 + tw.n * (W + 2) + flat_extra, ), SENTINEL, dtype=torch.float32, device=tw.dev)
    assert flat.data_ptr() % 8 == 0
    return flat, layouts, W


def rows_view(flat, n, off, stride):
    return flat[off:off + n * stride].view(n, stride)


def check_packed(tw, flat, rows, off, outs_a, what):
    """`rows` (a layout of `flat` from float `off`) against A's outputs, and the sentinel everywhere else"""
    import torch
    n, A, D = tw.n, tw.A, tw.D
    o, r, dn, _ = outs_a
    assert torch.equal(rows[:, :A * D].reshape(n, A, D), o), "packed observation differs, " + what
    assert torch.equal(rows[:, A * D:A * D + A], r), "packed reward differs, " + what
    assert torch.equal(rows[:, A * D + A:A * (D + 2)], dn.to(torch.float32)), "packed done differs, " + what
    assert bool((rows[:, A * (D + 2):] == SENTINEL).all()), "padding columns written, " + what
    assert bool((flat[:off] == SENTINEL).all()), "floats in front of the first row written, " + what
    assert bool((flat[off + n * rows.stride(0):] == SENTINEL).all()), "floats behind the last row written, " + what


@pytest.mark.parametrize("mode", ALL_MODES)
def test_packed_rows_in_four_layouts(descs, mode):
    """B: step_packed into each of the four layouts for 40 steps, 160 steps on one twin pair.  After every step the packed
    observation, reward and done columns against A's outputs, B's own reward / done / flags against A's, and the sentinel in the
    padding columns, in front of the first row and behind the last.  The observation part is not refilled between the steps of a
    layout (the marks may leave a row they know to be zero alone); the whole allocation is refilled when the layout changes."""
    import torch
    tw = Twins(descs, mode)
    flat, layouts, W = packed_layouts(tw)
    t = 0
    for k, (off, stride) in enumerate(layouts):
        tw.b.sync()
        flat.fill_(SENTINEL)
        rows = rows_view(flat, tw.n, off, stride)
        assert rows.data_ptr() % 8 == (4 if k == 3 else 0) and rows.stride(0) == stride
        for _ in range(40):
            act = tw.actions(t)
            outs_a = tw.step_a(act)
            got, r, dn, fl = tw.b.step_packed(torch.from_numpy(act).to(tw.dev), rows)
            tw.b.sync()
            what = "layout %d, step %d" % (k + 1, t)
            assert got is rows
            same_outputs(outs_a[1:], (r, dn, fl), what)
            check_packed(tw, flat, rows, off, outs_a, what)
            t += 1
    tw.same_state("after 160 packed steps")
    tw.finish("packed rows")


# ---------------------------------------------------------------------------------------------------------------------
# Protocol G
# ---------------------------------------------------------------------------------------------------------------------
def step_groups(b, order, at):
    for g in order:
        b.step_group(g, at)
    for g in order:
        b.group_sync(g)
    return b.obs, b.reward, b.done, b.flags


@pytest.mark.parametrize("mode,groups", GROUP_CASES)
def test_env_groups_step_like_one_batch(descs, mode, groups):
    """B: set_groups, then every step as one step_group per group, in an order that changes from step to step, all groups synchronised
    before the four outputs are compared with A's; 150 steps.  Then the last group (its first block unit is not 0) two steps on its
    own: its rows and state are A's after two more steps, every other row and the state of every other env are untouched."""
    import torch
    tw = Twins(descs, mode, n=GROUP_N.get(mode))
    b, n = tw.b, tw.n
    b.set_groups(groups)
    for t in range(150):
        act = tw.actions(t)
        outs_a = tw.step_a(act)
        at = torch.from_numpy(act).to(tw.dev)
        torch.cuda.synchronize(tw.dev)
        order = [(g + t) % groups for g in range(groups)]
        same_outputs(outs_a, step_groups(b, order[::-1] if t % 3 == 2 else order, at), "step %d" % t)
    tw.same_state("after 150 grouped steps")
    g1 = groups - 1
    sl = b.group_slice(g1)
    mine = np.zeros(n, dtype=bool)
    mine[sl] = True
    mine_t = torch.from_numpy(mine).to(tw.dev)
    before, state_before = [x.clone() for x in (b.obs, b.reward, b.done, b.flags)], state_of(b, skip=())
    for t in (150, 151):
        act = tw.actions(t)
        outs_a = tw.step_a(act)
        at = torch.from_numpy(act).to(tw.dev)
        torch.cuda.synchronize(tw.dev)
        after = step_groups(b, [g1], at)
    for xa, xb, x0, name in zip(outs_a, after, before, parity.OUTPUTS):
        assert torch.equal(xb[mine_t], xa[mine_t]), "%s of the group that went two steps ahead" % name
        assert torch.equal(xb[~mine_t], x0[~mine_t]), "%s of the other groups touched" % name
    tw.same_state("the group that went two steps ahead", mine)
    assert_same_state(state_of(b, skip=()), state_before, ~mine, "the groups that did not step")
    tw.finish("%d env groups" % groups)


def test_ego_only_engine_refuses_groups_of_partial_waves(descs):
    """The ego-only kernel steps four envs per wave: 66 envs in 2 groups would be 33 per group -- PGD_ERR_ARG, and the engine steps on,
    bit-identical to a twin that never asked."""
    import torch
    from pgdrive_amd.engine import PgdError
    tw = Twins(descs, "ego_only")
    b = tw.b
    assert tw.n == 66
    for t in range(140):
        if t == 5:
            torch.cuda.synchronize(tw.dev)
            assert b.L.pgd_set_groups(b.h, 2) == PGD_ERR_ARG
            with pytest.raises(PgdError):
                b.set_groups(2)
            tw.same_state("after the refused pgd_set_groups")
        act = tw.actions(t)
        outs_a = tw.step_a(act)
        outs_b, = step_all((b, ), act)
        same_outputs(outs_a, outs_b, "step %d" % t)
    tw.same_state("after 140 steps")
    tw.finish("refused groups")


def test_throughput_mode_engine_leaves_it_for_groups_of_partial_waves(descs):
    """Throughput mode steps three envs per wave: 65 envs in 5 groups are 13 per group, so pgd_set_groups switches the engine to one
    env per wave for good.  pgd_describe_step says so, and from then on every output and the state are those of a twin created with
    PGD_PACK=0 and stepped with plain steps."""
    import torch
    tw = Twins(descs, "pack")  # A is rebuilt below: the twin of this case is no throughput-mode engine
    assert tw.n == 65
    a = tw.a = tw.s.engine(env=dict(PGD_PACK="0"))
    b = tw.b
    a.reset(np.arange(tw.n) % tw.s.n_scen)
    b.set_groups(5)
    for t in range(135):
        act = tw.actions(t)
        outs_a = tw.step_a(act)
        at = torch.from_numpy(act).to(tw.dev)
        torch.cuda.synchronize(tw.dev)
        same_outputs(outs_a, step_groups(b, [(g + t) % 5 for g in range(5)], at), "step %d" % t)
    tw.same_state("after 135 grouped steps")
    desc = b.describe_step()
    assert desc.startswith("k_step: one env per wave") and "throughput mode switched off by pgd_set_groups" in desc, desc
    assert a.describe_step() == desc[:desc.index(" [")], (a.describe_step(), desc)
    tw.finish("throughput mode left for 5 groups", check_names=False)  # (neither twin is a throughput-mode engine: asserted above)


# ---------------------------------------------------------------------------------------------------------------------
# Protocol H
# ---------------------------------------------------------------------------------------------------------------------
def capture(tw, a_static, call):
    """Warm `call` up on a side stream (A takes the same step), then capture it alone, on one stream, and return the graph (the
    capture pass does not execute)."""
    import torch
    act = tw.actions(0)
    side = torch.cuda.Stream(device=tw.dev)
    side.wait_stream(torch.cuda.current_stream(tw.dev))
    with torch.cuda.stream(side):
        a_static.copy_(torch.from_numpy(act).to(tw.dev))
        call()
    torch.cuda.current_stream(tw.dev).wait_stream(side)
    torch.cuda.synchronize(tw.dev)
    outs_a = tw.step_a(act)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    torch.cuda.synchronize(tw.dev)
    return graph, outs_a


@pytest.mark.parametrize("mode", ALL_MODES)
def test_step_captured_in_a_hip_graph_matches_eager(descs, mode):
    """B: one Engine.step on a static action tensor, warmed up on a side stream, captured with torch.cuda.graph on a single stream
    and replayed 135 times; A steps eagerly.  All four outputs after the warm-up step and after every replay, the state at the end."""
    import torch
    tw = Twins(descs, mode)
    b = tw.b
    a_static = torch.zeros((tw.n, tw.A, 2), dtype=torch.float32, device=tw.dev)
    graph, outs_a = capture(tw, a_static, lambda: b.step(a_static))
    same_outputs(outs_a, (b.obs, b.reward, b.done, b.flags), "warm-up step")
    for t in range(1, 136):
        act = tw.actions(t)
        outs_a = tw.step_a(act)
        a_static.copy_(torch.from_numpy(act).to(tw.dev))
        graph.replay()
        torch.cuda.synchronize(tw.dev)
        same_outputs(outs_a, (b.obs, b.reward, b.done, b.flags), "replay %d" % t)
    tw.same_state("after 135 replays")
    tw.finish("HIP graph")


@pytest.mark.parametrize("mode", MARL_MODES)
def test_packed_rows_captured_in_a_hip_graph(descs, mode):
    """Multi-agent modes: a step_packed into layout 1 (exact stride) captured in a HIP graph, replayed in turns with eager step_packed
    calls into layout 2 (stride + 1) of the same allocation.  After every step the buffer just written holds A's outputs -- the
    zero-row marks a replay meets describe the other buffer -- and the other buffer, the gap between the two and the floats around
    them hold what they held."""
    import torch
    tw = Twins(descs, mode)
    b, n = tw.b, tw.n
    W = tw.A * (tw.D + 2)
    off1, off2 = 2, 2 + n * W + 2
    flat = torch.full((off2 + n * (W + 1) + 3, ), SENTINEL, dtype=torch.float32, device=tw.dev)
    rows1, rows2 = rows_view(flat, n, off1, W), rows_view(flat, n, off2, W + 1)
    a_static = torch.zeros((n, tw.A, 2), dtype=torch.float32, device=tw.dev)
    graph, outs_a = capture(tw, a_static, lambda: b.step_packed(a_static, rows1))

    def check(rows, off, outs_a, what):
        n_, A, D = n, tw.A, tw.D
        o, r, dn, fl = outs_a
        assert torch.equal(rows[:, :A * D].reshape(n_, A, D), o), "packed observation differs, " + what
        assert torch.equal(rows[:, A * D:A * D + A], r) and torch.equal(rows[:, A * D + A:W], dn.to(torch.float32)), "packed tail differs, " + what
        same_outputs(outs_a[1:], (b.reward, b.done, b.flags), what)

    check(rows1, off1, outs_a, "warm-up step")
    for t in range(1, 136):
        act = tw.actions(t)
        outs_a = tw.step_a(act)
        a_static.copy_(torch.from_numpy(act).to(tw.dev))
        other = (rows1 if t % 2 else rows2).clone()
        if t % 2:
            b.step_packed(a_static, rows2)
        else:
            graph.replay()
        torch.cuda.synchronize(tw.dev)
        what = ("eager step %d into layout 2" if t % 2 else "replay %d into layout 1") % t
        check(rows2 if t % 2 else rows1, off2 if t % 2 else off1, outs_a, what)
        assert torch.equal(rows1 if t % 2 else rows2, other), "the buffer that was not written changed, " + what
        assert bool((flat[:off1] == SENTINEL).all()) and bool((flat[off1 + n * W:off2] == SENTINEL).all()), "floats between the layouts written, " + what
        assert bool((rows2[:, W:] == SENTINEL).all()) and bool((flat[off2 + n * (W + 1):] == SENTINEL).all()), "padding written, " + what
    tw.same_state("after 135 steps")
    tw.finish("packed rows in a HIP graph")


# ---------------------------------------------------------------------------------------------------------------------
# Contracts
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["marl8", "marl40"])
def test_zero_row_marks_do_not_survive_a_reused_address_in_packed_rows(descs, mode):
    """tests/test_env_gpu.py::test_zero_row_marks_do_not_survive_a_reused_address through Engine.step_packed: a fresh, sentinel-filled
    torch.empty rows tensor per step.  torch's caching allocator hands a freed block out again, so a NEW tensor can have the address
    and the row stride the marks name; step_packed forgets the marks (pgd_forget_rows) for every tensor it has not seen alive.  The
    allocator did reuse an address, and every row that is not due reads zero in every fresh buffer."""
    import torch
    s = Setup(descs, mode)
    eng = s.engine()
    eng.reset(np.arange(s.n) % s.n_scen)
    n, A, D = s.n, eng.A, eng.D
    actions = s.actions()
    acts = [torch.from_numpy(actions(t)).to(eng.device) for t in range(60)]
    addresses, n_zero = set(), 0
    for t in range(60):
        # (nothing else is allocated on the device inside the loop: the block a tensor leaves is the best fit for the next one)
        rows = torch.empty((n, A * (D + 2)), dtype=torch.float32, device=eng.device)
        rows.fill_(SENTINEL)
        addresses.add(rows.data_ptr())
        _, _, _, fl = eng.step_packed(acts[t], rows)
        eng.sync()
        not_due = (fl.cpu().numpy().astype(np.uint32) & (_abi.F_REPORT | _abi.F_NEW)) == 0
        obs = rows.cpu().numpy()[:, :A * D].reshape(n, A, D)
        assert not obs[not_due].any(), "step %d: a row that is not due kept the sentinel of a fresh buffer" % t
        assert (obs[~not_due] != SENTINEL).all(), "step %d: a row that is due was not written" % t
        n_zero += int(not_due.sum())
        del rows
    s.check_name(eng)
    print("packed rows at recycled addresses:", mode, "distinct addresses", len(addresses), "of 60; rows not due", n_zero)
    assert len(addresses) < 60, "the allocator never re-used an address: the test did not exercise the hazard"
    assert n_zero > 100


@pytest.mark.parametrize("mode", ["default", "pack", "marl8"])
def test_misaligned_actions_are_refused_by_every_step_call(descs, mode):
    """k_step reads an agent's action pair with one 8-byte load: d_actions is 8-byte aligned (include/pgdrive_hip.h, pgd_step).  A view
    that starts one float into a buffer is PGD_ERR_ARG from pgd_step, pgd_step_n, pgd_step_packed and pgd_step_group, and an
    AssertionError from the Engine methods in front of them; nothing is launched -- state and output buffers keep their bits -- and the
    engine then steps on, bit-identical to its twin.  (pgd_step_lane_keep takes no action pointer.)  Env groups where the envs divide."""
    import torch
    tw = Twins(descs, mode)
    a, b, n, A = tw.a, tw.b, tw.n, tw.A
    grouped = n % 2 == 0
    if grouped:
        b.set_groups(2)
    for t in range(5):
        act = tw.actions(t)
        same_outputs(tw.step_a(act), step_all((b, ), act)[0], "step %d" % t)
    buf = torch.zeros((2 * n * A * 2 + 2, ), dtype=torch.float32, device=tw.dev)
    mis = buf[1:1 + n * A * 2].view(n, A, 2)
    ring = buf[1:1 + 2 * n * A * 2].view(2, n, A, 2)
    assert buf.data_ptr() % 8 == 0 and mis.data_ptr() % 8 == 4 and mis.is_contiguous()
    rows = torch.full((n, A * (b.D + 2)), SENTINEL, dtype=torch.float32, device=tw.dev)
    before = [x.clone() for x in (b.obs, b.reward, b.done, b.flags)]
    state_before = state_of(b, skip=())
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    out = [p(x) for x in (b.obs, b.reward, b.done, b.flags)]
    torch.cuda.synchronize(tw.dev)
    calls = dict(pgd_step=lambda: b.L.pgd_step(b.h, p(mis), *out),
                 pgd_step_n=lambda: b.L.pgd_step_n(b.h, p(ring), 2, 1, 1, *out),
                 pgd_step_packed=lambda: b.L.pgd_step_packed(b.h, p(mis), p(rows), int(rows.stride(0)), *out[1:]))
    if grouped:
        calls["pgd_step_group"] = lambda: b.L.pgd_step_group(b.h, 1, p(mis), *out)
    methods = [lambda: b.step(mis), lambda: b.step_packed(mis, rows), lambda: b.step_n(ring, 0, 1), lambda: b.step_group(0, mis)]

    def untouched(what):
        torch.cuda.synchronize(tw.dev)
        same_outputs(before, (b.obs, b.reward, b.done, b.flags), what)
        assert bool((rows == SENTINEL).all()), what
        assert_same_state(state_of(b, skip=()), state_before, tw.all_envs, what)

    for name, fn in calls.items():
        assert fn() == PGD_ERR_ARG, name
        untouched(name)
    for k, fn in enumerate(methods):
        with pytest.raises(AssertionError):
            fn()
        untouched("Engine method %d" % k)
    for t in range(5, 135):
        act = tw.actions(t)
        outs_a = tw.step_a(act)
        if grouped and t % 2:  # (both ways on: the refused group call left the groups as they were)
            at = torch.from_numpy(act).to(tw.dev)
            torch.cuda.synchronize(tw.dev)
            same_outputs(outs_a, step_groups(b, [1, 0], at), "grouped step %d" % t)
        else:
            same_outputs(outs_a, step_all((b, ), act)[0], "step %d" % t)
    tw.same_state("after 135 steps")
    tw.finish("misaligned actions refused")
