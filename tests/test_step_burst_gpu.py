"""The record burst at the head of k_step (profiles/burst_notes.md): an env's record block is 8 V pieces of 16 bytes, and the kernels
that own a whole block fetch it with ceil(8 V / 64) full-width reads into LDS (pgd_vehicle.h: rec_stage_issue / rec_stage_take)
instead of eight plane reads per lane.  What such a load can get wrong sits at the edges of the block: a last read that is partial,
exactly full, or one piece over; a block that starts off a 128-byte boundary; a last env with nothing behind its block; a slot that
gets another slot's pieces.  Small engines (3 envs) at the slot counts where those edges fall, teacher-forced against the oracle
with respawn traffic (every slot drives), and one case where every word of the parked records carries a pattern of its own.

V = 17 runs the specialised kernel (the staged load); the other slot counts run the general kernels (eight plane reads), whose
block arithmetic is the same and which a later staged load for them has to keep green.
"""
import numpy as np
import pytest

from pgdrive_amd import _abi
from tests import parity, util
from tests.parity import OBS_TOL, REW_TOL, STATE_OBS_TOL, closed_engines  # noqa: F401 (the fixture closes every engine a test made)

pytestmark = pytest.mark.gpu

N_ENVS = 3  # odd env indices start their block at an odd multiple of 8 V pieces; env 2 has nothing behind its block
N_STEPS = 40
# traffic slots -> V = 1 + traffic: 8 pieces (one partial read), 64 (exactly one full read), 72 (one full read + 8 lanes), 136 (the
# default: the staged load), 192 (exactly three full reads)
TRAFFIC = [0, 7, 8, 16, 23]


def forced_run(eng, ora, cfg, n_steps, seed=0):
    """The teacher-forced loop of parity.single_teacher_forced on engines that exist already: returns what its assertions look at."""
    n = cfg.num_envs
    rng = np.random.default_rng(seed)
    stats = parity.new_stats()
    worst = {}
    pose = 0.0
    idm_ties = active = 0
    for s in parity.teacher_forced(eng, ora, stats, n_steps, lambda t: util.driving_actions(rng, n)):
        agree = s.agree
        tie = s.idm_tie(agree, skip_slots=cfg.num_agents)
        idm_ties += int((tie & agree).sum())
        active += int((s.i[_abi.SI["STATUS"]][:, cfg.num_agents:] == _abi.ST_ACTIVE).sum())
        if agree.any():
            pose = max(pose, s.pose_error(agree & ~tie))
        s.compare_state(agree & ~tie, worst)
    return stats, worst, pose, idm_ties, active


def assert_forced(name, stats, worst, pose, idm_ties, active):
    print(name, stats, "pose", pose, "idm ties", idm_ties, "of", active, "state fields (x tolerance):", {k: round(v, 3) for k, v in worst.items()})
    parity.report(name, stats)
    assert stats["obs"] < OBS_TOL and stats["obs_state"] < STATE_OBS_TOL and stats["rew"] < REW_TOL and pose < 1e-3
    assert not util.state_failures(worst), util.state_failures(worst)
    assert idm_ties <= 2e-3 * max(active, 1) + 2
    assert stats["flag_mismatch"] == 0


def start(descs, num_traffic):
    eng, ora, cfg = parity.engines(descs, N_ENVS, num_traffic=num_traffic, num_lasers=240, traffic_mode="respawn")
    ids = np.arange(N_ENVS) % 8
    o0 = ora.reset(ids)
    g0 = eng.reset(ids).cpu().numpy()
    assert np.abs(g0 - o0).max() < OBS_TOL
    return eng, ora, cfg


@pytest.mark.parametrize("num_traffic", TRAFFIC, ids=["V%d" % (1 + t) for t in TRAFFIC])
def test_block_edges(descs, num_traffic):
    """Every state float within the harness's tolerances and no flag mismatch over 40 teacher-forced steps at each slot count."""
    eng, ora, cfg = start(descs, num_traffic)
    res = forced_run(eng, ora, cfg, N_STEPS)
    if num_traffic == 16:  # (describe_step: the kernel of the last step)
        assert "specialised" in (eng.describe_step() or ""), "V = 17 must run the kernel with the staged load"
    assert_forced("burst V=%d" % (1 + num_traffic), *res)


DERIVED_FLOATS = [_abi.SF["HX"], _abi.SF["HY"]]
FREE_FLOATS = [k for k in range(_abi.NF) if k not in DERIVED_FLOATS]


def patterned_step(eng, ora, cfg):
    """From a state a few steps in: every second traffic slot is parked (ST_EMPTY) with a distinct bit pattern in every float word
    (finite values in [1, 2); the integer words keep their values -- they index tables -- and so does the heading vector, which both
    sides derive from the heading angle when a state is set), set on both sides; one step.  Returns the
    harness's statistics for that step, the worst state error of the agreeing slots, and the words of the slots the oracle left as
    they were, as the engine held them before the step and as read back after it."""
    forced_run(eng, ora, cfg, 5, seed=3)  # (ends with the oracle's fp32-rounded state on both sides)
    f, i, ei = ora.get_state()
    f32 = np.asarray(f, dtype=np.float32).copy()
    i = i.copy()
    parked = np.zeros(i.shape[1:], dtype=bool)
    parked[:, cfg.num_agents + 1::2] = True
    i[_abi.SI["STATUS"]][parked] = _abi.ST_EMPTY
    words = f32.view(np.uint32)
    k = 0
    for fld in FREE_FLOATS:
        for e, s in zip(*np.nonzero(parked)):
            words[fld, e, s] = 0x3F800000 + 0x0101 * k + 0x10000 * (k % 61)  # distinct, finite, normal
            k += 1
    assert len(np.unique(words[FREE_FLOATS][:, parked])) == len(FREE_FLOATS) * int(parked.sum())
    ora.set_state(f32.astype(np.float64), i, ei)
    eng.set_state(f32, i, ei)
    bf, bi, _ = eng.get_state()  # what the engine holds for that state: the words a record keeps in a narrower form come back as it keeps them
    held = np.ascontiguousarray(bf).view(np.uint32)
    rng = np.random.default_rng(11)
    stats = parity.new_stats()
    parity.compare_step(eng, ora, util.driving_actions(rng, cfg.num_envs), stats)
    of, oi, oei = ora.get_state()
    gf, gi, gei = eng.get_state()
    agree = (gi == oi).all(axis=0) & (gei == oei).all(axis=0)[:, None]
    tie = util.idm_tie(gf, of, stats["ties"].mg)
    tie[:, :cfg.num_agents] = False
    worst = util.compare_state(gf, of, agree & ~tie & ~parked, {})
    untouched = parked & (np.asarray(of, dtype=np.float32).view(np.uint32) == words)[FREE_FLOATS].all(axis=0) & (oi == i).all(axis=0)
    heading = max(float(np.abs(gf[k].astype(np.float64) - of[k])[untouched].max()) for k in DERIVED_FLOATS) if untouched.any() else 0.0
    return stats, worst, agree, parked, untouched, heading, (held[FREE_FLOATS], bi, words[FREE_FLOATS]), (np.ascontiguousarray(gf).view(np.uint32)[FREE_FLOATS], gi)


@pytest.mark.parametrize("num_traffic", [8, 16], ids=["V9", "V17"])
def test_every_word_of_every_record(descs, num_traffic):
    """pgd_set_state with a pattern of its own in every float word of the parked records, one step, pgd_get_state: the driving slots
    match the oracle, every slot the step does not touch comes back bit for bit (a piece that reached another slot's registers, or
    another word of its own, shows in either).  V = 9: one full read + 8 lanes; V = 17: the staged load itself."""
    eng, ora, cfg = start(descs, num_traffic)
    stats, worst, agree, parked, untouched, heading, (w_held, i_held, w_set), (w_got, i_got) = patterned_step(eng, ora, cfg)
    names = [n for n, k in sorted(_abi.SF.items(), key=lambda kv: kv[1]) if k in FREE_FLOATS]
    changed = {n: int((w_got[j] != w_held[j])[untouched].sum()) for j, n in enumerate(names) if (w_got[j] != w_held[j])[untouched].any()}
    narrowed = {n: int((w_held[j] != w_set[j])[parked].sum()) for j, n in enumerate(names) if (w_held[j] != w_set[j])[parked].any()}
    print("patterned records V=%d:" % (1 + num_traffic), stats, "parked", int(parked.sum()), "untouched", int(untouched.sum()), "heading vector", heading,
          "words the step changed in untouched slots", changed, "words the engine holds in another form than set", narrowed, {k: round(v, 3) for k, v in worst.items()})
    assert stats["flag_mismatch"] == 0 and stats["obs"] < OBS_TOL and stats["obs_state"] < STATE_OBS_TOL and stats["rew"] < REW_TOL
    assert not util.state_failures(worst), util.state_failures(worst)
    assert agree.all()
    # (which slots the step leaves alone is the oracle's verdict: an env that restarts in this step rebuilds all of its slots)
    assert untouched.sum() >= parked.sum() // 2 and (untouched.sum(axis=1) > 0).sum() >= 2, "parked slots that the step leaves alone, in two envs at least"
    assert heading < 1e-6
    assert not changed and (i_got[:, untouched] == i_held[:, untouched]).all()
