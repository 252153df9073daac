"""Episode statistics of a rollout without a GPU: the two routines of the checker tests/rollout_episodes_ref.py against each other, the
seats mode against mode 0, one call of 2 T against two calls of T, the header and the ABI table, the exports and the refusals that need
no device, and the host logic of the three collectors on a recording engine."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import rollout_episodes_ref as er
from tests import recording_engine as rc
from tests.recording_engine import AllSwitchesEngine, collector as _collector

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _both(case, seats):
    a, b = er.by_definition(*case, seats=seats), er.kernel_order(*case, seats=seats)
    for key in ("ret_carry", "len_carry", "ep_return", "ep_length"):
        assert np.array_equal(er.bits(a[key]), er.bits(b[key])), key
    return a, b


# ---------------------------------------------------------------------------------------------------------------------
# the checker
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dones", ["some", "all", "none"])
def test_the_two_routines_agree_on_exact_inputs(dones):
    worst = 0.0
    for T, rows in er.EXACT_SHAPES:
        case = er.exact_case(T, rows, dones)
        a, b = _both(case, False)
        worst = max(worst, er.check_record(b["call"], a["call"], (T, rows, dones)))
        n = dict(some=None, all=T * rows, none=0)[dones]
        assert n is None or a["call"][0] == n
        assert a["call"][14] == T * rows and a["call"][13] == 0
        for s in a["samples"]:
            assert float(s[0]) == int(s[0]) and abs(s[0]) < 2 ** 24   # (an integer: exact in float32 in any order)
    print("by definition against the kernels' order, dones %s: %.1e (bound %.0e)" % (dones, worst, er.TOL_STATS))


@pytest.mark.parametrize("seats", [False, True])
def test_the_two_routines_agree_on_general_inputs(seats):
    for T, rows in ((33, 257), (16, 37), (2, 1000), (128, 70)):
        case = er.seat_case(T, rows) if seats else er.general_case(T, rows)
        a, b = _both(case, seats)
        err = er.check_record(b["call"], a["call"], (T, rows, seats))
        assert np.isfinite(a["call"][[0, 1, 2] + list(range(5, 16))]).all() and np.isfinite(a["ep_return"]).all()
        assert a["call"][0] == len(a["samples"]) > 0
        print("by definition against the kernels' order, %d x %d, seats %r: %.1e (bound %.0e)" % (T, rows, seats, err, er.TOL_STATS))


def test_a_worked_example():
    """One row, by hand: carry (2.5, 3); rewards 1, 2 | 4 | 8, 16 with dones behind 2 and 4: episodes (5.5, 5) and (4, 1), carry (24, 2)."""
    reward = np.array([1, 2, 4, 8, 16], np.float32).reshape(5, 1)
    done = np.array([0, 1, 1, 0, 0], np.uint8).reshape(5, 1)
    flags = np.array([1, 2 | 32, 1 | 4, 63, 63], np.int32).reshape(5, 1)   # (the causes of the entries that end nothing do not count)
    got = er.by_definition(reward, done, flags, [2.5], [3])
    assert [(float(s[0]), s[1]) for s in got["samples"]] == [(5.5, 5), (4.0, 1)]
    want = dict(episodes=2, return_mean=4.75, return_m2=1.125, return_min=4.0, return_max=5.5, length_sum=6, length_max=5, arrive=1,
                out_of_road=1, crash_vehicle=1, crash_object=0, crash_building=0, max_step=1, cut=0, steps=5, calls=1)
    assert dict(zip(er.FIELDS, got["call"])) == want
    assert got["ret_carry"].tolist() == [24.0] and got["len_carry"].tolist() == [2]
    assert got["ep_return"][:, 0].tolist() == [0, 5.5, 4, 0, 0] and got["ep_length"][:, 0].tolist() == [0, 5, 1, 0, 0]
    # the same row as a seat: nobody acts in step 0 (its NaN reaches nothing), step 3 is an env-wide restart without a done
    reward[0] = np.nan
    flags = flags | er.F_REPORT
    flags[0] &= ~er.F_REPORT
    flags[3] |= er.F_RESET
    got = er.by_definition(reward, done, flags, [2.5], [3], seats=True)
    assert [(float(s[0]), s[1], s[3]) for s in got["samples"]] == [(4.5, 4, 1), (4.0, 1, 1), (8.0, 1, 0)]
    assert got["call"][13] == 1 and got["call"][14] == 4 and got["ret_carry"].tolist() == [16.0] and got["len_carry"].tolist() == [1]
    assert np.array_equal(er.kernel_order(reward, done, flags, [2.5], [3], seats=True)["call"], got["call"])


def test_seats_mode_with_every_flag_report_and_no_reset_is_mode_0():
    for T, rows in ((1, 1), (16, 65), (33, 257)):
        reward, done, flags, rc_, lc = er.general_case(T, rows, p_done=0.2)
        flags = (flags | er.F_REPORT | np.where(np.random.default_rng(T).uniform(size=flags.shape) < 0.3, er.F_NEW, 0)).astype(np.int32)
        for routine in (er.by_definition, er.kernel_order):
            plain, seated = routine(reward, done, flags, rc_, lc), routine(reward, done, flags, rc_, lc, seats=True)
            for key in ("call", "ret_carry", "len_carry", "ep_return", "ep_length"):
                assert np.array_equal(er.bits(plain[key]), er.bits(seated[key])), (T, rows, key)


@pytest.mark.parametrize("seats", [False, True])
def test_one_call_of_2t_is_two_calls_of_t_through_the_carries(seats):
    T, rows = 16, 257
    reward, done, flags, rc_, lc = er.seat_case(2 * T, rows) if seats else er.general_case(2 * T, rows)
    whole = er.by_definition(reward, done, flags, rc_, lc, seats=seats)
    first = er.by_definition(reward[:T], done[:T], flags[:T], rc_, lc, seats=seats)
    second = er.by_definition(reward[T:], done[T:], flags[T:], first["ret_carry"], first["len_carry"], seats=seats)
    assert np.array_equal(er.bits(second["ret_carry"]), er.bits(whole["ret_carry"])) and np.array_equal(second["len_carry"], whole["len_carry"])
    key = lambda s: (er.bits(np.float32(s[0]).reshape(1))[0], ) + tuple(s[1:])
    assert sorted(map(key, first["samples"] + second["samples"])) == sorted(map(key, whole["samples"])), "other samples"
    assert np.array_equal(er.bits(np.concatenate([first["ep_return"], second["ep_return"]])), er.bits(whole["ep_return"]))
    assert np.array_equal(np.concatenate([first["ep_length"], second["ep_length"]]), whole["ep_length"])
    record = er.merge_record(er.merge_record(er.INIT, first["call"]), second["call"])
    want = er.merge_record(er.INIT, whole["call"])
    want[15] = 2.0
    er.check_record(record, want, "two calls")


def test_a_call_without_an_episode_moves_steps_and_calls_only():
    record = np.array([3.0, 1.5, 0.25, -1.0, 4.0, 17.0, 9.0, 1.0, 2.0, 0.0, 0.0, 0.0, 1.0, 0.0, 40.0, 2.0])
    reward, done, flags, rc_, lc = er.exact_case(4, 70, "none")
    call = er.by_definition(reward, done, flags, rc_, lc)["call"]
    assert np.array_equal(call, np.concatenate([er.INIT[:14], [280.0, 1.0]]))
    got = er.merge_record(record, call)
    assert np.array_equal(er.bits(got[:14]), er.bits(record[:14])) and got[14] == 320.0 and got[15] == 3.0


# ---------------------------------------------------------------------------------------------------------------------
# the header, the exports, what is refused without a device
# ---------------------------------------------------------------------------------------------------------------------
def test_the_abi_table_matches_the_header():
    from pgdrive_amd import _abi, engine
    text = open(os.path.join(ROOT, "include", "pgdrive_hip.h")).read()
    block = text[text.index("Episode statistics of a rollout"):text.index("#define PGD_EP_SEATS")]
    slots = re.findall(r"\b(\d+) ([a-z][a-z0-9_]*)\b", block[block.index("exact), 8-byte aligned:"):block.index("and starts as all zero")])
    assert [(int(i), name) for i, name in slots] == list(enumerate(_abi.ROLLOUT_EPISODES)) and len(slots) == 16
    assert _abi.ROLLOUT_EPISODES == er.FIELDS
    assert np.array_equal(er.bits(np.array(_abi.ROLLOUT_EPISODES_INIT)), er.bits(er.INIT))
    assert re.search(r"#define\s+PGD_EP_SEATS\s+1u", text) and _abi.EP_SEATS == 1
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+pgd_rollout_episodes\s*\(", src) and re.search(r"\bsize_t\s+pgd_rollout_episodes_work_bytes\s*\(", src)
    for bit, name in enumerate(er.CAUSES):   # the causes are bits 0 .. 5 of the flags, in the record's order
        assert re.search(r"#define\s+PGD_F_%s\s+\(1u << %d\)" % (name.upper(), bit), text), name
    assert re.search(r"#define\s+PGD_F_RESET\s+\(1u << 16\)", text) and re.search(r"#define\s+PGD_F_REPORT\s+\(1u << 17\)", text)
    for line in ("acted = f & PGD_F_REPORT;  cont = acted && !d && !(f & PGD_F_RESET);  ends = acted && !cont", "ONE plain fp32 add"):
        assert line in block, line
    sig = engine._SIGS["pgd_rollout_episodes"]
    assert sig[0] is C.c_int and len(sig[1]) == 15 and sig[1][6] is C.c_uint32 and sig[1][-1] is C.c_size_t
    for doc, what in (("DESIGN.md", "\n## 26. "), ("README.md", "episode_stats=True")):
        assert what in open(os.path.join(ROOT, doc)).read(), doc


def test_the_library_exports_the_two_symbols_and_refuses_without_a_gpu():
    from pgdrive_amd import engine
    L = engine.load_library()
    assert "pgd_rollout_episodes" in engine.EXPORTS and "pgd_rollout_episodes_work_bytes" in engine.EXPORTS
    assert hasattr(L, "pgd_rollout_episodes") and hasattr(L, "pgd_rollout_episodes_work_bytes")
    assert [L.pgd_rollout_episodes_work_bytes(r) for r in (-1, 0, 1, 64, 65, 4096)] == [0, 0, 128, 128, 256, 64 * 128]
    assert L.pgd_rollout_episodes(None, None, None, None, 1, 1, 0, None, None, None, None, None, None, None, C.c_size_t(0)) == 1


# ---------------------------------------------------------------------------------------------------------------------
# host logic: the collectors on a recording engine
# ---------------------------------------------------------------------------------------------------------------------
EP_KEYS = {"episode_stats", "episode_stats_rollout", "ep_returns", "ep_lengths"}


@pytest.mark.parametrize("kind", ["single", "safe", "marl"])
def test_switch_off_no_new_tensor_key_or_call(kind):
    import inspect
    eng, col = _collector(kind)
    eng.rollout_episodes = None   # (calling it would raise)
    batch = col.collect()
    assert set(batch) == dict(single=rc.TODAY, safe=rc.TODAY_SAFE, marl=rc.TODAY_MARL)[kind]
    assert not any("rollout_episodes" in c for c in eng.calls) and not col.episode_stats
    assert not any(hasattr(col, a) for a in ("ep_returns", "ep_lengths", "episode_record", "_ep_ret_carry"))
    assert col.state_dict() == {}
    assert inspect.signature(type(col).__init__).parameters["episode_stats"].default is False
    with pytest.raises(ValueError, match="episode_stats=False"):
        col.load_state_dict(dict(episode_stats=np.zeros(16)))
    with pytest.raises(ValueError, match="episode_stats=True"):
        col.episode_summary()
    with pytest.raises(ValueError, match="episode_stats=True"):
        col.clear_episode_stats()


@pytest.mark.parametrize("normalise", [False, True])
@pytest.mark.parametrize("kind", ["single", "safe", "marl"])
def test_switch_on_one_call_on_the_raw_rewards(kind, normalise):
    """One rollout_episodes call per collect(), in front of GAE, on the raw rewards; the batch's four new keys; three rollouts equal the
    checker carried by hand; the summary; clearing keeps the carries; a checkpoint round trip."""
    import torch
    marl = kind == "marl"
    eng, col = _collector(kind, episode_stats=True, normalise_rewards=normalise)
    script = eng.script
    rows = int(np.prod(script[0].shape[1:]))
    ret, length, record = np.zeros(rows, np.float32), np.zeros(rows, np.int32), er.INIT
    today = dict(single=rc.TODAY, safe=rc.TODAY_SAFE, marl=rc.TODAY_MARL)[kind] | ({"scaled_rewards", "return_norm"} if normalise else set())
    for k in range(3):
        del eng.calls[:]
        batch = col.collect()
        assert eng.calls.count("rollout_episodes(seats=%r)" % marl) == 1 and sum("rollout_episodes" in c for c in eng.calls) == 1
        assert eng.calls.index("rollout_episodes(seats=%r)" % marl) > max(i for i, c in enumerate(eng.calls) if c == "step")
        assert eng.episode_reward is col.rewards, "not the raw rewards"
        assert set(batch) == today | EP_KEYS
        sl = slice(k * rc.T, (k + 1) * rc.T)
        ref = er.by_definition(script[0][sl], script[1][sl], script[2][sl], ret, length, seats=marl)
        ret, length, record = ref["ret_carry"], ref["len_carry"], er.merge_record(record, ref["call"])
        assert np.array_equal(batch["episode_stats"].numpy(), record) and np.array_equal(batch["episode_stats_rollout"].numpy(), ref["call"])
        assert batch["ep_returns"].shape == batch["rewards"].shape and batch["ep_lengths"].dtype == torch.int32
        assert np.array_equal(batch["ep_returns"].numpy().reshape(rc.T, rows), ref["ep_return"])
        assert np.array_equal(batch["ep_lengths"].numpy().reshape(rc.T, rows), ref["ep_length"])
    assert record[0] > 0 and record[15] == 3
    s = col.episode_summary()
    assert set(s) == {"episodes", "mean_return", "std_return", "min_return", "max_return", "mean_length", "max_length", "arrive_rate",
                      "out_of_road_rate", "crash_vehicle_rate", "crash_object_rate", "max_step_rate", "cut_rate", "steps"}
    assert s["episodes"] == record[0] and s["mean_return"] == record[1] and s["std_return"] == np.sqrt(record[2] / record[0])
    assert s["mean_length"] == record[5] / record[0] and s["steps"] == record[14] and s["max_length"] == record[6]
    assert all(0.0 <= s[k] <= 1.0 for k in s if k.endswith("_rate")) and s["arrive_rate"] == record[7] / record[0]
    assert col.episode_summary(rollout=True)["episodes"] == ref["call"][0]
    # a checkpoint: the state into a fresh collector
    state = col.state_dict()
    assert set(state) == {"episode_return_carry", "episode_length_carry", "episode_stats"} | ({"return_norm_carry", "return_norm"} if normalise else set())
    assert np.array_equal(state["episode_return_carry"], ret) and np.array_equal(state["episode_length_carry"], length)
    assert np.array_equal(state["episode_stats"], record) and state["episode_length_carry"].dtype == np.int32
    eng2, col2 = _collector(kind, episode_stats=True, normalise_rewards=normalise)
    col2.load_state_dict(state)
    assert torch.equal(col2._ep_ret_carry, col._ep_ret_carry) and torch.equal(col2._ep_len_carry, col._ep_len_carry)
    assert torch.equal(col2.episode_record, col.episode_record)
    with pytest.raises(ValueError, match="rows"):
        col2.load_state_dict(dict(state, episode_return_carry=np.zeros(3)))
    # clearing: the initial record, the carries stay
    col.clear_episode_stats()
    assert np.array_equal(er.bits(col.episode_record.numpy()), er.bits(er.INIT)) and batch["episode_stats"] is col.episode_record
    assert np.array_equal(col._ep_ret_carry.numpy(), ret) and np.array_equal(col._ep_len_carry.numpy(), length)
    none = col.episode_summary()
    assert none["episodes"] == 0 and none["steps"] == 0 and all(none[k] is None for k in none if k not in ("episodes", "steps"))


# ---------------------------------------------------------------------------------------------------------------------
# the checkpoint of a collector with every switch on at once
# ---------------------------------------------------------------------------------------------------------------------
SWITCH_KEYS = {"normalise_rewards": {"return_norm_carry", "return_norm"},
               "episode_stats": {"episode_return_carry", "episode_length_carry", "episode_stats"},
               "normalise_obs": {"obs_norm_record"},
               "guardian": {"guardian_state", "guardian_prev_flags"}}
SWITCH_OFF = {"normalise_rewards": "normalise_rewards=False", "episode_stats": "episode_stats=False", "normalise_obs": "normalise_obs=False",
              "guardian": "guardian=None"}


def _all_switches(kind, **kw):
    return _collector(kind, engine=AllSwitchesEngine, **kw)


def _held(col):
    """state_dict()'s keys -> the collector's own tensors, for the switches that are on."""
    held = {}
    if col.normalise_rewards:
        held.update(return_norm_carry=col._rn_carry, return_norm=col.return_norm)
    if col.episode_stats:
        held.update(episode_return_carry=col._ep_ret_carry, episode_length_carry=col._ep_len_carry, episode_stats=col.episode_record)
    if col.normalise_obs:
        held.update(obs_norm_record=col.obs_norm_record)
    if col.guardian is not None:
        held.update(guardian_state=col._guard_state, guardian_prev_flags=col.flags[col.T - 1])
    return held


@pytest.mark.parametrize("kind", ["single", "safe", "marl"])
def test_every_switch_at_once_one_checkpoint(kind):
    """Every switch the collector has, on at once (the multi-agent one has no guardian): state_dict() holds the union of the switches' own
    keys behind ONE sync; a round trip restores every tensor exactly; a collector built without one switch refuses the state, and each
    of that switch's keys alone, by the switch's name."""
    import torch
    on = dict(normalise_rewards=True, episode_stats=True, normalise_obs=True)
    if kind != "marl":
        on["guardian"] = dict(weights=tuple(torch.zeros((rc.D, 1)) for _ in range(6)))
    eng, col = _all_switches(kind, **on)
    for _ in range(3):   # (the script's third rollout ends on a row with dones: the guardian's previous flags are not all zero)
        col.collect()
    del eng.calls[:]
    state = col.state_dict()
    assert eng.calls == ["sync"]
    assert set(state) == set().union(*(SWITCH_KEYS[s] for s in on))
    held = _held(col)
    assert set(held) == set(state)
    for key, x in held.items():
        assert state[key].dtype == x.numpy().dtype and np.array_equal(state[key].reshape(-1), x.numpy().reshape(-1)), key
        assert x.count_nonzero() > 0, "%s never moved: the round trip would prove nothing" % key
    eng2, col2 = _all_switches(kind, **on)
    assert not any(torch.equal(x2, held[key]) for key, x2 in _held(col2).items())
    col2.load_state_dict(state)
    for key, x2 in _held(col2).items():
        assert x2.dtype == held[key].dtype and x2.shape == held[key].shape and torch.equal(x2, held[key]), key
    for switch in on:
        eng3, col3 = _all_switches(kind, **{s: v for s, v in on.items() if s != switch})
        assert set(col3.state_dict()) == set(state) - SWITCH_KEYS[switch]
        with pytest.raises(ValueError, match=SWITCH_OFF[switch]):
            col3.load_state_dict(state)
        for key in SWITCH_KEYS[switch]:
            with pytest.raises(ValueError, match=SWITCH_OFF[switch]):
                col3.load_state_dict({key: state[key]})
