"""The floors of tests/test_launch_forms_gpu.py on the fp64 oracle alone: for every multi-agent mode of tests/modes.py, the mode's
configuration, seed, scenarios and action stream show at least twice the floor of rows that are not due in the first 130 steps (the
floor is half of the oracle's count), every such row reads zero, and every env has restarted by then (horizon 60)."""
import numpy as np
import pytest

from pgdrive_amd import _abi
from tests.modes import MODES, Setup

FLOORS = dict(marl8=8532, odd_marl8=8532, marl8_rows=8532, parking=9092, tollgate=7524, marl40=61148, odd_marl40=61148)


def test_the_floors_cover_the_multi_agent_modes():
    from tests import test_launch_forms_gpu as gpu
    assert gpu.NOT_DUE_FLOOR == FLOORS and set(FLOORS) == {m for m in MODES if "marl" in MODES[m]}


@pytest.mark.parametrize("mode", sorted(FLOORS))
def test_rows_not_due_on_the_oracle(descs, mode):
    from oracle import orc
    s = Setup(descs, mode)
    ora = orc.Oracle(s.make(), s.mb, s.sb)
    ora.reset(np.arange(s.n) % s.n_scen)
    actions = s.actions()
    not_due = 0
    restarted = np.zeros(s.n, dtype=bool)
    for t in range(130):
        obs, _, _, flags = ora.step(actions(t))
        idle = (flags & (_abi.F_REPORT | _abi.F_NEW)) == 0
        assert not obs[idle].any()
        not_due += int(idle.sum())
        restarted |= ((flags & _abi.F_RESET) != 0).any(axis=1)
    print("rows not due on the oracle:", mode, not_due, "floor", FLOORS[mode])
    assert FLOORS[mode] == not_due // 2 and restarted.all()
