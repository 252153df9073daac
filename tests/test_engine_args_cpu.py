"""The argument checks of pgdrive_amd/engine.py, without a GPU: the checker clause by clause on stand-ins, None where a
method allows it, the checks under `python -O`, and no `assert` statement left in the file."""
import ast
import os
import re
import subprocess
import sys

import pytest
import torch

from pgdrive_amd import engine
from pgdrive_amd.engine import Engine, PgdArgError, _dev, _opt, _p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class OnDevice:
    """What _dev looks at, for the accepting side: a tensor's description that says it is on the device."""
    is_cuda = True

    def __init__(self, dtype=torch.float32, n=8, contiguous=True, address=4096):
        self.dtype, self._n, self._contiguous, self._address = dtype, n, contiguous, address

    def numel(self):
        return self._n

    def is_contiguous(self):
        return self._contiguous

    def data_ptr(self):
        return self._address


def refused(t, *spec, **kw):
    with pytest.raises(PgdArgError) as e:
        _dev(t, *spec, **kw)
    assert isinstance(e.value, AssertionError)
    return str(e.value)


def test_every_form_of_a_device_buffer_is_accepted():
    f32, i32, u8 = torch.float32, torch.int32, torch.uint8
    t = OnDevice()
    assert _dev(t, f32, 8, "m", "x") is t                                       # an exact count
    assert _dev(t, f32, None, "m", "x", 8) is t and _dev(t, f32, None, "m", "x", 5) is t   # at least a count
    assert _dev(t, f32) is t and _dev(t, None) is t                             # no count; any dtype (scratch)
    one = OnDevice(i32, 1, contiguous=False)
    assert _dev(one, i32, 1, "m", "count", None, False) is one                  # one element: contiguity is not asked
    img = OnDevice(u8)
    assert _dev(img, (f32, u8), 8, "m", "out") is img and _dev(t, (f32, u8), 8, "m", "out") is t   # a choice of two dtypes
    for align in (4, 8, 16):
        a = OnDevice(address=4096 + align)
        assert _dev(a, f32, 8, "m", "x", None, True, align) is a


def test_each_clause_refuses_on_its_own():
    f32 = torch.float32
    msg = refused(torch.zeros(8), f32, 8, "gae", "reward")                      # everything right but the device
    assert msg.startswith("gae: reward: ") and "cpu float32" in msg
    msg = refused(OnDevice(torch.int32, 96), f32, 96, "ppo_grad", "logp_old")
    assert msg.startswith("ppo_grad: logp_old: ") and "float32 cuda tensor of 96 elements wanted, got int32 of 96" in msg
    assert "not contiguous" in refused(OnDevice(contiguous=False), f32, 8, "m", "x")
    for n in (7, 9):
        assert "of 8 elements wanted" in refused(OnDevice(n=n), f32, 8, "m", "x") and "m: x: " in refused(OnDevice(n=n), f32, 8, "m", "x")
    assert "at least 8 elements wanted" in refused(OnDevice(n=7), f32, None, "m", "rows", 8)
    assert "float32 or uint8" in refused(OnDevice(torch.int32), (f32, torch.uint8), 8, "observe_topdown", "out")
    for align in (4, 8, 16):
        assert "%d-byte aligned" % align in refused(OnDevice(address=4096 + align // 2), f32, 8, "m", "x", None, True, align)
    assert "not contiguous" in refused(OnDevice(contiguous=False), None, None, "m", "work")


def bare_engine(n=2, a=1):
    e = object.__new__(Engine)
    e.torch, e.N, e.A, e.D = torch, n, a, 18
    return e


def test_none_where_a_method_allows_it():
    assert _p(None) is None
    assert _opt(None, torch.float32, 2, "adv_mix", "adv_stats") is None
    t = OnDevice(n=2)
    assert _opt(t, torch.float32, 2, "adv_mix", "adv_stats") is t
    with pytest.raises(PgdArgError, match="adv_mix: adv_stats"):
        _opt(OnDevice(n=3), torch.float32, 2, "adv_mix", "adv_stats")
    assert Engine._list_args(bare_engine(), None, None, 8, "adv_stats") == (None, None)
    with pytest.raises(PgdArgError, match="adv_stats: count"):
        Engine._list_args(bare_engine(), None, OnDevice(torch.int32, 2), 8, "adv_stats")
    index, count = OnDevice(torch.int32, 9), OnDevice(torch.int32, 1, contiguous=False)
    ip, cp = Engine._list_args(bare_engine(), index, count, 8, "adv_stats")     # (a list may be longer than needed)
    assert ip.value == cp.value == 4096


def test_methods_refuse_host_tensors_before_they_touch_the_library():
    """A bare Engine has no library handle, no device and no stream: a method that got past its checks would raise AttributeError."""
    e = bare_engine()
    with pytest.raises(PgdArgError, match="step: actions"):
        Engine._check_actions(e, torch.zeros(2, 1, 2))
    with pytest.raises(PgdArgError, match="gae: reward"):
        Engine.gae(e, torch.zeros(2, 4), torch.zeros(3, 4), torch.zeros(2, 4, dtype=torch.uint8), 0.99, 0.95)
    with pytest.raises(PgdArgError, match="mlp_policy: obs"):
        Engine.mlp_policy(e, [torch.zeros(18, 256)], torch.zeros(2, 1, 2), obs=torch.zeros(2, 1, 18))
    with pytest.raises(PgdArgError, match="adam: param"):
        Engine.adam(e, *[torch.zeros(4)] * 4, torch.zeros(4, dtype=torch.int32), 3e-4)


CHILD = """
import sys, torch
from pgdrive_amd.engine import Engine
if __debug__:
    sys.exit(7)
e = object.__new__(Engine); e.torch = torch; e.N, e.A = 2, 1
caught = 0
try:
    Engine._check_actions(e, torch.zeros(2, 1, 2))
except AssertionError:
    caught += 1
try:
    Engine.gae(e, torch.zeros(2, 4), torch.zeros(3, 4), torch.zeros(2, 4, dtype=torch.uint8), 0.99, 0.95)
except AssertionError:
    caught += 2
sys.exit(40 + caught)
"""


def test_the_checks_stay_under_python_O():
    """`python -O` removes assert statements; the checks on buffers are exceptions and stay.  A fresh interpreter with -O: the action check
    on a host tensor and Engine.gae on host tensors both end in an AssertionError subclass (PgdArgError); a method that returned, or
    went on to a library it does not have, would not."""
    r = subprocess.run([sys.executable, "-O", "-c", CHILD], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode != 7, "the child did not run with -O"
    assert r.returncode == 43, "refused: %s of _check_actions (1) and gae (2)\n%s" % (r.returncode - 40, r.stderr[-2000:])


def test_no_assert_statement_is_left_in_the_engine_module():
    with open(engine.__file__) as f:
        tree = ast.parse(f.read())
    lines = [node.lineno for node in ast.walk(tree) if isinstance(node, ast.Assert)]
    assert not lines, "assert statements in engine.py at lines %s" % lines


def test_new_refusals_are_the_ones_design_section_32_lists():
    """The cases tests/test_engine_refusals_gpu.py marks as new are the rows of the table in DESIGN section 32, no more and no fewer."""
    from tests.test_engine_refusals_gpu import NEW_REFUSALS
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        section = f.read().split("\n## 32.")[1]
    listed = set(re.findall(r"^\| `(\w+)` \| `(\w+)` \|", section, flags=re.M))
    assert {(name, arg) for name, new in NEW_REFUSALS.items() for arg, _ in new} == listed
