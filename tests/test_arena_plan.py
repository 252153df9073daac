"""The plan of the table arena (pgd_plan_arena): offsets from made-up table sizes -- pure arithmetic, nothing of that size is allocated
and no GPU is touched.  The kernels form a table address as base + zext(offset + index * sizeof(T)) in unsigned 32-bit arithmetic, so
the plan has to keep every byte of every table below 4 GiB - 64 KiB, offsets above 2^31 are ordinary (unsigned), and a set of tables
that does not fit is refused."""
import ctypes as C

import numpy as np
import pytest

from pgdrive_amd import build

PGD_OK, PGD_ERR_ARG = 0, 1  # include/pgdrive_hip.h
LIMIT = (1 << 32) - (64 << 10)
ALIGN = 256
MIB, GIB = 1 << 20, 1 << 30


@pytest.fixture(scope="module")
def plan():
    from pgdrive_amd import engine
    build.build()
    L = engine.load_library()

    def run(sizes):
        n = len(sizes)
        b = (C.c_uint64 * n)(*sizes)
        off = (C.c_uint32 * n)(*([0xdeadbeef] * n))
        total = C.c_uint64(0xdeadbeef)
        return L.pgd_plan_arena(b, n, off, C.byref(total)), list(off), total.value
    return run


def _tables(total):
    """Sixteen made-up table sizes, odd ones among them, that sum to `total` bytes."""
    sizes = [64 * 3 + 1, 7, 0, 5 * MIB + 13, 96 * 1001, 4 * 99991, 32 * 77777, 16 * 77777, 32 * 4099, 0, 64 * 17, 128 * 17 * 1000, 8 * 17 * 1000,
             333 * MIB + 5, 1]
    return sizes + [total - sum(sizes)]


def _check(sizes, off, total):
    assert off[0] >= 0 and total <= LIMIT and total % ALIGN == 0
    at = off[0]
    for k, (o, b) in enumerate(zip(off, sizes)):
        assert o % ALIGN == 0 and o == at, "table %d starts at %d, expected %d" % (k, o, at)  # in order, aligned, no gaps beyond the alignment
        at = (o + b + ALIGN - 1) // ALIGN * ALIGN
    assert total == at


def test_under_two_gib_is_planned_in_order_and_aligned(plan):
    sizes = _tables(2 * GIB - MIB)
    rc, off, total = plan(sizes)
    assert rc == PGD_OK
    _check(sizes, off, total)
    assert max(off) < 1 << 31


def test_offsets_above_two_gib_are_unsigned(plan):
    sizes = _tables(2 * GIB + MIB)
    sizes[-1], sizes[3] = sizes[3], sizes[-1]  # the big table in the middle
    sizes += [96 * 1000]  # behind just over 2 GiB of tables: starts above 2^31
    rc, off, total = plan(sizes)
    assert rc == PGD_OK
    _check(sizes, off, total)
    high = [k for k, o in enumerate(off) if o >= 1 << 31]
    assert len(sizes) - 1 in high and all(o > 0 for o in off)  # (a signed 32-bit offset would be negative: ctypes reads them as c_uint32)
    # the kernels' arithmetic on the last table (96-byte elements): offset + index * size in uint32 lands where 64-bit arithmetic does
    o, n = np.uint32(off[-1]), sizes[-1] // 96
    idx = np.array([0, 1, n // 2, n - 1], dtype=np.uint32)
    with np.errstate(over="ignore"):
        a32 = o + idx * np.uint32(96)
    assert a32.dtype == np.uint32
    assert [int(a) for a in a32] == [off[-1] + int(i) * 96 for i in idx]
    assert int(a32[-1]) + 96 <= total
    # ... and an index of -1 as the kernels convert it (uint32) wraps back to the element in front of the table, not 4 GiB ahead
    with np.errstate(over="ignore"):
        back = np.uint32(off[-1]) + np.uint32(0xffffffff) * np.uint32(96)
    assert int(back) == off[-1] - 96


def test_the_largest_arena_that_fits(plan):
    sizes = [LIMIT - 4096 - ALIGN, ALIGN]
    rc, off, total = plan(sizes)
    assert rc == PGD_OK and total == LIMIT
    _check(sizes, off, total)


@pytest.mark.parametrize("sizes", [
    _tables(4 * GIB + MIB),          # the tables' sum is over 4 GiB
    _tables(LIMIT + 1),              # just over the limit
    [LIMIT - 4096 - ALIGN, ALIGN + 1],  # one byte more than the largest arena
    [1 << 63, 1 << 63, 7],           # 64-bit sizes whose sum wraps
    [0xffffffffffffffff],
])
def test_over_the_limit_is_refused(plan, sizes):
    rc, off, total = plan(sizes)
    assert rc == PGD_ERR_ARG
    assert total == 0xdeadbeef  # nothing planned, nothing to allocate from


def test_bad_arguments(plan):
    from pgdrive_amd import engine
    L = engine.load_library()
    t = C.c_uint64(0)
    assert L.pgd_plan_arena(None, 1, (C.c_uint32 * 1)(), C.byref(t)) == PGD_ERR_ARG
    assert L.pgd_plan_arena((C.c_uint64 * 1)(8), 0, (C.c_uint32 * 1)(), C.byref(t)) == PGD_ERR_ARG
