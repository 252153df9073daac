"""The checker tests/obs_norm_ref.py against itself and against two passes in extended precision (no GPU): the partitioned Chan merge,
calls that split a list, the empty call, the table rule and the normalised input."""
import numpy as np
import pytest

from tests import obs_norm_ref as on

P = on.PART


def _general(rng, n, D):
    """Columns of different offsets and scales, one of them constant."""
    x = (rng.normal(size=(n, D)) * rng.uniform(0.01, 30.0, size=D) + rng.normal(size=D) * 5.0).astype(np.float32)
    x[:, D // 2] = 0.625
    return x


def _held(record, x, calls=1):
    """`record` against the two-pass moments of x within the bounds derived from the sum lengths -> the largest share of a bound used."""
    D = x.shape[1]
    n, mean, m2 = on.two_pass(x)
    bm, bq = on.bounds(x, calls)
    assert record[0] == n
    em, eq = np.abs(record[1:1 + D] - mean), np.abs(record[1 + D:] - m2)
    assert (em <= bm).all() and (eq <= bq).all(), (float((em / np.maximum(bm, 1e-300)).max()), float((eq / np.maximum(bq, 1e-300)).max()))
    return float(max((em / np.maximum(bm, 1e-300)).max(), (eq / np.maximum(bq, 1e-300)).max()))


@pytest.mark.parametrize("n", [1, 2, P - 1, P, P + 1, 2 * P + 3])
def test_partitioned_merge_is_the_two_pass_moments(n):
    rng = np.random.default_rng(n)
    worst = 0.0
    for D in (4, 19):
        x = _general(rng, n, D)
        worst = max(worst, _held(on.update(on.empty_record(D), x), x))
        assert on.update(on.empty_record(D), x)[1 + D + D // 2] == 0.0   # (a constant column has no deviation, exactly)
    print("n = %d: the largest share of the derived bound used %.3f" % (n, worst))


def test_exact_inputs_have_exact_sums():
    """On the grid of exact_rows the checker's mean and m2 are the correctly rounded true values when n is a power of two."""
    rng = np.random.default_rng(0)
    x = on.exact_rows(rng, 256, 7)
    rec = on.update(on.empty_record(7), x)
    n, mean, m2 = on.two_pass(x)
    assert rec[0] == 256 and np.array_equal(rec[1:8], mean) and np.array_equal(rec[8:], m2)


@pytest.mark.parametrize("n", [2, P + 1, 2 * P + 3])
def test_two_calls_of_half_a_list_are_one_call(n):
    rng = np.random.default_rng(n + 1)
    D = 6
    x = _general(rng, n, D)
    half = n // 2
    split = on.update(on.update(on.empty_record(D), x[:half]), x[half:])
    _held(split, x, calls=2)
    _held(on.update(on.empty_record(D), x), x)


def test_an_empty_call_is_a_no_op():
    rng = np.random.default_rng(3)
    D = 5
    rec = on.update(on.empty_record(D), _general(rng, 40, D))
    again = on.update(rec, np.zeros((0, D)))
    assert np.array_equal(rec.view(np.uint64), again.view(np.uint64))
    assert np.array_equal(on.update(on.empty_record(D), np.zeros((0, D))), on.empty_record(D))


def test_the_table_rule():
    D, eps = 6, 1e-8
    t0 = on.table(on.empty_record(D), eps)
    assert t0.shape == (2, 8) and t0.dtype == np.float32 and (t0[0] == 0).all() and (t0[1] == 1).all()   # n == 0: the identity
    x = np.random.default_rng(4).normal(size=(100, D)).astype(np.float32) * 3.0 + 1.0
    x[:, 2] = -1.5   # a column of zero variance
    rec = on.update(on.empty_record(D), x)
    t = on.table(rec, eps)
    assert (t[0, D:] == 0).all() and (t[1, D:] == 1).all()   # the padding: always the identity
    assert t[0, 2] == np.float32(-1.5) and t[1, 2] == np.float32(1.0 / np.sqrt(eps))
    var = x.astype(np.float64).var(axis=0)   # the population variance
    assert on.within_one_ulp(t[0, :D], x.astype(np.float64).mean(axis=0).astype(np.float32))
    live = np.arange(D) != 2
    assert on.within_one_ulp(t[1, :D][live], (1.0 / np.sqrt(var + eps)).astype(np.float32)[live])
    assert on.table(rec, 0.0)[1, 2] == np.inf   # eps = 0 is allowed and is what it says


def test_the_normalised_input():
    rng = np.random.default_rng(5)
    D, stride, clip = 6, 11, 1.5
    x = rng.normal(size=(9, stride)).astype(np.float32) * 4.0
    x[:, D:] = np.nan
    tab = np.zeros((2, 8), np.float32)
    tab[0, :D], tab[1, :D] = rng.normal(size=D), rng.uniform(0.2, 3.0, size=D)
    tab[1, D:] = 1.0
    y = on.normalise(x, tab, clip, D)
    assert y.shape == x.shape and (y[:, D:] == 0).all() and np.isfinite(y).all()
    assert (y == clip).any() and (y == -clip).any() and (np.abs(y) <= clip).all()
    inner = np.abs(y[:, :D]) < clip
    want = (x[:, :D] - tab[0, :D]) * tab[1, :D]
    assert np.array_equal(y[:, :D][inner], want[inner])
    ident = np.zeros((2, 8), np.float32)
    ident[1] = 1.0
    assert np.array_equal(on.normalise(x, ident, np.inf, D)[:, :D].view(np.uint32), x[:, :D].view(np.uint32))
