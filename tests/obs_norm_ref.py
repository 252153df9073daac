"""Float64 checker of pgd_obs_norm_update / pgd_obs_norm_publish and of the normalised input of the bound network kernels
(include/pgdrive_hip.h states the rule), written from its formulas.  Shared by tests/test_obs_norm_cpu.py and tests/test_obs_norm_gpu.py.

The moments repeat the device's operations one for one: partitions of PART list positions (K = the first sample, s1 = sum (x - K),
s2 = sum (x - K)^2 in list order, mean = K + s1 / n, m2 = max(fma(-s1, s1 / n, s2), 0)), merged in partition order by Chan's update with
its two fused operations (mean = fma(delta, w, mean_a), m2 = fma(delta^2, n_a w, m2_a + m2_b)), the call's statistic then merged into the
record.  The fused operations are exact here (fractions); the per-sample term (x - K)^2 + s2 is a plain product and sum, which is the
device's fma wherever the product is exact -- on the exact inputs of the tests -- and within the bound below everywhere else."""
from fractions import Fraction

import numpy as np

PART = 512            # list positions per partition (ON_PART of pgdrive_amd/csrc/pgd_obs_norm.h)
DIM_MIN, DIM_MAX = 4, 416
U = 2.0 ** -53        # the unit roundoff of a double

_fma = np.frompyfunc(lambda a, b, c: float(Fraction(a) * Fraction(b) + Fraction(c)), 3, 1)


def fma64(a, b, c):
    """fma(a, b, c) in float64, exactly: the product and the sum as fractions, rounded once."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    return _fma(a, b, c).astype(np.float64)


def padded(in_dim):
    return (in_dim + 3) & ~3


def empty_record(in_dim):
    return np.zeros(1 + 2 * in_dim, np.float64)


def partition_stat(x):
    """(mean, m2) per column of the samples x [n, D] (n >= 1) as one partition forms them."""
    x = np.asarray(x, np.float64)
    K = x[0]
    s1, s2 = np.zeros_like(K), np.zeros_like(K)
    for row in x:
        dx = row - K
        s1 = s1 + dx
        s2 = s2 + dx * dx
    q = s1 / float(len(x))
    return K + q, np.maximum(fma64(-s1, q, s2), 0.0)


def merge(a, b):
    """Chan's update of a = (n, mean, m2) by b, per column; an empty a gives b's bits."""
    (na, ma, qa), (nb, mb, qb) = a, b
    tot = na + nb
    w = nb / tot if nb > 0 else 0.0
    delta = mb - ma
    return tot, fma64(delta, w, ma), fma64(delta * delta, na * w, qa + qb)


def call_stat(x):
    """(n, mean, m2) of the samples x [n, D] of one call: its partitions merged in partition order."""
    x = np.asarray(x, np.float64)
    D = x.shape[1]
    s = (0.0, np.zeros(D), np.zeros(D))
    for p0 in range(0, len(x), PART):
        part = x[p0:p0 + PART]
        s = merge(s, (float(len(part)), *partition_stat(part)))
    return s


def update(record, x):
    """One pgd_obs_norm_update: the samples x [n, D] (the listed rows, in list order, their first D columns) folded into `record`
    (float64 [1 + 2 D]) -> the new record.  n == 0: the record itself."""
    record = np.asarray(record, np.float64)
    x = np.asarray(x, np.float64)
    D = (record.size - 1) // 2
    if len(x) == 0:
        return record.copy()
    n, mean, m2 = merge((float(record[0]), record[1:1 + D], record[1 + D:]), call_stat(x.reshape(len(x), D)))
    return np.concatenate([[n], mean, m2])


def two_pass(x):
    """(n, mean, m2) per column of x [n, D] by two passes in extended precision: what the moments are held against."""
    x = np.asarray(x, np.float64).astype(np.longdouble)
    mean = x.mean(axis=0)
    return len(x), mean.astype(np.float64), ((x - mean) ** 2).sum(axis=0).astype(np.float64)


def bounds(x, calls=1):
    """(bound of |mean - exact|, bound of |m2 - exact|) per column for the samples x [n, D] folded by `calls` calls, from the lengths of
    the sums.  With R = max |x - mean| (the column's range) and A = max |x| (its magnitude):
    * the shifted sums work on differences: a sample enters a sequential sum of at most PART terms and then at most ceil(n / PART) +
      calls merges, L operations in sequence, each erring by at most U relative to a quantity bounded by R: L U R to first order;
    * a MEAN is stored M = 1 + ceil(n / PART) + calls times on that way (K + s1 / n, then one fma per merge), and each store rounds
      relative to the mean's own magnitude, which is A and not R (a column that sits at 0.49 with a range of 1e-3 still rounds at the
      ulp of 0.49): M U A;
    so |mean - exact| <= 4 U e with e = L R + M A, the factor 4 covering the handful of operations per step and the second-order terms.
    m2 sums squares of differences, n R^2 at most, over the same L operations, and each merge adds delta^2 n_a n_b / n with a delta that
    carries the means' error e U: a term of at most 2 R e U n.  Both are covered by |m2 - exact| <= 8 U n R e; a constant column has
    R = 0 and must have m2 = 0 exactly."""
    x = np.asarray(x, np.float64)
    n = len(x)
    R = np.abs(x - x.mean(axis=0)).max(axis=0)
    A = np.abs(x).max(axis=0)
    L = min(n, PART) + -(-n // PART) + calls + 4
    M = 1 + -(-n // PART) + calls
    e = L * R + M * A
    return 4.0 * U * e, 8.0 * U * n * R * e


def table(record, eps):
    """pgd_obs_norm_publish: record -> float32 [2, Dp] (shift | scale); the identity for n == 0 and in the padding columns."""
    record = np.asarray(record, np.float64)
    D = (record.size - 1) // 2
    out = np.zeros((2, padded(D)), np.float32)
    out[1] = 1.0
    if record[0] > 0:
        out[0, :D] = record[1:1 + D].astype(np.float32)
        with np.errstate(divide="ignore"):   # (eps = 0 and a constant column: inf, as the rule says)
            out[1, :D] = (1.0 / np.sqrt(record[1 + D:] / record[0] + eps)).astype(np.float32)
    return out


def normalise(x, tab, clip, in_dim):
    """The normalised input of rows x [rows, >= in_dim] float32: min(max((x - shift) * scale, -clip), clip) in float32, one subtraction and
    one multiplication; the columns at and beyond in_dim are 0 -> float32 of x's shape."""
    x = np.asarray(x, np.float32)
    tab = np.asarray(tab, np.float32)
    out = np.zeros_like(x)
    with np.errstate(invalid="ignore"):
        d = x[:, :in_dim] - tab[0, :in_dim]
        y = d * tab[1, :in_dim]
        out[:, :in_dim] = np.minimum(np.maximum(y, np.float32(-clip)), np.float32(clip))
    return out


def within_one_ulp(got, want):
    """float32 arrays: |got - want| <= one unit in the last place of the larger."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    return bool((d <= np.spacing(np.maximum(np.abs(got), np.abs(want)))).all())


def exact_rows(rng, n, stride):
    """Rows on a coarse binary grid: multiples of 1/8 in [-4, 4].  x - K is a multiple of 1/8 below 8, its square a multiple of 1/64
    below 64, and sums of up to 2^40 of them are exact in a double: s1 and s2 carry no rounding."""
    return (rng.integers(-32, 33, size=(n, stride)) / 8.0).astype(np.float32)
