"""pgd_shuffle_index and pgd_adam_gated (pgdrive_amd/csrc/pgd_minibatch.h; include/pgdrive_hip.h states both) restated in plain numpy: the
permutation in integers, so it is compared with `==`; the gated Adam in float64 around tests/ppo_ref.py's adam_f64.

The hash is tests/policy_ref.py's pgd_rng, here on arrays (uint64 holding 32-bit values) so that a permutation of 300001 entries, or 4000
epochs of one of 100, is one vectorised walk: every entry steps until it lands below c, the finished ones stand still."""
import numpy as np

from tests import ppo_ref as rf

M32 = np.uint64(0xffffffff)
KEY = 0x5b0ff1e5   # SHUF_KEY of the header
ROUNDS = 6


def _u(x):
    return np.asarray(x, dtype=np.uint64) & M32


def pcg_hash(x):
    state = (_u(x) * np.uint64(747796405) + np.uint64(2891336453)) & M32
    word = (((state >> ((state >> np.uint64(28)) + np.uint64(4))) ^ state) * np.uint64(277803737)) & M32
    return ((word >> np.uint64(22)) ^ word) & M32


def pgd_rng(seed, a, b, c):
    return pcg_hash(_u(seed) ^ pcg_hash(_u(a) ^ pcg_hash(_u(b) ^ pcg_hash((_u(c) + np.uint64(0x9e3779b9)) & M32))))


def widths(c):
    """(bl, br): the high and low bits of the Feistel domain of a list of c entries."""
    b = max(2, int(c - 1).bit_length())
    return b >> 1, b - (b >> 1)


def _network(x, bl, br, seed, e, rounds):
    L, R = x >> np.uint64(br), x & np.uint64((1 << br) - 1)
    lb, rb = bl, br
    for r in range(rounds):
        f = pgd_rng(seed ^ KEY, R, r, e) & np.uint64((1 << lb) - 1)
        L, R = R, L ^ f
        lb, rb = rb, lb
    return (L << np.uint64(rb)) | R


def walk(q, c, seed, e, rounds=ROUNDS):
    """pi(q) for an array of positions q < c under the epoch(s) e (a scalar, or an array of q's shape) -> (pi(q), the longest walk)."""
    bl, br = widths(c)
    x = _u(q).copy()
    e = np.broadcast_to(_u(e), x.shape)
    todo = np.ones(x.shape, dtype=bool)
    steps = 0
    while todo.any():
        x[todo] = _network(x[todo], bl, br, int(seed) & 0xffffffff, e[todo], rounds)
        todo &= x >= np.uint64(c)
        steps += 1
    return x.astype(np.int64), steps


def permutation(c, seed, epoch, epoch_dev=0, rounds=ROUNDS):
    """pi(0 .. c - 1) of epoch + epoch_dev (uint32 arithmetic), int64 [c]."""
    if c <= 0:
        return np.zeros((0, ), dtype=np.int64)
    e = (int(epoch) + (int(epoch_dev) & 0xffffffff)) & 0xffffffff
    return walk(np.arange(c), c, seed, e, rounds)[0]


def permutations(c, seed, epochs, rounds=ROUNDS):
    """The permutations of the epochs 0 .. epochs - 1, int64 [epochs, c]."""
    q = np.broadcast_to(np.arange(c), (epochs, c))
    e = np.broadcast_to(np.arange(epochs)[:, None], (epochs, c))
    return walk(q, c, seed, e, rounds)[0]


def shuffle_index(index, count, n_list, seed, epoch, epoch_dev=0, out=None):
    """What pgd_shuffle_index leaves in `out` (int32 [n_list]; None: zeros): the first clamp(count, 0, n_list) entries written."""
    out = np.zeros((n_list, ), dtype=np.int32) if out is None else np.array(out, dtype=np.int32)
    c = n_list if count is None else max(0, min(int(count), n_list))
    pi = permutation(c, seed, epoch, epoch_dev)
    out[:c] = pi if index is None else np.asarray(index)[pi]
    return out


def chi_square_sigmas(c, seed, epochs=4000, rounds=ROUNDS):
    """The chi-square of the (position, value) table of `epochs` permutations of c entries against the uniform expectation epochs / c, as
    a distance from its degrees of freedom (c - 1)^2 in standard deviations sqrt(2 dof)."""
    p = permutations(c, seed, epochs, rounds)
    table = np.zeros((c, c))
    np.add.at(table, (np.broadcast_to(np.arange(c), p.shape).reshape(-1), p.reshape(-1)), 1.0)
    want = epochs / c
    chi = float(((table - want) ** 2 / want).sum())
    dof = (c - 1) ** 2
    return (chi - dof) / np.sqrt(2.0 * dof)


GATE = ("stopped", "applied", "skipped", "skipped_now")   # _abi.ADAM_GATE


def adam_gated_f64(p, g, m, v, t, lr, gate, kl=None, kl_limit=0.0, lr_scale=None, count_gate=None, **hyper):
    """One pgd_adam_gated in float64 -> (p, m, v, t, gate, count_gate) after the call.  `gate`: four ints; `kl`, `lr_scale`, `count_gate`:
    numbers or None (the null pointers).  The applied step is ppo_ref.adam_f64 of step t + 1 with lr_eff = float32(lr) * float32(scale)."""
    gate = [int(x) for x in gate]
    if gate[0] != 0 or (kl is not None and not (float(kl) <= float(kl_limit))):
        gate[0], gate[2], gate[3] = 1, gate[2] + 1, 1
        return p, m, v, t, gate, (None if count_gate is None else 0)
    gate[1], gate[3] = gate[1] + 1, 0
    lr_eff = float(np.float32(lr)) if lr_scale is None else float(np.float32(lr) * np.float32(lr_scale))
    p2, m2, v2 = rf.adam_f64(p, g, m, v, t + 1, lr_eff, **hyper)
    return p2, m2, v2, t + 1, gate, count_gate
