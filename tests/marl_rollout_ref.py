"""The checker of pgdrive_amd/csrc/pgd_marl_rollout.h (k_compact, k_compact_scan, k_mlp_actor_critic_rows, k_gae_masked) and of
pgdrive_amd.rollout.MultiAgentRolloutCollector, in plain numpy:

* acted / cont / live      the predicates of include/pgdrive_hip.h over flag and done arrays;
* live_list / acted_index  the two index lists (np.flatnonzero);
* gae_masked_f64           the masked recursion in float64 -- what the device is held against;
* gae_masked_f32           the kernel's ARITHMETIC in float32 (the fma forms of actor_critic_ref.gae_f32, the selections of the
                           kernel).  Never compared with the device: its purpose is the half-tolerance rule of
                           tests/test_marl_rollout_cpu.py;
* segments                 the agent segments of a seat series, for the test that cuts them out and runs plain GAE on each;
* the seeded cases of the GPU module: flag patterns of the compaction (build_flags), seat histories of masked GAE (build_history).
  Pure functions of their arguments.

TOL_GAE_MASKED is MEASURED by the emulation over exactly the histories of the GPU test and doubled, as actor_critic_ref.TOL_GAE is.
"""
import numpy as np

from tests import actor_critic_ref as ar

F_RESET, F_REPORT, F_NEW = 1 << 16, 1 << 17, 1 << 18
OTHER_BITS = 0xffffffff & ~(F_RESET | F_REPORT | F_NEW)

# max |float32 recursion - float64| over gae_cases(), the histories with agents coming and going and the all-PGD_F_REPORT ones, with both
# lambdas, advantages and returns: 4.34e-6 (rewards N(0, 1), values N(0, 2), T up to 64); tests/test_marl_rollout_cpu.py measures it again
# and holds it below half of TOL_GAE_MASKED
TOL_GAE_MASKED_MEASURED = 4.34e-6
TOL_GAE_MASKED = 2.0 * TOL_GAE_MASKED_MEASURED

# the compaction's geometry (pgd_marl_rollout.h): a workgroup takes CMP_BLOCK indices in chunks of CMP_THREADS; the scan workgroup takes
# CMP_THREADS block counts per pass
CMP_THREADS, CMP_BLOCK = 256, 1024
SCAN_PASS = CMP_THREADS * CMP_BLOCK


# ---------------------------------------------------------------------------------------------------------------------
# predicates and lists
# ---------------------------------------------------------------------------------------------------------------------
def _u32(flags):
    return np.asarray(flags).astype(np.int64) & 0xffffffff


def acted(flags):
    return (_u32(flags) & F_REPORT) != 0


def cont(flags, done):
    return acted(flags) & (np.asarray(done) == 0) & ((_u32(flags) & F_RESET) == 0)


def live(flags, done):
    return ((_u32(flags) & F_NEW) != 0) | cont(flags, done)


def live_list(flags, done):
    """Ascending row numbers at which `live` holds (flags, done flattened)."""
    return np.flatnonzero(live(flags, done).reshape(-1)).astype(np.int32)


def acted_index(flags):
    """Ascending entries t * rows + r of a time-major flag array at which `acted` holds."""
    return np.flatnonzero(acted(flags).reshape(-1)).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------------
# masked GAE
# ---------------------------------------------------------------------------------------------------------------------
def gae_masked_f64(reward, value, done, flags, gamma, lam):
    """(adv, ret, mask): the recursion of include/pgdrive_hip.h (pgd_gae_masked) in float64; gamma, lam as the float32 the device is
    given.  Selections, not products: NaN in what is not read stays out."""
    r, v = np.asarray(reward, dtype=np.float64), np.asarray(value, dtype=np.float64)
    ac, co = acted(flags), cont(flags, done)
    g, gl = float(np.float32(gamma)), float(np.float32(gamma)) * float(np.float32(lam))
    adv, ret = np.zeros_like(r), np.zeros_like(r)
    a = np.zeros(r.shape[1:])
    for t in range(r.shape[0] - 1, -1, -1):
        delta = np.where(ac[t], r[t], 0.0) + g * np.where(co[t], v[t + 1], 0.0) - np.where(ac[t], v[t], 0.0)
        a = np.where(ac[t], delta + gl * np.where(co[t], a, 0.0), 0.0)
        adv[t] = a
        ret[t] = np.where(ac[t], a + np.where(ac[t], v[t], 0.0), 0.0)
    return adv, ret, ac.astype(np.uint8)


_f32 = ar._f32


def gae_masked_f32(reward, value, done, flags, gamma, lam):
    """k_gae_masked: delta = fma(gamma, cont ? v[t + 1] : 0, reward) - v[t]; a = acted ? fma(gamma lam, cont ? a : 0, delta) : 0;
    ret = acted ? a + v[t] : 0; float32."""
    ac, co = acted(flags), cont(flags, done)
    r = np.where(ac, _f32(reward), np.float32(0)).astype(np.float64)
    v = _f32(value).astype(np.float64)
    g = float(np.float32(gamma))
    gl = float(_f32(np.float32(gamma) * np.float32(lam)))
    adv, ret = np.zeros(r.shape, dtype=np.float32), np.zeros(r.shape, dtype=np.float32)
    a = np.zeros(r.shape[1:], dtype=np.float64)
    for t in range(r.shape[0] - 1, -1, -1):
        vt = np.where(ac[t], v[t], 0.0)
        delta = _f32(_f32(g * np.where(co[t], v[t + 1], 0.0) + r[t]).astype(np.float64) - vt).astype(np.float64)
        a = np.where(ac[t], _f32(gl * np.where(co[t], a, 0.0) + delta).astype(np.float64), 0.0)
        adv[t] = a
        ret[t] = np.where(ac[t], _f32(a + vt), np.float32(0))
    return adv, ret, ac.astype(np.uint8)


def segments(flags, done):
    """The agent segments of ONE seat series (flags, done of shape [T]): a list of (first, last, running) -- a maximal run of `acted`
    ended by !cont; running: the segment's agent still holds the seat behind step T - 1 (its bootstrap is value[T])."""
    ac, co = acted(flags), cont(flags, done)
    out, first = [], None
    for t in range(len(ac)):
        if not ac[t]:
            assert first is None  # (a seat whose agent continued acts in the next step: the generator's histories are consistent)
            continue
        if first is None:
            first = t
        if not co[t]:
            out.append((first, t, False))
            first = None
    if first is not None:
        out.append((first, len(ac) - 1, True))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# cases of the compaction
# ---------------------------------------------------------------------------------------------------------------------
PATTERNS = ("none", "all", "first", "last", "half", "combos")
# 1, 15, 16, 17, 63, 64, 65, 4099 and one below, at, one above: a chunk (256), a workgroup's block (1024), two blocks (2048)
LIVE_ROW_COUNTS = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4099)
# (T, rows): T * rows entries -- small ones, and 255, 256 and 257 blocks (one below, at, one above the scan workgroup's pass of 256
# block counts), then 261 blocks from a real shape
INDEX_SHAPES = ((1, 1), (3, 5), (7, 65), (2, 1024), (1, 1025), (5, 4099), (1, SCAN_PASS - CMP_BLOCK), (64, 4096), (1, SCAN_PASS + 1), (65, 4099))


def build_flags(n, pattern, predicate, seed=0):
    """(flags uint32 [n], done uint8 [n]) whose `predicate` ("live" or "acted") holds nowhere / everywhere / at the first / at the last
    index / at random with p = 0.5; "combos": all 16 combinations of PGD_F_REPORT, PGD_F_NEW, PGD_F_RESET and done, in random order.
    The other 29 flag bits are random in every pattern."""
    rng = np.random.default_rng([n, PATTERNS.index(pattern), ("live", "acted").index(predicate), seed])
    other = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64) & OTHER_BITS
    done = np.zeros(n, dtype=np.uint8)
    if pattern == "combos":
        c = rng.permutation(np.arange(n) % 16) if n >= 16 else rng.integers(0, 16, size=n)
        key = np.where(c & 1, F_REPORT, 0) | np.where(c & 2, F_NEW, 0) | np.where(c & 4, F_RESET, 0)
        done[:] = (c & 8) != 0
    else:
        on = dict(none=np.zeros(n, dtype=bool), all=np.ones(n, dtype=bool), first=np.arange(n) == 0, last=np.arange(n) == n - 1,
                  half=rng.uniform(size=n) < 0.5)[pattern]
        if predicate == "acted":
            key = np.where(on, F_REPORT, 0)
            done[:] = rng.uniform(size=n) < 0.5
        else:  # live: a new agent, or one that continues; not live: no agent, or one that ends (by done or by the reset)
            how = rng.integers(0, 3, size=n)
            key = np.where(on, np.where(how == 0, F_NEW, np.where(how == 1, F_REPORT, F_REPORT | F_NEW | F_RESET)),
                           np.where(how == 0, 0, np.where(how == 1, F_REPORT, F_REPORT | F_RESET)))
            done[:] = np.where(on, 0, how == 1)
    flags = (other | key.astype(np.uint64)).astype(np.uint32)
    want = live(flags, done) if predicate == "live" else acted(flags)
    if pattern != "combos":
        assert np.array_equal(want, on)
    return flags, done


# ---------------------------------------------------------------------------------------------------------------------
# cases of masked GAE
# ---------------------------------------------------------------------------------------------------------------------
GAE_T = (1, 2, 7, 64)
GAE_ROWS = (1, 63, 64, 65, 4099)
GAE_LAM = ar.GAE_LAM
GAE_GAMMA = ar.GAE_GAMMA
KINDS = ("never", "always", "done_last", "starts_mid", "reset_back_to_back", "reset_then_empty", "random")


def gae_cases():
    for T in GAE_T:
        for rows in GAE_ROWS:
            yield dict(T=T, rows=rows)


def build_history(T, rows, all_report=False):
    """(reward [T, rows] f32, value [T + 1, rows] f32, done uint8, flags uint32, kind [rows]): seat histories that are CONSISTENT
    (the seat acts in step t + 1 exactly if it was live behind step t).  Seat r has kind KINDS[r % 7] (seat 0 of a single row:
    "random"):
      never               no agent at all
      always              one agent from before the rollout to behind it (bootstrap value[T])
      done_last           one agent that ends by done in step T - 1
      starts_mid          empty, then PGD_F_NEW in step T // 2 - 1: a segment that starts at T // 2 (T = 1: never acts)
      reset_back_to_back  an agent cut by PGD_F_RESET without done in step T // 2, PGD_F_NEW in the same step: the next agent acts from
                          T // 2 + 1 on -- two segments back to back across a reset
      reset_then_empty    the same cut without a newcomer
      random              a chain: an agent ends by done with p = 0.1 and is cut by a reset with p = 0.05 (half of them with a newcomer);
                          an empty seat gets a newcomer with p = 0.2
    reward and value are NaN wherever the seat did not act (value[T]: wherever it is not live behind step T - 1); the other flag bits and
    the done of a seat without agent are random.  all_report: every flag is PGD_F_REPORT alone and nothing is NaN (the case that must
    equal pgd_gae bit for bit)."""
    rng = np.random.default_rng([T, rows, int(all_report), 0x3a51])
    reward = rng.normal(0, 1, size=(T, rows)).astype(np.float32)
    value = rng.normal(0, 2, size=(T + 1, rows)).astype(np.float32)
    done = np.zeros((T, rows), dtype=np.uint8)
    key = np.zeros((T, rows), dtype=np.int64)
    kind = np.arange(rows) % len(KINDS) if rows > 1 else np.array([len(KINDS) - 1])
    if all_report:
        done[:] = rng.uniform(size=(T, rows)) < 0.1
        return reward, value, done, np.full((T, rows), F_REPORT, dtype=np.uint32), kind
    u = rng.uniform(size=(T, rows, 3))
    occupied = np.isin(kind, [KINDS.index(k) for k in ("always", "done_last", "reset_back_to_back", "reset_then_empty")]) | \
        ((kind == KINDS.index("random")) & (rng.uniform(size=rows) < 0.5))
    mid = T // 2
    for t in range(T):
        f = np.where(occupied, F_REPORT, 0)
        d = np.zeros(rows, dtype=bool)
        k = lambda name: kind == KINDS.index(name)  # noqa: E731
        d |= k("done_last") & (t == T - 1)
        f |= np.where(k("starts_mid") & (t == mid - 1), F_NEW, 0)
        f |= np.where(k("reset_back_to_back") & (t == mid), F_RESET | F_NEW, 0)
        f |= np.where(k("reset_then_empty") & (t == mid), F_RESET, 0)
        rnd = k("random")
        d |= rnd & occupied & (u[t, :, 0] < 0.1)
        cut = rnd & occupied & ~d & (u[t, :, 0] > 0.95)
        f |= np.where(cut, F_RESET, 0) | np.where(cut & (u[t, :, 1] < 0.5), F_NEW, 0)
        f |= np.where(rnd & ~occupied & (u[t, :, 1] < 0.2), F_NEW, 0)
        d &= occupied
        key[t] = f
        done[t] = np.where(occupied, d, u[t, :, 2] < 0.1)
        reward[t] = np.where(occupied, reward[t], np.nan)
        value[t] = np.where(occupied, value[t], np.nan)
        occupied = live(f, done[t])
    value[T] = np.where(occupied, value[T], np.nan)
    other = rng.integers(0, 2 ** 32, size=(T, rows), dtype=np.uint64) & OTHER_BITS
    flags = (other | key.astype(np.uint64)).astype(np.uint32)
    return reward, value, done, flags, kind
