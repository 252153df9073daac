"""What tests/test_marl_rollout_gpu.py rests on, shown without a GPU (tests/marl_rollout_ref.py is the checker of both):

* masked GAE in float64 is plain GAE (actor_critic_ref.gae_f64) run separately on every agent segment cut out of a seat's series, and
  with every flag PGD_F_REPORT it is plain GAE on the whole array;
* TOL_GAE_MASKED is the float32 emulation's measured error over exactly the histories of the GPU test, doubled;
* the generated histories hold what the GPU test needs them to hold, and the flag patterns of the compaction are what their names say;
* the header compiles as C, declares the four entry points, the library exports them and refuses null arguments;
* MultiAgentRolloutCollector is importable without a GPU and sends a single-agent engine to RolloutCollector.
"""
import os
import re
import subprocess
import tempfile
import types

import numpy as np
import pytest

from tests import actor_critic_ref as ar
from tests import marl_rollout_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pgd_live_rows", "pgd_rollout_index", "pgd_mlp_actor_critic_rows", "pgd_gae_masked")


def test_masked_gae_is_plain_gae_on_every_agent_segment():
    n_seg = 0
    for c in mr.gae_cases():
        r, v, d, f, _ = mr.build_history(**c)
        T, rows = c["T"], c["rows"]
        for lam in mr.GAE_LAM + (1.0, ):
            adv, ret, mask = mr.gae_masked_f64(r, v, d, f, mr.GAE_GAMMA, lam)
            assert np.isfinite(adv).all() and np.isfinite(ret).all(), c
            assert np.array_equal(mask != 0, mr.acted(f))
            assert (adv[mask == 0] == 0).all() and (ret[mask == 0] == 0).all()
            for row in range(0, rows, max(1, rows // 130)):  # (every seat up to 130 rows, every 31st of 4099: all seven kinds)
                covered = np.zeros(T, dtype=bool)
                for first, last, running in mr.segments(f[:, row], d[:, row]):
                    n = last - first + 1
                    sv = np.concatenate([v[first:last + 1, row], [v[last + 1, row] if running else 0.0]]).astype(np.float64)
                    sd = np.zeros(n, dtype=np.uint8)
                    sd[-1] = 0 if running else 1
                    assert np.isfinite(sv).all() and np.isfinite(r[first:last + 1, row]).all(), (c, row, "NaN inside a segment")
                    a2, r2 = ar.gae_f64(r[first:last + 1, row][:, None], sv[:, None], sd[:, None], mr.GAE_GAMMA, lam)
                    assert np.abs(adv[first:last + 1, row] - a2[:, 0]).max() < 1e-12, (c, lam, row, first, last)
                    assert np.abs(ret[first:last + 1, row] - r2[:, 0]).max() < 1e-12, (c, lam, row, first, last)
                    covered[first:last + 1] = True
                    n_seg += 1
                assert np.array_equal(covered, mask[:, row] != 0)
    assert n_seg > 1000


def test_with_every_flag_report_masked_gae_is_plain_gae():
    for c in mr.gae_cases():
        r, v, d, f, _ = mr.build_history(all_report=True, **c)
        assert (f == mr.F_REPORT).all() and np.isfinite(r).all() and np.isfinite(v).all()
        for lam in mr.GAE_LAM:
            a1, r1, m = mr.gae_masked_f64(r, v, d, f, mr.GAE_GAMMA, lam)
            a2, r2 = ar.gae_f64(r, v, d, mr.GAE_GAMMA, lam)
            assert (m == 1).all() and np.array_equal(a1, a2) and np.array_equal(r1, r2), (c, lam)
            a3, r3, _ = mr.gae_masked_f32(r, v, d, f, mr.GAE_GAMMA, lam)
            a4, r4 = ar.gae_f32(r, v, d, mr.GAE_GAMMA, lam)
            assert np.array_equal(a3, a4) and np.array_equal(r3, r4), (c, lam, "the emulations differ")


def test_tol_gae_masked_is_the_emulations_error_over_the_gpu_histories_doubled():
    worst = 0.0
    for c in mr.gae_cases():
        for all_report in (False, True):
            r, v, d, f, _ = mr.build_history(all_report=all_report, **c)
            for lam in mr.GAE_LAM:
                a64, r64, m64 = mr.gae_masked_f64(r, v, d, f, mr.GAE_GAMMA, lam)
                a32, r32, m32 = mr.gae_masked_f32(r, v, d, f, mr.GAE_GAMMA, lam)
                assert np.array_equal(m64, m32) and np.isfinite(a32).all() and np.isfinite(r32).all()
                assert (a32[m32 == 0] == 0).all() and (r32[m32 == 0] == 0).all()
                worst = max(worst, float(np.abs(a32 - a64).max()), float(np.abs(r32 - r64).max()))
    print("float32 masked GAE against float64: %.3e (recorded %.2e, TOL_GAE_MASKED %.2e)" % (worst, mr.TOL_GAE_MASKED_MEASURED, mr.TOL_GAE_MASKED))
    assert mr.TOL_GAE_MASKED == 2.0 * mr.TOL_GAE_MASKED_MEASURED
    assert 0.8 * mr.TOL_GAE_MASKED_MEASURED < worst <= mr.TOL_GAE_MASKED / 2


def test_the_histories_hold_what_the_gpu_test_needs():
    """Consistent (acted(t + 1) == live(t)); NaN exactly where the seat did not act; and, from T = 7 on with at least 63 rows, every
    event the issue names."""
    for c in mr.gae_cases():
        r, v, d, f, kind = mr.build_history(**c)
        T, rows = c["T"], c["rows"]
        ac, co, lv = mr.acted(f), mr.cont(f, d), mr.live(f, d)
        assert np.array_equal(ac[1:], lv[:-1]), c
        assert np.array_equal(np.isnan(r), ~ac) and np.array_equal(np.isnan(v[:-1]), ~ac) and np.array_equal(np.isnan(v[-1]), ~lv[-1]), c
        assert ((f & mr.OTHER_BITS) != 0).mean() > 0.99
        if T >= 7 and rows >= 63:
            k = lambda name: kind == mr.KINDS.index(name)  # noqa: E731
            assert not ac[:, k("never")].any() and ac[:, k("always")].all() and co[:, k("always")].all()
            assert (d[T - 1, k("done_last")] == 1).all() and ac[T - 1, k("done_last")].all()
            sm = ac[:, k("starts_mid")]
            assert not sm[:T // 2].any() and sm[T // 2:].all()
            cut = (f[T // 2] & mr.F_RESET) != 0
            assert (cut & ac[T // 2] & (d[T // 2] == 0))[k("reset_back_to_back") | k("reset_then_empty")].all()  # ended by the reset alone
            assert ac[T // 2 + 1, k("reset_back_to_back")].all() and not ac[T // 2 + 1:, k("reset_then_empty")].any()
            nseg = [len(mr.segments(f[:, row], d[:, row])) for row in np.flatnonzero(k("random"))]
            assert T < 64 or max(nseg) >= 3


def test_the_flag_patterns_are_what_their_names_say():
    for pred, fn in (("live", lambda f, d: mr.live_list(f, d)), ("acted", lambda f, d: mr.acted_index(f))):
        for n in (1, 17, 4099):
            for p, count in (("none", 0), ("all", n), ("first", 1), ("last", 1)):
                f, d = mr.build_flags(n, p, pred)
                assert len(fn(f, d)) == count, (pred, n, p)
            f, d = mr.build_flags(n, "last", pred)
            assert fn(f, d)[0] == n - 1
        f, d = mr.build_flags(4099, "half", pred)
        assert 0.45 < len(fn(f, d)) / 4099 < 0.55
        f, d = mr.build_flags(4099, "combos", pred)
        key = ((f >> 17) & 1) | (((f >> 18) & 1) << 1) | (((f >> 16) & 1) << 2) | (d.astype(np.uint32) << 3)
        assert sorted(set(key.tolist())) == list(range(16))
        # of the 16 combinations: live = NEW (8) or REPORT without NEW, RESET and done (1); acted = REPORT (8)
        assert abs(len(fn(f, d)) / 4099 - (9 if pred == "live" else 8) / 16) < 0.01
    f2, d2 = mr.build_flags(4099, "half", "live")
    f3, d3 = mr.build_flags(4099, "half", "live")
    assert np.array_equal(f2, f3) and np.array_equal(d2, d3)  # pure functions of their arguments
    assert max(mr.LIVE_ROW_COUNTS) == 4099 and all(b + s in mr.LIVE_ROW_COUNTS for b in (mr.CMP_THREADS, mr.CMP_BLOCK, 2 * mr.CMP_BLOCK) for s in (-1, 0, 1))
    blocks = sorted(-(-T * rows // mr.CMP_BLOCK) for T, rows in mr.INDEX_SHAPES)
    assert all(b in blocks for b in (mr.CMP_THREADS - 1, mr.CMP_THREADS, mr.CMP_THREADS + 1))  # around the scan workgroup's pass


def test_header_compiles_as_c_and_declares_the_entry_points():
    from pgdrive_amd import engine
    prog = "#include <stdio.h>\n#include \"pgdrive_hip.h\"\nint main(void) {\n" + \
        "".join('  printf("%%d\\n", (int)(sizeof(&%s) > 0));\n' % fn for fn in ENTRY_POINTS) + "  return 0;\n}\n"
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "a.c")
        open(c, "w").write(prog)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", c, "-o", os.path.join(td, "a.o")])
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pgdrive_hip.h")).read(), flags=re.S)
    for fn in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(" % fn, src), fn
        assert fn in engine.EXPORTS


def test_the_library_exports_the_entry_points_and_refuses_null_arguments():
    from pgdrive_amd import engine
    L = engine.load_library()
    for fn in ENTRY_POINTS:
        assert hasattr(L, fn), fn
    assert L.pgd_live_rows(None, -1, None, None, None, None) == 1
    assert L.pgd_rollout_index(None, None, 1, 1, None, None) == 1
    assert L.pgd_mlp_actor_critic_rows(None, -1, None, 0, 0, None, 0, 0, 0, None, None, None, None, None) == 1
    assert L.pgd_gae_masked(None, None, None, None, None, 1, 1, 0.99, 0.95, None, None, None) == 1


def test_the_collector_is_importable_and_sends_single_agent_engines_to_rollout_collector():
    import pgdrive_amd
    from pgdrive_amd.rollout import MultiAgentRolloutCollector
    assert pgdrive_amd.MultiAgentRolloutCollector is MultiAgentRolloutCollector
    with pytest.raises(NotImplementedError, match="use RolloutCollector"):
        MultiAgentRolloutCollector(types.SimpleNamespace(A=1), None, None, T=4)
    with pytest.raises(NotImplementedError, match="single agent"):
        MultiAgentRolloutCollector(types.SimpleNamespace(engine=types.SimpleNamespace(A=1)), None, None, T=4)
