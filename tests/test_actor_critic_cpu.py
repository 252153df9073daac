"""What tests/test_actor_critic_gpu.py rests on, shown without a GPU (tests/actor_critic_ref.py is the checker of both):

* every GPU case keeps half of its tolerance when the kernel's float32 arithmetic is emulated, and its log_std stays in [-3, 1];
* TOL_Z and TOL_GAE are the emulation's measured errors over exactly the draws and shapes of the GPU tests, doubled;
* the noise the header defines is standard normal (524 k values: mean, variance, the correlation of z0 with z1 and of consecutive ticks
  within four standard errors) and finite;
* GAE by recursion is GAE by its definition;
* the largest accepted in_dim follows from the LDS formula;
* the Python mirror of pgd_actor_critic has the header's size and field offsets, and the header declares the entry points.
"""
import ctypes as C
import os
import re
import subprocess
import tempfile
import types

import numpy as np
import pytest

from tests import actor_critic_ref as ar
from tests import policy_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_gpu_case_keeps_half_its_tolerance_in_emulation():
    worst = dict(heads=0.0, action=0.0, logp=0.0)
    n = 0
    for c in ar.all_cases():
        x, p, v = ar.build_case(**c)
        k, oc = c["in_dim"], c["out_cols"]
        assert p[4].shape == (256, oc) and v[4].shape == (256, 1)
        assert np.isfinite(p[4][:, :4]).all() and np.isnan(p[4][:, 4:]).all() and np.isnan(p[5][4:]).all()
        assert np.isnan(x[:, k:]).all() and x.shape[1] > k
        mean, ls, val = ar.heads_f64(x[:, :k], p, v)
        assert ar.LOG_STD_RANGE[0] <= ls.min() and ls.max() <= ar.LOG_STD_RANGE[1], (c, ls.min(), ls.max())
        assert c["rows"] == 1 or (np.abs(mean).max() > 0.02 and np.abs(val).max() > 0.02 and np.ptp(ls) > 0.02), c
        em, els, ev = ar.emulate_heads(x[:, :k], p, v)
        heads = max(np.abs(em - mean).max(), np.abs(els - ls).max(), np.abs(ev - val).max())
        rows = np.arange(c["rows"])
        z64, z32 = ar.noise_f64(c["seed"], rows, c["tick"]), ar.noise_f32(c["seed"], rows, c["tick"])
        a64, l64 = ar.sample_f64(mean, ls, z64)
        a32, l32 = ar.emulate_sample(em, els, z32)
        fa = float((np.abs(a32 - a64) / ar.tol_action(mean, ls, z64)).max())
        fl = float((np.abs(l32 - l64) / ar.tol_logp(ls, z64)).max())
        assert heads < pr.TOL_EXACT / 2 and fa < 0.5 and fl < 0.5, (c, heads, fa, fl)
        worst = dict(heads=max(worst["heads"], heads), action=max(worst["action"], fa), logp=max(worst["logp"], fl))
        n += 1
    assert n == 2 * (len(ar.WIDTHS) + 1) + len(ar.ROW_COUNTS) + 6
    print("emulation over %d cases: heads %.2e (tolerance %.0e), action %.3f and logp %.3f of their tolerances" % (
        n, worst["heads"], pr.TOL_EXACT, worst["action"], worst["logp"]))


def test_the_hash_restated_for_arrays_is_the_scalar_one():
    rows = np.array([0, 1, 4098, 2 ** 31, 2 ** 32 - 1])
    for seed, tick in ((0, 0), (7, 2 ** 32 - 1), (0xdeadbeef, 2 ** 31)):
        r1, r2 = ar.draws(seed, rows, tick)
        for i, g in enumerate(rows):
            assert int(r1[i]) == pr.pgd_rng(seed ^ ar.K_SEED, int(g), ar.K_STREAM, tick)
            assert int(r2[i]) == pr.pgd_rng(seed ^ ar.K_SEED, int(g), ar.K_STREAM, tick ^ 0x80000000)
    u1, u2 = ar.units(0, np.arange(4099), 0)
    for u in (u1, u2):  # exact in float32, never 0 or 1
        assert (u.astype(np.float32).astype(np.float64) == u).all() and u.min() > 0.0 and u.max() < 1.0
    assert float(np.float32((2 ** 23 - 1) + 0.5)) == 2 ** 23 - 0.5  # the largest draw: 24 significant bits


def test_tol_z_is_the_emulations_error_over_the_gpu_draws_doubled():
    worst, n = 0.0, 0
    for seed, rows, tick in ar.all_draws():
        z64, z32 = ar.noise_f64(seed, rows, tick), ar.noise_f32(seed, rows, tick)
        assert np.isfinite(z32).all()
        worst = max(worst, float(np.abs(z32 - z64).max()))
        n += z64.size
    print("float32 Box-Muller against float64 over %d values: %.3e (recorded %.2e, TOL_Z %.2e)" % (n, worst, ar.TOL_Z_MEASURED, ar.TOL_Z))
    assert ar.TOL_Z == 2.0 * ar.TOL_Z_MEASURED
    assert 0.8 * ar.TOL_Z_MEASURED < worst <= ar.TOL_Z / 2


def test_tol_gae_is_the_emulations_error_over_the_gpu_shapes_doubled():
    worst = 0.0
    for c in ar.gae_cases():
        r, v, d = ar.build_gae(**c)
        if c["pattern"] == "bernoulli" and c["T"] * c["rows"] > 1000:
            assert 0.05 < d.mean() < 0.15
        for lam in ar.GAE_LAM:
            a64, r64 = ar.gae_f64(r, v, d, ar.GAE_GAMMA, lam)
            a32, r32 = ar.gae_f32(r, v, d, ar.GAE_GAMMA, lam)
            worst = max(worst, float(np.abs(a32 - a64).max()), float(np.abs(r32 - r64).max()))
    print("float32 GAE against float64: %.3e (recorded %.2e, TOL_GAE %.2e)" % (worst, ar.TOL_GAE_MEASURED, ar.TOL_GAE))
    assert ar.TOL_GAE == 2.0 * ar.TOL_GAE_MEASURED
    assert 0.8 * ar.TOL_GAE_MEASURED < worst <= ar.TOL_GAE / 2


def test_gae_by_recursion_is_gae_by_definition():
    for c in ar.gae_cases():
        if c["rows"] > 65:
            continue
        r, v, d = ar.build_gae(**c)
        for lam in ar.GAE_LAM + (1.0, ):
            a, ret = ar.gae_f64(r, v, d, ar.GAE_GAMMA, lam)
            a2, ret2 = ar.gae_by_definition_f64(r, v, d, ar.GAE_GAMMA, lam)
            assert np.abs(a - a2).max() < 1e-12 * max(1.0, np.abs(a2).max()) and np.abs(ret - ret2).max() < 1e-11, (c, lam)
            if lam == 0.0:  # the one-step TD error
                delta = r + float(np.float32(ar.GAE_GAMMA)) * v[1:].astype(np.float64) * (d == 0) - v[:-1]
                assert np.abs(a - delta).max() < 1e-12
            if c["pattern"] == "all":  # every step ends an episode: nothing is bootstrapped
                assert np.abs(ret - r).max() < 1e-12


def test_the_noise_is_standard_normal():
    """Seed 0, rows 0 .. 4095, ticks 0 .. 63, as the kernel computes it (float32)."""
    rows = np.arange(4096)
    z = np.stack([ar.noise_f32(0, rows, t) for t in range(64)]).astype(np.float64)  # [tick, row, 2]
    assert np.isfinite(z).all()
    n = z.size
    assert n == 524288
    assert abs(z.mean()) < 4.0 / np.sqrt(n)
    assert abs(z.var() - 1.0) < 4.0 * np.sqrt(2.0 / n)
    for i in (0, 1):
        assert abs(z[..., i].mean()) < 4.0 / np.sqrt(n / 2) and abs(z[..., i].var() - 1.0) < 4.0 * np.sqrt(4.0 / n)
    c01 = float((z[..., 0] * z[..., 1]).mean())
    assert abs(c01) < 4.0 / np.sqrt(n / 2)
    ct = float((z[:-1] * z[1:]).mean())
    assert abs(ct) < 4.0 / np.sqrt(z[1:].size)
    cr = float((z[:, :-1] * z[:, 1:]).mean())  # neighbouring rows
    assert abs(cr) < 4.0 / np.sqrt(z[:, 1:].size)
    print("noise: mean %.2e, variance - 1 %.2e, corr(z0, z1) %.2e, corr(tick, tick + 1) %.2e, corr(row, row + 1) %.2e; max |z| %.2f" % (
        z.mean(), z.var() - 1.0, c01, ct, cr, np.abs(z).max()))


def test_the_in_dim_limit_follows_from_the_lds_formula():
    kmax = ar.max_in_dim()
    assert kmax == 416
    assert ar.lds_bytes(kmax) <= pr.LDS_LIMIT < ar.lds_bytes(kmax + 1)
    assert ar.lds_bytes(kmax) > pr.LDS_DEFAULT  # the boundary case needs the raised limit
    for k in (4, 274, 416, 448):  # the head's weights: four rows of 256 instead of two
        assert ar.lds_bytes(k) == pr.lds_bytes_exact(k) + 2 * 256 * 4
    assert kmax < pr.max_in_dim()
    assert ar.PROLOGUE_SWITCH + 1 < kmax and all(k <= kmax for k in ar.WIDTHS)


def test_abi_mirror_of_pgd_actor_critic_and_declared_entry_points():
    """sizeof / offsetof of pgd_actor_critic from a C program compiled against the header == pgdrive_amd._abi.ActorCritic."""
    from pgdrive_amd import _abi, engine
    fields = [n for n, _ in _abi.ActorCritic._fields_]
    assert fields == ["w1", "b1", "w2", "b2", "w3", "b3", "out_cols", "vw1", "vb1", "vw2", "vb2", "vw3", "vb3"]
    lines = ['  printf("%s %%zu\\n", offsetof(pgd_actor_critic, %s));' % (n, n) for n in fields]
    prog = "#include <stdio.h>\n#include <stddef.h>\n#include \"pgdrive_hip.h\"\nint main(void) {\n" + "\n".join(lines) + \
        '\n  printf("sizeof %zu\\n", sizeof(pgd_actor_critic));\n  printf("det %u\\n", PGD_AC_DETERMINISTIC);\n  return 0;\n}\n'
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "a.c")
        open(c, "w").write(prog)
        exe = os.path.join(td, "a")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        out = dict(line.split() for line in subprocess.check_output([exe]).decode().strip().splitlines())
    for n in fields:
        assert int(out[n]) == getattr(_abi.ActorCritic, n).offset, n
    assert int(out["sizeof"]) == C.sizeof(_abi.ActorCritic) == 104
    assert int(out["det"]) == _abi.AC_DETERMINISTIC == 1
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pgdrive_hip.h")).read(), flags=re.S)
    for fn in ("pgd_mlp_actor_critic", "pgd_actor_critic_tick", "pgd_gae"):
        assert re.search(r"\bint\s+%s\s*\(" % fn, src), fn
        assert fn in engine.EXPORTS


def test_null_arguments_are_refused_without_a_gpu():
    from pgdrive_amd import engine
    L = engine.load_library()
    assert L.pgd_mlp_actor_critic(None, -1, None, 0, 0, None, 0, 0, 0, None, None, None) == 1
    assert L.pgd_gae(None, None, None, None, 1, 1, 0.99, 0.95, None, None) == 1
    assert L.pgd_actor_critic_tick(None, None) == 1


def test_the_collector_refuses_multi_agent_engines():
    import pgdrive_amd
    from pgdrive_amd.rollout import RolloutCollector
    assert pgdrive_amd.RolloutCollector is RolloutCollector
    with pytest.raises(NotImplementedError, match="single-agent"):
        RolloutCollector(types.SimpleNamespace(A=2), None, None, T=4)
    with pytest.raises(NotImplementedError, match="single-agent"):
        RolloutCollector(types.SimpleNamespace(engine=types.SimpleNamespace(A=40)), None, None, T=4)
