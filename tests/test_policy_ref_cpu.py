"""tests/policy_ref.py checked without a GPU: the emulated arithmetic of both policy kernels stays within HALF of the tolerance the GPU
test applies, for every case tests/test_policy_gpu.py uses (a case that does not is re-scaled, the tolerance is not widened); the
saturating scaling saturates; the derived acceptance limit; the counter hash restated in Python equals the oracle's."""
import numpy as np

from tests import policy_ref as pr


def _errors(case):
    x, w = pr.build_case(**case)
    xin = x[:, :case["in_dim"]]
    assert np.isfinite(xin).all() and np.isnan(x[:, case["in_dim"]:]).all() and x.shape[1] > case["in_dim"]
    worst = [0.0, 0.0]
    for ft in (False, True):
        want = pr.mlp_f64(xin, w, ft)
        assert np.isfinite(want).all()
        worst[0] = max(worst[0], float(np.abs(pr.emulate_exact(xin, w, ft) - want).max()))
        worst[1] = max(worst[1], float(np.abs(pr.emulate_bf16(xin, w, ft) - want).max()))
    return worst


def test_every_gpu_case_keeps_half_of_its_tolerance_in_emulation():
    cases = [c for c in pr.all_cases() if c["rows"] <= 64]  # (the 4099-row cases: same distribution, see the next test)
    assert len(cases) > 100
    worst = {}
    for c in cases:
        e = _errors(c)
        key = (c["name"], c["scaling"])
        worst[key] = np.maximum(worst.get(key, [0.0, 0.0]), e)
        assert e[0] <= 0.5 * pr.TOL_EXACT and e[1] <= 0.5 * pr.TOL_BF16, (c, e)
    for k in sorted(worst):
        print("emulation vs float64, %-9s %-10s: exact %.1e, split bf16 %.1e" % (k + tuple(worst[k])))


def test_the_largest_row_count_keeps_half_of_its_tolerance_in_emulation():
    for c in pr.row_cases():
        if c["rows"] > 64:
            e = _errors(c)
            assert e[0] <= 0.5 * pr.TOL_EXACT and e[1] <= 0.5 * pr.TOL_BF16, (c, e)


def test_saturating_cases_saturate_and_inputs_are_distinct():
    for c in pr.sweep_cases():
        x, w = pr.build_case(**c)
        xin = x[:, :c["in_dim"]]
        # distinct in every row and column: no two rows and no two columns alike, and hardly a value twice
        assert len(np.unique(xin, axis=0)) == xin.shape[0] and np.unique(xin, axis=1).shape[1] == xin.shape[1]
        assert len(np.unique(xin)) > 0.99 * xin.size
        if c["scaling"] == "normalised":
            assert xin.min() < -3.0 and xin.max() > 3.0 and np.abs(xin).max() <= 10.0
        if c["scaling"] == "saturating":
            p = np.abs(pr.hidden_preact_f64(xin, w))
            assert (p > 5.0).mean() > 0.1, (c, float((p > 5.0).mean()))
            assert (p > pr.CLAMP).any(), c
        assert np.isnan(w[4][:, 2:]).all() and np.isnan(w[5][2:]).all() and np.isfinite(w[4][:, :2]).all()


def test_cases_are_a_pure_function_of_their_arguments():
    c = dict(name="sweep", in_dim=33, rows=5, scaling="unit", out_cols=3)
    (x0, w0), (x1, w1) = pr.build_case(**c), pr.build_case(**c)
    assert np.array_equal(x0, x1, equal_nan=True) and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(w0, w1))
    x2, _ = pr.build_case(**dict(c, seed=1))
    assert not np.array_equal(x0, x2, equal_nan=True)


def test_bf16_split_rounds_to_nearest_even_and_carries_sixteen_bits():
    one = np.float32(1.0)
    # 1 + 2^-8 lies half way between the bf16 neighbours 1 and 1 + 2^-7: ties go to the even mantissa (1); 1 + 3 * 2^-8 goes up to 1 + 2^-6
    assert pr.bf16_rne(one + np.float32(2.0 ** -8)) == one
    assert pr.bf16_rne(one + np.float32(3 * 2.0 ** -8)) == one + np.float32(2.0 ** -6)
    x = np.random.default_rng(0).normal(0, 1, size=4096).astype(np.float32)
    hi, lo = pr.split_bf16(x)
    assert ((hi.view(np.uint32) & 0xffff) == 0).all() and ((lo.view(np.uint32) & 0xffff) == 0).all()
    assert (np.abs((hi.astype(np.float64) + lo) - x) <= np.abs(x) * 2.0 ** -16).all()


def test_tanh_emulation_saturates_and_matches_float64():
    x = np.linspace(-12, 12, 4801).astype(np.float32)
    assert np.abs(pr.tanh_f32(x) - np.tanh(x.astype(np.float64))).max() < 5e-7
    assert pr.tanh_f32(np.float32(50.0)) == 1.0 and pr.tanh_f32(np.float32(-50.0)) == -1.0


def test_acceptance_limit_follows_from_the_lds_formulas():
    k = pr.max_in_dim()
    assert k == 448
    assert (pr.lds_bytes_exact(448), pr.lds_bytes_exact(449)) == (63872, 65920)
    assert (pr.lds_bytes_bf16(448), pr.lds_bytes_bf16(449)) == (65024, 67072)
    # the width sweep crosses the line above which a launch first raises the kernel's LDS limit, in both directions
    over = [pr.lds_bytes_exact(w) > pr.LDS_DEFAULT for w in pr.WIDTHS], [pr.lds_bytes_bf16(w) > pr.LDS_DEFAULT for w in pr.WIDTHS]
    assert all(True in o and False in o for o in over)


def test_counter_hash_restated_in_python_equals_the_oracle():
    from oracle import orc
    L = orc.lib()
    rng = np.random.default_rng(1)
    args = rng.integers(0, 2 ** 32, size=(500, 4), dtype=np.uint64).tolist()
    args += [[0, 0, 0, 0], [pr.M32] * 4, [5 ^ 0x1a7e5eed, 77, 0x900dcafe, 2 ** 31], [1, 2, 3, pr.M32]]
    for s, a, b, c in args:
        assert pr.pgd_rng(s, a, b, c) == L.orc_rng(s, a, b, c), (s, a, b, c)


def test_lane_keep_reference_formula():
    o = np.array([[0.5, 0.5, 0.5, 31.0 / 81.0], [0.9, 0.1, 0.5, 0.0], [0.5, 0.5, 0.0, 1.0]])
    a, raw = pr.lane_keep_f64(o, seed=3, env_base=7, tick=0, noise=0.0)
    assert np.allclose(raw[0], [0.0, 0.0], atol=1e-12)           # centred, aligned, at the target speed
    assert np.allclose(raw[1], [1.8 * 0.8, 0.3 * 31.0], atol=1e-6) and (a[1] == [1.0, 1.0]).all()
    assert np.allclose(raw[2], [-2.0, 0.3 * (30.0 - 80.0)], atol=1e-6) and (a[2] == [-1.0, -1.0]).all()
    n = np.array([pr.lane_keep_noise(3, 7 + e, t) for e in range(64) for t in (0, 1, 2 ** 31, 2 ** 32 - 1)])
    assert (np.abs(n) <= 1.0).all() and (n[:, 0] != n[:, 1]).all() and len(np.unique(n)) > 500
