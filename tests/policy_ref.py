"""The checker of the policy kernels (pgdrive_amd/csrc/pgd_policy.h, lane_keep_action of pgd_device.h), in plain numpy:

* mlp_f64            numpy_expert.py:25-44 in float64 -- what tests/test_policy_gpu.py holds the device against;
* CASES / build_case the seeded cases of that module (weights, inputs, scalings), so that tests/test_policy_ref_cpu.py can run every
                     one of them without a GPU;
* emulate_exact / emulate_bf16
                     the two kernels' ARITHMETIC in numpy (f32 accumulation in k order; hi + lo bf16 split, round to nearest even,
                     the three products lo*hi + hi*lo + hi*hi; tanh as 1 - 2 / (exp(2x) + 1) in f32).  Not bit-exact to the device
                     (__expf, reciprocal division, the matrix instruction's internal order) and never compared with it: its purpose is
                     the half-tolerance rule of the CPU test -- a case whose arithmetic alone uses more than half of the tolerance is
                     re-scaled, the tolerance is not widened;
* the LDS formulas of the header restated (lds_bytes_*), from which the largest accepted in_dim is DERIVED;
* lane_keep_f64      the formula of include/pgdrive_hip.h in float64, with the counter hash restated (held against oracle.orc's
                     orc_rng by the CPU test).
"""
import numpy as np

TOL_EXACT = 2e-5   # pgd_mlp_policy against float64, per action (tests/test_env_gpu.py::test_mlp_policy_matches_the_numpy_expert)
TOL_BF16 = 1e-4    # pgd_mlp_policy_prepared (split bf16 operands), same test
TOL_LANE_KEEP = 1e-5
H = 256
CLAMP = 10.0       # mlp_tanh clamps its argument to +-10

WIDTHS = (4, 5, 6, 7, 8, 19, 31, 32, 33, 35, 63, 64, 65, 96, 127, 128, 129, 255, 256, 257, 274, 275, 288, 289, 319, 320, 321, 324, 352,
          392, 447, 448)
SCALINGS = ("unit", "normalised", "saturating")
# the weight scale `s` per scaling.  saturating: chosen on the CPU (emulation over the whole width sweep, tests/test_policy_ref_cpu.py):
#   s = 4    |pre-activation| > 5 for 9.3 % of the hidden units at in_dim 4 (too few), split bf16 4.0e-5
#   s = 5    14.7 % at the least saturated width, some beyond the clamp at every width, split bf16 4.0e-5 (half of TOL_BF16 is 5e-5)
#   s = 6    22 %, split bf16 5.7e-5: over half of the tolerance
SCALE = dict(unit=1.0, normalised=1.0, saturating=5.0)


def mlp_f64(x, weights, final_tanh):
    """pgdrive/examples/ppo_expert/numpy_expert.py:25-44 re-stated in float64: the action = the first two outputs."""
    w1, b1, w2, b2, w3, b3 = [np.asarray(w, dtype=np.float64) for w in weights]
    h = np.tanh(np.asarray(x, dtype=np.float64) @ w1 + b1)
    h = np.tanh(h @ w2 + b2)
    o = (h @ w3 + b3)[:, :2]
    return np.tanh(o) if final_tanh else o


def hidden_preact_f64(x, weights):
    """Pre-activations of both hidden layers in float64 [rows, 512] (what the saturating scaling is judged by)."""
    w1, b1, w2, b2 = [np.asarray(w, dtype=np.float64) for w in weights[:4]]
    p1 = np.asarray(x, dtype=np.float64) @ w1 + b1
    return np.concatenate([p1, np.tanh(p1) @ w2 + b2], axis=1)


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
def make_weights(rng, in_dim, s=1.0, out_cols=2, nan_unused=True):
    """Asymmetric random values everywhere: N(0, s / sqrt(in_dim)), N(0, s / 16) for the hidden layer and the head, biases N(0, 0.1).
    out_cols > 2: the unused columns of w3 / b3 hold NaN (they are never read)."""
    w3 = rng.normal(0, 1 / 16, size=(H, out_cols))
    b3 = rng.normal(0, 0.1, size=out_cols)
    if nan_unused:
        w3[:, 2:] = np.nan
        b3[2:] = np.nan
    w = [rng.normal(0, s / np.sqrt(in_dim), size=(in_dim, H)), rng.normal(0, 0.1, size=H), rng.normal(0, s / 16, size=(H, H)),
         rng.normal(0, 0.1, size=H), w3, b3]
    return [np.ascontiguousarray(v, dtype=np.float32) for v in w]


def make_inputs(rng, rows, in_dim, scaling, pad=None):
    """[rows, in_dim + pad] float32, distinct in every row and column, NaN in the padding columns (never read)."""
    pad = (3 + in_dim % 5) if pad is None else pad
    if scaling == "normalised":  # a caller that normalises its observations
        x = np.clip(rng.normal(0, 3, size=(rows, in_dim)), -10, 10)
    else:
        x = rng.uniform(0, 1, size=(rows, in_dim))
    out = np.full((rows, in_dim + pad), np.nan, dtype=np.float32)
    out[:, :in_dim] = x
    return out


def build_case(name, in_dim, rows, scaling="unit", out_cols=2, seed=0):
    """(x [rows, stride] float32 with NaN padding, weights as six float32 arrays); a pure function of its arguments."""
    import zlib
    rng = np.random.default_rng([zlib.crc32(name.encode()), in_dim, rows, SCALINGS.index(scaling), out_cols, seed])
    return make_inputs(rng, rows, in_dim, scaling), make_weights(rng, in_dim, SCALE[scaling], out_cols)


SWEEP_ROWS = 48
ROW_COUNTS = (1, 15, 16, 17, 33, 4099)
ROW_WIDTHS = (274, 392)  # one width for each form of the row prologue


def sweep_cases():
    """The width sweep: every width in every scaling; out_cols cycles through 2, 3, 4."""
    for i, k in enumerate(WIDTHS):
        for j, sc in enumerate(SCALINGS):
            yield dict(name="sweep", in_dim=k, rows=SWEEP_ROWS, scaling=sc, out_cols=2 + (i + j) % 3)


def row_cases():
    for n in ROW_COUNTS:
        for k in ROW_WIDTHS:
            yield dict(name="rows", in_dim=k, rows=n, scaling="unit", out_cols=2)


def other_cases():
    yield dict(name="boundary", in_dim=max_in_dim(), rows=20, scaling="unit", out_cols=2)
    yield dict(name="boundary", in_dim=max_in_dim(), rows=20, scaling="normalised", out_cols=3)
    for k in (35, 274, 392):
        yield dict(name="permute", in_dim=k, rows=40, scaling="normalised", out_cols=2)
    for rows in (8 * 8, 5 * 6):  # multi-agent engines: rows = N * A
        for k in (274, 392):
            yield dict(name="marl", in_dim=k, rows=rows, scaling="unit", out_cols=2)
    for oc in (3, 4):
        for k in (31, 274, 324):
            yield dict(name="out_cols", in_dim=k, rows=24, scaling="normalised", out_cols=oc)
    for seed in (0, 1):
        for k in (33, 275, 352):
            yield dict(name="prepared", in_dim=k, rows=24, scaling="unit", out_cols=2 + seed, seed=seed)


def all_cases():
    """Every case tests/test_policy_gpu.py evaluates on the device with weights and inputs of this module."""
    for gen in (sweep_cases, row_cases, other_cases):
        for c in gen():
            yield c


# ---------------------------------------------------------------------------------------------------------------------
# the kernels' arithmetic
# ---------------------------------------------------------------------------------------------------------------------
def _f32(x):
    return np.asarray(x, dtype=np.float32)


def tanh_f32(x):
    """mlp_tanh: 1 - 2 / (exp(2 clamp(x)) + 1), every step rounded to float32."""
    x = np.clip(_f32(x), np.float32(-CLAMP), np.float32(CLAMP))
    e = _f32(np.exp((np.float32(2.0) * x).astype(np.float64)))
    return _f32(np.float32(1.0) - _f32(np.float32(2.0) / _f32(e + np.float32(1.0))))


def _fma_chain(a, w):
    """acc[r, c] = fma(a[r, k], w[k, c], acc) for k = 0, 1, ... in float32 (the product of two floats is exact in float64)."""
    a64, w64 = a.astype(np.float64), w.astype(np.float64)
    acc = np.zeros((a.shape[0], w.shape[1]), dtype=np.float32)
    for k in range(a.shape[1]):
        acc = _f32(acc.astype(np.float64) + a64[:, k, None] * w64[None, k, :])
    return acc


def _head(h2, w3, b3, final_tanh):
    """32 dot products of 256 over eight lanes each (lane p takes k = p, p + 8, ...), then a butterfly sum; f32."""
    h64, w64 = h2.astype(np.float64), w3[:, :2].astype(np.float64)
    part = np.zeros((8, h2.shape[0], 2), dtype=np.float32)
    for k in range(H):
        part[k % 8] = _f32(part[k % 8].astype(np.float64) + h64[:, k, None] * w64[None, k, :])
    for d in (4, 2, 1):
        part = _f32(part + part[np.arange(8) ^ d])
    v = _f32(part[0] + _f32(b3[:2]))
    return tanh_f32(v) if final_tanh else v


def emulate_exact(x, weights, final_tanh):
    """k_mlp_policy: f32 fma chains in k order on the matrix cores, bias + tanh in f32."""
    w1, b1, w2, b2, w3, b3 = [_f32(w) for w in weights]
    h1 = tanh_f32(_f32(_fma_chain(_f32(x), w1) + b1))
    h2 = tanh_f32(_f32(_fma_chain(h1, w2) + b2))
    return _head(h2, w3, b3, final_tanh)


def bf16_rne(x):
    """float32 -> the nearest bf16 (ties to even), returned as float32 (mlp_bf16_rne; finite inputs)."""
    u = _f32(x).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) >> 16 << 16
    return (u & 0xffffffff).astype(np.uint32).view(np.float32)


def split_bf16(x):
    x = _f32(x)
    hi = bf16_rne(x)
    return hi, bf16_rne(_f32(x - hi))


def _layer_bf16(a, w):
    """Chunks of 32 in k order; per chunk the three matrix instructions aL*bH, aH*bL, aH*bH, each adding its 32 exact products to
    the f32 accumulator (summed here in float64, rounded once per instruction)."""
    aH, aL = [v.astype(np.float64) for v in split_bf16(a)]
    bH, bL = [v.astype(np.float64) for v in split_bf16(w)]
    acc = np.zeros((a.shape[0], w.shape[1]), dtype=np.float32)
    for c in range(0, a.shape[1], 32):
        s = slice(c, c + 32)
        for p, q in ((aL, bH), (aH, bL), (aH, bH)):
            acc = _f32(acc.astype(np.float64) + p[:, s] @ q[s])
    return acc


def emulate_bf16(x, weights, final_tanh):
    """k_mlp_policy_bf on weights split by k_mlp_prepare; the head in f32 on hi + lo of the second hidden layer."""
    w1, b1, w2, b2, w3, b3 = [_f32(w) for w in weights]
    h1 = tanh_f32(_f32(_layer_bf16(_f32(x), w1) + b1))
    h2 = tanh_f32(_f32(_layer_bf16(h1, w2) + b2))
    hi, lo = split_bf16(h2)
    return _head(_f32(hi + lo), w3, b3, final_tanh)


# ---------------------------------------------------------------------------------------------------------------------
# LDS use of the two kernels (pgd_policy.h: mlp_lds_bytes, mlp_bf_lds_bytes) and the acceptance limit that follows from it
# ---------------------------------------------------------------------------------------------------------------------
LDS_LIMIT = 65536      # the library refuses a launch that needs more
LDS_DEFAULT = 49152    # above this the launch first raises the kernel's dynamic LDS limit, once per engine and kernel form


def lds_bytes_exact(in_dim):  # X tile | H1 | H2 | the head's weights [2][256], f32
    kp = (in_dim + 3) & ~3
    xs = kp + ((2 - kp) % 32 + 32) % 32
    return 4 * (16 * (xs + 2 * (H + 2)) + 2 * H)


def lds_bytes_bf16(in_dim):  # hi and lo planes of X (padded to chunks of 32), H1, H2 as bf16, the head's weights as f32
    kp = 32 * ((in_dim + 31) // 32)
    return 2 * 16 * (2 * (kp + 8) + 4 * (H + 8)) + 4 * 2 * H


def max_in_dim():
    """The largest in_dim BOTH kernels accept: the header's 4096 cut down by the LDS a workgroup may have."""
    k = 4
    while k < 4096 and max(lds_bytes_exact(k + 1), lds_bytes_bf16(k + 1)) <= LDS_LIMIT:
        k += 1
    return k


# ---------------------------------------------------------------------------------------------------------------------
# the scripted lane-keeping policy (include/pgdrive_hip.h, pgd_lane_keep_actions)
# ---------------------------------------------------------------------------------------------------------------------
M32 = 0xffffffff


def pcg_hash(x):
    state = (x * 747796405 + 2891336453) & M32
    word = (((state >> ((state >> 28) + 4)) ^ state) * 277803737) & M32
    return ((word >> 22) ^ word) & M32


def pgd_rng(seed, a, b, c):
    """The device's counter hash (pgd_device.h, pgd_rng) restated; equals oracle/pgd_oracle.c's orc_rng."""
    return pcg_hash((seed & M32) ^ pcg_hash((a & M32) ^ pcg_hash((b & M32) ^ pcg_hash((c + 0x9e3779b9) & M32))))


def lane_keep_noise(seed, env_global, tick):
    """n1, n2 ~ U(-1, 1): the low and the high half-word of one draw of the counter RNG (seed, env, tick)."""
    r = pgd_rng(seed ^ 0x1a7e5eed, env_global, 0x900dcafe, tick)
    return (r & 0xffff) * 2.0 / 65535.0 - 1.0, (r >> 16) * 2.0 / 65535.0 - 1.0


def lane_keep_f64(obs, seed, env_base, tick, k_lat=1.0, k_head=2.0, v_target_kmh=30.0, noise=0.05):
    """steering = clip(k_lat * 18 * (o0 - o1) / 10 + k_head * (2 o2 - 1) + noise * n1, -1, 1)
    throttle = clip(0.3 * (v_target_kmh - v_kmh) + noise * n2, -1, 1), v_kmh = 81 o3 - 1 (state_obs.py:82); float64.
    Returns (actions [N, 2], unclipped [N, 2])."""
    o = np.asarray(obs, dtype=np.float64)
    n = np.array([lane_keep_noise(seed, env_base + e, tick) for e in range(o.shape[0])], dtype=np.float64).reshape(-1, 2)
    # (the float arguments reach the device as float32)
    k_lat, k_head, v_t, nz = [float(np.float32(v)) for v in (k_lat, k_head, v_target_kmh, noise)]
    st = k_lat * 18.0 * (o[:, 0] - o[:, 1]) / 10.0 + k_head * (2.0 * o[:, 2] - 1.0) + nz * n[:, 0]
    th = 0.3 * (v_t - (81.0 * o[:, 3] - 1.0)) + nz * n[:, 1]
    raw = np.stack([st, th], axis=1)
    return np.clip(raw, -1.0, 1.0), raw
