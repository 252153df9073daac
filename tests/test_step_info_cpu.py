"""Step info (include/pgdrive_hip.h pgd_step_info): what can be held without a GPU -- the ctypes mirror of the struct, the config
key of the vec env, and the literal a run-time step kernel is generated with."""
import ctypes as C
import os
import subprocess
import tempfile

from pgdrive_amd import _abi, jit, vec_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_step_info_struct_matches_c():
    """sizeof(pgd_step_info) and the offset of every field, from a tiny C program compiled against the header (the pattern of
    tests/test_abi.py), equal the ctypes struct."""
    names = [n for n, _ in _abi.StepInfo._fields_]
    lines = ['  printf("%%zu\\n", offsetof(pgd_step_info, %s));' % n for n in names]
    prog = "#include <stdio.h>\n#include <stddef.h>\n#include \"pgdrive_hip.h\"\nint main(void) {\n" \
           "  printf(\"%zu\\n\", sizeof(pgd_step_info));\n" + "\n".join(lines) + "\n  return 0;\n}\n"
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "s.c")
        open(c, "w").write(prog)
        exe = os.path.join(td, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        out = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    assert out[0] == C.sizeof(_abi.StepInfo) == 16 + 18 * C.sizeof(C.c_void_p)
    assert out[1:] == [getattr(_abi.StepInfo, n).offset for n in names]
    assert set(_abi.STEP_INFO_FIELDS) == set(names) - {"out_of_road_cost", "crash_vehicle_cost", "crash_object_cost", "pad", "final_obs"}


def test_step_info_is_a_config_key_of_the_vec_env():
    assert vec_env.DEFAULT_CONFIG["step_info"] is False
    c = vec_env.merge_config(vec_env.DEFAULT_CONFIG, dict(step_info=True, out_of_road_cost=2.0))
    assert c["step_info"] is True and c["out_of_road_cost"] == 2.0
    # not one of the reference's keys that are dropped or refused: it reaches merge_config as it is
    user = dict(step_info=True, use_render=False, debug=True)
    assert vec_env.strip_reference_only_keys(user) == dict(step_info=True)


def test_run_time_kernel_of_an_engine_with_step_info_never_resets():
    """Engine.specialise() on an engine with step info generates auto_reset as the literal 0 (k_step_info restarts the envs), whatever
    the engine's configuration says -- and another cache key than the plain engine's module."""
    cfg = _abi.make_config(64, num_lasers=72, num_traffic=12, auto_reset=1)
    geom = dict(zip(jit.GEOM, (64, 1, 12, 13, 90, 832, 1, 4, 0, 13, 0)))
    plain, info = jit.header_text(cfg, geom, False, True), jit.header_text(cfg, geom, False, True, step_info=True)
    assert "F(c.auto_reset, 1)" in plain and "F(c.auto_reset, 0)" not in plain
    assert "F(c.auto_reset, 0)" in info and "F(c.auto_reset, 1)" not in info
    assert plain.replace("F(c.auto_reset, 1)", "F(c.auto_reset, 0)") == info
