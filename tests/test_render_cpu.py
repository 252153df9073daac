"""Top-down scene rendering, host side (no GPU): the film geometry against the reference's own bounding boxes, the pixel definition
of tests/render_ref.py on known answers, the palette against the header, and the render() argument rules."""
import json
import math
import os
import re

import numpy as np
import pytest

from pgdrive_amd import bank, render

from . import render_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "render_bbox_v0.json")))


def test_bounding_box_matches_the_reference_for_pgdrive_v0():
    descs = {d["seed"]: d for d in bank.load_descriptions()}
    assert len(GOLDEN["pg"]) == 100
    for seed, box in GOLDEN["pg"].items():
        got = render.bounding_box(descs[int(seed)])
        assert np.allclose(got, box, rtol=0, atol=1e-9), (seed, got, box)


def test_bounding_box_matches_the_reference_for_the_multi_agent_maps():
    from pgdrive_amd import marl_env
    envs = dict(roundabout=marl_env.MultiAgentRoundaboutVecEnv, intersection=marl_env.MultiAgentIntersectionVecEnv,
                bottleneck=marl_env.MultiAgentBottleneckVecEnv, tollgate=marl_env.MultiAgentTollgateVecEnv,
                parking_lot=marl_env.MultiAgentParkingLotVecEnv)
    assert set(GOLDEN["ma"]) == set(envs)
    for name, cls in envs.items():
        desc = cls._generate_map(cls.DEFAULTS["map_config"])
        got = render.bounding_box(desc)
        assert np.allclose(got, GOLDEN["ma"][name], rtol=0, atol=1e-9), (name, got, GOLDEN["ma"][name])


def test_film_transform_hand_cases():
    # a straight road along x from 0 to 100 m, one lane 4 m wide: contour points 0.1 m in, 2 + 3 m out on both sides
    lane = dict(type=0, start=[0.0, 0.0], end=[100.0, 0.0], direction=[1.0, 0.0], heading=0.0, length=100.0, width=4.0)
    desc = dict(lanes=[lane], roads=[dict(first_lane=0, n_lanes=1)])
    assert render.bounding_box(desc) == pytest.approx((0.1, 99.9, -5.0, 5.0), abs=1e-12)
    sc, ox, oy = render.film_geometry(desc, 1000, 1000)
    assert sc == pytest.approx(1000 / 99.8 - 0.1)
    assert ox == pytest.approx(50.0 - 500 / sc) and oy == pytest.approx(0.0 - 500 / sc)
    # the box centre lands on the film centre; pix truncates toward zero; no y flip (row grows with y)
    assert render.pos2pix(50.0, 0.0, (sc, ox, oy)) == (int(500 / sc * sc), int(500 / sc * sc))
    assert render.pix(-0.5, 1.0) == 0 and render.pix(1.99, 1.0) == 1
    u0, v0 = render.pos2pix(50.0, 0.0, (2.0, 0.0, 0.0))
    u1, v1 = render.pos2pix(50.0, 10.0, (2.0, 0.0, 0.0))
    assert (u0, v0, u1, v1) == (100, 0, 100, 20)
    # a non-square film: scaling follows film_h, the origin centres both axes
    sc2, ox2, oy2 = render.film_geometry(desc, 800, 400)
    assert sc2 == pytest.approx(400 / 99.8 - 0.1) and ox2 == pytest.approx(50.0 - 400 / sc2) and oy2 == pytest.approx(-200 / sc2)


def test_film_transform_of_a_curved_road_includes_the_quarter_turn_points():
    d = 1
    lane = dict(type=1, center=[0.0, 0.0], radius=20.0, start_phase=-math.pi / 2, end_phase=0.3, direction=d, length=20.0 * (0.3 + math.pi / 2),
                width=4.0)
    desc = dict(lanes=[lane], roads=[dict(first_lane=0, n_lanes=1)])
    x0, x1, y0, y1 = render.bounding_box(desc)
    # the point at phase 0 of the outer edge (radius 20 + 5) is the rightmost point
    assert x1 == pytest.approx(25.0)
    assert y0 < -24.9 and x0 < 1.0 and y1 > 0


def _blank(W=40, H=30):
    return np.full((H, W, 3), 255, np.uint8), np.zeros((H, W), bool)


def test_one_vehicle_at_the_centre_with_heading_zero_is_its_pixel_rectangle():
    img, amb = _blank()
    b = dict(cu=20, cv=15, ax=1.0, ay=0.0, len=10, wid=4)
    render_ref.paint_box(img, amb, b, (1, 2, 3), contour=False)
    ys, xs = np.nonzero(np.any(img != 255, axis=-1))
    # |u + 0.5 - 20| <= 5 -> u in 15..24 ; |v + 0.5 - 15| <= 2 -> v in 13..16
    assert (xs.min(), xs.max(), ys.min(), ys.max()) == (15, 24, 13, 16)
    assert len(xs) == 10 * 4 and not amb.any()


def test_the_two_degree_snap():
    for th, snapped in ((math.radians(1.99), True), (-math.radians(1.999), True), (math.radians(2.01), False), (-0.5, False)):
        assert (abs(float(np.float32(th))) <= render_ref.SNAP) == snapped
    # a snapped box is drawn axis-aligned; 2.5 degrees already move pixels of a long box
    img, amb = _blank(60, 30)
    render_ref.paint_box(img, amb, dict(cu=30, cv=15, ax=1.0, ay=0.0, len=40, wid=4), (0, 0, 0), contour=False)
    img2, amb2 = _blank(60, 30)
    a = math.radians(2.5)
    render_ref.paint_box(img2, amb2, dict(cu=30, cv=15, ax=math.cos(a), ay=math.sin(a), len=40, wid=4), (0, 0, 0), contour=False)
    assert not np.array_equal(img, img2)


def test_the_contour_band():
    img, amb = _blank()
    render_ref.paint_box(img, amb, dict(cu=20, cv=15, ax=1.0, ay=0.0, len=12, wid=8), (10, 20, 30), contour=True)
    inner = np.all(img == (10, 20, 30), axis=-1)
    edge = np.all(img == render.CONTOUR_RGB, axis=-1)
    # box: u 14..25, v 11..18 (12 x 8); band: centres within 2 px of the edge -> the inner fill is u 16..23, v 13..16 (8 x 4)
    ys, xs = np.nonzero(inner)
    assert (xs.min(), xs.max(), ys.min(), ys.max()) == (16, 23, 13, 16) and inner.sum() == 32
    assert edge.sum() == 12 * 8 - 32


def test_the_fifteen_fade_colours():
    c = render.PALETTE[0]
    cols = [render_ref.fade(c, i, 15) for i in range(1, 16)]
    assert cols[-1] == (255, 255, 255)  # the oldest frame (i = n) is white
    assert render_ref.fade(c, 0, 15) == c
    for i, col in enumerate(cols, 1):
        assert col == tuple(int(x + (i / 15) * (255 - x)) for x in c)
    assert cols[0] == (17, 124, 183) and cols[6] == (119, 180, 213)  # 1 + 254 * 7 / 15 = 119.5, 115 + 140 * 7 / 15 = 180.3, ...
    assert all(a <= b for a, b in zip(cols[0], cols[1]))


def test_the_dead_disk():
    img, amb = _blank()
    render_ref.paint_disk(img, amb, 20, 15)
    red = np.all(img == (255, 0, 0), axis=-1)
    vv, uu = np.nonzero(red)
    assert np.all((uu + 0.5 - 20) ** 2 + (vv + 0.5 - 15) ** 2 <= 25) and red.sum() == 80  # the integer pairs (i + 0.5, j + 0.5) within radius 5


def test_palette_matches_the_header():
    src = open(os.path.join(ROOT, "include", "pgdrive_hip.h")).read()
    body = src[src.index("#define PGD_RENDER_PALETTE"):]
    body = body[:body.index("}}") + 2]
    nums = [int(x) for x in re.findall(r"\d+", body)]
    assert tuple(tuple(nums[k:k + 3]) for k in range(0, 30, 3)) == render.PALETTE


def test_agent_colour_hash_is_the_device_counter_hash():
    # pcg_hash(0) and a chained value computed by hand from pgd_device.h's definition
    assert render._pcg(0) == 129708002
    k = render.agent_colour(0, 0, 0)
    assert 0 <= k < 10 and k == render.rng(0, 0, render.COLOUR_KEY, 0) % 10
    assert len({render.agent_colour(0, e, a) for e in range(8) for a in range(8)}) == 10


def test_render_kwargs_accepted_and_refused():
    s = render.parse_kwargs("top_down", {})
    assert s == dict(render.DEFAULTS)
    s = render.parse_kwargs("top_down", dict(film_size=(200, 100), num_stack=3, history_smooth=2, light_background=False,
                                             road_color=(1, 2, 3), draw_traffic=True, zoomin=3.0))
    assert s["film_size"] == (200, 100) and s["num_stack"] == 3 and s["history_smooth"] == 2 and not s["light_background"]
    assert s["road_color"] == (1, 2, 3) and s["draw_traffic"]
    c = render.make_config(s)
    assert (c.film_w, c.film_h, c.num_stack, c.history_smooth, c.light_background, c.draw_traffic) == (200, 100, 3, 2, 0, 1)
    assert list(c.road_rgb) == [1, 2, 3]
    for kw, word in ((dict(track=True), "track"), (dict(show_agent_name=True), "show_agent_name"), (dict(screen_size=(10, 10)), "screen_size")):
        with pytest.raises(NotImplementedError, match=word):
            render.parse_kwargs("top_down", kw)
    with pytest.raises(TypeError):
        render.parse_kwargs("top_down", dict(colour="red"))
    for mode in ("human", "rgb_array", None):
        with pytest.raises(NotImplementedError, match="use_render"):
            render.parse_kwargs(mode, {})


def test_render_config_matches_the_c_struct():
    import ctypes as C
    import subprocess
    import tempfile
    from pgdrive_amd import _abi
    prog = '#include <stdio.h>\n#include "pgdrive_hip.h"\nint main(void) { printf("%zu\\n", sizeof(pgd_render_config)); return 0; }\n'
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "s.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(td, "s.c"), "-o", os.path.join(td, "s")])
        size = int(subprocess.check_output([os.path.join(td, "s")]).decode())
    assert size == C.sizeof(_abi.RenderConfig) == 36


def test_vec_env_render_refuses_other_modes_before_touching_the_gpu():
    from pgdrive_amd import env as env_mod, marl_env, vec_env
    for cls in (vec_env.PGDriveVecEnv, marl_env.MultiAgentRoundaboutVecEnv):
        obj = cls.__new__(cls)  # (no engine: the mode is refused first)
        with pytest.raises(NotImplementedError, match="use_render"):
            obj.render(mode="human")
    assert "top_down" in env_mod.PGDriveEnv.metadata["render.modes"]


def test_film_sizes_and_limits():
    # any film of 16 .. 16384 px a side, also those whose pixel count is no multiple of 16 (the kernel writes a partial last chunk)
    for size in ((250, 250), (750, 750), (1000, 1000), (16, 16), (333, 17)):
        assert render.parse_kwargs("top_down", dict(film_size=size))["film_size"] == size
    for size in ((8, 100), (100, 15), (20000, 100)):
        with pytest.raises(ValueError, match="film_size"):
            render.parse_kwargs("top_down", dict(film_size=size))
    for kw, word in ((dict(num_stack=0), "num_stack"), (dict(num_stack=65), "num_stack"), (dict(history_smooth=-1), "history_smooth"),
                     (dict(road_color=(0, 0, 256)), "road_color")):
        with pytest.raises(ValueError, match=word):
            render.parse_kwargs("top_down", kw)
    render.check_capacity(15, 64)  # 15 x 64 + 256 = 1216 draw ops
    render.check_capacity(44, 40)  # 1760 + 256 = 2016
    with pytest.raises(ValueError, match="num_stack"):
        render.check_capacity(48, 40)
