"""Top-down scene rendering on the host side: the film geometry of the reference's TopDownRenderer and the render() kwargs.

The reference's `BaseEnv.render(mode="top_down")` (envs/base_env.py:240-248, 463-468) draws the whole map and the agents with
pygame (obs/top_down_renderer.py).  Here the frames are drawn by the HIP kernels of pgdrive_amd/csrc/pgd_render.h; this module
restates what the host must hand them:

  bounding box   RoadNetwork.get_bounding_box() (component/road/road_network.py:105-118): the union over the roads of the box of
                 a few contour points of the road's outermost lanes, pushed 3 m (extra_lateral) beyond their outer edges
                 (utils/scene_utils.py:74-...): for a straight road the two ends (0.1 m in) of both outer edges; for a curved road
                 the same four points plus every quarter-turn point of the arc (the multiples of 90 degrees from the start phase
                 on, while they lie before the end phase) of both outer edges.
  film transform scaling = film_h / max(x extent, y extent) - 0.1 [px / m]; origin = box centre - (film_w / 2, film_h / 2) / scaling;
                 pos2pix(x, y) = (int((x - ox) * scaling), int((y - oy) * scaling)) = (column, row); no y flip
                 (top_down_renderer.py:31-36, obs/top_down_obs_impl.py:123-171).
"""
import math

# seaborn's "colorblind" palette as 8-bit values: PGD_RENDER_PALETTE of include/pgdrive_hip.h (tests/test_render_cpu.py compares)
PALETTE = ((1, 115, 178), (222, 143, 5), (2, 158, 115), (213, 94, 0), (204, 120, 188), (202, 145, 97), (251, 175, 228),
           (148, 148, 148), (236, 225, 51), (86, 180, 233))
TRAFFIC_RGB = (100, 200, 255)  # VehicleGraphics.BLUE (obs/top_down_obs_impl.py:199-206): IDM traffic with draw_traffic=True
OBJECT_RGB = (200, 0, 150)     # VehicleGraphics.PURPLE: traffic objects with draw_traffic=True
CONTOUR_RGB = (60, 60, 60)     # VehicleGraphics.BLACK: the outline of the newest frame
DEAD_RGB = (255, 0, 0)
EXTRA_LATERAL = 3.0            # get_road_bounding_box(lanes, extra_lateral=3)
COLOUR_KEY = 0x7e4d0c01        # the third key of an agent's colour hash (pgd_render.h)

MIN_FILM, MAX_FILM = 16, 16384  # film side limits of pgd_render_enable (a 16-pixel chunk spans at most two rows)
MAX_STACK = 64                  # frames of history per env
DEAD_CAP, MAX_OPS = 256, 2048   # RD_DEAD_CAP / RD_MAX_OPS of pgd_render.h

DEFAULTS = dict(film_size=(1000, 1000), num_stack=15, history_smooth=0, light_background=True, road_color=(255, 255, 255),
                draw_traffic=False)


def _road_lanes(desc):
    for r in desc["roads"]:
        if r["n_lanes"] > 0:
            yield desc["lanes"][r["first_lane"]:r["first_lane"] + r["n_lanes"]]


def _outline_points(lanes, extra):
    """The points get_road_bounding_box() boxes for one road: its two outer edges -- the left edge of the first lane and the right
    edge of the last lane, each `extra` metres further out -- at both ends (0.1 m in from the lane's ends), and, on a curved road, at
    the quarter-turn phases the edge sweeps (see _quarter_turns)."""
    from .mapdata import lane_position
    edges = ((lanes[0], -(lanes[0]["width"] / 2.0 + extra)), (lanes[-1], lanes[-1]["width"] / 2.0 + extra))  # (lane, lateral offset)
    pts = [lane_position(lane, s, lat) for lane, lat in edges for s in (0.1, lane["length"] - 0.1)]
    if lanes[0]["type"] == 1:  # a road is curved when its first lane is
        for lane, lat in edges:
            edge_r = lane["radius"] - lat * lane["direction"]  # CircularLane.position: the lateral offset shrinks the radius
            cx, cy = lane["center"]
            pts += [(cx + edge_r * math.cos(phi), cy + edge_r * math.sin(phi)) for phi in _quarter_turns(lane)]
    return pts


def _quarter_turns(lane):
    """The multiples of 90 degrees an arc passes, at most four, counted from its start phase in its direction of travel and kept
    while they do not lie past its end phase.  A counter-clockwise arc (direction +1) counts from the first multiple strictly
    above its start phase, a clockwise arc from the last multiple at or below it."""
    q, d = math.pi / 2.0, lane["direction"]
    first = int(math.floor(lane["start_phase"] / q)) + (1 if d == 1 else 0)
    out = []
    for k in range(4):
        phi = (first + d * k) * q
        if d * phi > d * lane["end_phase"]:
            break
        out.append(phi)
    return out


def bounding_box(desc):
    """(x_min, x_max, y_min, y_max) of the map's RoadNetwork, as get_bounding_box() returns it."""
    pts = [p for lanes in _road_lanes(desc) for p in _outline_points(lanes, EXTRA_LATERAL)]
    xs, ys = [p[0] for p in pts], [p[1] for p in pts]
    return min(xs), max(xs), min(ys), max(ys)


def film_geometry(desc, film_w, film_h):
    """(scaling [px / m], ox, oy [m]) of the film of `desc`: the row pgd_render_enable takes per map."""
    x0, x1, y0, y1 = bounding_box(desc)
    scaling = film_h / max(x1 - x0, y1 - y0) - 0.1
    return scaling, (x0 + x1) / 2.0 - 0.5 * film_w / scaling, (y0 + y1) / 2.0 - 0.5 * film_h / scaling


def pix(length, scaling):
    return int(length * scaling)


def pos2pix(x, y, geom):
    """(column, row) of a world point on the film whose geometry is (scaling, ox, oy)."""
    sc, ox, oy = geom
    return pix(x - ox, sc), pix(y - oy, sc)


def parse_kwargs(mode, kw):
    """The renderer's settings from the arguments of env.render(mode, **kw): a dict with the keys of DEFAULTS.
    As upstream (base_env.py:463-468) the first call creates the renderer; the caller ignores the kwargs of later calls."""
    if mode != "top_down":
        raise NotImplementedError("render(mode=%r): only mode='top_down' is built; the Panda3D window of use_render=True (onscreen / "
                                  "rgb_array rendering) is not" % (mode, ))
    kw = dict(kw)
    if kw.pop("track", False):
        raise NotImplementedError("render(track=True): following an agent is not built")
    if kw.pop("show_agent_name", False):
        raise NotImplementedError("render(show_agent_name=True): agent name labels are not built")
    if kw.pop("screen_size", None) is not None:
        raise NotImplementedError("render(screen_size=...): screen crops are not built (the whole film is returned)")
    kw.pop("zoomin", None)  # no effect on the reference's returned image (top_down_renderer.py:165-170)
    out = dict(DEFAULTS)
    for k in list(kw):
        if k not in DEFAULTS:
            raise TypeError("render(): unexpected keyword argument %r" % (k, ))
        out[k] = kw.pop(k)
    w, h = (int(v) for v in out["film_size"])
    if not (MIN_FILM <= w <= MAX_FILM and MIN_FILM <= h <= MAX_FILM):
        raise ValueError("render(film_size=%r): each side must be %d .. %d pixels" % ((w, h), MIN_FILM, MAX_FILM))
    out["film_size"] = (w, h)
    out["road_color"] = tuple(int(c) for c in out["road_color"])
    if len(out["road_color"]) != 3 or not all(0 <= c <= 255 for c in out["road_color"]):
        raise ValueError("render(road_color=%r): three values in 0 .. 255" % (out["road_color"], ))
    out["num_stack"], out["history_smooth"] = int(out["num_stack"]), int(out["history_smooth"])
    if not 1 <= out["num_stack"] <= MAX_STACK:
        raise ValueError("render(num_stack=%d): 1 .. %d frames" % (out["num_stack"], MAX_STACK))
    if out["history_smooth"] < 0:
        raise ValueError("render(history_smooth=%d): must be >= 0" % out["history_smooth"])
    out["light_background"], out["draw_traffic"] = bool(out["light_background"]), bool(out["draw_traffic"])
    return out


def check_capacity(num_stack, num_slots):
    """The frame kernel holds an env's draw list in LDS: num_stack x (vehicle slots) boxes + the dead list must fit MAX_OPS."""
    if num_stack * num_slots + DEAD_CAP > MAX_OPS:
        raise ValueError("render(num_stack=%d): with %d vehicle slots per env at most %d frames fit the draw list (%d ops)" % (
            num_stack, num_slots, (MAX_OPS - DEAD_CAP) // num_slots, MAX_OPS))


def make_config(settings):
    """pgd_render_config of parse_kwargs' settings."""
    from . import _abi
    c = _abi.RenderConfig()
    c.film_w, c.film_h = settings["film_size"]
    c.num_stack, c.history_smooth = settings["num_stack"], settings["history_smooth"]
    c.light_background, c.draw_traffic = int(settings["light_background"]), int(settings["draw_traffic"])
    for k in range(3):
        c.road_rgb[k] = settings["road_color"][k]
    return c


def _pcg(x):
    x &= 0xFFFFFFFF
    state = (x * 747796405 + 2891336453) & 0xFFFFFFFF
    word = (((state >> ((state >> 28) + 4)) ^ state) * 277803737) & 0xFFFFFFFF
    return ((word >> 22) ^ word) & 0xFFFFFFFF


def rng(seed, a, b, c):
    """pgd_rng (pgdrive_amd/csrc/pgd_device.h): the counter hash of the device RNG streams."""
    return _pcg(seed ^ _pcg(a ^ _pcg(b ^ _pcg((c + 0x9E3779B9) & 0xFFFFFFFF))))


def agent_colour(seed, env_global, agent_id):
    """Index into PALETTE of agent `agent_id` of the env with global index `env_global`."""
    return rng(seed & 0xFFFFFFFF, env_global & 0xFFFFFFFF, COLOUR_KEY, agent_id & 0xFFFFFFFF) % 10


def vec_render(venv, mode, env_ids, kw):
    """VecEnv.render: the first call creates the renderer from its kwargs, later calls ignore theirs (base_env.py:463-468)."""
    if getattr(venv, "_render_settings", None) is None:
        settings = parse_kwargs(mode, kw)
        venv.engine.enable_render(make_config(settings))
        venv._render_settings = settings
    else:
        parse_kwargs(mode, {})  # (the mode is checked at every call)
    return venv.engine.render_topdown(env_ids)
