"""The GPU-free preparation behind the ABI entry points (pgdrive_amd/csrc/pgd_host_prep.h): launch geometry, the device forms of the map and
scenario tables, the state conversion.  tests/host_prep_main.cpp -- that header and a main(), nothing of HIP -- is built here with the host
compiler under the address and undefined-behaviour sanitizers and run as an ordinary child process over files of raw arrays; a sanitizer
report ends the child with a non-zero status and fails the test.  Expected values: tests/host_prep_ref.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from pgdrive_amd import _abi, mapdata, scenario
from tests import host_prep_ref as ref
from tests import util

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ["-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
OK, ERR_ARG = ref.OK, ref.ERR_ARG


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("host_prep") / "host_prep")
    cxx = [shutil.which("g++")] if shutil.which("g++") else [shutil.which("hipcc") or "/opt/rocm/bin/hipcc", "-x", "c++"]
    subprocess.check_call(cxx + FLAGS + ["-o", exe, os.path.join(HERE, "host_prep_main.cpp")])
    return exe


def run(prog, *args):
    """The child's stdout as a dict; exit status 0 or the test fails with what the child (or a sanitizer) wrote."""
    p = subprocess.run([prog] + [str(a) for a in args], capture_output=True, text=True)
    assert p.returncode == 0, "%s %s: exit status %d\n%s" % (os.path.basename(prog), args[0], p.returncode, p.stderr[-4000:])
    return dict(line.split(None, 1) for line in p.stdout.splitlines())


# ---------------------------------------------------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------------------------------------------------
def geometry(prog, tmp, cases):
    """cases: (PgdConfig, pack, imask) -> (rc, dict of the geometry)"""
    rec = np.zeros(len(cases), dtype=ref.GEOMETRY_IN_DT)
    for k, (cfg, pack, imask) in enumerate(cases):
        rec[k] = (np.frombuffer(bytes(cfg), dtype=np.uint8), pack, imask)
    rec.tofile(tmp / "geom.in")
    run(prog, "geometry", tmp / "geom.in", tmp / "geom.out")
    out = np.fromfile(tmp / "geom.out", dtype=ref.GEOMETRY_OUT_DT)
    assert len(out) == len(cases)
    return [(int(o["rc"]), {k: int(o["g"][k]) for k in ref.GEOM}) for o in out]


def marl_cfg(n, seats, **kw):
    return _abi.make_config(n, num_agents=seats, num_traffic=0, num_lasers=72, num_others=0, multi_agent=True, horizon=1000, **kw)


ONE_ENV = dict(V=17, D=274, sstride=17, sub=3, epw=1, pack_obs=0, use_imask=0)
PACKED = dict(V=17, D=274, sstride=17, sub=1, epw=3, pack_obs=1, use_imask=1)
GEOMETRY_CASES = [
    # name, config, PGD_PACK, PGD_IMASK (-1: not forced), expected
    ("1 + 16, 4096 envs", lambda: _abi.make_config(4096), -1, -1, dict(ONE_ENV, NV=4096 * 17)),
    ("1 + 16, 32768 envs", lambda: _abi.make_config(32768), -1, -1, dict(PACKED, NV=32768 * 17)),
    ("32768 envs, PGD_PACK=0", lambda: _abi.make_config(32768), 0, -1, dict(ONE_ENV, NV=32768 * 17)),
    ("4096 envs, PGD_PACK=1", lambda: _abi.make_config(4096), 1, -1, dict(PACKED, NV=4096 * 17)),
    ("4096 envs, PGD_IMASK", lambda: _abi.make_config(4096), -1, 1, dict(ONE_ENV, NV=4096 * 17, use_imask=1)),
    ("4096 envs, PGD_NO_IMASK", lambda: _abi.make_config(4096), -1, 0, dict(ONE_ENV, NV=4096 * 17)),
    ("32768 envs, PGD_IMASK", lambda: _abi.make_config(32768), -1, 1, dict(PACKED, NV=32768 * 17)),
    ("32768 envs, PGD_NO_IMASK", lambda: _abi.make_config(32768), -1, 0, dict(PACKED, NV=32768 * 17, use_imask=0)),
    ("1 + 0, no lidar", lambda: _abi.make_config(4096, num_traffic=0, num_lasers=0), -1, -1,
     dict(V=1, D=18, NV=4096, sstride=1, sub=16, epw=4, pack_obs=0, use_imask=0)),
    ("1 + 0, no lidar, 32768 envs, PGD_PACK=1", lambda: _abi.make_config(32768, num_traffic=0, num_lasers=0), 1, -1,
     dict(V=1, D=18, NV=32768, sstride=1, sub=16, epw=4, pack_obs=0, use_imask=0)),
    ("1 + 30", lambda: _abi.make_config(4096, num_traffic=30), -1, -1, dict(V=31, D=274, NV=4096 * 31, sstride=31, sub=2, epw=1, pack_obs=0, use_imask=0)),
    ("1 + 30, 32768 envs, PGD_PACK=1 (62 lanes > 52)", lambda: _abi.make_config(32768, num_traffic=30), 1, -1,
     dict(V=31, D=274, NV=32768 * 31, sstride=31, sub=2, epw=1, pack_obs=0, use_imask=0)),
    ("multi-agent, 8 seats", lambda: marl_cfg(64, 8), -1, -1, dict(V=8, D=90, NV=512, sstride=8, sub=8, epw=1, pack_obs=0, use_imask=0)),
    ("multi-agent, 8 seats, 32768 envs, PGD_PACK=1", lambda: marl_cfg(32768, 8), 1, -1,
     dict(V=8, D=90, NV=32768 * 8, sstride=8, sub=8, epw=1, pack_obs=0, use_imask=0)),
    ("multi-agent, 40 seats, 4 x 3 respawn records", lambda: marl_cfg(64, 40, respawn_places=4, respawn_dests=3), -1, -1,
     dict(V=40, D=90, NV=2560, sstride=52, sub=1, epw=1, pack_obs=0, use_imask=0)),
]


def test_geometry_of_the_engine_modes(prog, tmp_path):
    got = geometry(prog, tmp_path, [(make(), pack, imask) for _, make, pack, imask, _ in GEOMETRY_CASES])
    for (name, _, _, _, want), (rc, g) in zip(GEOMETRY_CASES, got):
        assert rc == OK, name
        assert g == want, name


def _edit(cfg, **fields):
    for k, v in fields.items():
        setattr(cfg, k, v)
    return cfg


REFUSED_CONFIGS = [
    ("no envs", lambda: _abi.make_config(0)),
    ("no agents", lambda: _edit(_abi.make_config(4), num_agents=0)),
    ("65 slots", lambda: _abi.make_config(4, num_traffic=64)),
    ("17 neighbour rows", lambda: _abi.make_config(4, num_others=17)),
    ("a negative beam count", lambda: _edit(_abi.make_config(4), num_lasers=-1)),
    ("multi-agent, respawn_places -1", lambda: marl_cfg(4, 8, respawn_places=-1, respawn_dests=1)),
    ("multi-agent, respawn_places 65", lambda: marl_cfg(4, 8, respawn_places=65, respawn_dests=1)),
    ("multi-agent, respawn_dests -1", lambda: marl_cfg(4, 8, respawn_places=1, respawn_dests=-1)),
    ("idm_agent on a multi-agent engine", lambda: _edit(marl_cfg(4, 1), idm_agent=1)),
    ("idm_agent with two agents", lambda: _abi.make_config(4, num_agents=2, idm_agent=True)),
    ("multi-agent, horizon 0x8000", lambda: _edit(marl_cfg(4, 8), horizon=0x8000)),
]
ACCEPTED_AT_THE_LIMIT = [
    ("64 slots", lambda: _abi.make_config(4, num_traffic=63)),
    ("16 neighbour rows", lambda: _abi.make_config(4, num_others=16)),
    ("multi-agent, respawn_places 64", lambda: marl_cfg(4, 8, respawn_places=64, respawn_dests=1)),
    ("multi-agent, horizon 0x7fff", lambda: _edit(marl_cfg(4, 8), horizon=0x7fff)),
    ("single agent, horizon 0x8000", lambda: _abi.make_config(4, horizon=0x8000)),
    ("idm_agent, one agent", lambda: _abi.make_config(4, idm_agent=True)),
]


def test_every_refusal_of_pgd_create_on_its_own_config(prog, tmp_path):
    got = geometry(prog, tmp_path, [(make(), -1, -1) for _, make in REFUSED_CONFIGS + ACCEPTED_AT_THE_LIMIT])
    for (name, _), (rc, _) in zip(REFUSED_CONFIGS + ACCEPTED_AT_THE_LIMIT, got):
        assert rc == (ERR_ARG if any(name == n for n, _ in REFUSED_CONFIGS) else OK), name


def test_the_library_refuses_a_config_before_it_looks_for_a_device():
    """pgd_create holds its configuration refusals in front of its first HIP call: PGD_ERR_ARG with or without a GPU."""
    from pgdrive_amd import build, engine
    build.build()
    L = engine.load_library()
    h = C.c_void_p()
    for name, make in REFUSED_CONFIGS:
        cfg = make()
        assert L.pgd_create(C.byref(cfg), 0, None, C.byref(h)) == ERR_ARG, name
        assert not h.value


def test_regrouping(prog, tmp_path):
    def geom(**kw):
        return tuple(kw[k] for k in ref.GEOM)
    packed = geom(NV=0, **PACKED)
    ego = geom(V=1, D=18, NV=8, sstride=1, sub=16, epw=4, pack_obs=0, use_imask=0)
    cases = [  # geometry, N, n_groups, PGD_IMASK -> rc, the geometry fields that change, left throughput mode
        (packed, 32768, 4, -1, OK, dict(sub=3, epw=1, pack_obs=0, use_imask=0), 1),
        (packed, 49152, 4, -1, OK, {}, 0),
        (packed, 32768, 4, 1, OK, dict(sub=3, epw=1, pack_obs=0), 1),  # (a forced mask stays)
        (packed, 32768, 1, -1, OK, dict(sub=3, epw=1, pack_obs=0, use_imask=0), 1),  # (one group is no whole number of three-env waves either)
        (ego, 8, 4, -1, ERR_ARG, {}, 0),
        (ego, 8, 2, -1, OK, {}, 0),
        (packed, 32768, 3, -1, ERR_ARG, {}, 0),  # N % n_groups != 0
        (packed, 49152, 0, -1, ERR_ARG, {}, 0),
        (packed, 49152, 65, -1, ERR_ARG, {}, 0),
        (packed, 49152, 64, -1, OK, {}, 0),
    ]
    rec = np.zeros(len(cases), dtype=ref.REGROUP_IN_DT)
    for k, (g, n, groups, imask, _, _, _) in enumerate(cases):
        rec[k] = (g, n, groups, imask)
    rec.tofile(tmp_path / "regroup.in")
    run(prog, "regroup", tmp_path / "regroup.in", tmp_path / "regroup.out")
    out = np.fromfile(tmp_path / "regroup.out", dtype=ref.REGROUP_OUT_DT)
    for (g, n, groups, imask, rc, change, left), o in zip(cases, out):
        what = "N=%d groups=%d imask=%d" % (n, groups, imask)
        assert int(o["rc"]) == rc and int(o["left"]) == left, what
        want = dict(zip(ref.GEOM, g), **change)  # (a refusal returns the input geometry untouched)
        assert {k: int(o["g"][k]) for k in ref.GEOM} == want, what


# ---------------------------------------------------------------------------------------------------------------------
# map tables
# ---------------------------------------------------------------------------------------------------------------------
class Bank:
    """The six arrays of pgd_upload_maps."""
    NAMES = ("maps", "lanes", "roads", "boxes", "cell_start", "cell_items")

    def __init__(self, mb):
        for k in self.NAMES:
            setattr(self, k, np.array(getattr(mb, k)))


def map_tables(prog, tmp, bank, nulls=0):
    for k in Bank.NAMES:
        getattr(bank, k).tofile(tmp / k)
    out = run(prog, "maps", *[tmp / k for k in Bank.NAMES], nulls, tmp / "out")
    if int(out["rc"]) != OK:
        return int(out["rc"]), None
    read = dict(lanes=mapdata.LANE_DT, nav=ref.LANE_NAV_DT, cbox=mapdata.BOX_DT, cext=ref.LANE_EXT_DT, cs=np.int32)
    return OK, {k: np.fromfile(str(tmp / "out") + "." + k, dtype=dt) for k, dt in read.items()}


@pytest.fixture(scope="module", params=["two generated maps", "multi-agent roundabout"])
def tables(request, prog, descs, tmp_path_factory):
    mb = util.make_banks(descs, n_maps=2)[0] if request.param.startswith("two") else util.make_marl_banks()[1]
    bank = Bank(mb)
    rc, out = map_tables(prog, tmp_path_factory.mktemp("maps"), bank)
    assert rc == OK
    return bank, out


def _lanes_of(bank, m):
    return slice(int(m["lane_off"]), int(m["lane_off"]) + int(m["n_lanes"]))


def test_lane_table_keeps_everything_but_the_device_private_fields(tables):
    bank, out = tables
    assert len(out["lanes"]) == len(bank.lanes)
    for k in mapdata.LANE_DT.names:
        if k not in ("ex", "ey", "pad"):
            assert np.array_equal(out["lanes"][k], bank.lanes[k]), k


def test_related_lanes_mask(tables):
    bank, out = tables
    for m in bank.maps:
        got = out["lanes"]["ey"][_lanes_of(bank, m)].view(np.uint32)
        assert np.array_equal(got, ref.related_lanes(bank.lanes[_lanes_of(bank, m)]))


def test_pad_is_the_from_node_of_the_lanes_road(tables):
    bank, out = tables
    for m in bank.maps:
        L = bank.lanes[_lanes_of(bank, m)]
        assert np.array_equal(out["lanes"]["pad"][_lanes_of(bank, m)], bank.roads["frm"][int(m["road_off"]) + L["road"]])


def test_strip_width(tables):
    bank, out = tables
    n_strips = 0
    for m in bank.maps:
        boxes = bank.boxes[int(m["box_off"]):int(m["box_off"]) + int(m["n_boxes"])]
        L = bank.lanes[_lanes_of(bank, m)]
        want = np.array([ref.strip_width(lane, boxes) for lane in L], dtype=np.float32)
        got = out["lanes"]["ex"][_lanes_of(bank, m)]
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.flatnonzero(got != want)[:8]
        assert (got[L["dir"] != 0.0] == 0.0).all()
        n_strips += int((got > 0.0).sum())
    assert n_strips > 0  # (the banks have straight lanes with a free strip: the comparison above is not one of zeros)


def test_lane_nav(tables):
    bank, out = tables
    want, got = ref.lane_nav(bank.lanes), out["nav"]
    st = bank.lanes["dir"] == 0.0
    assert st.any() and (~st).any()
    for k in ref.LANE_NAV_DT.names:  # straight lanes, and everything but the cos / sin products on arcs: equal
        rows = st if k in ("ex", "ey", "nx", "ny") else np.ones(len(st), dtype=bool)
        assert np.array_equal(got[k][rows].view(np.uint32), want[k][rows].view(np.uint32)), k
    assert (got["radius"][st] == 0.0).all() and (got["dir"][st] == 0.0).all() and (got["angle"][st] == 0.0).all()
    for k in ("ex", "ey", "nx", "ny"):  # arcs: libm and numpy may differ in the last bit of cos / sin, nothing else may
        assert (np.abs(got[k][~st].astype(np.float64) - want[k][~st].astype(np.float64)) <= np.spacing(np.abs(want[k][~st]))).all(), k


def test_cell_major_boxes(tables):
    bank, out = tables
    assert len(out["cs"]) == len(bank.cell_start) and len(out["cbox"]) == len(bank.cell_items)
    n_lane_boxes = 0
    for m in bank.maps:
        cb, cx, packed = ref.cell_major(m, bank.lanes, bank.boxes, bank.cell_start, bank.cell_items)
        items = slice(int(m["item_off"]), int(m["item_off"]) + len(cb))
        cells = slice(int(m["cell_off"]), int(m["cell_off"]) + len(packed))
        assert out["cbox"][items].tobytes() == cb.tobytes()
        assert out["cext"][items].tobytes() == cx.tobytes()
        assert np.array_equal(out["cs"][cells], packed)
        n_lane_boxes += int((packed[:-1] >> 24).sum())
    assert n_lane_boxes > 0


def tiny_bank():
    """One map of one road, one straight lane, one cell: a lane box and a line box."""
    b = Bank.__new__(Bank)
    b.maps = np.zeros(1, dtype=mapdata.MAP_DT)
    b.maps[0] = (0, 1, 0, 1, 0, 2, 0, 0, 1, 1, 0.0, 0.0, 8.0, 3.5, (0, 0))
    b.lanes = np.zeros(1, dtype=mapdata.LANE_DT)
    b.lanes[0] = (0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 8.0, 3.5, 8.0, 0.0, 0, 0, 0, 0, (-1, ) * mapdata.MAX_SUCC)
    b.roads = np.zeros(1, dtype=mapdata.ROAD_DT)
    b.roads[0] = (3, 4, 0, 1, 0, ord("a"), 1, 0, 0)
    b.boxes = np.zeros(2, dtype=mapdata.BOX_DT)
    b.boxes[0] = (4.0, 0.0, 1.0, 0.0, 4.0, 1.75, mapdata.BOX_LANE, 0)
    b.boxes[1] = (4.0, 1.75, 1.0, 0.0, 4.0, 0.05, mapdata.BOX_WHITE, -1)
    b.cell_start = np.array([0, 2], dtype=np.int32)
    b.cell_items = np.array([0, 1], dtype=np.int32)
    return b


def test_tiny_bank_is_taken(prog, tmp_path):
    rc, out = map_tables(prog, tmp_path, tiny_bank())
    assert rc == OK
    assert out["lanes"]["pad"][0] == 3 and out["lanes"]["ey"].view(np.uint32)[0] == 1
    b = tiny_bank()  # the line's near edge, 1.75 - 0.05 m from the axis, less 3 cm
    assert out["lanes"]["ex"][0] == ref.strip_width(b.lanes[0], b.boxes) == np.float32(np.float64(np.float32(1.75)) - np.float64(np.float32(0.05)) - 0.03)
    assert out["cs"].tolist() == [1 << 24, 2]


def _set(name, index, field, value):
    def edit(b):
        a = getattr(b, name)
        (a if field is None else a[field])[index] = value
    return edit


def _grow(name, n):
    def edit(b):
        setattr(b, name, np.repeat(getattr(b, name)[:1], n))
        b.maps[0]["n_" + name] = n
    return edit


def _many_lane_boxes(b):
    b.boxes = np.repeat(b.boxes[:1], 256)
    b.maps[0]["n_boxes"] = 256
    b.cell_items = np.arange(256, dtype=np.int32)
    b.cell_start = np.array([0, 256], dtype=np.int32)


def _many_items(b):
    b.cell_items = np.zeros(1 << 24, dtype=np.int32)
    b.cell_start = np.array([0, 1 << 24], dtype=np.int32)


MAP_REFUSALS = [  # the refusals pgd_upload_maps always had ...
    ("4096 roads", _grow("roads", 4096)),
    ("65536 lanes", _grow("lanes", 65536)),
    ("a lane of road 1 of 1", _set("lanes", 0, "road", 1)),
    ("a lane of road -1", _set("lanes", 0, "road", -1)),
    ("first_lane + index != k", _set("lanes", 0, "index", 1)),
    ("2^24 items", _many_items),
    ("256 lane boxes in a cell", _many_lane_boxes),
    ("a lane box of lane 1 of 1", _set("boxes", 0, "lane", 1)),
    ("a lane box of lane -1", _set("boxes", 0, "lane", -1)),
    # ... and the ones that keep every index inside the array it indexes
    ("lane_off one past", _set("maps", 0, "lane_off", 1)),
    ("n_lanes one past", _set("maps", 0, "n_lanes", 2)),
    ("lane_off negative", _set("maps", 0, "lane_off", -1)),
    ("road_off one past", _set("maps", 0, "road_off", 1)),
    ("n_roads one past", _set("maps", 0, "n_roads", 2)),
    ("road_off negative", _set("maps", 0, "road_off", -1)),
    ("box_off one past", _set("maps", 0, "box_off", 1)),
    ("n_boxes one past", _set("maps", 0, "n_boxes", 3)),
    ("box_off negative", _set("maps", 0, "box_off", -1)),
    ("cell_off one past", _set("maps", 0, "cell_off", 1)),
    ("cells one past", _set("maps", 0, "gx", 2)),
    ("cell_off negative", _set("maps", 0, "cell_off", -1)),
    ("a negative grid size", _set("maps", 0, "gy", -1)),
    ("item_off one past", _set("maps", 0, "item_off", 1)),
    ("items one past", _set("cell_start", 1, None, 3)),
    ("item_off negative", _set("maps", 0, "item_off", -1)),
    ("a cell that starts before 0", _set("cell_start", 0, None, -1)),
    ("a cell that ends before it starts", _set("cell_start", 0, None, 3)),
    ("a cell item one past the map's boxes", _set("cell_items", 1, None, 2)),
    ("a negative cell item", _set("cell_items", 1, None, -1)),
] + [("null " + name, k) for k, name in enumerate(Bank.NAMES)]


@pytest.mark.parametrize("name,edit", MAP_REFUSALS, ids=[n for n, _ in MAP_REFUSALS])
def test_malformed_map_bank_is_refused_without_a_read_out_of_bounds(prog, tmp_path, name, edit):
    b = tiny_bank()
    nulls = 0
    if callable(edit):
        edit(b)
    else:
        nulls = 1 << edit
    rc, _ = map_tables(prog, tmp_path, b, nulls)
    assert rc == ERR_ARG


# ---------------------------------------------------------------------------------------------------------------------
# scenario tables
# ---------------------------------------------------------------------------------------------------------------------
def tiny_scenarios():
    """2 scenarios x 3 slots: slots 0 and 1 used (one body size), slot 2 unused."""
    scen = np.zeros(2, dtype=scenario.SCEN_DT)
    sp = np.zeros(6, dtype=scenario.SPAWN_DT)
    sp["length"], sp["width"], sp["max_steer"] = 4.5, 1.8, 0.7
    sp["lane"] = [0, 1, -1, 2, 0, -1]
    sp["n_ckpt"] = [5, 1, 0, 32, 2, 7]
    sp["ckpt"] = np.arange(6 * mapdata.MAX_CKPT).reshape(6, -1) % 50
    sp["ckpt_road"] = 3
    return scen, sp


def scenario_tables(prog, tmp, scen, sp, sstride=3, no_uni=0):
    scen.tofile(tmp / "scen")
    sp.tofile(tmp / "spawns")
    out = run(prog, "scen", tmp / "scen", tmp / "spawns", sstride, no_uni, tmp / "out")
    if int(out["rc"]) != OK:
        return int(out["rc"]), None, None
    flags = (bool(int(out["has_objects"])), int(out["no_groups"]), float.fromhex(out["uni_len"]), float.fromhex(out["uni_wid"]))
    return OK, flags, np.fromfile(str(tmp / "out") + ".spawns", dtype=scenario.SPAWN_DT)


def test_route_end_marks(prog, tmp_path):
    scen, sp = tiny_scenarios()
    rc, flags, dev = scenario_tables(prog, tmp_path, scen, sp)
    assert rc == OK
    for q, d in zip(sp, dev):
        first = max(int(q["n_ckpt"]) - 1, 0)
        assert (d["ckpt"][first:] == ref.CKPT_END).all() and np.array_equal(d["ckpt"][:first], q["ckpt"][:first])
    want = ref.spawn_marks(sp)
    assert dev.tobytes() == want.tobytes()  # (nothing else of a record moves)
    assert flags == ref.scenario_flags(scen, sp) == (False, 1, float(np.float32(4.5)), float(np.float32(1.8)))


def test_scenario_flags(prog, tmp_path):
    def flags(edit, **kw):
        scen, sp = tiny_scenarios()
        edit(scen, sp)
        rc, got, _ = scenario_tables(prog, tmp_path, scen, sp, **kw)
        assert rc == OK and got == ref.scenario_flags(scen, sp, no_uni=bool(kw.get("no_uni")))
        return got
    ul, uw = float(np.float32(4.5)), float(np.float32(1.8))
    assert flags(lambda scen, sp: None) == (False, 1, ul, uw)
    # a traffic object in a used slot selects the OBJ kernels (and ends the one body size); in an unused slot it is nothing
    assert flags(lambda scen, sp: sp["kind"].__setitem__(4, 1)) == (True, 1, 0.0, 0.0)
    assert flags(lambda scen, sp: sp["kind"].__setitem__(5, 1)) == (False, 1, ul, uw)
    assert flags(lambda scen, sp: scen["n_groups"].__setitem__(1, 1)) == (False, 0, ul, uw)
    # one body size: every used slot, and a positive one
    assert flags(lambda scen, sp: sp["length"].__setitem__(3, 4.25)) == (False, 1, 0.0, 0.0)
    assert flags(lambda scen, sp: sp["width"].__setitem__(0, 1.7)) == (False, 1, 0.0, 0.0)
    assert flags(lambda scen, sp: sp["length"].__setitem__(2, 9.0)) == (False, 1, ul, uw)  # (an unused slot)
    assert flags(lambda scen, sp: sp["width"].__setitem__(slice(None), 0.0)) == (False, 1, 0.0, 0.0)
    assert flags(lambda scen, sp: None, no_uni=1) == (False, 1, 0.0, 0.0)


@pytest.mark.parametrize("field,value", [("max_steer", 1.5), ("max_steer", float("nan")), ("n_ckpt", 33)])
def test_scenario_refusals_look_at_used_slots_only(prog, tmp_path, field, value):
    scen, sp = tiny_scenarios()
    sp[field][2] = value  # an unused slot
    assert scenario_tables(prog, tmp_path, scen, sp)[0] == OK
    sp[field][4] = value
    assert scenario_tables(prog, tmp_path, scen, sp)[0] == ERR_ARG
    scen, sp = tiny_scenarios()
    sp["max_steer"][:] = 1.0  # (the limit itself is taken)
    assert scenario_tables(prog, tmp_path, scen, sp)[0] == OK


# ---------------------------------------------------------------------------------------------------------------------
# state conversion
# ---------------------------------------------------------------------------------------------------------------------
N, V = 2, 3
INT_RANGES = dict(STATUS=(0, 15), LANE=(0, 0xffff), CK0=(0, mapdata.MAX_CKPT - 1), CK1=(0, mapdata.MAX_CKPT - 1), RLANE=(-1, 0x7fff),
                  TIMER=(0, 0xffff), VFLAGS=(0, 0xffff), SPAWN=(0, 0xffff))


def random_state(seed=0):
    rng = np.random.default_rng(seed)
    f = rng.normal(0, 30, size=(_abi.NF, N * V)).astype(np.float32)
    f[_abi.SF["HX"]], f[_abi.SF["HY"]] = np.cos(f[_abi.SF["THETA"]].astype(np.float64)), np.sin(f[_abi.SF["THETA"]].astype(np.float64))
    i = np.zeros((_abi.NI, N * V), dtype=np.int32)
    for name, (lo, hi) in INT_RANGES.items():
        i[_abi.SI[name]] = rng.integers(lo, hi + 1, size=N * V)
        i[_abi.SI[name], 0], i[_abi.SI[name], 1] = lo, hi  # both ends of every range
    ei = rng.integers(-2**31, 2**31, size=(_abi.NEI, N), dtype=np.int64).astype(np.int32)
    return f, i, ei


def state_in(prog, tmp, f, i, ei):
    f.tofile(tmp / "f"), i.tofile(tmp / "i"), ei.tofile(tmp / "ei")
    return int(run(prog, "state_in", tmp / "f", tmp / "i", tmp / "ei", N, V, tmp / "dev")["rc"])


def round_trip(prog, tmp, f, i, ei):
    assert state_in(prog, tmp, f, i, ei) == OK
    run(prog, "state_out", str(tmp / "dev") + ".rec", str(tmp / "dev") + ".env", N, V, tmp / "back")
    back = str(tmp / "back")
    return (np.fromfile(back + ".f", dtype=np.float32).reshape(f.shape), np.fromfile(back + ".i", dtype=np.int32).reshape(i.shape),
            np.fromfile(back + ".ei", dtype=np.int32).reshape(ei.shape))


def test_fields_to_records_and_back(prog, tmp_path):
    f, i, ei = random_state()
    f2, i2, ei2 = round_trip(prog, tmp_path, f, i, ei)
    want_f, want_ei = f.copy(), ei.copy()
    want_f[_abi.SF["THROTTLE"]] = f[_abi.SF["ACT1T"]]  # not stored: returned as the newer entry of the action deque
    want_ei[_abi.EI["NEAR"]] = 0                       # device-private hints
    assert np.array_equal(f2.view(np.uint32), want_f.view(np.uint32))
    assert np.array_equal(i2, i) and np.array_equal(ei2, want_ei)
    assert (f[_abi.SF["THROTTLE"]] != f[_abi.SF["ACT1T"]]).all() and (ei[_abi.EI["NEAR"]] != 0).all()  # (the inputs did differ)


def test_env_hints_go_in_as_unknown(prog, tmp_path):
    f, i, ei = random_state()
    ei[_abi.EI["NEAR"]] = 7
    assert state_in(prog, tmp_path, f, i, ei) == OK
    env = np.fromfile(str(tmp_path / "dev") + ".env", dtype=np.int32).reshape(N, _abi.NEI)
    assert (env[:, _abi.EI["NEAR"]] == 1).all()
    assert np.array_equal(np.delete(env, _abi.EI["NEAR"], axis=1), np.delete(ei.T, _abi.EI["NEAR"], axis=1))
    assert (round_trip(prog, tmp_path, f, i, ei)[2][_abi.EI["NEAR"]] == 0).all()


def test_heading_vector_is_kept_only_while_it_agrees_with_theta(prog, tmp_path):
    f, i, ei = random_state()
    c = np.cos(f[_abi.SF["THETA"]].astype(np.float64))
    f[_abi.SF["HX"], 0] = c[0] + 2e-4
    f[_abi.SF["HX"], 1] = c[1] + 5e-5
    f2 = round_trip(prog, tmp_path, f, i, ei)[0]
    assert f2[_abi.SF["HX"], 0] == np.float32(c[0]) and f2[_abi.SF["HY"], 0] == np.float32(np.sin(np.float64(f[_abi.SF["THETA"], 0])))
    assert f2[_abi.SF["HX"], 1] == f[_abi.SF["HX"], 1] != np.float32(c[1])
    assert np.array_equal(f2[_abi.SF["HX"], 2:], f[_abi.SF["HX"], 2:]) and np.array_equal(f2[_abi.SF["HY"], 1:], f[_abi.SF["HY"], 1:])


def test_timer_saturates(prog, tmp_path):
    f, i, ei = random_state()
    i[_abi.SI["TIMER"], 2] = 70000
    i2 = round_trip(prog, tmp_path, f, i, ei)[1]
    assert i2[_abi.SI["TIMER"], 2] == 65535
    i[_abi.SI["TIMER"], 2] = 65535
    assert np.array_equal(i2, i)


@pytest.mark.parametrize("name", sorted(INT_RANGES))
def test_int_fields_one_past_either_end_are_refused(prog, tmp_path, name):
    lo, hi = INT_RANGES[name]
    for value in (lo - 1, hi + 1):
        f, i, ei = random_state()
        i[_abi.SI[name], 4] = value
        assert state_in(prog, tmp_path, f, i, ei) == (OK if (name, value) == ("TIMER", hi + 1) else ERR_ARG), (name, value)


def test_records_to_planes_and_back(prog, tmp_path):
    rec = np.random.default_rng(3).integers(0, 256, size=(N * V, 128), dtype=np.uint8)
    rec.tofile(tmp_path / "rec")
    run(prog, "planes", tmp_path / "rec", V, tmp_path / "out")
    planes = np.fromfile(str(tmp_path / "out") + ".planes", dtype=np.uint8).reshape(N, 8, V, 16)
    assert np.array_equal(planes.transpose(0, 2, 1, 3).reshape(N * V, 128), rec)  # piece p of slot s of env e: plane p, entry s of the env's block
    assert np.array_equal(np.fromfile(str(tmp_path / "out") + ".back", dtype=np.uint8).reshape(N * V, 128), rec)
