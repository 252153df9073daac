"""The checker of the host preparation (pgdrive_amd/csrc/pgd_host_prep.h), in numpy: the device forms of the map and scenario tables
restated from their definitions, in float64 where the C++ computes in double -- the same operations in the same order, rounded to float32
once, so the results are held to equality -- plus the dtypes of the device-private records and of the driver's files
(tests/host_prep_main.cpp)."""
import ctypes as C

import numpy as np

from pgdrive_amd import _abi, mapdata

OK, ERR_ARG = 0, 1  # include/pgdrive_hip.h
WAVE, FUSE_MAX_AGENTS, SUBV = 64, 8, 52  # pgd_records.h
CKPT_END = -32768
BOX_LANE, OBJ_VEHICLE = 0, 0

LANE_EXT_DT = np.dtype([("ax", "<f4"), ("ay", "<f4"), ("dir", "<f4"), ("road", "<i4")])
LANE_NAV_DT = np.dtype([("ex", "<f4"), ("ey", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("radius", "<f4"), ("dir", "<f4"), ("angle", "<f4"),
                        ("pad", "<f4")])
GEOM = ("V", "D", "NV", "sstride", "sub", "epw", "pack_obs", "use_imask")
GEOM_DT = np.dtype([(k, "<i4") for k in GEOM])
CONFIG_BYTES = C.sizeof(_abi.PgdConfig)
GEOMETRY_IN_DT = np.dtype([("cfg", "u1", (CONFIG_BYTES, )), ("pack", "<i4"), ("imask", "<i4")])
GEOMETRY_OUT_DT = np.dtype([("rc", "<i4"), ("g", GEOM_DT)])
REGROUP_IN_DT = np.dtype([("g", GEOM_DT), ("N", "<i4"), ("n_groups", "<i4"), ("imask", "<i4")])
REGROUP_OUT_DT = np.dtype([("rc", "<i4"), ("g", GEOM_DT), ("left", "<i4")])
assert LANE_EXT_DT.itemsize == 16 and LANE_NAV_DT.itemsize == 32 and CONFIG_BYTES % 4 == 0


def related_lanes(lanes):
    """`ey` of every lane of ONE map, as uint32: the set {id & 31} over the lane, its successors and its predecessors."""
    n = len(lanes)
    sets = [{k} for k in range(n)]
    for k in range(n):
        for s in lanes["succ"][k]:
            if 0 <= s < n:
                sets[k].add(int(s))
                sets[int(s)].add(k)
    return np.array([sum(1 << b for b in {i & 31 for i in st}) for st in sets], dtype=np.uint32)


def strip_width(lane, boxes):
    """`ex` of one lane against the boxes of its map: 0 on a curved lane; on a straight one the half-width of the strip around its axis
    that no non-lane box reaches, among the boxes that overlap [-0.05, length + 0.05] along the lane -- 0 if one of them straddles the
    axis, else the least |lateral| of their corners minus 0.03, floored at 0, and 0 where nothing bounds it.  float64, in the order of
    build_map_tables."""
    if lane["dir"] != 0.0:
        return np.float32(0.0)
    b = boxes[boxes["kind"] != BOX_LANE]
    cx, cy, ux, uy, hl, hw = (b[k].astype(np.float64) for k in ("cx", "cy", "ux", "uy", "hl", "hw"))
    ax, ay, bx, by, length = (np.float64(lane[k]) for k in ("ax", "ay", "bx", "by", "length"))
    lon, lat = [], []
    for q in range(4):
        sl, sw = (1.0 if q & 1 else -1.0), (1.0 if q & 2 else -1.0)
        px = cx + sl * hl * ux - sw * hw * uy
        py = cy + sl * hl * uy + sw * hw * ux
        dx, dy = px - ax, py - ay
        lon.append(dx * bx + dy * by)
        lat.append(dy * bx - dx * by)
    lon, lat = np.array(lon).reshape(4, -1), np.array(lat).reshape(4, -1)
    near = ~((lon.max(0) < -0.05) | (lon.min(0) > length + 0.05))
    lo, hi = lat.min(0)[near], lat.max(0)[near]
    if not near.any():
        return np.float32(0.0)
    if ((lo <= 0.0) & (hi >= 0.0)).any():
        return np.float32(0.0)
    clear = np.minimum(np.abs(lo), np.abs(hi)).min()
    return np.float32(max(0.0, clear - 0.03))


def lane_nav(lanes):
    """LaneNav of every lane: the end point and the lateral direction at the end, float64 rounded once; on an arc also radius, direction
    and the swept angle (a float32 difference, as in the C++)."""
    out = np.zeros(len(lanes), dtype=LANE_NAV_DT)
    f64 = {k: lanes[k].astype(np.float64) for k in ("ax", "ay", "bx", "by", "dir", "length")}
    st = lanes["dir"] == 0.0
    out["ex"][st] = (f64["ax"] + f64["length"] * f64["bx"])[st]
    out["ey"][st] = (f64["ay"] + f64["length"] * f64["by"])[st]
    out["nx"][st], out["ny"][st] = -lanes["by"][st], lanes["bx"][st]
    with np.errstate(all="ignore"):  # (evaluated on the straight lanes too, whose bx is a direction component; not used there)
        phi = f64["dir"] * f64["length"] / f64["bx"] + f64["by"]
        c, s = np.cos(phi), np.sin(phi)
    cv = ~st
    out["ex"][cv], out["ey"][cv] = (f64["ax"] + f64["bx"] * c)[cv], (f64["ay"] + f64["bx"] * s)[cv]
    out["nx"][cv], out["ny"][cv] = (-f64["dir"] * c)[cv], (-f64["dir"] * s)[cv]
    out["radius"][cv], out["dir"][cv] = lanes["bx"][cv], lanes["dir"][cv]
    out["angle"][cv] = np.where(lanes["dir"] == 1.0, lanes["c"] - lanes["by"], lanes["by"] - lanes["c"])[cv]
    return out


def cell_major(m, lanes, boxes, cs, ci):
    """One map (header `m`, bank-wide arrays): per cell the stable partition of its boxes, lane boxes first, the LaneExt of each entry and
    the packed cell_start.  Returns (boxes, ext, start) over the map's items / cells."""
    L = lanes[m["lane_off"]:m["lane_off"] + m["n_lanes"]]
    B = boxes[m["box_off"]:m["box_off"] + m["n_boxes"]]
    n_cells = int(m["gx"]) * int(m["gy"])
    start = cs[m["cell_off"]:m["cell_off"] + n_cells + 1]
    items = ci[m["item_off"]:m["item_off"] + start[-1]]
    cb = np.zeros(len(items), dtype=mapdata.BOX_DT)
    cx = np.zeros(len(items), dtype=LANE_EXT_DT)
    cx["road"] = -1
    packed = start.copy()
    for c in range(n_cells):
        a, b = int(start[c]), int(start[c + 1])
        bx = B[items[a:b]]
        is_lane = bx["kind"] == BOX_LANE
        order = np.concatenate([np.flatnonzero(is_lane), np.flatnonzero(~is_lane)])
        cb[a:b] = bx[order]
        n_lane = int(is_lane.sum())
        packed[c] = a | (n_lane << 24)
        ln = L[bx[order][:n_lane]["lane"]]
        straight = ln["dir"] == 0.0
        cx["ax"][a:a + n_lane] = np.where(straight, ln["bx"], ln["ax"])
        cx["ay"][a:a + n_lane] = np.where(straight, ln["by"], ln["ay"])
        cx["dir"][a:a + n_lane] = ln["dir"]
        cx["road"][a:a + n_lane] = ln["road"]
    return cb, cx, packed


def spawn_marks(spawns):
    """The device spawn records: PGD_CKPT_END from the route's last node on."""
    out = spawns.copy()
    for q in out:
        q["ckpt"][max(min(int(q["n_ckpt"]), mapdata.MAX_CKPT) - 1, 0):] = CKPT_END
    return out


def scenario_flags(scen, spawns, no_uni=False):
    """(has_objects, no_groups, uni_len, uni_wid) of an upload: over the used slots (lane >= 0) only."""
    used = spawns[spawns["lane"] >= 0]
    has_objects = bool((used["kind"] != OBJ_VEHICLE).any())
    sizes = {(float(q["length"]), float(q["width"])) for q in used}
    uni = len(sizes) == 1 and not has_objects and not no_uni and min(next(iter(sizes))) > 0.0
    ul, uw = next(iter(sizes)) if uni else (0.0, 0.0)
    return has_objects, int(not (scen["n_groups"] > 0).any()), ul, uw
