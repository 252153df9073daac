"""Brute-force numpy restatement of the top-down scene rendering (pgdrive_amd/csrc/pgd_render.h), for the render tests.

Every pixel is decided at its centre (u + 0.5, v + 0.5) in fp64, one draw at a time in painter's order.  `ambiguous` marks the
pixels whose centre lies within EDGE_PX of an edge that decided them (a box side, the contour band, a disk, a lane line's reach):
there the kernel's fp32 arithmetic may fall on the other side.
"""
import math

import numpy as np

from pgdrive_amd import _abi, render

EDGE_PX = 1e-3
SNAP = 2.0 * math.pi / 180.0


def pos2pix(x, y, geom):
    """(int((x - ox) * scaling), int((y - oy) * scaling)): the reference's WorldSurface.pos2pix."""
    sc, ox, oy = geom
    return int((x - ox) * sc), int((y - oy) * sc)


def _pcg(x):
    s = (x * 747796405 + 2891336453) & 0xFFFFFFFF
    w = (((s >> ((s >> 28) + 4)) ^ s) * 277803737) & 0xFFFFFFFF
    return (w >> 22) ^ w


def agent_colour(seed, env_global, agent_id):
    """Palette index of an agent: the device counter hash pgd_rng(seed, env, 0x7e4d0c01, agent id) % 10 (pgd_device.h)."""
    c = _pcg((agent_id + 0x9E3779B9) & 0xFFFFFFFF)
    return _pcg(seed ^ _pcg(env_global ^ _pcg(0x7E4D0C01 ^ c))) % 10


def fade(c, i, n):
    return tuple(int(x + (i / n) * (255 - x)) for x in c)


def background(bank, m, geom, W, H, light=True, road=(255, 255, 255)):
    """(rgb [H, W, 3], ambiguous [H, W]) of map m: a lane line where the pixel centre is within 0.5 * pix(1) / scaling of a line box."""
    sc, ox, oy = geom
    line_r = 0.5 * int(1.0 * sc) / sc
    mp = bank.maps[m]
    boxes = bank.boxes[int(mp["box_off"]):int(mp["box_off"]) + int(mp["n_boxes"])]
    line = np.zeros((H, W), dtype=bool)
    amb = np.zeros((H, W), dtype=bool)
    for b in boxes:
        if int(b["kind"]) not in (1, 2, 3):  # white / yellow continuous and broken line boxes: not lane surfaces, not sidewalks
            continue
        cx, cy, ux, uy, hl, hw = (float(b[k]) for k in ("cx", "cy", "ux", "uy", "hl", "hw"))
        reach = abs(hl * ux) + abs(hw * uy) + line_r, abs(hl * uy) + abs(hw * ux) + line_r
        u0, u1 = int(math.floor((cx - reach[0] - ox) * sc)) - 1, int(math.ceil((cx + reach[0] - ox) * sc)) + 1
        v0, v1 = int(math.floor((cy - reach[1] - oy) * sc)) - 1, int(math.ceil((cy + reach[1] - oy) * sc)) + 1
        u0, v0, u1, v1 = max(u0, 0), max(v0, 0), min(u1, W - 1), min(v1, H - 1)
        if u0 > u1 or v0 > v1:
            continue
        uu, vv = np.meshgrid(np.arange(u0, u1 + 1), np.arange(v0, v1 + 1))
        wx, wy = ox + (uu + 0.5) / sc, oy + (vv + 0.5) / sc
        dx, dy = wx - cx, wy - cy
        a = np.maximum(np.abs(dx * ux + dy * uy) - hl, 0.0)
        c = np.maximum(np.abs(dy * ux - dx * uy) - hw, 0.0)
        dist = np.sqrt(a * a + c * c)
        line[v0:v1 + 1, u0:u1 + 1] |= dist <= line_r
        amb[v0:v1 + 1, u0:u1 + 1] |= np.abs(dist - line_r) * sc < EDGE_PX
    lc = np.array([255 - x for x in road] if light else list(road), dtype=np.uint8)
    img = np.full((H, W, 3), 255 if light else 0, dtype=np.uint8)
    img[line] = lc
    return img, amb


class RefRenderer:
    """The renderer of one engine: per env a ring of the last num_stack frames and a dead list (pgd_render.h)."""

    def __init__(self, engine, settings):
        self.eng = engine
        self.s = settings
        self.W, self.H = settings["film_size"]
        self.geoms = engine.film_geom
        sb = engine.scen
        self.sstride = len(sb.spawns) // len(sb.scenarios)
        self.rings = {}
        self.deads = {}
        self.last_ep = {}
        self.bg = {}

    def forget(self, envs):
        for e in envs:
            self.last_ep[e] = None

    def frame_of(self, e, f, i, ei):
        """The vehicles of env e in the state (f, i, ei): list of dicts (slot order)."""
        eng, sb = self.eng, self.eng.scen
        scen = int(ei[_abi.EI["SCEN"], e])
        m = int(sb.scenarios["map"][scen])
        geom = self.geoms[m]
        out = []
        for s in range(eng.V):
            st = int(i[_abi.SI["STATUS"], e, s])
            sp = sb.spawns[scen * self.sstride + int(i[_abi.SI["SPAWN"], e, s])]
            kind = int(sp["kind"])
            agent = s < eng.A
            if agent:
                present = st in (_abi.ST_ACTIVE, _abi.ST_DYING)
            else:
                present = bool(self.s["draw_traffic"]) and st in (_abi.ST_PENDING, _abi.ST_ACTIVE) and kind != 3
            done = agent and st == _abi.ST_DYING
            x, y = float(f[_abi.SF["X"], e, s]), float(f[_abi.SF["Y"], e, s])
            cu, cv = pos2pix(x, y, geom)
            visible = -50 < cu < self.W + 50 and -50 < cv < self.H + 50
            th = float(f[_abi.SF["THETA"], e, s])
            snap = abs(th) <= SNAP
            ax, ay = (1.0, 0.0) if snap else (float(f[_abi.SF["HX"], e, s]), float(f[_abi.SF["HY"], e, s]))
            if agent:
                col = render.PALETTE[agent_colour(int(eng.cfg.seed), int(eng.cfg.env_base) + e, int(f[_abi.SF["AGENT_ID"], e, s]))]
            else:
                col = render.TRAFFIC_RGB if kind == 0 else render.OBJECT_RGB
            wid = float(sp["length"]) if kind == 1 else float(sp["width"])
            out.append(dict(drawn=present and visible, done=done, cu=cu, cv=cv, ax=ax, ay=ay, len=int(float(sp["length"]) * geom[0]),
                            wid=int(wid * geom[0]), col=col))
        return out, m

    def render(self, e, f, i, ei):
        """Append env e's present state and return (image [H, W, 3] uint8, ambiguous [H, W] bool)."""
        ep = int(ei[_abi.EI["EPISODES"], e])
        if self.last_ep.get(e, "x") != ep:
            self.rings[e], self.deads[e] = [], []
        self.last_ep[e] = ep
        fr, m = self.frame_of(e, f, i, ei)
        ring, deads = self.rings[e], self.deads[e]
        prev = ring[-1] if ring else None
        for s, b in enumerate(fr):
            if b["done"] and not (prev is not None and prev[s]["done"] and prev[s]["cu"] == b["cu"] and prev[s]["cv"] == b["cv"]):
                deads.append((b["cu"], b["cv"]))
        del deads[:-256]
        ring.append(fr)
        del ring[:-self.s["num_stack"]]
        if m not in self.bg:
            self.bg[m] = background(self.eng.bank, m, self.geoms[m], self.W, self.H, self.s["light_background"], self.s["road_color"])
        img, amb = self.bg[m][0].copy(), self.bg[m][1].copy()
        n, hs = len(ring), self.s["history_smooth"]
        for k, frame in enumerate(ring[:-1]):
            ii = n - k
            if hs != 0 and ii % hs != 0:
                continue
            for b in frame:
                if b["drawn"]:
                    paint_box(img, amb, b, fade(b["col"], ii, n), contour=False)
        for b in ring[-1]:
            if b["drawn"]:
                paint_box(img, amb, b, tuple(b["col"]), contour=True)
        for (cu, cv) in deads:
            paint_disk(img, amb, cu, cv)
        return img, amb


def _window(img, cu, cv, r):
    H, W = img.shape[:2]
    u0, u1, v0, v1 = max(cu - r, 0), min(cu + r, W - 1), max(cv - r, 0), min(cv + r, H - 1)
    if u0 > u1 or v0 > v1:
        return None
    uu, vv = np.meshgrid(np.arange(u0, u1 + 1), np.arange(v0, v1 + 1))
    return (slice(v0, v1 + 1), slice(u0, u1 + 1)), uu + 0.5 - cu, vv + 0.5 - cv


def paint_box(img, amb, b, rgb, contour):
    hl, hw = 0.5 * b["len"], 0.5 * b["wid"]
    w = _window(img, b["cu"], b["cv"], int(math.ceil(hl + hw)) + 2)
    if w is None:
        return
    sl, dx, dy = w
    la = np.abs(dx * b["ax"] + dy * b["ay"])
    lb = np.abs(dy * b["ax"] - dx * b["ay"])
    inside = (la <= hl) & (lb <= hw)
    near = (np.abs(la - hl) < EDGE_PX) | (np.abs(lb - hw) < EDGE_PX)
    sub, a = img[sl], amb[sl]
    a[inside | near] = False  # a later draw decides these pixels
    a[near] = True
    sub[inside] = rgb
    if contour:
        edge = inside & ((la >= hl - 2.0) | (lb >= hw - 2.0))
        sub[edge] = render.CONTOUR_RGB
        a[inside & ((np.abs(la - (hl - 2.0)) < EDGE_PX) | (np.abs(lb - (hw - 2.0)) < EDGE_PX))] = True


def paint_disk(img, amb, cu, cv):
    w = _window(img, cu, cv, 6)
    if w is None:
        return
    sl, dx, dy = w
    r2 = dx * dx + dy * dy
    inside = r2 <= 25.0
    img[sl][inside] = render.DEAD_RGB
    amb[sl][inside] = False


def compare(gpu, ref, amb):
    """(number of differing pixels, whether every one of them is ambiguous)."""
    diff = np.any(gpu != ref, axis=-1)
    return int(diff.sum()), bool(np.all(amb[diff]))
