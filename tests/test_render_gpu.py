"""Top-down scene rendering on the GPU (pgdrive_amd/csrc/pgd_render.h): frames against the numpy restatement of tests/render_ref.py,
trails, resets, dead markers, env subsets, no effect on the simulation, throughput mode, and the env surfaces."""
import numpy as np
import pytest

from pgdrive_amd import _abi, render
from tests import render_ref, util

pytestmark = pytest.mark.gpu
SF, SI, EI = _abi.SF, _abi.SI, _abi.EI


def _engine(descs, n, seed=3, **kw):
    from pgdrive_amd.engine import Engine
    mb, sb = util.make_banks(descs, n_maps=8)
    kw.setdefault("num_lasers", 0)
    cfg = _abi.make_config(n, num_agents=1, num_traffic=16, seed=seed, **kw)
    eng = Engine(cfg, mb, sb)
    eng.reset(np.arange(n) % 8)
    return eng


def _traffic_into_view(eng, rng):
    """Waiting traffic moved next to every ego (as tests/test_topdown_gpu.py does), so that draw_traffic has boxes to draw."""
    f, i, ei = eng.get_state()
    n = eng.N
    for k in range(1, 6):
        th = f[SF["THETA"], :, 0]
        fw, lt = rng.uniform(6, 26, n), rng.uniform(-9, 9, n)
        f[SF["X"], :, k] = f[SF["X"], :, 0] + fw * np.cos(th) - lt * np.sin(th)
        f[SF["Y"], :, k] = f[SF["Y"], :, 0] + fw * np.sin(th) + lt * np.cos(th)
        f[SF["THETA"], :, k] = th + rng.uniform(-3.0, 3.0, n) * (k % 2)
        f[SF["HX"], :, k] = f[SF["HY"], :, k] = 0.0
        i[SI["STATUS"], :, k] = _abi.ST_PENDING
    eng.set_state(util.round_state_f32(f), i, ei)


def _check(eng, ref, frames, envs, stats):
    f, i, ei = eng.get_state()
    g = frames.cpu().numpy()
    for k, e in enumerate(envs):
        img, amb = ref.render(e, f, i, ei)
        nd, ok = render_ref.compare(g[k], img, amb)
        assert ok, "env %d: %d pixels differ away from any edge" % (e, nd)
        stats["diff"] += nd
        stats["pix"] += img.shape[0] * img.shape[1]
        stats["veh"] += int(np.sum(np.any((img != 255) & (img != 0), axis=-1)))
        stats["red"] += int(np.sum(np.all(img == (255, 0, 0), axis=-1)))


def _settings(**kw):
    s = render.parse_kwargs("top_down", dict(dict(film_size=(256, 256)), **kw))
    return s


def test_render_parity_single_agent_with_traffic(descs):
    """8 single-agent envs with draw_traffic: every frame of 40 driven steps (auto-resets included) against render_ref, exact but
    for pixel centres within 1e-3 px of an edge (fp32 against fp64), at most 1e-4 of all pixels."""
    import torch
    n = 8
    eng = _engine(descs, n)
    s = _settings(draw_traffic=True)
    eng.enable_render(render.make_config(s))
    ref = render_ref.RefRenderer(eng, s)
    rng = np.random.default_rng(1)
    _traffic_into_view(eng, rng)
    stats = dict(diff=0, pix=0, veh=0, red=0)
    _check(eng, ref, eng.render_topdown(), range(n), stats)
    for t in range(40):
        eng.step(torch.from_numpy(util.driving_actions(rng, n)).cuda())
        fr = eng.render_topdown()
        eng.sync()
        _check(eng, ref, fr, range(n), stats)
    assert stats["veh"] > 1000
    assert stats["diff"] <= 1e-4 * stats["pix"], stats


def _roundabout(n=4, **kw):
    from pgdrive_amd.marl_env import MultiAgentRoundaboutVecEnv
    return MultiAgentRoundaboutVecEnv(dict(dict(num_envs=n, seed=5), **kw))


def test_render_parity_roundabout_with_dying_agents_and_dead_markers():
    """4 roundabout envs driven at random for 60 steps: agents crash and wait in the delay-done queue; every frame against
    render_ref; a dying agent leaves a red disk at its terminal position in every later frame of the episode."""
    import torch
    venv = _roundabout()
    eng = venv.engine
    venv.reset()
    s = _settings()
    eng.enable_render(render.make_config(s))
    ref = render_ref.RefRenderer(eng, s)
    rng = np.random.default_rng(4)
    stats = dict(diff=0, pix=0, veh=0, red=0)
    deaths = {}  # env -> list of (episode, pixel)
    _check(eng, ref, eng.render_topdown(), range(venv.num_envs), stats)
    for t in range(60):
        a = rng.uniform(-1, 1, size=(venv.num_envs, venv.A, 2)).astype(np.float32)
        a[..., 1] = np.abs(a[..., 1])
        venv.step(torch.from_numpy(a).cuda())
        fr = eng.render_topdown()
        eng.sync()
        _check(eng, ref, fr, range(venv.num_envs), stats)
        f, i, ei = eng.get_state()
        g = fr.cpu().numpy()
        for e in range(venv.num_envs):
            ep = int(ei[EI["EPISODES"], e])
            m = int(eng.scen.scenarios["map"][int(ei[EI["SCEN"], e])])
            for sl in np.nonzero(i[SI["STATUS"], e, :venv.A] == _abi.ST_DYING)[0]:
                u, v = render.pos2pix(float(f[SF["X"], e, sl]), float(f[SF["Y"], e, sl]), eng.film_geom[m])
                if 0 <= u < 256 and 0 <= v < 256:
                    deaths.setdefault(e, set()).add((ep, u, v))
            for (ep0, u, v) in deaths.get(e, ()):
                if ep0 == ep:
                    assert tuple(g[e, v, u]) == (255, 0, 0)
    assert stats["red"] > 0 and sum(len(v) for v in deaths.values()) > 0
    assert stats["diff"] <= 1e-4 * stats["pix"], stats
    venv.close()


@pytest.mark.parametrize("num_stack,history_smooth", [(15, 0), (3, 0), (15, 2)])
def test_render_history_colours_and_order(descs, num_stack, history_smooth):
    """The ego's trail: frame by frame against render_ref, and the faded colours the newest frames leave are the fade table's."""
    import torch
    eng = _engine(descs, 1, auto_reset=0)
    s = _settings(film_size=(1000, 1000), num_stack=num_stack, history_smooth=history_smooth)
    eng.enable_render(render.make_config(s))
    ref = render_ref.RefRenderer(eng, s)
    stats = dict(diff=0, pix=0, veh=0, red=0)
    act = np.zeros((1, 1, 2), np.float32)
    act[..., 1] = 1.0
    for t in range(20):
        eng.step(torch.from_numpy(act).cuda())
        fr = eng.render_topdown()
        eng.sync()
        _check(eng, ref, fr, range(1), stats)
    g = fr.cpu().numpy()[0]
    col = render.PALETTE[render.agent_colour(3, 0, 0)]
    n = min(20, num_stack)
    shown = {render_ref.fade(col, k, n) for k in range(2, n + 1) if history_smooth == 0 or k % history_smooth == 0}
    present = {tuple(int(x) for x in p) for p in g.reshape(-1, 3)}
    assert tuple(col) in present and render.CONTOUR_RGB in present
    # the trail: a strip of every older frame the newer boxes leave uncovered (the first, slow steps may leave none)
    seen = shown - {(255, 255, 255)}
    assert len(seen & present) >= max(1, len(seen) // 2), (sorted(seen), num_stack, history_smooth)
    hidden = {render_ref.fade(col, k, n) for k in range(2, n + 1)} - shown
    for c in hidden - {(255, 255, 255)}:
        assert c not in present


def test_render_reset_clears_trails(descs):
    """After reset() and after an auto-reset the first frame holds only the present vehicles."""
    import torch
    eng = _engine(descs, 4)
    s = _settings()
    eng.enable_render(render.make_config(s))
    act = np.zeros((4, 1, 2), np.float32)
    act[..., 1] = 1.0
    for t in range(8):
        eng.step(torch.from_numpy(act).cuda())
        eng.render_topdown()
    eng.reset(np.arange(4) % 8)
    fr = eng.render_topdown().cpu().numpy()
    fresh = render_ref.RefRenderer(eng, s)
    f, i, ei = eng.get_state()
    for e in range(4):
        img, amb = fresh.render(e, f, i, ei)
        nd, ok = render_ref.compare(fr[e], img, amb)
        assert ok and nd <= 10
    # auto-reset: drive hard to the right until an episode ends, then the next frame shows no trail
    act[..., 0] = 1.0
    ep0 = eng.get_state()[2][EI["EPISODES"]].copy()
    for t in range(200):
        eng.step(torch.from_numpy(act).cuda())
        fr = eng.render_topdown().cpu().numpy()
        f, i, ei = eng.get_state()
        new = np.nonzero(ei[EI["EPISODES"]] != ep0)[0]
        if len(new):
            e = int(new[0])
            fresh = render_ref.RefRenderer(eng, s)
            img, amb = fresh.render(e, f, i, ei)
            nd, ok = render_ref.compare(fr[e], img, amb)
            assert ok and nd <= 10
            break
    else:
        pytest.fail("no auto-reset in 200 steps")


def test_render_env_subset(descs):
    """Rendering env_ids=[3, 7] advances only those rings and gives the frames a full render gives for those envs."""
    import torch
    a, b = _engine(descs, 8), _engine(descs, 8)
    s = _settings()
    a.enable_render(render.make_config(s))
    b.enable_render(render.make_config(s))
    rng = np.random.default_rng(7)
    for t in range(12):
        act = torch.from_numpy(util.driving_actions(rng, 8)).cuda()
        a.step(act)
        b.step(act)
        fa = a.render_topdown().cpu().numpy()
        fb = b.render_topdown(env_ids=[3, 7]).cpu().numpy()
        assert np.array_equal(fa[[3, 7]], fb)
    # the other envs of b never advanced: their first render shows no trail; envs 3 and 7 go on with theirs
    fa = a.render_topdown().cpu().numpy()
    fb = b.render_topdown().cpu().numpy()
    assert np.array_equal(fa[[3, 7]], fb[[3, 7]])
    fresh = render_ref.RefRenderer(b, s)
    f, i, ei = b.get_state()
    for e in (0, 1, 2, 4, 5, 6):
        img, amb = fresh.render(e, f, i, ei)
        nd, ok = render_ref.compare(fb[e], img, amb)
        assert ok and nd <= 10


def test_render_does_not_change_the_simulation(descs):
    """Two twin engines, the same actions; one renders after every step.  100 steps: bit-identical outputs and state."""
    import torch
    from pgdrive_amd.engine import Engine
    mb, sb = util.make_banks(descs, n_maps=8)
    cfg = _abi.make_config(16, num_agents=1, num_traffic=16, seed=3)
    a, b = Engine(cfg, mb, sb), Engine(cfg, mb, sb)
    ids = np.arange(16) % 8
    a.reset(ids)
    b.reset(ids)
    b.enable_render(render.make_config(_settings(draw_traffic=True)))
    rng = np.random.default_rng(9)
    for t in range(100):
        act = torch.from_numpy(util.driving_actions(rng, 16)).cuda()
        ra = [x.clone() for x in a.step(act)]
        rb = [x.clone() for x in b.step(act)]
        b.render_topdown()
        for x, y in zip(ra, rb):
            assert torch.equal(x, y)
    for x, y in zip(a.get_state(), b.get_state()):
        assert np.array_equal(x, y)


def test_render_throughput_mode_matches(descs, monkeypatch):
    """An engine created under PGD_PACK=1 (several envs per wave) renders the frames of its one-env-per-wave twin."""
    import torch
    monkeypatch.setenv("PGD_PACK", "1")
    packed = _engine(descs, 15, num_lasers=240)  # (throughput mode: lidar engines, three envs of 17 slots per wave)
    monkeypatch.delenv("PGD_PACK")
    plain = _engine(descs, 15, num_lasers=240)
    s = _settings(draw_traffic=True)
    packed.enable_render(render.make_config(s))
    plain.enable_render(render.make_config(s))
    rng = np.random.default_rng(11)
    for t in range(20):
        act = torch.from_numpy(util.driving_actions(rng, 15)).cuda()
        packed.step(act)
        plain.step(act)
        assert torch.equal(packed.render_topdown(), plain.render_topdown())
    assert "throughput" in packed.describe_step() or "several" in packed.describe_step()


def test_env_surfaces_render():
    from pgdrive_amd.env import PGDriveEnv
    from pgdrive_amd.marl_env import MultiAgentRoundaboutEnv
    env = PGDriveEnv(dict(environment_num=2))
    env.reset()
    img = env.render(mode="top_down")
    assert img.shape == (1000, 1000, 3) and img.dtype == np.uint8
    env.step([0.0, 1.0])
    img2 = env.render(mode="top_down", film_size=(200, 200))  # later kwargs are ignored
    assert img2.shape == (1000, 1000, 3)
    with pytest.raises(NotImplementedError):
        env.render(mode="human")
    env.close()
    menv = MultiAgentRoundaboutEnv()
    menv.reset()
    img = menv.render(mode="top_down")
    assert img.shape == (1000, 1000, 3) and img.dtype == np.uint8
    assert np.sum(np.any((img != 255) & (img != 0), axis=-1)) > 0
    menv.close()


def test_render_film_with_a_partial_last_chunk(descs):
    """A 250 x 250 film: 62500 pixels end in a partial 16-pixel chunk, and the frames of envs 1 and 2 start off a 16-byte boundary."""
    import torch
    n = 3
    eng = _engine(descs, n)
    s = _settings(film_size=(250, 250), draw_traffic=True)
    eng.enable_render(render.make_config(s))
    ref = render_ref.RefRenderer(eng, s)
    rng = np.random.default_rng(5)
    _traffic_into_view(eng, rng)
    stats = dict(diff=0, pix=0, veh=0, red=0)
    for t in range(10):
        eng.step(torch.from_numpy(util.driving_actions(rng, n)).cuda())
        fr = eng.render_topdown()
        eng.sync()
        _check(eng, ref, fr, range(n), stats)
    assert stats["diff"] <= 1e-4 * stats["pix"], stats


def test_render_traffic_objects_and_toll_booths():
    """draw_traffic with the accident scenes of SafePGDriveEnv (cones, warning tripods, barriers, broken-down vehicles) and with the
    toll booths of the tollgate map: frames against render_ref; objects are drawn, toll booths (invisible walls) are not."""
    import torch
    from pgdrive_amd import PGDriveVecEnv
    from pgdrive_amd.marl_env import MultiAgentTollgateVecEnv
    venv = PGDriveVecEnv(dict(num_envs=4, start_seed=1000, environment_num=50, accident_prob=0.8, traffic_density=0.05))
    eng = venv.engine
    venv.reset(force_seed=[1000, 1003, 1017, 1042])
    s = _settings(film_size=(1000, 1000), draw_traffic=True)
    eng.enable_render(render.make_config(s))
    ref = render_ref.RefRenderer(eng, s)
    stats = dict(diff=0, pix=0, veh=0, red=0)
    rng = np.random.default_rng(6)
    for t in range(4):
        venv.step(torch.from_numpy(util.driving_actions(rng, 4).reshape(4, 2)).cuda())
        fr = eng.render_topdown()
        eng.sync()
        _check(eng, ref, fr, range(4), stats)
    assert stats["diff"] <= 1e-4 * stats["pix"], stats
    f, i, ei = eng.get_state()
    g = fr.cpu().numpy()
    sstride = len(eng.scen.spawns) // len(eng.scen.scenarios)
    outlined = n_obj = 0
    for e in range(4):
        scen = int(ei[EI["SCEN"], e])
        m = int(eng.scen.scenarios["map"][scen])
        for sl in range(1, eng.V):
            kind = int(eng.scen.spawns[scen * sstride + int(i[SI["SPAWN"], e, sl])]["kind"])
            if kind in (1, 2) and int(i[SI["STATUS"], e, sl]) in (_abi.ST_PENDING, _abi.ST_ACTIVE):
                u, v = render_ref.pos2pix(float(f[SF["X"], e, sl]), float(f[SF["Y"], e, sl]), eng.film_geom[m])
                if 0 <= u < 1000 and 0 <= v < 1000:
                    n_obj += 1
                    outlined += tuple(g[e, v, u]) == render.CONTOUR_RGB
    assert n_obj > 0 and outlined > 0, (n_obj, outlined)
    venv.close()
    tv = MultiAgentTollgateVecEnv(dict(num_envs=2))
    eng = tv.engine
    tv.reset()
    s = _settings(film_size=(512, 512), draw_traffic=True)
    eng.enable_render(render.make_config(s))
    ref = render_ref.RefRenderer(eng, s)
    stats = dict(diff=0, pix=0, veh=0, red=0)
    fr = eng.render_topdown()
    eng.sync()
    _check(eng, ref, fr, range(2), stats)
    f, i, ei = eng.get_state()
    g = fr.cpu().numpy()
    booths = 0
    for e in range(2):
        scen = int(ei[EI["SCEN"], e])
        m = int(eng.scen.scenarios["map"][scen])
        sstride = len(eng.scen.spawns) // len(eng.scen.scenarios)
        for sl in range(tv.A, eng.V):
            if int(eng.scen.spawns[scen * sstride + int(i[SI["SPAWN"], e, sl])]["kind"]) == 3:
                u, v = render_ref.pos2pix(float(f[SF["X"], e, sl]), float(f[SF["Y"], e, sl]), eng.film_geom[m])
                if 0 <= u < 512 and 0 <= v < 512:
                    booths += 1
                    assert tuple(g[e, v, u]) not in (render.CONTOUR_RGB, render.TRAFFIC_RGB, render.OBJECT_RGB)
    assert booths > 0
    tv.close()


def test_render_dead_list_keeps_the_newest_256():
    """More than 256 agents die in one episode: the dead list drops its oldest entries (frames against render_ref, which keeps the
    same 256), so the first disks are gone and the 256 newest are there."""
    venv = _roundabout(n=2)
    eng = venv.engine
    venv.reset()
    s = _settings()
    eng.enable_render(render.make_config(s))
    ref = render_ref.RefRenderer(eng, s)
    stats = dict(diff=0, pix=0, veh=0, red=0)
    A = venv.A
    rounds = (300 + A - 1) // A
    pix_of = {}
    for r in range(rounds):
        f, i, ei = eng.get_state()
        for e in range(2):
            m = int(eng.scen.scenarios["map"][int(ei[EI["SCEN"], e])])
            sc, ox, oy = eng.film_geom[m]
            for sl in range(A):
                j = r * A + sl
                u, v = 4 + 12 * (j % 20), 4 + 12 * (j // 20)
                pix_of[j] = (u, v)
                f[SF["X"], e, sl], f[SF["Y"], e, sl] = ox + (u + 0.5) / sc, oy + (v + 0.5) / sc
                f[SF["THETA"], e, sl], f[SF["HX"], e, sl], f[SF["HY"], e, sl] = 0.0, 1.0, 0.0
                i[SI["STATUS"], e, sl], i[SI["TIMER"], e, sl] = _abi.ST_DYING, 200
        eng.set_state(util.round_state_f32(f), i, ei)
        fr = eng.render_topdown()
        eng.sync()
        _check(eng, ref, fr, range(2), stats)
    assert stats["diff"] <= 1e-4 * stats["pix"], stats
    total = rounds * A
    assert total > 256 and len(ref.deads[0]) == 256
    g = fr.cpu().numpy()
    dropped, kept = pix_of[0], pix_of[total - 256]
    for e in range(2):
        assert tuple(g[e, dropped[1], dropped[0]]) != (255, 0, 0)
        assert tuple(g[e, kept[1], kept[0]]) == (255, 0, 0)
    venv.close()
