"""A refused upload leaves the engine exactly as it was: pgd_upload_scenarios and pgd_upload_maps build and check the device forms of their
tables on the host (pgd_host_prep.h) before they touch the arena or the handle.  Two engines from the same banks; one of them is offered a
scenario bank with a spawn record the engine refuses, later a map bank whose header points past the lane array; both then step on one
action stream and every output and the whole state stay equal bit for bit."""
import numpy as np
import pytest

from pgdrive_amd import _abi, mapdata, scenario
from pgdrive_amd.engine import _np_p
from tests import parity, util
from tests.parity import closed_engines  # noqa: F401  (autouse: engines are closed when a test ends)

PGD_ERR_ARG = 1


@pytest.mark.gpu
def test_a_refused_upload_leaves_the_engine_as_it_was(descs):
    n = 8  # the smallest engine that steps: 1 agent + 4 traffic, 30 beams, 2 scenarios on 1 map
    d = descs[0]
    mb = mapdata.MapBank([d])
    sb = scenario.ScenarioBank([d, d], [d["seed"]] * 2, num_traffic=4, traffic_seeds=[1, 2])
    sb.scenarios["map"] = 0
    cfg = _abi.make_config(n, num_traffic=4, num_lasers=30, seed=3)
    a, b = parity.engine(cfg, mb, sb), parity.engine(cfg, mb, sb)
    a.reset(np.arange(n) % 2)
    b.reset(np.arange(n) % 2)
    rng = np.random.default_rng(7)

    def ten_steps():
        for t, outs_a, outs_b in parity.twins(a, b, 10, lambda t: util.driving_actions(rng, n)):
            parity.same_bits(t, outs_a, outs_b, a, b)

    bad = sb.spawns.copy()
    bad["max_steer"][np.flatnonzero(bad["lane"] >= 0)[0]] = 1.5
    assert a.L.pgd_upload_scenarios(a.h, _np_p(sb.scenarios), len(sb.scenarios), _np_p(bad)) == PGD_ERR_ARG
    ten_steps()
    maps = mb.maps.copy()
    maps["lane_off"][0] = len(mb.lanes)  # one past the lane array
    assert a.L.pgd_upload_maps(a.h, _np_p(maps), len(maps), _np_p(mb.lanes), len(mb.lanes), _np_p(mb.roads), len(mb.roads), _np_p(mb.boxes),
                               len(mb.boxes), _np_p(mb.cell_start), len(mb.cell_start), _np_p(mb.cell_items), len(mb.cell_items)) == PGD_ERR_ARG
    ten_steps()
    assert int(a.get_state()[2][_abi.EI["STEPS_TOTAL"]].min()) == 20  # (both engines did step)
