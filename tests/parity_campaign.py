"""Large differential campaign (profiles/r01_parity_campaign.md): teacher-forced GPU vs oracle parity on all 100 PGDrive-v0 maps.
The loop is parity.campaign, the one tests/test_parity_wide_gpu.py::test_all_maps_campaign runs at suite size (its counters are
named as there: radius_rows, idm_ties, active)."""
import sys, time, json; sys.path.insert(0, '.')
import numpy as np
from tests import parity, util
from pgdrive_amd import _abi, bank
descs = bank.load_descriptions()
out = []
for mode, steps in (("driving", 1500), ("uniform", 600), ("straight", 900), ("driving-respawn", 500), ("idm-agent-respawn", 500)):
    n_envs = 1024
    # (last streams, round 4: respawn-mode traffic -- every IDM vehicle drives from the first step: the dense rows of bench.py;
    # then the same with the ego driven by the IDM policy, IDM_agent)
    mb, sb = util.make_banks(descs, n_maps=100, **(dict(traffic_mode="respawn") if mode.endswith("respawn") else {}))
    cfg = _abi.make_config(n_envs, num_agents=1, num_traffic=16, num_lasers=240, auto_reset=1, seed=11, idm_agent=1 if mode.startswith("idm-agent") else 0)
    eng, ora = parity.engine(cfg, mb, sb), parity.oracle(cfg, mb, sb)
    ids = np.arange(n_envs) % 100
    o0 = ora.reset(ids); g0 = eng.reset(ids).cpu().numpy()
    assert np.abs(g0 - o0).max() < parity.OBS_TOL
    rng = np.random.default_rng(17)
    stream = "driving" if mode.startswith("driving") else "uniform" if mode == "uniform" else "straight"
    t0 = time.time()
    # every mismatch is a tie only where the oracle's decision margins say so (tests/util.py: admissible); the rest is counted as
    # flag_mismatch / int_mismatch / beams_not_admitted or stays in "obs"
    st, worst = parity.campaign(eng, ora, "campaign " + mode, steps, lambda t: parity.stream_actions(stream, rng, n_envs), threads=64)
    ties = st["ties"]
    st["state_fields_x_tol"] = {k: round(v, 3) for k, v in worst.items()}
    st["mode"] = mode; st["seconds"] = round(time.time() - t0, 1)
    st["ties"] = dict(ties.summary(), cases=ties.cases, rejected=ties.rejected)  # admitted ties by class, with their margins
    print(json.dumps(st)); out.append(st); parity.close_engines()
open('gpurun_out/campaign.json','w').write(json.dumps(out,indent=1))
