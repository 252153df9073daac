"""The engine modes a feature is swept over (tests/test_partial_reset_gpu.py, tests/test_launch_forms_gpu.py): per mode the number of
envs, what Engine() is built from and the pgd_describe_step text that names the step kernel the mode is about; Setup builds the banks,
engines and action streams of a mode; step_all / state_of / assert_same_state / mask_of compare twin engines bit for bit.
Importing this module needs no GPU and creates no engine."""
import numpy as np

from pgdrive_amd import _abi
from tests import parity, util

EI = _abi.EI

TOLL = dict(tollgate=True, plain_reward=True, side_lasers=72, side_dist=20.0, lane_line_lasers=4, lane_line_dist=20.0,
            num_lasers=72, lidar_dist=20.0, speed_reward=0.0, overspeed_penalty=0.5, min_pass_steps=30)
ONE_ENV = "k_step: one env per wave"
# mode -> envs, what Engine() is built from, and the pgd_describe_step text that names the mode's step kernel
MODES = dict(
    default=dict(n=64, kw=dict(num_traffic=16, num_lasers=240), name=ONE_ENV + ", specialised for the default single-agent configuration"),
    general=dict(n=64, kw=dict(num_traffic=12, num_lasers=72, side_lasers=6, side_dist=50.0, lane_line_lasers=4, lane_line_dist=20.0,
                               discrete_action=True), name=ONE_ENV, general=True),
    pack=dict(n=65, env=dict(PGD_PACK="1"), kw=dict(), name="throughput mode"),  # three envs per wave: 65 leaves the last wave partly empty
    ego_only=dict(n=66, kw=dict(num_traffic=0, num_lasers=0), name="specialised for the ego-only"),  # four envs per wave
    imask_40=dict(n=48, env=dict(PGD_IMASK="1"), kw=dict(num_traffic=40), name=ONE_ENV, general=True),
    safe=dict(n=48, n_maps=16, kw=dict(num_traffic=56, accident_prob=0.8, safe_rl_env=True, density=0.05, use_lateral=False),
              name="specialised for the SafePGDriveEnv"),
    marl8=dict(n=48, marl=(8, "roundabout"), kw=dict(), name="multi-agent configuration with 8 agent seats x 72 beams"),
    marl40=dict(n=48, marl=(40, "roundabout"), kw=dict(), name="multi-agent configuration with 40 agent seats x 72 beams"),
    # neighbour rows that are state vectors, one block per row (PGD_ROW_OBSERVE): k_observe after the step, which forgets the zero-row marks
    marl8_rows=dict(n=48, marl=(8, "roundabout"), env=dict(PGD_ROW_OBSERVE="1"), kw=dict(others_state=True, num_others=4), name=ONE_ENV,
                    general=True),
    parking=dict(n=48, marl=(8, "parking"), kw=dict(parking=True, enable_reverse=True), name=ONE_ENV, general=True),
    tollgate=dict(n=48, marl=(8, "tollgate"), kw=dict(TOLL), name=ONE_ENV, general=True),
    # the default step kernel without the fused row: the stand-alone k_observe<256> (one block per row) writes it after the step
    no_fuse=dict(n=64, env=dict(PGD_NO_FUSE="1"), kw=dict(num_traffic=16, num_lasers=240),
                 name=ONE_ENV + ", specialised for the default single-agent configuration"),
    no_lidar=dict(n=64, kw=dict(num_traffic=16, num_lasers=0), name="specialised for the top-down envs"),  # D = 18
    # odd row widths: the 4-byte side of every store-width guard of the observation code (even widths take the 8-byte side)
    odd_std=dict(n=64, kw=dict(num_traffic=16, num_lasers=241), name=ONE_ENV, general=True),  # the default row layout, fused row, D = 275
    odd_fans=dict(n=64, kw=dict(num_traffic=12, num_lasers=71, side_lasers=5, side_dist=50.0, lane_line_lasers=3, lane_line_dist=20.0),
                  name=ONE_ENV, general=True),  # D = 111
    odd_pack=dict(n=65, env=dict(PGD_PACK="1"), kw=dict(num_traffic=16, num_lasers=241), name="throughput mode", general=True),
    # the beam count is a run-time value of the instantiation for the multi-agent defaults (PGD_FIXM_FIELDS): 73 beams run it, without
    # the folded seat count of the 72- and 240-beam instantiations.  8 seats: rows appended to the step, D = 91; 40 seats: the four-wave
    # k_observe_env behind the step, which writes the rows' state blocks (state_rows)
    odd_marl8=dict(n=48, marl=(8, "roundabout"), kw=dict(num_lasers=73), name=ONE_ENV + ", specialised for the default multi-agent configuration"),
    odd_marl40=dict(n=48, marl=(40, "roundabout"), kw=dict(num_lasers=73),
                    name=ONE_ENV + ", specialised for the default multi-agent configuration"),
)


class Setup:
    """The banks of a mode and engines of its configuration (every engine is closed when the test ends)."""
    def __init__(self, descs, mode):
        m = self.m = MODES[mode]
        self.mode, self.n = mode, m["n"]
        base = dict(dict(horizon=60, seed=7), **m["kw"])
        if "marl" in m:
            seats, kind = m["marl"]
            _, self.mb, self.sb = util.make_marl_banks(num_agents=seats, capacity=seats, kind=kind)
            self.make = lambda **kw: util.marl_config(self.n, self.sb, **dict(base, **kw))
        else:
            self.mb, self.sb, _ = parity.banks_and_config(descs, self.n, m.get("n_maps", 8), **base)
            self.make = lambda **kw: _abi.make_config(self.n, **{k: v for k, v in dict(base, **kw).items() if k in parity.CONFIG_KEYS})
        self.n_scen = len(self.sb.scenarios)
        self.A = self.sb.A if "marl" in m else 1

    def engine(self, env=None, **cfg_kw):
        return parity.engine(self.make(**cfg_kw), self.mb, self.sb, env=dict(self.m.get("env", {}), **(env or {})))

    def oracle(self, **cfg_kw):
        return parity.oracle(self.make(**cfg_kw), self.mb, self.sb)

    def actions(self, seed=17):
        rng = np.random.default_rng(seed)
        if self.A > 1:
            return lambda t: util.marl_actions(rng, self.n, self.A)
        if self.m["kw"].get("discrete_action"):
            return lambda t: rng.integers(0, 5, size=(self.n, 1, 2)).astype(np.float32)
        return parity.driving_with_bursts(rng, self.n)

    def stagger(self, *engines):
        """The discrete actions of the `general` mode only ever brake (upstream clips them before the conversion): its episodes end
        by the horizon alone, all in the same step.  Give the envs different step counts so that the lists differ from step to step."""
        if self.m["kw"].get("discrete_action"):
            f, i, ei = engines[0].get_state()
            ei[EI["EP_STEPS"]] = np.arange(self.n) % 37
            for e in engines:
                e.set_state(f, i, ei)

    def check_name(self, eng):
        """the step kernel the mode is about has run (a case cannot silently test another one)"""
        desc = eng.describe_step()
        assert self.m["name"] in desc and ("specialised" not in desc) == bool(self.m.get("general")), desc

    @property
    def tail(self):
        return 2 if self.m["kw"].get("tollgate") else 0  # the toll floats stand behind the lidar


def step_all(engines, act):
    """One step of every engine on the same actions: the four outputs of each, cloned, after a sync."""
    import torch
    at = torch.from_numpy(act).to(engines[0].device)
    outs = [[x.clone() for x in e.step(at)] for e in engines]
    for e in engines:
        e.sync()
    return outs


def state_of(eng, skip=("EPISODES", )):
    """(float state as int32 bits, integer state, env counters without `skip`); pgd_get_state masks EI_NEAR itself"""
    f, i, ei = eng.get_state()
    return f.view(np.int32), i, ei[[k for name, k in EI.items() if name not in skip]]


def assert_same_state(sa, sb, envs, what):
    """bit-identical state of the envs `envs` (bool [N])"""
    for xa, xb, name in zip(sa, sb, ("float state", "integer state", "env counters")):
        assert np.array_equal(xa[:, envs], xb[:, envs]), "%s: %s differs in envs %s" % (what, name, np.nonzero((xa != xb).reshape(len(xa), len(envs), -1).any(axis=(0, 2)) & envs)[0][:8])


def mask_of(n, ids):
    m = np.zeros(n, dtype=bool)
    m[np.asarray(ids, dtype=np.int64)] = True
    return m
