"""What the CPU tests of the collectors' host logic share (test_return_norm_cpu, test_timelimit_cpu, test_rollout_episodes_cpu): one fake
Engine on CPU tensors that records every call by name, its scripts, and the collectors built on it."""
import types

import numpy as np

from tests import actor_critic_ref as ar
from tests import marl_rollout_ref as mr
from tests import return_norm_ref as rn
from tests import rollout_episodes_ref as er
from tests import safe_ppo_ref as sr
from tests import timelimit_ref as tl

N, A, D, T = 5, 3, 6, 7
W6 = tuple(range(6))   # the weights are handed through, never looked at
TODAY = {"obs", "actions", "logp", "values", "rewards", "dones", "flags", "advantages", "returns"}
TODAY_SAFE = TODAY | {"costs", "cost_values", "cost_advantages", "cost_returns", "ep_cost_sum", "ep_cost_count"}
TODAY_MARL = TODAY | {"mask", "index", "count"}
PRIME = ["actor_critic_tick", "%s", "actor_critic_tick"]
CALLS = dict(single=("mlp_actor_critic", ["step", "mlp_actor_critic"], ["gae"], []),
             safe=("mlp_actor_critic_cost", ["step", "mlp_actor_critic_cost"], ["gae"], ["cost_gae"]),
             marl=("mlp_actor_critic_rows", ["step", "live_rows", "mlp_actor_critic_rows"], ["gae_masked", "rollout_index"], []))


class RecordingEngine:
    """What the collectors ask of an Engine, on CPU tensors: every call is recorded by name.  The step writes the script's (reward, done,
    flags) of its step number, the networks write the constants `value` and `cost_value`, and every GAE form, return_norm and
    rollout_episodes are the float64 checkers."""
    def __init__(self, N, A, D, script, value=0.5, cost_value=0.25, step_info=None):
        import torch
        self.torch, self.N, self.A, self.D, self.device = torch, N, A, D, "cpu"
        self.obs = torch.zeros((N, A, D))
        self.step_info = step_info
        self.calls, self.script, self.value, self.cost_value, self.t = [], script, value, cost_value, 0

    def _write(self, pairs):
        for dst, src in pairs:
            dst.copy_(self.torch.from_numpy(np.asarray(src)).to(dst.dtype).view(dst.shape))

    def sync(self):
        self.calls.append("sync")

    def get_state(self):
        from pgdrive_amd import _abi
        si = np.zeros((_abi.NI, self.N, self.A), dtype=np.int32)
        si[_abi.SI["STATUS"]] = _abi.ST_ACTIVE
        return None, si, None

    def enable_step_info(self, costs=(1.0, 1.0, 1.0), final_obs=True):
        self.calls.append("enable_step_info(final_obs=%r)" % final_obs)
        self.step_info = {"final_observation": self.torch.full((self.N, self.D), float("nan")) if final_obs else None}
        return self.step_info

    def actor_critic_tick(self, counter):
        self.calls.append("actor_critic_tick")

    def mlp_actor_critic(self, pw, vw, out, logp, value, seed, tick, obs=None, **kw):
        self.calls.append("mlp_actor_critic")
        value.fill_(self.value)

    def mlp_actor_critic_cost(self, pw, vw, cw, out, logp, value, cost_value, seed, tick, obs=None, **kw):
        self.calls.append("mlp_actor_critic_cost")
        value.fill_(self.value)
        cost_value.fill_(self.cost_value)

    def mlp_actor_critic_rows(self, pw, vw, rows, count, out, logp, value, seed, tick, obs=None, **kw):
        self.calls.append("mlp_actor_critic_rows")
        value.fill_(self.value)

    def mlp_terminal_value(self, vw, cw, term_obs, flags, done, term_value, term_cost_value=None, **kw):
        from pgdrive_amd.rollout import truncated
        self.calls.append("mlp_terminal_value")
        assert term_obs is self.step_info["final_observation"] and (cw is None) == (term_cost_value is None)
        tr = truncated(flags, done)
        term_value.copy_(tr.to(term_value.dtype) * self.value)
        if term_cost_value is not None:
            term_cost_value.copy_(tr.to(term_value.dtype) * self.cost_value)

    def live_rows(self, flags, done, rows=None, count=None, group=-1):
        self.calls.append("live_rows")

    def rollout_index(self, flags, index=None, count=None):
        self.calls.append("rollout_index")

    def step(self, actions, out=None):
        self.calls.append("step")
        obs, rew, done, flags = out
        r, d, f = [x[self.t % len(x)] for x in self.script]
        self._write(((rew, r), (done, d), (flags, f)))
        self.t += 1

    def gae(self, reward, value, done, gamma, lam, adv=None, ret=None):
        self.calls.append("gae")
        self.gae_reward = reward
        a, r = ar.gae_f64(reward.numpy(), value.numpy(), done.numpy(), gamma, lam)
        self._write(((adv, a), (ret, r)))

    def gae_bootstrap(self, reward, value, done, term_value, gamma, lam, adv=None, ret=None):
        self.calls.append("gae_bootstrap")
        a, r = tl.gae_bootstrap_f64(reward.numpy(), value.numpy(), done.numpy(), term_value.numpy(), gamma, lam)
        self._write(((adv, a), (ret, r)))

    def gae_masked(self, reward, value, done, flags, gamma, lam, adv=None, ret=None, mask=None):
        self.calls.append("gae_masked")
        self.gae_reward = reward
        a, r, m = mr.gae_masked_f64(reward.numpy(), value.numpy(), done.numpy(), flags.numpy().view(np.uint32), gamma, lam)
        self._write(((adv, a), (ret, r), (mask, m)))

    def _write_costs(self, ref, cost, adv, ret, run, ep_sum, ep_count):
        self._write(((cost, ref["cost"]), (adv, ref["cadv"]), (ret, ref["cret"]), (run, ref["run"]), (ep_sum, ref["ep_sum"]), (ep_count, ref["ep_count"])))

    def cost_gae(self, flags, done, cost_value, costs, gamma, lam, run, cost=None, adv=None, ret=None, ep_sum=None, ep_count=None):
        self.calls.append("cost_gae")
        ref = sr.cost_gae_f64(flags.numpy(), done.numpy(), cost_value.numpy(), costs, gamma, lam, run.numpy())
        self._write_costs(ref, cost, adv, ret, run, ep_sum, ep_count)

    def cost_gae_bootstrap(self, flags, done, cost_value, term_cost_value, costs, gamma, lam, run, cost=None, adv=None, ret=None, ep_sum=None,
                           ep_count=None):
        self.calls.append("cost_gae_bootstrap")
        ref = tl.cost_gae_bootstrap_f64(flags.numpy(), done.numpy(), cost_value.numpy(), term_cost_value.numpy(), costs, gamma, lam, run.numpy())
        self._write_costs(ref, cost, adv, ret, run, ep_sum, ep_count)

    def return_norm_work_bytes(self, rows):
        return 24 * ((rows + 63) // 64)

    def return_norm_state(self, rows):
        t = self.torch
        return t.zeros((rows, ), dtype=t.float32), t.tensor(rn.RECORD_INIT, dtype=t.float64)

    def return_norm(self, reward, done, gamma, carry, record, flags=None, eps=1e-8, clip=10.0, freeze=False, out=None, work=None):
        self.calls.append("return_norm(freeze=%r)" % bool(freeze))
        assert work.numel() * work.element_size() >= self.return_norm_work_bytes(carry.numel())
        ref = rn.return_norm_f64(reward.numpy(), done.numpy(), gamma, carry.numpy().reshape(reward.shape[1:]), record.numpy(),
                                 flags=None if flags is None else flags.numpy(), eps=eps, clip=clip, freeze=freeze)
        self._write(((carry, ref["carry"]), (record, ref["record"]), (out, ref["scaled"])))
        return out

    def rollout_episodes_work_bytes(self, rows):
        return 128 * ((rows + 63) // 64)

    def rollout_episodes_state(self, rows):
        t = self.torch
        return t.zeros((rows, ), dtype=t.float32), t.zeros((rows, ), dtype=t.int32), t.tensor(er.INIT, dtype=t.float64)

    def rollout_episodes(self, reward, done, flags, ret_carry, len_carry, record=None, call=None, seats=False, ep_return=None, ep_length=None,
                         work=None):
        self.calls.append("rollout_episodes(seats=%r)" % bool(seats))
        self.episode_reward = reward
        assert work.numel() * work.element_size() >= self.rollout_episodes_work_bytes(ret_carry.numel())
        ref = er.by_definition(reward.numpy(), done.numpy(), flags.numpy(), ret_carry.numpy(), len_carry.numpy(), seats=seats)
        self._write(((ret_carry, ref["ret_carry"]), (len_carry, ref["len_carry"]), (call, ref["call"]),
                     (record, er.merge_record(record.numpy(), ref["call"])), (ep_return, ref["ep_return"]), (ep_length, ref["ep_length"])))
        return record, call


class AllSwitchesEngine(RecordingEngine):
    """RecordingEngine with the two switches it lacks, as recorded calls that move their state: the observation normalisation (the fold
    counts the rows it was given) and the guardian (the takeover state alternates with the tick)."""
    cfg = types.SimpleNamespace(idm_agent=False, discrete_action=False, lidar_gaussian_noise=0.0, lidar_dropout_prob=0.0, num_lasers=40)

    def obs_norm_work_bytes(self, D, rows):
        return 8

    def obs_norm_state(self, D):
        t = self.torch
        return t.zeros((1 + 2 * D, ), dtype=t.float64), t.zeros((2, (D + 3) & ~3), dtype=t.float32)

    def obs_norm_publish(self, record, table, eps=1e-8):
        self.calls.append("obs_norm_publish")

    def obs_norm_bind(self, table, D, clip):
        self.calls.append("obs_norm_bind")

    def obs_norm_update(self, obs, record, index=None, count=None, n_list=None, work=None):
        self.calls.append("obs_norm_update")
        record.add_(float(n_list))

    def guardian(self, weights, save_level, agent, state, applied, info, seed, tick, **kw):
        self.calls.append("guardian")
        state.copy_((self.torch.arange(state.numel()) + tick) % 2)


def script(shape, marl):
    """(reward, done, flags) of 3 T steps: integer rewards times 25 (returns in the hundreds), dones at rate 0.2 or a seat history."""
    rng = np.random.default_rng(3)
    reward = rng.integers(-8, 9, size=(3 * T, *shape)).astype(np.float32) * 25.0
    if marl:
        flags, done = rn.seat_history(rng, 3 * T, int(np.prod(shape)))
        return reward, done.reshape(reward.shape), flags.reshape(reward.shape)
    done = (rng.uniform(size=reward.shape) < 0.2).astype(np.uint8)
    return reward, done, (done.astype(np.int32) * (32 | 1 << 16))


def truncation_script(reward, trunc):
    """(reward, done, flags) of a constant reward and a boolean [steps, N] `trunc`: PGD_F_MAX_STEP | PGD_F_RESET and a done where it is set."""
    return np.full(trunc.shape, reward, np.float32), trunc.astype(np.uint8), trunc.astype(np.int32) * (32 | 1 << 16)


def collector(kind, engine=RecordingEngine, **kw):
    """-> (engine, collector of `kind` on it), gamma = lam = 0.5."""
    from pgdrive_amd.rollout import MultiAgentRolloutCollector, RolloutCollector, SafeRolloutCollector
    marl = kind == "marl"
    eng = engine(N, A if marl else 1, D, script((N, A) if marl else (N, ), marl))
    if kind == "safe":
        return eng, SafeRolloutCollector(eng, W6, W6, W6, T, gamma=0.5, lam=0.5, **kw)
    return eng, (MultiAgentRolloutCollector if marl else RolloutCollector)(eng, W6, W6, T, gamma=0.5, lam=0.5, **kw)
