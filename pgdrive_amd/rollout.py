"""On-device PPO rollouts of a single-agent engine: T steps of policy -> step with the sampled action, its log-probability and the
value estimate from one launch per step (Engine.mlp_actor_critic), then advantages and returns (Engine.gae).

What a trainer otherwise composes per step from framework ops -- two networks of three GEMMs, a randn, the log-probability, and a
python loop over T for GAE -- around env.step (the reference: `expert(obs, deterministic=False)` and `value(obs)` of
pgdrive/examples/ppo_expert/numpy_expert.py:38-78 per env and step, GAE in the RL library).

    col = RolloutCollector(env, policy_weights, value_weights, T=128)
    while training:
        batch = col.collect()                 # a dict of cuda tensors, valid until the next collect()
        ... update the networks from batch ...
        col.set_weights(new_policy_weights, new_value_weights)

Layout: every tensor is time-major and preallocated once; row t + 1 of the observation, action, log-probability and value arrays is what
the step of row t produced and what the networks made of it, so the step writes its observation, reward and done STRAIGHT into the
rollout (Engine.step(out=...)) and the networks read and write it in place: no copy per step.  Row T (the observation behind the last
step, its action, log-probability and value -- the bootstrap of GAE) is carried into row 0 of the next rollout by four row copies per
collect(): every observation is evaluated exactly once, with the weights of the rollout it was observed in, and the action stream
stays the sampled one.  Nothing in collect() waits for the device.

The noise of evaluation j (counted over the collector's life) is that of tick j: the kernel adds its `tick` argument (the row, 0 .. T)
to a counter in device memory that collect() advances by T on the stream, so a collect() captured in a HIP graph draws new noise at every
replay and equals the eager call bit for bit.

A done ends the episode for GAE, whatever ended it: there is no bootstrap through a horizon truncation from the terminal observation.
bootstrap_truncations=True (RolloutCollector, SafeRolloutCollector) changes that: the critic's value of the terminal observation of every
env a step truncated is computed in that step and GAE takes it as the one-step target (`truncated`, below).

Constrained RL on the safe env: SafeRolloutCollector, below -- this collector with a cost critic in the step's launch, the costs
from the flags, their GAE and the books of episode costs.

Multi-agent engines: MultiAgentRolloutCollector, below -- the same layout and carry with a seat axis, the networks over the rows of live
seats only, GAE per agent and not per seat, and the index of the transitions a trainer may use.

normalise_rewards=True (every collector): GAE reads the rewards divided by the standard deviation of the running discounted return -- the
norm_reward half of Stable-Baselines3's VecNormalize, one call behind the T steps (Engine.return_norm).  The collector
owns the running return of every row and the record (count, mean, m2, scale) on the device; a rollout is divided by the scale that
already includes its own samples, then clamped to [-clip_reward, clip_reward].  The batch gains scaled_rewards [T, ...] and return_norm
(the record, float64 [4]); `rewards` stays raw.  The critic then learns in scaled units (with bootstrap_truncations its terminal values
are in those units already: they are its own outputs).  The safe collector's costs are not scaled: the cost limit is in raw cost units.
state_dict() / load_state_dict() hold the running returns and the record for a checkpoint; freeze_return_norm(True) stops both from
moving, for evaluation rollouts.  False (the default): the calls and the batch of before.

episode_stats=True (every collector): how the policy is doing -- return, length and the causes of the end of every episode that finished,
gym's RecordEpisodeStatistics as one call behind the T steps (Engine.rollout_episodes).  The collector owns the return
and the length of every row's unfinished episode and two records of 16 doubles (_abi.ROLLOUT_EPISODES) on the device: the running one
and the last rollout's.  The call reads the RAW rewards, whatever normalise_rewards says; the multi-agent collector makes it per seat
(an agent's episode ends at its done or at an env-wide restart).  The batch gains episode_stats (the running record, float64 [16]),
episode_stats_rollout, and ep_returns float32 / ep_lengths int32 [T, ...]: the finished episode's return and length at the entry where it
ended, 0 everywhere else.  episode_summary() reads a record as a dict (one synchronisation), clear_episode_stats() starts the running
record afresh and keeps the unfinished episodes; state_dict() holds the carries and the running record.  False (the default): no new
tensor, batch key or engine call.

normalise_obs=True, clip_obs, obs_eps (every collector): the networks are fed clip((obs - mean) / sqrt(var + obs_eps), -clip_obs, clip_obs)
with the running mean and variance of every observation column -- the norm_obs half of VecNormalize.  No normalised
copy exists: the collector owns the record (n, means, sums of squared deviations: float64 [1 + 2 D]), the table the kernels read (float32
[2, Dp]: shift | scale) and the scratch on the device; Engine.obs_norm_bind makes the network launches normalise the rows as they load
them.  collect() publishes the record into the table first, carries row T into row 0, binds the table around the T steps (the
terminal-value launch of bootstrap_truncations included), unbinds, and -- unless frozen -- folds obs[:T] into the record with one
Engine.obs_norm_update behind GAE (the multi-agent collector: the rows of batch["index"] / batch["count"] only, those at which an agent
acted).  prime() publishes before its evaluation.  So a rollout is collected AND trained on with one table (it changes only at the next
collect(); PPOLearner.update binds the same table); every observation is folded exactly once, row T as row 0 of the next rollout; and the
carried row 0 was evaluated under the previous table, exactly as it was evaluated under the previous weights -- it is not evaluated
again.  Unlike SB3's RunningMeanStd there is no phantom initial count (mean 0, variance 1, count 1e-4): the record starts empty, the
first rollout runs on raw observations and the statistics are those of the samples alone.  The batch gains obs_norm (the table) and
obs_norm_record; batch["obs"] stays RAW.  freeze_obs_norm(True) stops the record from moving, for evaluation rollouts; state_dict() holds
obs_norm_record (the table is republished by the next collect() / prime()).  Not served: the policy-only kernels (Engine.mlp_policy
ignores the binding), statistics exchanged between the ranks of a multi-GPU run, image observations.  False (the default): no new
tensor, batch key or engine call.

guardian=dict(weights=..., save_level=0.5, deterministic=False, immediate=False) (RolloutCollector, SafeRolloutCollector): the expert
guardian of the reference's use_saver / save_level (policy/AI_protect_policy.py; Engine.guardian) watches the rollout.
Per step t, behind the evaluation of row t, one more launch reads the sampled action of row t, observation row t and the flags of step
t - 1 and writes the action the step is to apply into a buffer of its own; the step reads that buffer.  `weights`: the expert's six
policy tensors (cuda float32), fc_1 with D rows, or with D + 1 rows for the reference's shipped expert.  The expert's noise is drawn with
seed ^ GUARDIAN_SEED_XOR and the tick of the row's evaluation, so it is not the agent's.  The batch gains applied_actions [T, N, 2],
takeover uint8 [T, N] (bit 0 takeover, 1 takeover_start, 2 takeover_end) and expert_actions [T, N, 2] (a view of guardian_trace
[T, N, 4]: expert steering, throttle, lateral float, f).  `actions`, `logp` and `values` stay the agent's OWN -- what it sampled, whatever
was applied; what a trainer makes of the difference is the trainer's business.  A bound observation normalisation does not reach the
expert.  The takeover state [N] survives from rollout to rollout and is part of state_dict() (guardian_state).  None (the default): the
launches and the batch of before.

action_head="categorical", bins=(ks, kt) (RolloutCollector, MultiAgentRolloutCollector): the policy is two independent categorical
distributions over ks steering and kt throttle bins in place of the Gaussian (Engine.mlp_actor_critic_cat / _cat_rows; DESIGN section
33), 2 <= ks, kt and ks + kt <= 16, the policy's w3 [256, >= ks + kt].  The collector owns action_index [T + 1, rows, 2] int32, carried like
`actions`; the batch gains action_index [T, ...]; `actions` stays what the step was fed -- the grid value i * 2 / (K - 1) - 1 of the
sampled index on an engine with continuous actions (recommended), the index itself on a discrete_action engine, whose dims the bins must
equal.  No other switch looks at the head, so they compose unchanged; the guardian and the safe collector refuse it.  "gaussian" (the
default): the launches and the batch of before; on a discrete_action engine that still means Gaussian samples clipped and converted by
the step, and one warning that says so.
"""
import numpy as np

GUARDIAN_SEED_XOR = 0x6a7d1a4b  # the guardian's noise seed = the collector's (the vec env's) seed ^ this: the expert's draws are not the agent's

F_NATURAL = 1 | 2 | 4 | 8 | 16   # PGD_F_ARRIVE | OUT_OF_ROAD | CRASH_VEHICLE | CRASH_OBJECT | CRASH_BUILDING
F_CRASH_COST = 4 | 8             # PGD_F_CRASH_VEHICLE | CRASH_OBJECT: with safe_rl_env a cost, not a termination
F_MAX_STEP = 32                  # PGD_F_MAX_STEP


def truncated(flags, done, safe_rl_env=False):
    """Which dones of a single-agent step are truncations (include/pgdrive_hip.h, `truncated`): the step set PGD_F_MAX_STEP (horizon or
    the scenario's max_steps) and none of its own causes of a done; a termination on the same step wins.  `flags`, `done`: numpy arrays
    or torch tensors of one shape (or python ints) -> a bool array / tensor of that shape."""
    natural = (flags & F_NATURAL) != 0
    if safe_rl_env:
        natural = natural & ((flags & F_CRASH_COST) == 0)
    return (done != 0) & ((flags & F_MAX_STEP) != 0) & ~natural


def action_head_options(name, action_head, bins, w3_cols, discrete_action=False, discrete_dims=None, guardian=None, safe=False):
    """A collector's head switches checked -> (head, bins or None, emit_index).  No device needed.  "gaussian" (the default): bins must be
    None; on a discrete_action engine the behaviour of before stays (the step clips and converts the Gaussian samples) and ONE warning
    names action_head="categorical".  "categorical": bins = (ks, kt) required, 2 <= each, ks + kt <= 16 (ValueError); the policy's w3 needs
    ks + kt columns (ValueError); on a discrete_action engine the bins must be its (discrete_steering_dim, discrete_throttle_dim)
    (ValueError) and the launches emit the index; the guardian and the safe collector are refused (NotImplementedError)."""
    from . import _abi
    if action_head not in ("gaussian", "categorical"):
        raise ValueError("%s: action_head = %r is neither \"gaussian\" nor \"categorical\"" % (name, action_head))
    if action_head == "gaussian":
        if bins is not None:
            raise ValueError("%s: bins = %r come with action_head=\"categorical\"" % (name, bins))
        if discrete_action:
            import warnings
            warnings.warn("%s: a discrete_action engine is fed Gaussian samples, which the step clips to [-1, 1] and converts as if they were "
                          "indices; action_head=\"categorical\" with bins=%r samples the env's own MultiDiscrete space" %
                          (name, tuple(discrete_dims) if discrete_dims is not None else None), stacklevel=3)
        return "gaussian", None, False
    if bins is None:
        raise ValueError("%s: action_head=\"categorical\" needs bins=(steering, throttle)" % name)
    bins = _abi.cat_bins(bins, name)
    if safe:
        raise NotImplementedError("%s: the categorical head is not served by the three-network kernels of the safe path" % name)
    if guardian is not None:
        raise NotImplementedError("%s: the expert guardian compares continuous actions; it does not serve the categorical head" % name)
    if int(w3_cols) < sum(bins):
        raise ValueError("%s: the policy's w3 has %d columns, bins %r need %d" % (name, int(w3_cols), bins, sum(bins)))
    if discrete_action and tuple(int(d) for d in discrete_dims) != bins:
        raise ValueError("%s: bins %r on a discrete_action engine whose MultiDiscrete space is %r" % (name, bins, tuple(discrete_dims)))
    return "categorical", bins, bool(discrete_action)


class _Collector:
    """What the collectors share: the time-major buffers over rows of shape (N, ) or (N, A), the carry of row T into row 0, the tick
    protocol around the engine's launches and the step loop.  A subclass refuses the engines it does not serve and gives
    _evaluate(row) -- the networks on observation row `row` --, _stepped(t) -- between step t and that evaluation -- and _finish() --
    GAE and what follows it."""
    def _allocate(self, eng, rows, policy_weights, value_weights, T, gamma, lam, seed):
        t = eng.torch
        self.engine, self.T, self.gamma, self.lam, self.seed = eng, int(T), float(gamma), float(lam), int(seed)
        T, D, dev = self.T, eng.D, eng.device
        f32 = dict(dtype=t.float32, device=dev)
        self._obs = t.zeros((T + 1, *rows, D), **f32)
        self._actions = t.zeros((T + 1, *rows, 2), **f32)
        self._logp = t.zeros((T + 1, *rows), **f32)
        self.values = t.zeros((T + 1, *rows), **f32)
        self.rewards = t.zeros((T, *rows), **f32)
        self.dones = t.zeros((T, *rows), dtype=t.uint8, device=dev)
        self.flags = t.zeros((T, *rows), dtype=t.int32, device=dev)
        self.advantages = t.zeros((T, *rows), **f32)
        self.returns = t.zeros((T, *rows), **f32)
        self._tick = t.zeros((1, ), dtype=t.int32, device=dev)  # evaluations before this rollout (modulo 2^32)
        self._carry = (self._obs, self._actions, self._logp, self.values)
        self._checkpointed = []  # (key, the attribute that holds its tensor, what the switch's state is called, the switch when off, on)
        self._primed = False
        self.set_weights(policy_weights, value_weights)
        self.batch = dict(obs=self._obs[:T], actions=self._actions[:T], logp=self._logp[:T], values=self.values, rewards=self.rewards,
                          dones=self.dones, flags=self.flags, advantages=self.advantages, returns=self.returns)

    def set_weights(self, policy_weights, value_weights):
        """The networks of the rollouts from now on (between two collect() calls): tuples as for Engine.mlp_actor_critic."""
        self.policy_weights, self.value_weights = tuple(policy_weights), tuple(value_weights)

    @staticmethod
    def _head_options(name, eng, policy_weights, action_head, bins, guardian=None, safe=False):
        """action_head_options for this engine and policy (in front of _allocate: a refusal allocates nothing)."""
        cfg = getattr(eng, "cfg", None)  # (an engine stand-in of the tests has none: continuous actions)
        discrete = bool(getattr(cfg, "discrete_action", 0))
        dims = (int(cfg.discrete_steering_dim), int(cfg.discrete_throttle_dim)) if discrete else None
        w3 = tuple(policy_weights)[4]
        return action_head_options(name, action_head, bins, int(w3.shape[1]) if hasattr(w3, "shape") else 0, discrete, dims, guardian, safe)

    def _head(self, head):
        """The policy head (behind _allocate; `head`: what _head_options returned).  Categorical: the collector owns action_index
        [T + 1, rows, 2] int32, carried row T -> 0 like `actions`, and the batch gains action_index [T, ...]; `actions` stays what the step
        was fed (the grid value, or the index on a discrete_action engine)."""
        self.action_head, self.bins, self.emit_index = head
        if self.action_head != "categorical":
            return
        t = self.engine.torch
        self._action_index = t.zeros(self._actions.shape, dtype=t.int32, device=self.engine.device)
        self._carry = self._carry + (self._action_index, )
        self.batch.update(action_index=self._action_index[:self.T])

    def _checkpoint(self, on, what, off, **entries):
        """A switch's setup says what state_dict() holds for it -- key=the name of the attribute that holds the tensor -- and what
        load_state_dict() calls that state and the switch when it refuses its keys."""
        self._checkpointed += [(key, attr, what, off, bool(on)) for key, attr in entries.items()]

    def _normalise(self, normalise_rewards, clip_reward, reward_eps):
        """The reward side of VecNormalize (behind _allocate): switched on, the collector owns the running returns, the record, the
        scratch and scaled_rewards, and the batch gains scaled_rewards and return_norm."""
        self.normalise_rewards, self.clip_reward, self.reward_eps = bool(normalise_rewards), float(clip_reward), float(reward_eps)
        self._rn_frozen = False
        self._checkpoint(self.normalise_rewards, "a reward normalisation state", "normalise_rewards=False", return_norm_carry="_rn_carry",
                         return_norm="return_norm")
        if not self.normalise_rewards:
            return
        if not self.reward_eps >= 0.0:
            raise ValueError("%s: reward_eps = %r" % (type(self).__name__, reward_eps))
        eng, t = self.engine, self.engine.torch
        rows = self.rewards[0].numel()
        self.scaled_rewards = t.zeros_like(self.rewards)
        self._rn_carry, self.return_norm = eng.return_norm_state(rows)
        self._rn_work = t.empty(((eng.return_norm_work_bytes(rows) + 7) // 8, ), dtype=t.float64, device=eng.device)
        self.batch.update(scaled_rewards=self.scaled_rewards, return_norm=self.return_norm)

    def _gae_rewards(self, flags=None):
        """The rewards GAE reads: the rollout's own, or (normalise_rewards) scaled by the running return -- one Engine.return_norm call."""
        if not self.normalise_rewards:
            return self.rewards
        return self.engine.return_norm(self.rewards, self.dones, self.gamma, self._rn_carry, self.return_norm, flags=flags, eps=self.reward_eps,
                                       clip=self.clip_reward, freeze=self._rn_frozen, out=self.scaled_rewards, work=self._rn_work)

    def _obs_norm(self, normalise_obs, clip_obs, obs_eps):
        """The observation side of VecNormalize (behind _allocate): switched on, the collector owns the record, the table and the
        scratch of the fold, and the batch gains obs_norm and obs_norm_record."""
        self.normalise_obs, self.clip_obs, self.obs_eps = bool(normalise_obs), float(clip_obs), float(obs_eps)
        self._on_frozen = False
        self._checkpoint(self.normalise_obs, "an observation normalisation state", "normalise_obs=False", obs_norm_record="obs_norm_record")
        if not self.normalise_obs:
            return
        eng, t, name = self.engine, self.engine.torch, type(self).__name__
        if not (self.clip_obs > 0.0 and self.obs_eps >= 0.0):
            raise ValueError("%s: clip_obs = %r, obs_eps = %r" % (name, clip_obs, obs_eps))
        need = eng.obs_norm_work_bytes(eng.D, self.rewards.numel())
        if need == 0:
            raise ValueError("%s: the observation width %d is outside what pgd_obs_norm_update accepts" % (name, eng.D))
        self.obs_norm_record, self.obs_norm = eng.obs_norm_state(eng.D)
        self._on_work = t.empty(((need + 7) // 8, ), dtype=t.float64, device=eng.device)
        self.batch.update(obs_norm=self.obs_norm, obs_norm_record=self.obs_norm_record)

    def _publish_obs_norm(self):
        """The record, as the last fold left it, into the table: in front of everything prime() / collect() evaluates."""
        if self.normalise_obs:
            self.engine.obs_norm_publish(self.obs_norm_record, self.obs_norm, eps=self.obs_eps)

    def _bind_obs_norm(self, bound):
        """The table bound around the network launches of prime() / collect(), as the tick counter is."""
        if self.normalise_obs:
            self.engine.obs_norm_bind(self.obs_norm if bound else None, self.engine.D, self.clip_obs)

    def _fold_obs(self, index=None, count=None):
        """The one fold of normalise_obs (the end of _finish()): obs[:T] into the record, every row or the listed ones."""
        if self.normalise_obs and not self._on_frozen:
            self.engine.obs_norm_update(self._obs[:self.T], self.obs_norm_record, index=index, count=count, n_list=self.rewards.numel(),
                                        work=self._on_work)

    def freeze_obs_norm(self, frozen=True):
        """Evaluation rollouts: from the next collect() on the record of normalise_obs is read and not written (True), or moves again
        (False).  Call it between two collect() calls; a captured collect() keeps the mode it was captured with."""
        self._on_frozen = bool(frozen)

    def _guardian(self, guardian):
        """The expert guardian (behind _allocate): switched on, the collector owns the takeover state, the applied actions, the info bits
        and the trace, and the batch gains applied_actions, takeover, expert_actions and guardian_trace."""
        self.guardian = None
        # (with the last flags row: the guardian of the next rollout's first step reads it)
        self._checkpoint(guardian is not None, "a guardian state", "guardian=None", guardian_state="_guard_state",
                         guardian_prev_flags="_guard_prev_flags")
        if guardian is None:
            return
        from . import _abi
        eng, t, name = self.engine, self.engine.torch, type(self).__name__
        g = dict(save_level=0.5, deterministic=False, immediate=False)
        unknown = set(guardian) - set(g) - {"weights"}
        if unknown or "weights" not in guardian:
            raise ValueError("%s: guardian takes weights, save_level, deterministic, immediate (got %s)" % (name, sorted(guardian)))
        g.update(guardian)
        g["weights"] = tuple(g["weights"])
        why = _abi.guardian_unserved(eng.cfg)
        if why:
            raise NotImplementedError("%s: the guardian with %s" % (name, why))
        if len(g["weights"]) != 6 or int(g["weights"][0].shape[0]) not in (eng.D, eng.D + 1):
            raise ValueError("%s: the guardian's expert takes %d inputs (or %d with the lateral float)" % (name, eng.D, eng.D + 1))
        self.guardian = g
        T, N, dev = self.T, eng.N, eng.device
        self.applied_actions = t.zeros((T, N, 2), dtype=t.float32, device=dev)
        self.takeover = t.zeros((T, N), dtype=t.uint8, device=dev)
        self.guardian_trace = t.zeros((T, N, 4), dtype=t.float32, device=dev)
        self._guard_state = t.zeros((N, ), dtype=t.uint8, device=dev)
        self._guard_prev_flags = self.flags[T - 1]
        self.batch.update(applied_actions=self.applied_actions, takeover=self.takeover, expert_actions=self.guardian_trace[..., :2],
                          guardian_trace=self.guardian_trace)

    def _applied(self, t):
        """The action buffer step t reads: the sampled row, or (guardian) what the guardian makes of it."""
        if self.guardian is None:
            return self._actions[t]
        g, T = self.guardian, self.T
        # (the flags of step t - 1: at t = 0 row T - 1 still holds the last step of the previous rollout -- zeros before the first)
        self.engine.guardian(g["weights"], g["save_level"], self._actions[t].view(-1, 1, 2), self._guard_state,
                             self.applied_actions[t].view(-1, 1, 2), self.takeover[t], self.seed ^ GUARDIAN_SEED_XOR, t,
                             prev_flags=self.flags[(t - 1) % T], trace=self.guardian_trace[t], obs=self._obs[t],
                             deterministic=g["deterministic"], immediate=g["immediate"])
        return self.applied_actions[t]

    def _episodes(self, episode_stats, seats=False):
        """The episode statistics (behind _normalise): switched on, the collector owns the carries, the two records, the scratch and
        ep_returns / ep_lengths, and the batch gains episode_stats, episode_stats_rollout, ep_returns and ep_lengths."""
        self.episode_stats, self._ep_seats = bool(episode_stats), bool(seats)
        self._checkpoint(self.episode_stats, "an episode statistics state", "episode_stats=False", episode_return_carry="_ep_ret_carry",
                         episode_length_carry="_ep_len_carry", episode_stats="episode_record")
        if not self.episode_stats:
            return
        eng, t = self.engine, self.engine.torch
        rows = self.rewards[0].numel()
        self._ep_ret_carry, self._ep_len_carry, self.episode_record = eng.rollout_episodes_state(rows)
        self._ep_init = self.episode_record.clone()
        self.episode_record_rollout = self.episode_record.clone()
        self.ep_returns = t.zeros_like(self.rewards)
        self.ep_lengths = t.zeros_like(self.flags)
        self._ep_work = t.empty(((eng.rollout_episodes_work_bytes(rows) + 7) // 8, ), dtype=t.float64, device=eng.device)
        self.batch.update(episode_stats=self.episode_record, episode_stats_rollout=self.episode_record_rollout, ep_returns=self.ep_returns,
                          ep_lengths=self.ep_lengths)

    def _episode_call(self):
        """The one call of episode_stats, on the raw rewards (in _finish())."""
        if self.episode_stats:
            self.engine.rollout_episodes(self.rewards, self.dones, self.flags, self._ep_ret_carry, self._ep_len_carry, record=self.episode_record,
                                         call=self.episode_record_rollout, seats=self._ep_seats, ep_return=self.ep_returns,
                                         ep_length=self.ep_lengths, work=self._ep_work)

    def episode_summary(self, rollout=False):
        """The running record (rollout: the last rollout's) as a dict, with the key names of Engine.episode_stats(): episodes,
        mean_return, std_return, min_return, max_return, mean_length, max_length, the rates arrive_rate, out_of_road_rate,
        crash_vehicle_rate, crash_object_rate, max_step_rate and cut_rate (the share of the episodes that ended with that flag set; cut:
        ended by an env-wide restart, without a done), and steps.  None where no episode ended.  One synchronisation: call it outside
        collect() and outside a graph capture."""
        if not self.episode_stats:
            raise ValueError("%s: episode_summary needs episode_stats=True" % type(self).__name__)
        from . import _abi
        rec = dict(zip(_abi.ROLLOUT_EPISODES, (self.episode_record_rollout if rollout else self.episode_record).cpu().numpy().tolist()))
        n = int(rec["episodes"])
        val = (lambda x: float(x)) if n else (lambda x: None)
        rate = (lambda k: rec[k] / n) if n else (lambda k: None)
        return dict(episodes=n, mean_return=val(rec["return_mean"]), std_return=val(np.sqrt(rec["return_m2"] / max(n, 1))),
                    min_return=val(rec["return_min"]), max_return=val(rec["return_max"]), mean_length=rate("length_sum"),
                    max_length=int(rec["length_max"]) if n else None, arrive_rate=rate("arrive"), out_of_road_rate=rate("out_of_road"),
                    crash_vehicle_rate=rate("crash_vehicle"), crash_object_rate=rate("crash_object"), max_step_rate=rate("max_step"),
                    cut_rate=rate("cut"), steps=int(rec["steps"]))

    def clear_episode_stats(self):
        """The running record starts afresh (a device copy; call it between two collect() calls, a captured collect() continues from
        it).  The carries stay: an unfinished episode is not lost."""
        if not self.episode_stats:
            raise ValueError("%s: clear_episode_stats needs episode_stats=True" % type(self).__name__)
        self.episode_record.copy_(self._ep_init)

    def freeze_return_norm(self, frozen=True):
        """Evaluation rollouts: from the next collect() on the running returns and the record are read and not written (True), or move
        again (False).  Call it between two collect() calls; a captured collect() keeps the mode it was captured with."""
        self._rn_frozen = bool(frozen)

    def state_dict(self):
        """Host copies of what the collector carries from rollout to rollout beside the engine's state, for a checkpoint.
        normalise_rewards: return_norm_carry (float32, one entry per row) and return_norm (float64 [4]: count, mean, m2, scale).
        episode_stats: episode_return_carry (float32) and episode_length_carry (int32), one entry per row, and episode_stats (the running
        record, float64 [16]).  normalise_obs: obs_norm_record (float64 [1 + 2 D]; the table is republished from it by the next
        collect() / prime()).  Empty with every switch off.  Waits for the device: call it outside collect() and outside a graph
        capture."""
        held = [(key, getattr(self, attr)) for key, attr, _, _, on in self._checkpointed if on]
        if not held:
            return {}
        self.engine.sync()
        return {key: x.cpu().numpy().copy() for key, x in held}

    def load_state_dict(self, state):
        """Put back what state_dict() returned (into the collector's own tensors: a captured collect() continues from them).  The keys of
        a switch this collector was built without are refused; those of its own switches must be there, with the collector's sizes."""
        t, name = self.engine.torch, type(self).__name__
        for key, attr, what, off, on in self._checkpointed:
            if not on and key in state:
                raise ValueError("%s: %s for a collector built with %s" % (name, what, off))
        put = []
        for key, attr, what, off, on in self._checkpointed:
            if not on:
                continue
            x = getattr(self, attr)
            src = t.from_numpy(np.ascontiguousarray(state[key]).reshape(-1)).to(x.dtype)
            if src.numel() != x.numel():
                raise ValueError("%s: %s whose %s holds %d values, %d here: a collector of other rows or observation columns" %
                                 (name, what, key, src.numel(), x.numel()))
            put.append((x, src))
        for x, src in put:
            x.view(-1).copy_(src)

    def _stepped(self, t):
        pass

    def prime(self):
        """Take the engine's present observation (what reset wrote into Engine.obs) as the start of the first rollout.  collect() calls
        it once by itself; call it before capturing collect() in a graph."""
        eng, T = self.engine, self.T
        self._obs[T].copy_(eng.obs.view(self._obs[T].shape))
        self._tick.sub_(T)  # (this evaluation is number 0: row T, counter -T)
        eng.actor_critic_tick(self._tick)
        self._publish_obs_norm()
        self._bind_obs_norm(True)
        self._evaluate(T)
        self._bind_obs_norm(False)
        eng.actor_critic_tick(None)
        self._tick.add_(T)
        self._primed = True

    def collect(self):
        """T steps.  Returns the dict of the collector's tensors (the same objects every time, valid until the next call):
        obs [T, N, D], actions [T, N, 2] (as sampled; the step clips), logp [T, N], values [T + 1, N], rewards, dones (uint8), flags,
        advantages, returns [T, N]."""
        eng, T = self.engine, self.T
        if not self._primed:
            self.prime()
        self._publish_obs_norm()  # (this rollout's table, and the update's behind it)
        for buf in self._carry:
            buf[0].copy_(buf[T])
        eng.actor_critic_tick(self._tick)  # (the engine's launches add the counter only while the collector is at work)
        self._bind_obs_norm(True)
        for t in range(T):
            eng.step(self._applied(t), out=(self._obs[t + 1], self.rewards[t], self.dones[t], self.flags[t]))
            self._stepped(t)
            self._evaluate(t + 1)
        self._bind_obs_norm(False)
        eng.actor_critic_tick(None)
        self._finish()
        self._tick.add_(T)
        return self.batch


class RolloutCollector(_Collector):
    """bootstrap_truncations=True: GAE bootstraps through a time limit.  The collector uses the engine's step info (it enables it with
    final_obs=True when it is off; an engine whose step info has no final_observation -- image observations -- is refused).  After every
    step one more launch (Engine.mlp_terminal_value) writes `term_values[t]`: the critic's value, with the weights of this rollout, of
    step_info["final_observation"] where the step truncated the env, 0 elsewhere; Engine.gae_bootstrap takes it as the one-step target
    of the done rows.  The batch gains term_values [T, N].  False (the default): the calls and the batch of before.
    normalise_rewards=True, clip_reward, reward_eps: GAE reads the rewards scaled by the running return (the module's docstring); the
    batch gains scaled_rewards [T, N] and return_norm (float64 [4]).
    episode_stats=True: the statistics of the episodes that finished (the module's docstring); the batch gains episode_stats,
    episode_stats_rollout (float64 [16]), ep_returns and ep_lengths [T, N].
    normalise_obs=True, clip_obs, obs_eps: the networks (the terminal-value launch included) read the observations normalised by their
    running mean and variance (the module's docstring); the batch gains obs_norm (float32 [2, Dp]) and obs_norm_record (float64
    [1 + 2 D]); `obs` stays raw.
    action_head="categorical", bins=(ks, kt): the policy is two independent categorical distributions over ks steering and kt throttle bins
    (Engine.mlp_actor_critic_cat) -- w3 [256, >= ks + kt].  The batch gains action_index int32 [T, N, 2]; `actions` is what
    the step was fed: the grid value i * 2 / (K - 1) - 1 on an engine with continuous actions (recommended for training), the index itself on
    a discrete_action engine, whose (discrete_steering_dim, discrete_throttle_dim) the bins must then equal.  Not with guardian=.  A
    discrete_action engine with the default Gaussian head behaves as before and warns once."""
    _SAFE = False  # (SafeRolloutCollector: the categorical head is refused)

    def __init__(self, env_or_engine, policy_weights, value_weights, T, gamma=0.99, lam=0.95, seed=0, bootstrap_truncations=False,
                 normalise_rewards=False, clip_reward=10.0, reward_eps=1e-8, episode_stats=False, normalise_obs=False, clip_obs=10.0,
                 obs_eps=1e-8, guardian=None, action_head="gaussian", bins=None):
        eng = getattr(env_or_engine, "engine", env_or_engine)
        if eng.A != 1:
            raise NotImplementedError(
                "RolloutCollector serves single-agent engines: with %d agent seats per env the rows of seats that are not due need a mask "
                "that this class does not know -- use MultiAgentRolloutCollector" % eng.A)
        if int(T) < 1:
            raise ValueError("RolloutCollector: T = %r" % (T, ))
        self.bootstrap_truncations = bool(bootstrap_truncations)
        if self.bootstrap_truncations:
            if eng.step_info is None:
                eng.enable_step_info(final_obs=True)
            if eng.step_info.get("final_observation") is None:
                raise ValueError("bootstrap_truncations needs the terminal observation of the step info, and this engine's step info has no "
                                 "final_observation (image observations: enable_step_info(final_obs=False))")
        head = self._head_options(type(self).__name__, eng, policy_weights, action_head, bins, guardian, self._SAFE)
        self._allocate(eng, (eng.N, ), policy_weights, value_weights, T, gamma, lam, seed)
        self._head(head)
        self._normalise(normalise_rewards, clip_reward, reward_eps)
        self._episodes(episode_stats)
        self._obs_norm(normalise_obs, clip_obs, obs_eps)
        self._guardian(guardian)
        if self.bootstrap_truncations:
            self.term_values = eng.torch.zeros((self.T, eng.N), dtype=eng.torch.float32, device=eng.device)
            self.batch.update(term_values=self.term_values)

    def _evaluate(self, row):
        if self.action_head == "categorical":
            self.engine.mlp_actor_critic_cat(self.policy_weights, self.value_weights, self.bins, self._actions[row], self._action_index[row],
                                             self._logp[row], self.values[row], self.seed, row, obs=self._obs[row], emit_index=self.emit_index)
            return
        self.engine.mlp_actor_critic(self.policy_weights, self.value_weights, self._actions[row], self._logp[row], self.values[row], self.seed,
                                     row, obs=self._obs[row])

    def _cost_side(self, t):
        """(cost_weights, term_cost_values[t]) of the terminal-value launch: none here."""
        return None, None

    def _stepped(self, t):
        if self.bootstrap_truncations:
            cw, tcv = self._cost_side(t)
            self.engine.mlp_terminal_value(self.value_weights, cw, self.engine.step_info["final_observation"], self.flags[t], self.dones[t],
                                           self.term_values[t], tcv)

    def _finish(self):
        self._episode_call()
        rewards = self._gae_rewards()
        if self.bootstrap_truncations:
            self.engine.gae_bootstrap(rewards, self.values, self.dones, self.term_values, self.gamma, self.lam, adv=self.advantages,
                                      ret=self.returns)
        else:
            self.engine.gae(rewards, self.values, self.dones, self.gamma, self.lam, adv=self.advantages, ret=self.returns)
        self._fold_obs()


class SafeRolloutCollector(RolloutCollector):
    """RolloutCollector for constrained RL on the safe env (SafePGDriveEnv: a crash is a cost, not a termination):

        col = SafeRolloutCollector(env, policy_weights, value_weights, cost_weights, T=128)
        batch = col.collect()        # RolloutCollector's batch plus the cost side

    A cost critic (a third network of the value network's shapes) is evaluated beside actor and critic by the ONE launch of every step
    (Engine.mlp_actor_critic_cost); its stream `cost_values` [T + 1, N] is carried from rollout to rollout like `values`.  Behind the T
    steps Engine.cost_gae turns the flags into costs -- out_of_road ? c0 : crash_vehicle ? c1 : crash_object ? c2 : 0, the precedence of
    PGDriveEnv.cost_function --, forms their advantages and returns (cost_gamma, cost_lam) and keeps the books of episode costs.
    `costs` = (out_of_road, crash_vehicle, crash_object); None: the three `*_cost` keys of the env's config, (1, 1, 1) for a bare engine.

    Batch additions: costs, cost_advantages, cost_returns [T, N]; cost_values [T + 1, N]; ep_cost_sum float32 and ep_cost_count int32 [N]
    -- the summed costs and the number of the episodes that FINISHED in this rollout, per env (what PPOLagLearner's multiplier reads).
    The cost of an env's unfinished episode is carried in the collector's `running_cost` [N]: a caller who resets envs by hand (rather
    than by the engine's auto reset, which reports a done) zeroes their entries.  A done finishes an episode for this bookkeeping
    whatever ended it, a horizon truncation included, as it does for GAE.  Nothing in collect() waits for the device, and a captured
    collect() equals the eager call bit for bit.

    bootstrap_truncations=True: as for RolloutCollector, with the cost critic in the same terminal-value launch; the batch gains
    term_values and term_cost_values [T, N], and Engine.cost_gae_bootstrap takes the latter as the cost side's one-step target.  The
    books of episode costs are unchanged: a truncated episode still finishes for them.

    action_head="categorical" is refused (NotImplementedError): the three-network kernels know the Gaussian head only."""
    _SAFE = True

    def __init__(self, env_or_engine, policy_weights, value_weights, cost_weights, T, costs=None, gamma=0.99, lam=0.95, cost_gamma=0.99,
                 cost_lam=0.95, seed=0, bootstrap_truncations=False, normalise_rewards=False, clip_reward=10.0, reward_eps=1e-8,
                 episode_stats=False, normalise_obs=False, clip_obs=10.0, obs_eps=1e-8, guardian=None, action_head="gaussian", bins=None):
        self.cost_weights = tuple(cost_weights)
        super().__init__(env_or_engine, policy_weights, value_weights, T, gamma=gamma, lam=lam, seed=seed,
                         bootstrap_truncations=bootstrap_truncations, normalise_rewards=normalise_rewards, clip_reward=clip_reward,
                         reward_eps=reward_eps, episode_stats=episode_stats, normalise_obs=normalise_obs, clip_obs=clip_obs, obs_eps=obs_eps,
                         guardian=guardian, action_head=action_head, bins=bins)
        eng = self.engine
        t = eng.torch
        if costs is None:
            cfg = getattr(env_or_engine, "config", None)
            costs = (1.0, 1.0, 1.0) if cfg is None or not hasattr(env_or_engine, "engine") else \
                (cfg["out_of_road_cost"], cfg["crash_vehicle_cost"], cfg["crash_object_cost"])
        self.costs = tuple(float(c) for c in costs)
        if len(self.costs) != 3:
            raise ValueError("SafeRolloutCollector: costs = %r" % (costs, ))
        self.cost_gamma, self.cost_lam = float(cost_gamma), float(cost_lam)
        T, N = self.T, eng.N
        f32 = dict(dtype=t.float32, device=eng.device)
        self.cost_values = t.zeros((T + 1, N), **f32)
        self.cost = t.zeros((T, N), **f32)
        self.cost_advantages = t.zeros((T, N), **f32)
        self.cost_returns = t.zeros((T, N), **f32)
        self.running_cost = t.zeros((N, ), **f32)
        self.ep_cost_sum = t.zeros((N, ), **f32)
        self.ep_cost_count = t.zeros((N, ), dtype=t.int32, device=eng.device)
        self._carry = self._carry + (self.cost_values, )
        self.batch.update(costs=self.cost, cost_values=self.cost_values, cost_advantages=self.cost_advantages, cost_returns=self.cost_returns,
                          ep_cost_sum=self.ep_cost_sum, ep_cost_count=self.ep_cost_count)
        if self.bootstrap_truncations:
            self.term_cost_values = t.zeros((T, N), **f32)
            self.batch.update(term_cost_values=self.term_cost_values)

    def set_weights(self, policy_weights, value_weights, cost_weights=None):
        """The networks of the rollouts from now on; cost_weights None: the cost critic stays what it is."""
        super().set_weights(policy_weights, value_weights)
        if cost_weights is not None:
            self.cost_weights = tuple(cost_weights)

    def _evaluate(self, row):
        self.engine.mlp_actor_critic_cost(self.policy_weights, self.value_weights, self.cost_weights, self._actions[row], self._logp[row],
                                          self.values[row], self.cost_values[row], self.seed, row, obs=self._obs[row])

    def _cost_side(self, t):
        return self.cost_weights, self.term_cost_values[t]

    def collect(self):
        """T steps.  Returns RolloutCollector's dict with costs, cost_values, cost_advantages, cost_returns, ep_cost_sum, ep_cost_count
        (the same objects every time, valid until the next call)."""
        super().collect()
        eng = self.engine
        gae, term = (eng.cost_gae_bootstrap, (self.term_cost_values, )) if self.bootstrap_truncations else (eng.cost_gae, ())
        gae(self.flags, self.dones, self.cost_values, *term, self.costs, self.cost_gamma, self.cost_lam, self.running_cost, cost=self.cost,
            adv=self.cost_advantages, ret=self.cost_returns, ep_sum=self.ep_cost_sum, ep_count=self.ep_cost_count)
        return self.batch


class MultiAgentRolloutCollector(_Collector):
    """RolloutCollector for multi-agent engines (A seats per env; include/pgdrive_hip.h states acted / cont / live):

        col = MultiAgentRolloutCollector(env, policy_weights, value_weights, T=128)
        batch = col.collect()
        idx = batch["index"][:int(batch["count"])]      # the (t, env, seat) transitions of agents, flattened; minibatches come from here

    Per step t: Engine.step(actions[t]) writes obs[t + 1], rewards[t], dones[t], flags[t]; Engine.live_rows lists the seats whose row
    t + 1 holds an observation an agent will act on; Engine.mlp_actor_critic_rows evaluates the networks on those rows and writes row
    t + 1 of actions, logp and values (zeros in every other seat -- the step ignores the action of a seat without an agent).  Behind the T
    steps: Engine.gae_masked (an agent's episode ends at its done or at an env-wide restart; a seat's next agent starts afresh) and
    Engine.rollout_index.  Row T is carried into row 0 of the next rollout and the tick counter advances by T, as in RolloutCollector;
    nothing in collect() waits for the device.

    prime() takes the live seats of the FIRST observation from the engine's state (status == ACTIVE): one host read, and the first call
    of rollout_index allocates its scratch -- so prime() is called (by the first collect(), or explicitly) BEFORE collect() is captured
    in a HIP graph.

    The step is handed another observation row at every step, so the engine's marks of seats whose zero row is already in place
    (pgd_forget_rows) never carry over: every step of a rollout writes the zero row of every seat that is not due.

    episode_stats=True: the statistics of the agents' episodes, per seat (the module's docstring); cut_rate of episode_summary() is the
    share of the agents an env-wide restart took out.

    normalise_obs=True: as for RolloutCollector (the module's docstring); the fold takes the rows of `index` / `count` only, those at
    which an agent acted -- the zero rows of seats that are not due are no samples.

    action_head="categorical", bins=(ks, kt): as for RolloutCollector, over the live rows (Engine.mlp_actor_critic_cat_rows); the batch gains
    action_index int32 [T, N, A, 2], zeros in every seat that is not due."""
    def __init__(self, env_or_engine, policy_weights, value_weights, T, gamma=0.99, lam=0.95, seed=0, normalise_rewards=False, clip_reward=10.0,
                 reward_eps=1e-8, episode_stats=False, normalise_obs=False, clip_obs=10.0, obs_eps=1e-8, guardian=None, action_head="gaussian",
                 bins=None):
        if guardian is not None:
            raise NotImplementedError("MultiAgentRolloutCollector: the expert guardian serves single-agent engines only (pgd_guardian)")
        eng = getattr(env_or_engine, "engine", env_or_engine)
        if eng.A == 1:
            raise NotImplementedError("MultiAgentRolloutCollector serves multi-agent engines: this one has a single agent seat per env and "
                                      "never reports PGD_F_REPORT -- use RolloutCollector")
        if int(T) < 1:
            raise ValueError("MultiAgentRolloutCollector: T = %r" % (T, ))
        head = self._head_options("MultiAgentRolloutCollector", eng, policy_weights, action_head, bins)
        self._allocate(eng, (eng.N, eng.A), policy_weights, value_weights, T, gamma, lam, seed)
        self._head(head)
        self._normalise(normalise_rewards, clip_reward, reward_eps)
        self._episodes(episode_stats, seats=True)
        self._obs_norm(normalise_obs, clip_obs, obs_eps)
        self._guardian(None)
        t = eng.torch
        i32 = dict(dtype=t.int32, device=eng.device)
        self.mask = t.zeros(self.flags.shape, dtype=t.uint8, device=eng.device)
        self.index = t.zeros((self.flags.numel(), ), **i32)
        self.count = t.zeros((1, ), **i32)
        self._rows = t.zeros((eng.N * eng.A, ), **i32)    # the live rows of the observation just written
        self._n_rows = t.zeros((1, ), **i32)
        self.batch.update(mask=self.mask, index=self.index, count=self.count)

    def _evaluate(self, row):
        if self.action_head == "categorical":
            self.engine.mlp_actor_critic_cat_rows(self.policy_weights, self.value_weights, self.bins, self._rows, self._n_rows, self._actions[row],
                                                  self._action_index[row], self._logp[row], self.values[row], self.seed, row,
                                                  obs=self._obs[row], emit_index=self.emit_index)
            return
        self.engine.mlp_actor_critic_rows(self.policy_weights, self.value_weights, self._rows, self._n_rows, self._actions[row], self._logp[row],
                                          self.values[row], self.seed, row, obs=self._obs[row])

    def _stepped(self, t):
        self.engine.live_rows(self.flags[t], self.dones[t], rows=self._rows, count=self._n_rows)

    def _finish(self):
        self._episode_call()
        self.engine.gae_masked(self._gae_rewards(flags=self.flags), self.values, self.dones, self.flags, self.gamma, self.lam, adv=self.advantages,
                               ret=self.returns, mask=self.mask)
        self.engine.rollout_index(self.flags, index=self.index, count=self.count)
        self._fold_obs(self.index, self.count)

    def prime(self):
        """Take the engine's present observation (what reset wrote into Engine.obs) as the start of the first rollout; its live seats
        are those whose agent is ACTIVE in the engine's state (a host read).  collect() calls it once by itself; call it before
        capturing collect() in a graph."""
        from . import _abi
        eng = self.engine
        eng.sync()
        _, si, _ = eng.get_state()
        live = np.flatnonzero(si[_abi.SI["STATUS"], :, :eng.A].reshape(-1) == _abi.ST_ACTIVE).astype(np.int32)
        self._rows[:len(live)].copy_(eng.torch.from_numpy(live))
        self._n_rows.fill_(len(live))
        super().prime()
        eng.rollout_index(self.flags, index=self.index, count=self.count)  # (its scratch, allocated outside any capture; flags are zero)

    def collect(self):
        """T steps.  Returns the dict of the collector's tensors (the same objects every time, valid until the next call):
        obs [T, N, A, D], actions [T, N, A, 2] (as sampled; the step clips), logp [T, N, A], values [T + 1, N, A], rewards, dones (uint8),
        flags, advantages, returns [T, N, A] -- as RolloutCollector's with a seat axis -- and mask [T, N, A] uint8 (an agent acted),
        index [T * N * A] int32 (the flattened positions where mask is 1, ascending; valid up to count), count [1] int32."""
        return super().collect()
