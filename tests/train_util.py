"""What the GPU tests of the training path share: tensors and cheap engines, the pointer structs of the C ABI, bit
comparisons, the engine-and-network fixtures, the collectors' and the learners' calls made one at a time, the snapshot of a learner and
the eager-then-graph comparison.  A new collector or learner switch adds an option here and a row in its test's table, not a copy."""
import numpy as np

SENT = 7.0   # what an output buffer holds before a launch
ERR_ARG = 1  # PGD_ERR_ARG
SIX = ("w1", "b1", "w2", "b2", "w3", "b3")
KEYS = ("obs", "actions", "logp", "values", "rewards", "dones", "flags", "advantages", "returns")   # every collector's batch


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ego_engine(descs, n, **kw):
    """n envs, ego only, no lidar: cheap to create; the network kernels only need its row count, env_base, groups, device and streams."""
    from pgdrive_amd import _abi
    from pgdrive_amd.engine import Engine
    from tests import util
    mb, sb = util.make_banks(descs, n_maps=4, num_traffic=0)
    args = dict(num_agents=1, num_traffic=0, num_lasers=0, seed=2)
    args.update(kw)
    return Engine(_abi.make_config(n, **args), mb, sb)


def six(st, tensors, prefix=""):
    """The six pointer fields <prefix>w1 .. <prefix>b3 of an ABI struct from six tensors -> the struct."""
    for name, t in zip(SIX, tensors):
        setattr(st, prefix + name, t.data_ptr())
    return st


def ac_nets(pw, vw, out_cols=None):
    """pgd_actor_critic of the policy tensors `pw` and the value tensors `vw` (None: no critic); out_cols: instead of the head's width."""
    from pgdrive_amd import _abi
    nets = six(_abi.ActorCritic(), pw)
    nets.out_cols = int(pw[4].shape[1]) if out_cols is None else out_cols
    return nets if vw is None else six(nets, vw, "v")


# ---------------------------------------------------------------------------------------------------------------------
# the same bits
# ---------------------------------------------------------------------------------------------------------------------
def snapshot(batch, keys):
    import torch
    torch.cuda.synchronize()
    return {k: batch[k].clone() for k in keys}


def bits_equal(a, b):
    import torch
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def np_bits(a):
    """A numpy array's bits as unsigned integers of its item size (integer arrays as they are)."""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def holds(got, need, where):
    assert set(need) <= set(got), "%s: nothing to compare for %s" % (where, sorted(set(need) - set(got)))
    return got


def assert_same(got, want, where, need=()):
    """Every tensor of `got` has the bits of `want`'s of the same key; `need`: keys that `got` has to hold."""
    for key in holds(got, need, where):
        assert bits_equal(got[key], want[key]), "%s: %s differs" % (where, key)


# ---------------------------------------------------------------------------------------------------------------------
# fixtures: an engine freshly reset, `first` (its first observation), the networks on the host (p, v, c) and on the device (pw, vw, cw),
# and the T and seed its collector runs with
# ---------------------------------------------------------------------------------------------------------------------
def _networks(S, D, nets=None, steer_bias=None, wide=False):
    """Random networks of the expert's shape, a third one as cost critic, from one generator; the policy's head bent so that the cars
    drive (wide: log_std around 0 instead of the small steering)."""
    from tests import actor_critic_ref as ar
    if nets is None:
        rng = np.random.default_rng(0)
        p, v = ar.make_networks(rng, D, 4)
        _, c = ar.make_networks(rng, D, 4)
        if wide:
            p[5][2:4] += 1.0     # (log_std around 0)
        else:
            p[4][:, 0] *= 0.05   # (steering: the cars stay on the road for a while, tests/test_policy_gpu.py)
        p[5][1] = 0.5            # (throttle: they drive)
        if steer_bias is not None:
            p[5][0] = steer_bias
        nets = (p, v, c)
    S.p, S.v, S.c = nets
    S.pw, S.vw, S.cw = [tuple(dev(w) for w in n) for n in nets]


class Traffic:
    """n envs of the default configuration with traffic over 8 maps, auto_reset, engine seed 5 and a short horizon, freshly reset.
    step_info_costs: the step info is on, with these costs and NaN in final_observation; steer_bias: the policy steers to one side
    (the guardian has something to do); expert: a weight file -> `expert` and the collectors' `guardian` argument."""
    live0 = None

    def __init__(self, descs, n, T, seed, horizon=12, safe=False, step_info_costs=None, nets=None, steer_bias=None, expert=None):
        import torch
        from pgdrive_amd import _abi
        from pgdrive_amd.engine import Engine
        from tests import util
        mb, sb = util.make_banks(descs, n_maps=8)
        self.T, self.seed, self.safe = T, seed, safe
        self.eng = eng = Engine(_abi.make_config(n, auto_reset=1, horizon=horizon, seed=5, safe_rl_env=safe), mb, sb)
        if step_info_costs is not None:
            eng.enable_step_info(costs=step_info_costs)
            eng.step_info["final_observation"].fill_(float("nan"))
        self.first = eng.reset(np.arange(n) % 8).view(n, -1).clone()
        _networks(self, eng.D, nets, steer_bias)
        if expert is not None:
            from pgdrive_amd.vec_env import load_saver_weights
            self.expert = tuple(dev(w) for w in load_saver_weights(dict(saver_weights=expert), eng.D))
            self.guardian = dict(weights=self.expert, save_level=0.5)
        eng.sync()
        torch.cuda.synchronize()


class Ego:
    """6 envs, ego only, no lidar, horizon 5 < T = 8 (every env ends at least once per rollout), freshly reset."""
    N, live0 = 6, None

    def __init__(self, descs, safe, T=8, seed=3, horizon=5):
        import torch
        self.T, self.seed, self.safe = T, seed, safe
        self.eng = eng = ego_engine(descs, self.N, auto_reset=1, horizon=horizon, seed=5, safe_rl_env=safe)
        self.first = eng.reset(np.arange(self.N) % 4).view(self.N, -1).clone()
        _networks(self, eng.D)
        eng.sync()
        torch.cuda.synchronize()


class Roundabout:
    """The roundabout with 5 seats, 6 envs, horizon 40, delay_done 3, freshly reset; random networks of the expert's shape with
    log_std around 0 (the sampled actions are wide: agents leave the road and crash within a rollout).
    Envs 4 and 5 start with their episode clock at 5 x horizon - 12, set through the checkpoint interface: from a fresh reset the env-wide
    cut at 5 x horizon cannot be reached while an agent still drives -- no agent is spawned once the clock has passed the horizon, and
    every agent ends within `horizon` steps of its own -- so a rollout that starts at a reset would never hold a PGD_F_RESET on an
    agent that is not done.  active0: the state's ACTIVE seats; live0: their rows, the list the first evaluation runs over."""
    N, A, HORIZON, DELAY, CUT_ENVS, CUT_AT = 6, 5, 40, 3, (4, 5), 12
    safe = False

    def __init__(self, T=32, seed=3):
        import torch
        from pgdrive_amd import _abi
        from pgdrive_amd.engine import Engine
        from tests import util
        _, mb, sb = util.make_marl_banks(num_agents=self.A)
        self.T, self.seed = T, seed
        self.eng = eng = Engine(util.marl_config(self.N, sb, horizon=self.HORIZON, delay_done=self.DELAY, seed=5), mb, sb)
        self.first = eng.reset(np.arange(self.N) % len(sb.scenarios)).clone()
        f, i, ei = eng.get_state()
        ei[_abi.EI["EP_STEPS"], list(self.CUT_ENVS)] = 5 * self.HORIZON - self.CUT_AT
        eng.set_state(f, i, ei)
        self.active0 = (i[_abi.SI["STATUS"], :, :self.A] == _abi.ST_ACTIVE)
        self.live0 = np.flatnonzero(self.active0.reshape(-1)).astype(np.int32)
        _networks(self, eng.D, wide=True)
        eng.sync()
        torch.cuda.synchronize()


def make_collector(kind, S, **switches):
    """The collector of `kind` ("single", "safe", "marl") on the fixture's engine and networks, with its T and seed."""
    from pgdrive_amd.rollout import MultiAgentRolloutCollector, RolloutCollector, SafeRolloutCollector
    if kind == "safe":
        return SafeRolloutCollector(S.eng, S.pw, S.vw, S.cw, S.T, seed=S.seed, **switches)
    return (MultiAgentRolloutCollector if kind == "marl" else RolloutCollector)(S.eng, S.pw, S.vw, S.T, seed=S.seed, **switches)


LEARN_KW = dict(lr=3e-4, epochs=1, minibatches=2)


def make(kind, descs, learn=True, **switches):
    """-> (fixture, collector, learner or None) of a fresh engine: Ego for "single" and "safe", Roundabout for "marl"."""
    from pgdrive_amd.learner import PPOLagLearner, PPOLearner
    S = Roundabout() if kind == "marl" else Ego(descs, kind == "safe")
    col = make_collector(kind, S, **switches)
    if not learn:
        return S, col, None
    return S, col, PPOLagLearner(col, cost_limit=1.0, **LEARN_KW) if kind == "safe" else PPOLearner(col, **LEARN_KW)


# ---------------------------------------------------------------------------------------------------------------------
# the collectors' calls by hand
# ---------------------------------------------------------------------------------------------------------------------
def hand_gae(eng, batch, marl=False, bootstrap=False):
    """The GAE call of a collector that normalises its rewards, on its own batch -> (advantages, returns)."""
    rewards = batch["scaled_rewards"]
    if marl:
        return eng.gae_masked(rewards, batch["values"], batch["dones"], batch["flags"], 0.99, 0.95)[:2]
    if bootstrap:
        return eng.gae_bootstrap(rewards, batch["values"], batch["dones"], batch["term_values"], 0.99, 0.95)
    return eng.gae(rewards, batch["values"], batch["dones"], 0.99, 0.95)


def synchronised_rollouts(S, n_rollouts, cost_critic=False, bootstrap=False, costs=None, guardian=False):
    """The calls of a collector on the fixture `S` made one at a time into fresh sentinel-filled buffers, a device synchronisation behind
    each; evaluation j has tick j.  -> per rollout the batch's tensors (KEYS and what the engine and the options add).
    Single-agent engines: mlp_actor_critic, step, ..., gae.  Multi-agent engines (S.live0: the live rows of the first observation):
    live rows, mlp_actor_critic_rows, step, ..., gae_masked, rollout_index.
    cost_critic: mlp_actor_critic_cost -> "cost_values".  bootstrap: mlp_terminal_value behind every step -> "term_values"
    ("term_cost_values"), "final_obs" (a copy of step_info["final_observation"] behind every step), gae_bootstrap, and with the cost
    critic cost_gae_bootstrap over `costs` with the running cost carried from rollout to rollout.  guardian: the guardian of row j in
    front of step j with tick j and the seed xor GUARDIAN_SEED_XOR, its state and the previous flags carried -> "applied_actions",
    "takeover", "guardian_trace"."""
    import torch
    from pgdrive_amd.rollout import GUARDIAN_SEED_XOR
    eng, T, seed = S.eng, S.T, S.seed
    N, A, D = eng.N, eng.A, eng.D
    marl = S.live0 is not None
    shape = (N, A) if marl else (N, )

    def fresh(*tail, dtype=torch.float32):
        return torch.full((N, A) + tail, SENT, dtype=dtype, device="cuda")

    def evaluate(obs, tick, rows, count):
        a, lp, v, cv = fresh(2), fresh(), fresh(), fresh()
        if marl:
            eng.mlp_actor_critic_rows(S.pw, S.vw, rows, count, a, lp, v, seed, tick, obs=obs)
        elif cost_critic:
            eng.mlp_actor_critic_cost(S.pw, S.vw, S.cw, a, lp, v, cv, seed, tick, obs=obs)
        else:
            eng.mlp_actor_critic(S.pw, S.vw, a, lp, v, seed, tick, obs=obs)
        torch.cuda.synchronize()
        return a, lp, v, cv

    obs = S.first.clone()
    rows = count = None
    if marl:
        rows = torch.zeros((N * A, ), dtype=torch.int32, device="cuda")
        rows[:len(S.live0)] = dev(S.live0)
        count = dev(np.array([len(S.live0)], dtype=np.int32))
    a, lp, v, cv = evaluate(obs, 0, rows, count)
    run = torch.zeros(N, device="cuda")                              # the running cost, carried
    g_state = torch.zeros(N, dtype=torch.uint8, device="cuda")       # the guardian's takeover state, carried
    prev = torch.zeros((N, 1), dtype=torch.int32, device="cuda")     # the flags of the step before, carried
    out = []
    for k in range(n_rollouts):
        rec = {}

        def put(**kw):
            for key, x in kw.items():
                rec.setdefault(key, []).append(x)

        for t in range(T):
            put(obs=obs.view(*shape, D), actions=a.view(*shape, 2), logp=lp.view(shape), values=v.view(shape))
            if cost_critic:
                put(cost_values=cv.view(shape))
            applied = a
            if guardian:
                applied, info, trace = fresh(2), fresh(dtype=torch.uint8).view(N), fresh(4).view(N, 4)
                eng.guardian(S.expert, S.guardian["save_level"], a, g_state, applied, info, seed ^ GUARDIAN_SEED_XOR, k * T + t, prev_flags=prev,
                             trace=trace, obs=obs)
                torch.cuda.synchronize()
                put(applied_actions=applied.view(N, 2), takeover=info, guardian_trace=trace)
            obs, rew, done, flags = eng.step(applied, out=eng.make_outputs())
            torch.cuda.synchronize()
            prev = flags.clone()
            put(rewards=rew.view(shape), dones=done.view(shape), flags=flags.view(shape))
            if bootstrap:
                put(final_obs=eng.step_info["final_observation"].clone())
                tv, tcv = fresh().view(N), fresh().view(N)
                eng.mlp_terminal_value(S.vw, S.cw if cost_critic else None, eng.step_info["final_observation"], flags.view(N), done.view(N), tv,
                                       tcv if cost_critic else None)
                torch.cuda.synchronize()
                put(term_values=tv, term_cost_values=tcv)
            if marl:
                rows, count = eng.live_rows(flags, done)
                torch.cuda.synchronize()
            a, lp, v, cv = evaluate(obs, k * T + t + 1, rows, count)
        put(values=v.view(shape))
        if cost_critic:
            put(cost_values=cv.view(shape))
        r = {key: torch.stack(x) for key, x in rec.items()}
        if marl:
            r["advantages"], r["returns"], r["mask"] = eng.gae_masked(r["rewards"], r["values"], r["dones"], r["flags"], 0.99, 0.95)
            torch.cuda.synchronize()
            index = torch.zeros((T * N * A, ), dtype=torch.int32, device="cuda")
            r["index"], r["count"] = eng.rollout_index(r["flags"], index=index)
        elif bootstrap:
            r["advantages"], r["returns"] = eng.gae_bootstrap(r["rewards"], r["values"], r["dones"], r["term_values"], 0.99, 0.95)
            if cost_critic:
                r["costs"], r["cost_advantages"], r["cost_returns"], r["ep_cost_sum"], r["ep_cost_count"] = eng.cost_gae_bootstrap(
                    r["flags"], r["dones"], r["cost_values"], r["term_cost_values"], costs, 0.99, 0.95, run)
        else:
            r["advantages"], r["returns"] = eng.gae(r["rewards"], r["values"], r["dones"], 0.99, 0.95)
        torch.cuda.synchronize()
        out.append(r)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the learners: what they own, and update() by hand
# ---------------------------------------------------------------------------------------------------------------------
EVERY_LEARNER = ("params", "grads", "m", "v", "step", "stats", "adv_stats")   # what a comparison of two learners has to hold at least
LAGRANGIAN = EVERY_LEARNER + ("lagrange_state", "mixed", "cadv_stats")
LEARNER_TENSORS = LAGRANGIAN + ("shuffled", "live_count", "gate", "_epoch")


def learner_state(L):
    """A copy of every tensor the learner owns (those of the switches that are on, and the Lagrangian ones where it has them)."""
    import torch
    torch.cuda.synchronize()
    return {k: getattr(L, k).clone() for k in LEARNER_TENSORS if getattr(L, k, None) is not None}


def restore(L, state):
    for k, x in state.items():
        getattr(L, k).copy_(x)


def update_by_hand(eng, L, batch, epochs, minibatches, lr=3e-4, n_steps=None, index=None, count=None, shuffle=None, lagrange=None, gate=None,
                   kl_limit=0.0):
    """update() restated in Engine calls on L's buffers: adv_stats, then ppo_grad + adam per epoch and strided minibatch over the list
    as it lies (`index` / `count`: a collector's list); n_steps: stop after that many.
    shuffle = dict(seed, shuffled, live, epoch), the caller's tensors: shuffle_index in front of every epoch over `live` entries, the
    epochs counted on the device.  lagrange = dict(cost_limit, lambda_lr): the multiplier's step, both statistics and adv_mix in front,
    ppo_grad_cost over the mixed advantages.  gate (with kl_limit): adam_gated on the minibatch's own KL estimate, gating `count`."""
    n_list = L.n_list
    if lagrange is not None:
        eng.lagrange(batch["ep_cost_sum"], batch["ep_cost_count"], L.lagrange_state, lagrange["cost_limit"], lagrange["lambda_lr"], 100.0)
    norm = eng.adv_stats(batch["advantages"], out=L.adv_stats, index=index, count=count, n_list=None if index is None else n_list)
    if lagrange is not None:
        cnorm = eng.adv_stats(batch["cost_advantages"], out=L.cadv_stats)
        eng.adv_mix(batch["advantages"], batch["cost_advantages"], L.lagrange_state, out=L.mixed, adv_stats=norm, cadv_stats=cnorm)
    if shuffle is not None:
        shuffle["live"].fill_(n_list)
        index, count = shuffle["shuffled"], shuffle["live"]
    k = 0
    for e in range(epochs):
        if shuffle is not None:
            eng.shuffle_index(None, shuffle["live"], n_list, shuffle["seed"], e, epoch_dev=shuffle["epoch"], out=shuffle["shuffled"])
        for j in range(minibatches):
            if n_steps is not None and k == n_steps:
                return
            mb = dict(start=j, stride=minibatches, rows=-(-(n_list - j) // minibatches), index=index, count=count, n_list=n_list)
            if lagrange is not None:
                eng.ppo_grad_cost(L.policy_weights, L.value_weights, L.cost_weights, L.policy_grads, L.value_grads, L.cost_grads, batch["obs"],
                                  batch["actions"], batch["logp"], L.mixed, batch["returns"], batch["cost_returns"], L.stats[k], L.work,
                                  cvf_coef=0.5, **mb)
            else:
                eng.ppo_grad(L.policy_weights, L.value_weights, L.policy_grads, L.value_grads, batch["obs"], batch["actions"], batch["logp"],
                             batch["advantages"], batch["returns"], L.stats[k], L.work, adv_stats=norm, **mb)
            if gate is not None:
                eng.adam_gated(L.params, L.grads, L.m, L.v, L.step, lr, gate, eps=1e-5, max_grad_norm=0.5, kl=L.stats[k, 4:], kl_limit=kl_limit,
                               count_gate=count)
            else:
                eng.adam(L.params, L.grads, L.m, L.v, L.step, lr, eps=1e-5, max_grad_norm=0.5)
            k += 1
    if shuffle is not None:
        shuffle["epoch"].add_(epochs)


# ---------------------------------------------------------------------------------------------------------------------
# one eager iteration, then the next one captured and replayed
# ---------------------------------------------------------------------------------------------------------------------
def eager_then_graph(iteration, state, want, replays=2, compare=assert_same, need=()):
    """On a side stream: `iteration()` once eagerly, `state()` compared with want[0]; the next `iteration()` captured in a HIP graph;
    `replays` replays, `state()` behind replay k compared with want[k].  compare(got, want, where) asserts; `state` synchronises and
    has to hold the keys `need`."""
    import torch

    def check(k, where):
        compare(holds(state(), need, where), want[k], where)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        iteration()
        check(0, "the eager iteration in front of the capture")
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph, stream=s):
        iteration()
    torch.cuda.synchronize()
    with torch.cuda.stream(s), torch.no_grad():
        for k in range(1, replays + 1):
            graph.replay()
            check(k, "graph replay %d" % k)
    del graph
