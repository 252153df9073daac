"""The PPO update behind an on-device rollout: `collect() -> update()` is a complete training iteration made of the engine's own launches.

    col = RolloutCollector(env, policy_weights, value_weights, T=128)      # or MultiAgentRolloutCollector
    learner = PPOLearner(col, lr=3e-4)
    while training:
        batch = col.collect()
        stats = learner.update(batch)       # [epochs * minibatches, 8] on the device: _abi.PPO_STATS

What a trainer otherwise writes as framework code: an autograd pass over two 3-layer networks, an optimiser step, a gather of minibatch
rows out of the time-major rollout and -- for the multi-agent collector -- a host read of batch["count"] before a minibatch can be sized.  (Constrained RL on the safe env: PPOLagLearner,
below, the same update with a cost critic and a Lagrange multiplier.)
Here: Engine.adv_stats once, then Engine.ppo_grad + Engine.adam for every epoch and minibatch.  Nothing in update() waits for the device
or reads a device scalar, so one `collect(); update()` can be captured in a HIP graph and replayed: the Adam step number and the tick of
the rollout's noise live in device memory and advance with every replay.  A collector built with normalise_obs=True: update() binds the
collector's table (Engine.obs_norm_bind) before its first ppo_grad and unbinds behind the last adam, so the gradients see the inputs the
rollout's evaluations saw.

Minibatch j of n takes the list positions j, j + n, j + 2 n, ...: the n minibatches partition the rollout's transitions whatever their
number is, with no shuffle tensor.  For RolloutCollector the list is every (t, env) row; for MultiAgentRolloutCollector it is
batch["index"] / batch["count"] as they lie on the device (the transitions at which an agent acted).

The learner owns ONE flat parameter buffer; the twelve weight tensors are views into it (every offset a multiple of 4 floats: the
16-byte alignment the network kernels demand).  It hands the views to collector.set_weights once; updates are in place, so the collector
sees them without another call.  As rollout.py documents, the carried row T of a rollout was evaluated with the weights of the rollout
it was observed in and is not evaluated again.
"""

NAMES = ("w1", "b1", "w2", "b2", "w3", "b3")
H = 256


def flat_layout(in_dim, out_cols, has_critic=True, has_cost_critic=False):
    """[(name, shape, offset)] of the weight tensors in the flat buffer, and its length in floats; offsets are multiples of 4.  The cost
    critic's six (cw1 .. cb3) lie behind the others."""
    shapes = [("w1", (in_dim, H)), ("b1", (H, )), ("w2", (H, H)), ("b2", (H, )), ("w3", (H, out_cols)), ("b3", (out_cols, ))]
    if has_critic:
        shapes += [("vw1", (in_dim, H)), ("vb1", (H, )), ("vw2", (H, H)), ("vb2", (H, )), ("vw3", (H, 1)), ("vb3", (1, ))]
    if has_cost_critic:
        shapes += [("cw1", (in_dim, H)), ("cb1", (H, )), ("cw2", (H, H)), ("cb2", (H, )), ("cw3", (H, 1)), ("cb3", (1, ))]
    out, o = [], 0
    for name, shape in shapes:
        n = 1
        for d in shape:
            n *= d
        out.append((name, shape, o))
        o += (n + 3) & ~3
    return out, o


def minibatch_plan(n_list, minibatches):
    """[(start, stride, rows)] of the strided minibatches over a list of up to n_list entries: minibatch j takes the positions j + i *
    minibatches, i < rows, of which those below the list's count are live."""
    n_mb = int(minibatches)
    return [(j, n_mb, max(1, -(-(int(n_list) - j) // n_mb))) for j in range(n_mb)]


def live_positions(start, stride, rows, count):
    """The live list positions of a minibatch (what the kernels do with the count they read on the device), in plain Python."""
    return [start + i * stride for i in range(rows) if start + i * stride < count]


class PPOLearner:
    NETS = ("policy", "value")  # the collector's networks, in flat_layout's order
    GRAD = "pgd_ppo_grad"

    def __init__(self, collector, lr=3e-4, clip=0.2, vf_coef=0.5, ent_coef=0.0, epochs=4, minibatches=4, max_grad_norm=0.5, betas=(0.9, 0.999),
                 eps=1e-5, normalise_advantages=True):
        eng = collector.engine
        t = eng.torch
        name, cost = type(self).__name__, len(self.NETS) == 3
        if int(epochs) < 1 or int(minibatches) < 1:
            raise ValueError("%s: epochs = %r, minibatches = %r" % (name, epochs, minibatches))
        self.collector, self.engine = collector, eng
        self.lr, self.clip, self.vf_coef, self.ent_coef = float(lr), float(clip), float(vf_coef), float(ent_coef)
        self.epochs, self.minibatches, self.max_grad_norm = int(epochs), int(minibatches), float(max_grad_norm)
        self.betas, self.eps, self.normalise_advantages = (float(betas[0]), float(betas[1])), float(eps), bool(normalise_advantages)
        nets = [getattr(collector, n + "_weights") for n in self.NETS]
        self.in_dim, self.out_cols = int(nets[0][0].shape[0]), int(nets[0][4].shape[1])
        layout, total = flat_layout(self.in_dim, self.out_cols, has_cost_critic=cost)
        f32 = dict(dtype=t.float32, device=eng.device)
        self.params, self.grads = t.zeros((total, ), **f32), t.zeros((total, ), **f32)
        self.m, self.v = t.zeros((total, ), **f32), t.zeros((total, ), **f32)
        self.step = t.zeros((4, ), dtype=t.int32, device=eng.device)  # pgd_adam's counter and record

        def views(flat):
            return tuple(flat[o:o + int(t.Size(shape).numel())].view(shape) for _, shape, o in layout)

        wv, gv = views(self.params), views(self.grads)
        for dst, src in zip(wv, [w for net in nets for w in net]):
            dst.copy_(src.view(dst.shape))
        for i, n in enumerate(self.NETS):  # policy_weights, policy_grads, value_weights, ...
            setattr(self, n + "_weights", wv[6 * i:6 * i + 6])
            setattr(self, n + "_grads", gv[6 * i:6 * i + 6])
        collector.set_weights(*[getattr(self, n + "_weights") for n in self.NETS])
        self.n_list = int(collector.rewards.numel())  # T * N (* A): every row of the rollout
        self.plan = minibatch_plan(self.n_list, self.minibatches)
        rows = max(rows for _, _, rows in self.plan)
        need = eng.ppo_cost_work_bytes(self.in_dim, rows) if cost else eng.ppo_work_bytes(self.in_dim, rows, True)
        if need == 0:
            raise ValueError("%s: the networks' input width %d is outside what %s accepts" % (name, self.in_dim, self.GRAD))
        self.work = t.empty(((need + 3) // 4, ), **f32)
        self.adv_stats = t.zeros((2, ), **f32)
        self.stats = t.zeros((self.epochs * self.minibatches, 8), **f32)

    def _advantages(self, batch, index, count):
        """The advantage tensor the gradient calls read and the statistics they normalise it with (None: as it is)."""
        adv = batch["advantages"]
        if not self.normalise_advantages:
            return adv, None
        return adv, self.engine.adv_stats(adv, out=self.adv_stats, index=index, count=count, n_list=self.n_list)

    def _grad(self, batch, adv, stats, **minibatch):
        self.engine.ppo_grad(self.policy_weights, self.value_weights, self.policy_grads, self.value_grads, batch["obs"], batch["actions"],
                             batch["logp"], adv, batch["returns"], stats, self.work, vf_coef=self.vf_coef, **minibatch)

    def update(self, batch):
        """epochs x minibatches gradient steps on the rollout `batch` (what collector.collect() returned).  Returns the statistics
        tensor [epochs * minibatches, 8] (the same object every time).  Asynchronous: nothing here waits for the device."""
        eng = self.engine
        index, count = batch.get("index"), batch.get("count")  # (the multi-agent collector's list; None: every row)
        adv, norm = self._advantages(batch, index, count)
        normalise_obs = getattr(self.collector, "normalise_obs", False)
        if normalise_obs:  # (the rollout's own table: it moves at the next collect() only)
            eng.obs_norm_bind(self.collector.obs_norm, self.in_dim, self.collector.clip_obs)
        k = 0
        for _ in range(self.epochs):
            for start, stride, rows in self.plan:
                self._grad(batch, adv, self.stats[k], start=start, stride=stride, rows=rows, index=index, count=count, n_list=self.n_list,
                           adv_stats=norm, clip=self.clip, ent_coef=self.ent_coef, in_dim=self.in_dim)
                eng.adam(self.params, self.grads, self.m, self.v, self.step, self.lr, betas=self.betas, eps=self.eps,
                         max_grad_norm=self.max_grad_norm)
                k += 1
        if normalise_obs:
            eng.obs_norm_bind(None)
        return self.stats


class PPOLagLearner(PPOLearner):
    """PPO-Lagrangian behind a SafeRolloutCollector: PPOLearner's update with a cost critic and a multiplier that holds the policy under
    `cost_limit` (the mean cost of an episode), all on the device:

        col = SafeRolloutCollector(env, policy_weights, value_weights, cost_weights, T=128)
        learner = PPOLagLearner(col, cost_limit=1.0)
        while training:
            stats = learner.update(col.collect())     # [epochs * minibatches, 8]: _abi.PPO_COST_STATS
        learner.lagrange_state                        # 4 floats on the device: _abi.LAGRANGE_STATE

    update(batch) runs, in order: Engine.lagrange (lambda <- clamp(lambda + lambda_lr (J_c - cost_limit), 0, lambda_max) from the
    episodes that finished in the rollout; none: unchanged), Engine.adv_stats for the reward and for the cost advantages, Engine.adv_mix
    (((adv - m) s - lambda (cadv - m_c)) / (1 + lambda): the cost advantage centred, not rescaled), then Engine.ppo_grad_cost +
    Engine.adam for every epoch and minibatch.  No host read: `collect(); update()` is capturable in one HIP graph, and a replay takes
    the next multiplier step from the lambda it finds.  ONE flat buffer holds the eighteen weight tensors (flat_layout(...,
    has_cost_critic=True)); the collector is handed the views.  `ppo_kwargs`: PPOLearner's arguments (normalise_advantages False: no
    scaling of the reward advantage and no centring of either)."""
    NETS = ("policy", "value", "cost")
    GRAD = "pgd_ppo_grad_cost"

    def __init__(self, collector, cost_limit, lambda_lr=0.05, lambda_init=0.0, lambda_max=100.0, cvf_coef=0.5, lr=3e-4, clip=0.2, vf_coef=0.5,
                 ent_coef=0.0, epochs=4, minibatches=4, max_grad_norm=0.5, betas=(0.9, 0.999), eps=1e-5, normalise_advantages=True):
        if not (0.0 <= float(lambda_init) <= float(lambda_max)):
            raise ValueError("PPOLagLearner: lambda_init = %r outside [0, lambda_max = %r]" % (lambda_init, lambda_max))
        super().__init__(collector, lr, clip, vf_coef, ent_coef, epochs, minibatches, max_grad_norm, betas, eps, normalise_advantages)
        self.cost_limit, self.lambda_lr, self.lambda_max, self.cvf_coef = float(cost_limit), float(lambda_lr), float(lambda_max), float(cvf_coef)
        t = self.engine.torch
        f32 = dict(dtype=t.float32, device=self.engine.device)
        self.cadv_stats = t.zeros((2, ), **f32)
        self.mixed = t.zeros((self.n_list, ), **f32)  # the advantage the policy sees
        self.lagrange_state = t.zeros((4, ), **f32)
        self.lagrange_state[0] = float(lambda_init)

    def _advantages(self, batch, index, count):
        """One multiplier step, then the mixed advantage (already normalised: no statistics for the gradient calls)."""
        eng = self.engine
        eng.lagrange(batch["ep_cost_sum"], batch["ep_cost_count"], self.lagrange_state, self.cost_limit, self.lambda_lr, self.lambda_max)
        adv, cadv = batch["advantages"], batch["cost_advantages"]
        norm = cnorm = None
        if self.normalise_advantages:
            norm = eng.adv_stats(adv, out=self.adv_stats, n_list=self.n_list)
            cnorm = eng.adv_stats(cadv, out=self.cadv_stats, n_list=self.n_list)
        eng.adv_mix(adv, cadv, self.lagrange_state, out=self.mixed, adv_stats=norm, cadv_stats=cnorm)
        return self.mixed, None

    def _grad(self, batch, adv, stats, **minibatch):
        self.engine.ppo_grad_cost(self.policy_weights, self.value_weights, self.cost_weights, self.policy_grads, self.value_grads, self.cost_grads,
                                  batch["obs"], batch["actions"], batch["logp"], adv, batch["returns"], batch["cost_returns"], stats, self.work,
                                  vf_coef=self.vf_coef, cvf_coef=self.cvf_coef, **minibatch)
