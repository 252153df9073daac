"""The PPO update behind an on-device rollout: `collect() -> update()` is a complete training iteration made of the engine's own launches.

    col = RolloutCollector(env, policy_weights, value_weights, T=128)      # or MultiAgentRolloutCollector
    learner = PPOLearner(col, lr=3e-4)
    while training:
        batch = col.collect()
        stats = learner.update(batch)       # [epochs * minibatches, 8] on the device: _abi.PPO_STATS ([.., 12] with guide=)

What a trainer otherwise writes as framework code: an autograd pass over two 3-layer networks, an optimiser step, a gather of minibatch
rows out of the time-major rollout and -- for the multi-agent collector -- a host read of batch["count"] before a minibatch can be sized.  (Constrained RL on the safe env: PPOLagLearner,
below, the same update with a cost critic and a Lagrange multiplier.)
Here: Engine.adv_stats once, then Engine.ppo_grad + Engine.adam for every epoch and minibatch.  Nothing in update() waits for the device
or reads a device scalar, so one `collect(); update()` can be captured in a HIP graph and replayed: the Adam step number and the tick of
the rollout's noise live in device memory and advance with every replay.  A collector built with normalise_obs=True: update() binds the
collector's table (Engine.obs_norm_bind) before its first ppo_grad and unbinds behind the last adam, so the gradients see the inputs the
rollout's evaluations saw.  A collector built with action_head="categorical": the learner reads the head and the bins off it, sizes its
scratch with Engine.ppo_cat_work_bytes and calls Engine.ppo_grad_cat with batch["action_index"]; everything else here is unchanged.
A collector built with guardian=: under a takeover the applied action is not the sampled one and the plain update trains on a wrong
gradient there.  guide="takeover" makes every gradient call Engine.ppo_grad_guided: the overridden rows drop their clipped surrogate
(keep_surrogate=True: keep it) and imitate batch["applied_actions"] with the weight bc_coef; guide="all": every row imitates the expert
(batch["guardian_trace"]) -- behaviour cloning on the visited states, the critics still learn.  guide_options() states the two; the
statistics tensor is then [epochs * minibatches, 12] (_abi.PPO_GUIDED_STATS: guided_rows and bc_loss in slots 8 and 9).  DESIGN section 35.

Minibatch j of n takes the list positions j, j + n, j + 2 n, ...: the n minibatches partition the rollout's transitions whatever their
number is.  For RolloutCollector the list is every (t, env) row; for MultiAgentRolloutCollector it is batch["index"] / batch["count"] as
they lie on the device (the transitions at which an agent acted).  With shuffle=False (the default) that list is followed as it lies,
with no shuffle tensor: for RolloutCollector with N a multiple of n, minibatch j is then the envs with env % n == j at every t, the same
in every epoch.  shuffle=True is what SB3, CleanRL and Spinning Up do: every epoch draws a fresh permutation of the live list
(Engine.shuffle_index into `shuffled`, one small launch per epoch, keyed by shuffle_seed and an epoch counter in device memory, so a
replayed graph draws new ones) and the same strided plan runs over it.

target_kl=x stops an update early ON THE DEVICE: every Adam call is Engine.adam_gated, which tests the minibatch's statistic
mean(logp_old - logp) (stats[k, 4], Spinning Up's estimator) against 1.5 x before it applies the step (SB3's granularity).  A stop shuts
`gate` (_abi.ADAM_GATE) for the rest of the update and zeroes `live_count`, the count every later gradient call reads: their tiles end
before they read a weight, their statistics rows have n = 0.  lr_scale=True: `lr_scale`, one device float the gated Adam multiplies lr
with -- a schedule writes it between iterations (a plain device write, legal between the replays of a captured graph, into which the
float `lr` is frozen).  state_dict() / load_state_dict(): params, m, v, step and, where they exist, the epoch counter and lr_scale.

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


def minibatch_options(name, shuffle, shuffle_seed, target_kl, lr_scale):
    """The learner's minibatch switches checked (ValueError) -> (shuffle, shuffle_seed, kl_limit or None, lr_scale).  No device needed."""
    if not isinstance(shuffle, (bool, int)) or shuffle not in (0, 1):
        raise ValueError("%s: shuffle = %r is not a bool" % (name, shuffle))
    if not isinstance(lr_scale, (bool, int)) or lr_scale not in (0, 1):
        raise ValueError("%s: lr_scale = %r is a switch (the factor is the device tensor learner.lr_scale), not a bool" % (name, lr_scale))
    if isinstance(shuffle_seed, bool) or not isinstance(shuffle_seed, int) or not (0 <= shuffle_seed < 2 ** 32):
        raise ValueError("%s: shuffle_seed = %r is not an integer in [0, 2^32)" % (name, shuffle_seed))
    kl_limit = None
    if target_kl is not None:
        kl_limit = 1.5 * float(target_kl)
        if not (0.0 < kl_limit < float("inf")):
            raise ValueError("%s: target_kl = %r is not a positive finite number (None: no stop)" % (name, target_kl))
    return bool(shuffle), int(shuffle_seed), kl_limit, bool(lr_scale)


def collector_head(name, collector, cost=False):
    """(head, bins) a learner reads off its collector: ("gaussian", None) for a collector of before, ("categorical", (ks, kt)) for one built
    with action_head="categorical" -- which the Lagrangian learner refuses (NotImplementedError: the three-network kernels know the Gaussian
    head only).  No device needed."""
    head, bins = getattr(collector, "action_head", "gaussian"), getattr(collector, "bins", None)
    if head == "categorical" and cost:
        raise NotImplementedError("%s: the categorical head is not served by pgd_ppo_grad_cost" % name)
    return head, bins


GUIDES = ("takeover", "all")


def guide_options(name, guide, bc_coef, keep_surrogate, guardian):
    """The learner's guide switches checked (ValueError) -> None (guide=None: today's calls), or what Engine.ppo_grad_guided is handed:
    dict(target, mask: keys of the batch (mask None: every row is guided), mask_bits, bc_coef, keep_surrogate).  `guardian`: the
    collector's guardian settings (collector.guardian; None: built without guardian=).  No device needed.
    "takeover": the rows whose applied action is not the sampled one imitate batch["applied_actions"] -- what the return credits, agent
    and expert components mixed.  Those rows are (takeover & 1) != 0, and with the guardian's immediate=True, which also applies the
    correction of a takeover's first step, (takeover & 3) != 0 (bit 1: takeover_start).
    "all": every row imitates the expert's steering and throttle, columns 0 and 1 of batch["guardian_trace"]; with keep_surrogate=False
    that is behaviour cloning of the expert on the states the guarded agent visits (DAgger)."""
    if not isinstance(keep_surrogate, (bool, int)) or keep_surrogate not in (0, 1):
        raise ValueError("%s: keep_surrogate = %r is not a bool" % (name, keep_surrogate))
    if guide is None:
        if keep_surrogate:
            raise ValueError("%s: keep_surrogate=True without guide= (one of %s)" % (name, ", ".join(map(repr, GUIDES))))
        return None
    if guide not in GUIDES:
        raise ValueError("%s: guide = %r is not one of None, %s" % (name, guide, ", ".join(map(repr, GUIDES))))
    if guardian is None:
        raise ValueError("%s: guide=%r reads what the expert guardian records: build the collector with guardian=dict(weights=...)" % (name, guide))
    try:
        bc = float(bc_coef)
    except (TypeError, ValueError):
        bc = float("nan")
    if isinstance(bc_coef, bool) or not (0.0 <= bc < float("inf")):
        raise ValueError("%s: bc_coef = %r is not a finite number >= 0" % (name, bc_coef))
    if guide == "takeover":
        return dict(target="applied_actions", mask="takeover", mask_bits=3 if guardian.get("immediate") else 1, bc_coef=bc,
                    keep_surrogate=bool(keep_surrogate))
    return dict(target="guardian_trace", mask=None, mask_bits=1, bc_coef=bc, keep_surrogate=bool(keep_surrogate))


class PPOLearner:
    NETS = ("policy", "value")  # the collector's networks, in flat_layout's order
    GRAD = "pgd_ppo_grad"

    def __init__(self, collector, lr=3e-4, clip=0.2, vf_coef=0.5, ent_coef=0.0, epochs=4, minibatches=4, max_grad_norm=0.5, betas=(0.9, 0.999),
                 eps=1e-5, normalise_advantages=True, shuffle=False, shuffle_seed=0, target_kl=None, lr_scale=False, guide=None, bc_coef=1.0,
                 keep_surrogate=False):
        name, cost = type(self).__name__, len(self.NETS) == 3
        self.shuffle, self.shuffle_seed, self.kl_limit, scaled = minibatch_options(name, shuffle, shuffle_seed, target_kl, lr_scale)
        self.guide = guide_options(name, guide, bc_coef, keep_surrogate, getattr(collector, "guardian", None))
        self.target_kl = None if target_kl is None else float(target_kl)
        self.action_head, self.bins = collector_head(name, collector, cost)
        eng = collector.engine
        t = eng.torch
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
        work_bytes = eng.ppo_cat_work_bytes if self.action_head == "categorical" else eng.ppo_work_bytes
        need = eng.ppo_cost_work_bytes(self.in_dim, rows) if cost else work_bytes(self.in_dim, rows, True)
        if need == 0:
            raise ValueError("%s: the networks' input width %d is outside what %s accepts" % (name, self.in_dim, self.GRAD))
        self.work = t.empty(((need + 3) // 4, ), **f32)
        self.adv_stats = t.zeros((2, ), **f32)
        self.stats = t.zeros((self.epochs * self.minibatches, 8 if self.guide is None else 12), **f32)  # (guided: _abi.PPO_GUIDED_STATS)
        # the minibatch switches' device state; None where a switch is off (then update() makes today's calls and no others)
        i32 = dict(dtype=t.int32, device=eng.device)
        self.shuffled = t.zeros((self.n_list, ), **i32) if self.shuffle else None
        self._epoch = t.zeros((1, ), **i32) if self.shuffle else None  # epochs drawn so far: a replayed graph draws new permutations
        self.live_count = t.zeros((1, ), **i32) if self.shuffle or self.kl_limit is not None else None  # the count the gradient calls read
        self.gate = t.zeros((4, ), **i32) if scaled or self.kl_limit is not None else None  # _abi.ADAM_GATE
        self.lr_scale = t.ones((1, ), **f32) if scaled else None

    def state_dict(self):
        """What a checkpoint of the learner holds (clones on the device): the flat parameters, Adam's moments and step record and, where
        the switches made them, the epoch counter of the permutations and lr_scale (None otherwise)."""
        own = {"params": self.params, "m": self.m, "v": self.v, "step": self.step, "_epoch": self._epoch, "lr_scale": self.lr_scale}
        return {k: (None if x is None else x.clone()) for k, x in own.items()}

    def load_state_dict(self, state):
        """state_dict()'s tensors copied back IN PLACE (the collector holds views of `params`).  An entry this learner has no tensor for
        (a checkpoint of a shuffled run loaded into an unshuffled learner) must be None; one it has must be there."""
        own = {"params": self.params, "m": self.m, "v": self.v, "step": self.step, "_epoch": self._epoch, "lr_scale": self.lr_scale}
        for k, x in own.items():
            src = state.get(k)
            if (x is None) != (src is None):
                raise ValueError("%s.load_state_dict: %r is %s in the checkpoint and %s here" %
                                 (type(self).__name__, k, "missing" if src is None else "present", "missing" if x is None else "present"))
            if x is not None and (tuple(src.shape) != tuple(x.shape) or src.dtype != x.dtype):
                raise ValueError("%s.load_state_dict: %r is %s %s, expected %s %s" %
                                 (type(self).__name__, k, tuple(src.shape), src.dtype, tuple(x.shape), x.dtype))
        for k, x in own.items():
            if x is not None:
                x.copy_(state[k])

    def _advantages(self, batch, index, count):
        """The advantage tensor the gradient calls read and the statistics they normalise it with (None: as it is)."""
        adv = batch["advantages"]
        if not self.normalise_advantages:
            return adv, None
        return adv, self.engine.adv_stats(adv, out=self.adv_stats, index=index, count=count, n_list=self.n_list)

    def _guided_cost(self, batch):
        """The cost critic's arguments of Engine.ppo_grad_guided: none here."""
        return {}

    def _grad(self, batch, adv, stats, **minibatch):
        if self.guide is not None:  # (a collector with a guardian has the Gaussian head)
            g = self.guide
            self.engine.ppo_grad_guided(self.policy_weights, self.value_weights, self.policy_grads, self.value_grads, batch["obs"],
                                        batch["actions"], batch["logp"], adv, batch["returns"], stats, self.work, batch[g["target"]],
                                        mask=None if g["mask"] is None else batch[g["mask"]], mask_bits=g["mask_bits"], bc_coef=g["bc_coef"],
                                        keep_surrogate=g["keep_surrogate"], vf_coef=self.vf_coef, **self._guided_cost(batch), **minibatch)
            return
        if self.action_head == "categorical":
            self.engine.ppo_grad_cat(self.policy_weights, self.value_weights, self.policy_grads, self.value_grads, self.bins, batch["obs"],
                                     batch["action_index"], batch["logp"], adv, batch["returns"], stats, self.work, vf_coef=self.vf_coef,
                                     **minibatch)
            return
        self.engine.ppo_grad(self.policy_weights, self.value_weights, self.policy_grads, self.value_grads, batch["obs"], batch["actions"],
                             batch["logp"], adv, batch["returns"], stats, self.work, vf_coef=self.vf_coef, **minibatch)

    def update(self, batch):
        """epochs x minibatches gradient steps on the rollout `batch` (what collector.collect() returned).  Returns the statistics
        tensor [epochs * minibatches, 8] -- with guide= [epochs * minibatches, 12], _abi.PPO_GUIDED_STATS -- (the same object every time).
        Asynchronous: nothing here waits for the device."""
        eng = self.engine
        index, count = batch.get("index"), batch.get("count")  # (the multi-agent collector's list; None: every row)
        adv, norm = self._advantages(batch, index, count)
        normalise_obs = getattr(self.collector, "normalise_obs", False)
        if normalise_obs:  # (the rollout's own table: it moves at the next collect() only)
            eng.obs_norm_bind(self.collector.obs_norm, self.in_dim, self.collector.clip_obs)
        if self.live_count is not None:  # the learner's own copy of the count: a stop zeroes it, the collector's stays
            if count is not None:
                self.live_count.copy_(count.view(1))
            else:
                self.live_count.fill_(self.n_list)
            count = self.live_count
        if self.gate is not None:
            self.gate.zero_()
        k = 0
        for epoch in range(self.epochs):
            if self.shuffle:  # (adv_stats above read the collector's own list: the same entries in another order)
                eng.shuffle_index(batch.get("index"), count, self.n_list, self.shuffle_seed, epoch, epoch_dev=self._epoch, out=self.shuffled)
                index = self.shuffled
            for start, stride, rows in self.plan:
                self._grad(batch, adv, self.stats[k], start=start, stride=stride, rows=rows, index=index, count=count, n_list=self.n_list,
                           adv_stats=norm, clip=self.clip, ent_coef=self.ent_coef, in_dim=self.in_dim)
                if self.gate is None:
                    eng.adam(self.params, self.grads, self.m, self.v, self.step, self.lr, betas=self.betas, eps=self.eps,
                             max_grad_norm=self.max_grad_norm)
                else:
                    stop = self.kl_limit is not None
                    eng.adam_gated(self.params, self.grads, self.m, self.v, self.step, self.lr, self.gate, betas=self.betas, eps=self.eps,
                                   max_grad_norm=self.max_grad_norm, lr_scale=self.lr_scale, kl=self.stats[k, 4:] if stop else None,
                                   kl_limit=self.kl_limit if stop else 0.0, count_gate=self.live_count if stop else None)
                k += 1
        if self.shuffle:
            self._epoch.add_(self.epochs)
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
    the next multiplier step from the lambda it finds.  guide=, bc_coef=, keep_surrogate= as for PPOLearner (Engine.ppo_grad_guided with the
    cost critic's arguments; statistics [.., 12]).  ONE flat buffer holds the eighteen weight tensors (flat_layout(...,
    has_cost_critic=True)); the collector is handed the views.  `ppo_kwargs`: PPOLearner's arguments (normalise_advantages False: no
    scaling of the reward advantage and no centring of either; shuffle, shuffle_seed, target_kl, lr_scale as there: the permutation is
    drawn over every row, the stop reads the same statistics slot, the multiplier step is taken before the gate is looked at)."""
    NETS = ("policy", "value", "cost")
    GRAD = "pgd_ppo_grad_cost"

    def __init__(self, collector, cost_limit, lambda_lr=0.05, lambda_init=0.0, lambda_max=100.0, cvf_coef=0.5, lr=3e-4, clip=0.2, vf_coef=0.5,
                 ent_coef=0.0, epochs=4, minibatches=4, max_grad_norm=0.5, betas=(0.9, 0.999), eps=1e-5, normalise_advantages=True, shuffle=False,
                 shuffle_seed=0, target_kl=None, lr_scale=False, guide=None, bc_coef=1.0, keep_surrogate=False):
        if not (0.0 <= float(lambda_init) <= float(lambda_max)):
            raise ValueError("PPOLagLearner: lambda_init = %r outside [0, lambda_max = %r]" % (lambda_init, lambda_max))
        super().__init__(collector, lr, clip, vf_coef, ent_coef, epochs, minibatches, max_grad_norm, betas, eps, normalise_advantages,
                         shuffle=shuffle, shuffle_seed=shuffle_seed, target_kl=target_kl, lr_scale=lr_scale, guide=guide, bc_coef=bc_coef,
                         keep_surrogate=keep_surrogate)
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

    def _guided_cost(self, batch):
        return dict(cost_weights=self.cost_weights, cost_grads=self.cost_grads, cost_ret=batch["cost_returns"], cvf_coef=self.cvf_coef)

    def _grad(self, batch, adv, stats, **minibatch):
        if self.guide is not None:
            return super()._grad(batch, adv, stats, **minibatch)
        self.engine.ppo_grad_cost(self.policy_weights, self.value_weights, self.cost_weights, self.policy_grads, self.value_grads, self.cost_grads,
                                  batch["obs"], batch["actions"], batch["logp"], adv, batch["returns"], batch["cost_returns"], stats, self.work,
                                  vf_coef=self.vf_coef, cvf_coef=self.cvf_coef, **minibatch)
