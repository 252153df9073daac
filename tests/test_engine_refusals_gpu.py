"""Every Engine method that takes a device tensor refuses a defective one before anything is launched.

One table, one row per method: a function that builds a valid argument set (inputs zero or a valid list, every output filled with
train_util.SENT) and a call on it.  The valid set is accepted; then the call is repeated on a second set with one tensor at a time
replaced by a defective one -- a wrong dtype, one element short, non-contiguous -- and must raise AssertionError (PgdArgError is one; the
base class lets this file run on an engine.py that still asserts).  Afterwards every tensor of the second set and every defective tensor
holds the bits it held: a refused call launched nothing.

THE RULE THAT MAKES THIS SAFE ON A SHARED MACHINE: no defective tensor could cause an out-of-bounds access if its refusal were missing.
The short tensor is a view big[:n - 1] of an allocation of n elements; the wrong dtype has at least as many bytes per element (int32
for float32, float32 for int32 and uint8, int64 for float64); the non-contiguous tensor is every second element of an allocation twice
the size; a defective input holds zero bits (row 0, count 0, flags 0), never a number a kernel could take for a far index.  A missing
check then shows as a failed test with overwritten sentinels, never as a fault.  There is no not-cuda case here: a host address must
never reach the library, so that clause is tested on the CPU (tests/test_engine_args_cpu.py).

NEW_REFUSALS are the cases the engine.py before section 32 let through to a kernel; they have tests of their own, named new_refusal."""
import numpy as np
import pytest

from tests.train_util import SENT, SIX, bits_equal, ego_engine

pytestmark = pytest.mark.gpu

N, T = 4, 2
ALL = ("dtype", "short", "strided")
ONE = ("dtype", "short")  # one-element tensors: contiguity is not asked


def _t():
    import torch
    return torch


def zeros(*shape, dtype=None):
    return _t().zeros(shape, dtype=dtype or _t().float32, device="cuda")


def sent(*shape, dtype=None):
    return _t().full(shape, SENT, dtype=dtype or _t().float32, device="cuda")


def arange(n):
    return _t().arange(n, dtype=_t().int32, device="cuda")


def i32(*values):
    return _t().tensor(values, dtype=_t().int32, device="cuda")


def defective(v, kind, fill):
    """-> (the defective stand-in for `v`, the allocation it is a view of)."""
    t = _t()
    if kind == "dtype":
        other = {t.float32: t.int32, t.int32: t.float32, t.uint8: t.float32, t.float64: t.int64}[v.dtype]
        base = t.full(tuple(v.shape), fill, dtype=other, device="cuda")
        return base, base
    if kind == "short":
        base = t.full((v.numel(), ), fill, dtype=v.dtype, device="cuda")
        return base[:v.numel() - 1], base
    base = t.full(tuple(v.shape) + (2, ), fill, dtype=v.dtype, device="cuda")
    return base[..., 0], base


class World:
    """The engines and networks the rows share: `eng` 4 envs, ego only, D = 18; `grouped` 8 such envs in two groups; `lidar` 4 envs with
    40 beams (the guardian wants a lidar); `image` 4 envs with the top-down observation and the renderer on."""
    def __init__(self, descs):
        import torch
        from pgdrive_amd import _abi, render
        from tests import actor_critic_ref as ar
        from tests.train_util import dev
        self.eng = ego_engine(descs, N)
        self.grouped = ego_engine(descs, 2 * N)
        self.lidar = ego_engine(descs, N, num_lasers=40)
        self.image = ego_engine(descs, N)
        for e in (self.eng, self.grouped, self.lidar, self.image):
            e.reset(np.arange(e.N) % 4)
        self.grouped.set_groups(2)
        self.image.enable_topdown(_abi.make_topdown_config(resolution=16))
        self.image.enable_render(render.make_config(render.parse_kwargs("top_down", dict(film_size=(64, 64)))))
        self.D = self.eng.D
        rng = np.random.default_rng(0)
        p, v = ar.make_networks(rng, self.D, 4)
        _, c = ar.make_networks(rng, self.D, 4)
        self.p, self.v, self.c = [tuple(dev(w) for w in n) for n in (p, v, c)]
        self.expert = tuple(dev(w) for w in ar.make_networks(rng, self.lidar.D, 4)[0])
        torch.cuda.synchronize()


@pytest.fixture(scope="module")
def world(descs):
    return World(descs)


def nets(a, **named):
    """The six tensors of each named network as arguments <name>_w1 .. <name>_b3 (copies: an argument set owns its tensors)."""
    for name, six in named.items():
        a.update({"%s_%s" % (name, k): w.clone() for k, w in zip(SIX, six)})
    return a


def grads(a, **named):
    for name, six in named.items():
        a.update({"%s_%s" % (name, k): _t().full_like(w, SENT) for k, w in zip(SIX, six)})
    return a


def six(a, name):
    return tuple(a["%s_%s" % (name, k)] for k in SIX)


# ---------------------------------------------------------------------------------------------------------------------
# the table: name -> build(world) -> (call(args), args, outputs, cases); cases: argument -> the defects that apply (default ALL)
# ---------------------------------------------------------------------------------------------------------------------
ROWS = {}
NEW_REFUSALS = {}


def row(new=(), **cases):
    def add(build):
        name = build.__name__
        ROWS[name] = (build, cases)
        if new:
            NEW_REFUSALS[name] = frozenset(new)
        return build
    return add


def _obs(w, *lead):
    return zeros(*lead, w.D)


@row()
def reset(w):
    return lambda a: w.eng.reset(np.arange(N) % 4, out=a["out"]), dict(out=sent(N, 1, w.D)), ("out", )


@row(new=[(k, d) for k in ("obs", "reward", "done", "flags") for d in ALL])
def step(w):
    t = _t()
    a = dict(actions=zeros(N, 1, 2), obs=sent(N, 1, w.D), reward=sent(N, 1), done=sent(N, 1, dtype=t.uint8), flags=sent(N, 1, dtype=t.int32))
    return lambda a: w.eng.step(a["actions"], out=(a["obs"], a["reward"], a["done"], a["flags"])), a, ("obs", "reward", "done", "flags")


@row()
def step_group(w):
    return lambda a: w.grouped.step_group(0, a["actions"]), dict(actions=zeros(2 * N, 1, 2)), ()


@row()
def step_packed(w):
    return lambda a: w.eng.step_packed(a["actions"], a["rows"]), dict(actions=zeros(N, 1, 2), rows=sent(N, w.D + 2)), ("rows", )


@row()
def step_n(w):
    return lambda a: w.eng.step_n(a["action_ring"], 0, 1), dict(action_ring=zeros(2, N, 1, 2)), ()


@row(new=[("p_b1", "short"), ("p_b2", "short"), ("p_b3", "short")])
def mlp_prepare(w):
    return lambda a: w.eng.mlp_prepare(six(a, "p")), nets({}, p=w.p), ()


@row(new=[("p_b1", "short"), ("p_b2", "short"), ("p_b3", "short")])
def mlp_policy(w):
    return (lambda a: w.eng.mlp_policy(six(a, "p"), a["out"], obs=a["obs"]), nets(dict(out=sent(N, 1, 2), obs=_obs(w, N, 1)), p=w.p),
            ("out", ))


@row(new=[("prepared", d) for d in ALL])
def mlp_policy_prepared(w):
    a = dict(out=sent(N, 1, 2), obs=_obs(w, N, 1), prepared=w.eng.mlp_prepare(w.p))
    return lambda a: w.eng.mlp_policy(None, a["out"], obs=a["obs"], in_dim=w.D, prepared=a["prepared"]), a, ("out", )


@row(new=[("obs", d) for d in ALL])
def lane_keep_actions(w):
    return lambda a: w.eng.lane_keep_actions(a["out"], 0, obs=a["obs"]), dict(out=sent(N, 1, 2), obs=_obs(w, N, 1)), ("out", )


def _ac(w, **more):
    return nets(dict(out=sent(N, 1, 2), logp=sent(N, 1), value=sent(N, 1), obs=_obs(w, N, 1), **more), p=w.p, v=w.v)


@row()
def mlp_actor_critic(w):
    return (lambda a: w.eng.mlp_actor_critic(six(a, "p"), six(a, "v"), a["out"], a["logp"], a["value"], 1, 0, obs=a["obs"]), _ac(w),
            ("out", "logp", "value"))


@row(count=ONE)
def mlp_actor_critic_rows(w):
    return (lambda a: w.eng.mlp_actor_critic_rows(six(a, "p"), six(a, "v"), a["rows"], a["count"], a["out"], a["logp"], a["value"], 1, 0,
                                                  obs=a["obs"]), _ac(w, rows=arange(N), count=i32(N)), ("out", "logp", "value"))


@row()
def mlp_actor_critic_cost(w):
    return (lambda a: w.eng.mlp_actor_critic_cost(six(a, "p"), six(a, "v"), six(a, "c"), a["out"], a["logp"], a["value"], a["cost_value"], 1, 0,
                                                  obs=a["obs"]), nets(_ac(w, cost_value=sent(N, 1)), c=w.c),
            ("out", "logp", "value", "cost_value"))


@row()
def mlp_terminal_value(w):
    t = _t()
    a = nets(dict(term_obs=_obs(w, N), flags=zeros(N, dtype=t.int32), done=zeros(N, dtype=t.uint8), term_value=sent(N), term_cost_value=sent(N)),
             v=w.v, c=w.c)
    return (lambda a: w.eng.mlp_terminal_value(six(a, "v"), six(a, "c"), a["term_obs"], a["flags"], a["done"], a["term_value"],
                                               a["term_cost_value"]), a, ("term_value", "term_cost_value"))


@row()
def guardian(w):
    t = _t()
    e = w.lidar
    a = nets(dict(actions=zeros(N, 1, 2), state=zeros(N, dtype=t.uint8), applied=sent(N, 1, 2), info=sent(N, dtype=t.uint8),
                  prev_flags=zeros(N, 1, dtype=t.int32), trace=sent(N, 4), obs=zeros(N, 1, e.D)), x=w.expert)
    return (lambda a: e.guardian(six(a, "x"), 0.5, a["actions"], a["state"], a["applied"], a["info"], 1, 0, prev_flags=a["prev_flags"],
                                 trace=a["trace"], obs=a["obs"]), a, ("applied", "info", "trace"))


@row(counter=ONE)
def actor_critic_tick(w):
    def call(a):
        w.eng.actor_critic_tick(a["counter"])
        w.eng.actor_critic_tick(None)
    return call, dict(counter=zeros(1, dtype=_t().int32)), ()


def _rollout(**more):
    return dict(reward=zeros(T, N), value=zeros(T + 1, N), done=zeros(T, N, dtype=_t().uint8), adv=sent(T, N), ret=sent(T, N), **more)


@row()
def gae(w):
    return lambda a: w.eng.gae(a["reward"], a["value"], a["done"], 0.99, 0.95, adv=a["adv"], ret=a["ret"]), _rollout(), ("adv", "ret")


@row()
def gae_masked(w):
    t = _t()
    return (lambda a: w.eng.gae_masked(a["reward"], a["value"], a["done"], a["flags"], 0.99, 0.95, adv=a["adv"], ret=a["ret"], mask=a["mask"]),
            _rollout(flags=zeros(T, N, dtype=t.int32), mask=sent(T, N, dtype=t.uint8)), ("adv", "ret", "mask"))


@row()
def gae_bootstrap(w):
    return (lambda a: w.eng.gae_bootstrap(a["reward"], a["value"], a["done"], a["term_value"], 0.99, 0.95, adv=a["adv"], ret=a["ret"]),
            _rollout(term_value=zeros(T, N)), ("adv", "ret"))


def _cost_rollout(**more):
    t = _t()
    return dict(flags=zeros(T, N, dtype=t.int32), done=zeros(T, N, dtype=t.uint8), cost_value=zeros(T + 1, N), run=zeros(N), cost=sent(T, N),
                adv=sent(T, N), ret=sent(T, N), ep_sum=sent(N), ep_count=sent(N, dtype=t.int32), **more)


COST_OUT = ("cost", "adv", "ret", "ep_sum", "ep_count")


@row()
def cost_gae(w):
    return (lambda a: w.eng.cost_gae(a["flags"], a["done"], a["cost_value"], (1.0, 1.0, 1.0), 0.99, 0.95, a["run"],
                                     **{k: a[k] for k in COST_OUT}), _cost_rollout(), COST_OUT)


@row()
def cost_gae_bootstrap(w):
    return (lambda a: w.eng.cost_gae_bootstrap(a["flags"], a["done"], a["cost_value"], a["term_cost_value"], (1.0, 1.0, 1.0), 0.99, 0.95,
                                               a["run"], **{k: a[k] for k in COST_OUT}), _cost_rollout(term_cost_value=zeros(T, N)), COST_OUT)


@row(count=ONE)
def live_rows(w):
    t = _t()
    a = dict(flags=zeros(N, 1, dtype=t.int32), done=zeros(N, 1, dtype=t.uint8), rows=sent(N, dtype=t.int32), count=sent(1, dtype=t.int32))
    return lambda a: w.eng.live_rows(a["flags"], a["done"], rows=a["rows"], count=a["count"]), a, ("rows", "count")


@row(flags=("dtype", "strided"), count=ONE)  # (a shorter `flags` is a shorter rollout: the tensor states its own length)
def rollout_index(w):
    t = _t()
    a = dict(flags=zeros(T, N, dtype=t.int32), index=sent(T * N, dtype=t.int32), count=sent(1, dtype=t.int32))
    return lambda a: w.eng.rollout_index(a["flags"], index=a["index"], count=a["count"]), a, ("index", "count")


@row()
def adv_stats(w):
    return lambda a: w.eng.adv_stats(a["adv"], out=a["out"], n_list=T * N), dict(adv=zeros(T, N), out=sent(2)), ("out", )


@row()
def adv_mix(w):
    a = dict(adv=zeros(T, N), cadv=zeros(T, N), state=zeros(4), out=sent(T, N), adv_stats=zeros(2), cadv_stats=zeros(2))
    return (lambda a: w.eng.adv_mix(a["adv"], a["cadv"], a["state"], out=a["out"], adv_stats=a["adv_stats"], cadv_stats=a["cadv_stats"]), a,
            ("out", ))


@row()
def lagrange(w):
    a = dict(ep_sum=zeros(N), ep_count=zeros(N, dtype=_t().int32), state=zeros(4))
    return lambda a: w.eng.lagrange(a["ep_sum"], a["ep_count"], a["state"], 1.0, 0.01), a, ()


def _ppo(w, work_bytes, **more):
    t = _t()
    a = dict(obs=_obs(w, T, N), actions=zeros(T, N, 2), logp_old=zeros(T, N), adv=zeros(T, N), ret=zeros(T, N), stats=sent(8),
             work=zeros(work_bytes, dtype=t.uint8), index=arange(T * N), count=i32(T * N), adv_stats=zeros(2), **more)
    return grads(nets(a, p=w.p, v=w.v), pg=w.p, vg=w.v)


PPO_CASES = dict(work=("short", "strided"), count=ONE)  # (`work` may be of any dtype)
PPO_OUT = tuple("%s_%s" % (n, k) for n in ("pg", "vg") for k in SIX) + ("stats", )


@row(**PPO_CASES)
def ppo_grad(w):
    return (lambda a: w.eng.ppo_grad(six(a, "p"), six(a, "v"), six(a, "pg"), six(a, "vg"), a["obs"], a["actions"], a["logp_old"], a["adv"],
                                     a["ret"], a["stats"], a["work"], index=a["index"], count=a["count"], n_list=T * N, adv_stats=a["adv_stats"]),
            _ppo(w, w.eng.ppo_work_bytes(w.D, T * N)), PPO_OUT)


@row(**PPO_CASES)
def ppo_grad_cost(w):
    a = grads(nets(_ppo(w, w.eng.ppo_cost_work_bytes(w.D, T * N), cost_ret=zeros(T, N)), c=w.c), cg=w.c)
    return (lambda a: w.eng.ppo_grad_cost(six(a, "p"), six(a, "v"), six(a, "c"), six(a, "pg"), six(a, "vg"), six(a, "cg"), a["obs"],
                                          a["actions"], a["logp_old"], a["adv"], a["ret"], a["cost_ret"], a["stats"], a["work"],
                                          index=a["index"], count=a["count"], n_list=T * N, adv_stats=a["adv_stats"]), a,
            PPO_OUT + tuple("cg_%s" % k for k in SIX))


def _adam(**more):
    return dict(param=zeros(16), grad=zeros(16), m=zeros(16), v=zeros(16), step=zeros(4, dtype=_t().int32), **more)


@row()
def adam(w):
    return lambda a: w.eng.adam(a["param"], a["grad"], a["m"], a["v"], a["step"], 3e-4), _adam(), ()


@row(lr_scale=ONE, kl=ONE, count_gate=ONE)
def adam_gated(w):
    t = _t()
    return (lambda a: w.eng.adam_gated(a["param"], a["grad"], a["m"], a["v"], a["step"], 3e-4, a["gate"], lr_scale=a["lr_scale"], kl=a["kl"],
                                       kl_limit=1.0, count_gate=a["count_gate"]),
            _adam(gate=zeros(4, dtype=t.int32), lr_scale=zeros(1), kl=zeros(1), count_gate=zeros(1, dtype=t.int32)), ())


@row(count=ONE, epoch_dev=ONE)
def shuffle_index(w):
    t = _t()
    a = dict(index=arange(T * N), count=i32(T * N), epoch_dev=zeros(1, dtype=t.int32), out=sent(T * N, dtype=t.int32))
    return lambda a: w.eng.shuffle_index(a["index"], a["count"], T * N, 1, 0, epoch_dev=a["epoch_dev"], out=a["out"]), a, ("out", )


def _f64_work(n_bytes):
    return zeros((n_bytes + 7) // 8, dtype=_t().float64)


WORK = ("strided", )  # (the size of a caller's `work` is the library's to refuse, its dtype is free)


@row(work=WORK)
def return_norm(w):
    t = _t()
    from pgdrive_amd import _abi
    a = dict(reward=zeros(T, N), done=zeros(T, N, dtype=t.uint8), flags=zeros(T, N, dtype=t.int32), carry=zeros(N),
             record=t.tensor(_abi.RETURN_NORM_INIT, dtype=t.float64, device="cuda"), out=sent(T, N), work=_f64_work(w.eng.return_norm_work_bytes(N)))
    return (lambda a: w.eng.return_norm(a["reward"], a["done"], 0.99, a["carry"], a["record"], flags=a["flags"], out=a["out"], work=a["work"]), a,
            ("out", ))


@row(work=WORK, count=ONE)
def obs_norm_update(w):
    t = _t()
    a = dict(obs=_obs(w, T, N), record=zeros(1 + 2 * w.D, dtype=t.float64), index=arange(T * N), count=i32(T * N),
             work=_f64_work(w.eng.obs_norm_work_bytes(w.D, T * N)))
    return lambda a: w.eng.obs_norm_update(a["obs"], a["record"], index=a["index"], count=a["count"], n_list=T * N, work=a["work"]), a, ()


def _table(w):
    return sent(2, (w.D + 3) & ~3)


@row()
def obs_norm_publish(w):
    return (lambda a: w.eng.obs_norm_publish(a["record"], a["table"]), dict(record=zeros(1 + 2 * w.D, dtype=_t().float64), table=_table(w)),
            ("table", ))


@row()
def obs_norm_bind(w):
    def call(a):
        w.eng.obs_norm_bind(a["table"])
        w.eng.obs_norm_bind(None)
    return call, dict(table=_table(w)), ()


@row(work=WORK)
def rollout_episodes(w):
    t = _t()
    from pgdrive_amd import _abi
    a = dict(reward=zeros(T, N), done=zeros(T, N, dtype=t.uint8), flags=zeros(T, N, dtype=t.int32), ret_carry=zeros(N),
             len_carry=zeros(N, dtype=t.int32), record=t.tensor(_abi.ROLLOUT_EPISODES_INIT, dtype=t.float64, device="cuda"),
             call=sent(len(_abi.ROLLOUT_EPISODES), dtype=t.float64), ep_return=sent(T, N), ep_length=sent(T, N, dtype=t.int32),
             work=_f64_work(w.eng.rollout_episodes_work_bytes(N)))
    return (lambda a: w.eng.rollout_episodes(a["reward"], a["done"], a["flags"], a["ret_carry"], a["len_carry"], record=a["record"],
                                             call=a["call"], ep_return=a["ep_return"], ep_length=a["ep_length"], work=a["work"]), a,
            ("call", "ep_return", "ep_length"))


@row()
def observe_topdown(w):
    return lambda a: w.image.observe_topdown(out=a["out"]), dict(out=sent(*w.image.img.shape)), ("out", )


@row()
def render_topdown(w):
    c = w.image.render_cfg
    return lambda a: w.image.render_topdown(out=a["out"]), dict(out=sent(N, c.film_h, c.film_w, 3, dtype=_t().uint8)), ("out", )


# ---------------------------------------------------------------------------------------------------------------------
def _run(world, name, new):
    """The row's cases that are (new) / are not (not new) in NEW_REFUSALS."""
    torch = _t()
    build, cases = ROWS[name]
    call, valid, _ = build(world)
    call(valid)  # accepted: a status other than 0 raises PgdError
    call, args, outputs = build(world)
    before = {k: v.clone() for k, v in args.items()}
    watched = []
    for arg in args:
        for kind in cases.get(arg, ALL):
            if ((arg, kind) in NEW_REFUSALS.get(name, ())) != new or (kind == "strided" and args[arg].numel() < 2):
                continue  # (a tensor of one element is contiguous whatever its stride)
            fill = SENT if arg in outputs else 0
            bad, base = defective(args[arg], kind, fill)
            watched.append((arg, kind, base, fill))
            with pytest.raises(AssertionError):
                call(dict(args, **{arg: bad}))
                pytest.fail("%s accepted %s: %s" % (name, arg, kind), pytrace=False)
    assert watched, "no case ran"
    torch.cuda.synchronize()
    for k, v in args.items():
        assert bits_equal(v, before[k]), "%s: a refused call wrote %s" % (name, k)
    for k in outputs:
        assert bool((args[k] == SENT).all()), "%s: a refused call wrote %s" % (name, k)
    for arg, kind, base, fill in watched:
        assert bool((base == fill).all()), "%s: a refused call wrote the defective %s (%s)" % (name, arg, kind)


@pytest.mark.parametrize("name", sorted(ROWS))
def test_defective_tensor_is_refused(world, name):
    _run(world, name, new=False)


@pytest.mark.parametrize("name", sorted(NEW_REFUSALS))
def test_new_refusal(world, name):
    _run(world, name, new=True)

