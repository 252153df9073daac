"""What the GPU tests of the training path share (test_actor_critic_gpu, test_marl_rollout_gpu, test_ppo_update_gpu, test_safe_ppo_gpu,
test_policy_gpu): tensors and cheap engines, the pointer structs of the C ABI, bit comparisons, and the collectors' calls made one at a
time."""
import numpy as np

SENT = 7.0   # what an output buffer holds before a launch
ERR_ARG = 1  # PGD_ERR_ARG
SIX = ("w1", "b1", "w2", "b2", "w3", "b3")


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


def snapshot(batch, keys):
    import torch
    torch.cuda.synchronize()
    return {k: batch[k].clone() for k in keys}


def bits_equal(a, b):
    import torch
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def synchronised_rollouts(S, n_rollouts, T, seed, keys, live0=None):
    """The calls of a collector made one at a time into fresh buffers, a device synchronisation behind each; evaluation j has tick j.
    `S`: eng, first (the first observation), pw, vw.  Single-agent engines: mlp_actor_critic, step, ..., gae.  Multi-agent engines
    (`live0`: the live rows of the first observation, from the state): live rows, mlp_actor_critic_rows, step, ..., gae_masked,
    rollout_index."""
    import torch
    eng = S.eng
    N, A, D = eng.N, eng.A, eng.D
    marl = live0 is not None
    shape = (N, A) if marl else (N, )

    def evaluate(obs, tick, rows, count):
        a = torch.full((N, A, 2), SENT, dtype=torch.float32, device="cuda")
        lp = torch.full((N, A), SENT, dtype=torch.float32, device="cuda")
        v = torch.full((N, A), SENT, dtype=torch.float32, device="cuda")
        if marl:
            eng.mlp_actor_critic_rows(S.pw, S.vw, rows, count, a, lp, v, seed, tick, obs=obs)
        else:
            eng.mlp_actor_critic(S.pw, S.vw, a, lp, v, seed, tick, obs=obs)
        torch.cuda.synchronize()
        return a, lp, v

    obs = S.first.clone()
    rows = count = None
    if marl:
        rows = torch.zeros((N * A, ), dtype=torch.int32, device="cuda")
        rows[:len(live0)] = dev(live0)
        count = dev(np.array([len(live0)], dtype=np.int32))
    a, lp, v = evaluate(obs, 0, rows, count)
    out = []
    for k in range(n_rollouts):
        rec = {key: [] for key in keys}
        for t in range(T):
            rec["obs"].append(obs.view(*shape, D))
            rec["actions"].append(a.view(*shape, 2))
            rec["logp"].append(lp.view(shape))
            rec["values"].append(v.view(shape))
            obs, rew, done, flags = eng.step(a, out=eng.make_outputs())
            torch.cuda.synchronize()
            rec["rewards"].append(rew.view(shape))
            rec["dones"].append(done.view(shape))
            rec["flags"].append(flags.view(shape))
            if marl:
                rows, count = eng.live_rows(flags, done)
                torch.cuda.synchronize()
            a, lp, v = evaluate(obs, k * T + t + 1, rows, count)
        rec["values"].append(v.view(shape))
        r = {key: torch.stack(rec[key]) for key in keys if rec[key]}
        if marl:
            r["advantages"], r["returns"], r["mask"] = eng.gae_masked(r["rewards"], r["values"], r["dones"], r["flags"], 0.99, 0.95)
            torch.cuda.synchronize()
            index = torch.zeros((T * N * A, ), dtype=torch.int32, device="cuda")
            r["index"], r["count"] = eng.rollout_index(r["flags"], index=index)
        else:
            r["advantages"], r["returns"] = eng.gae(r["rewards"], r["values"], r["dones"], 0.99, 0.95)
        torch.cuda.synchronize()
        out.append(r)
    return out
