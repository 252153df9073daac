"""What the GPU tests of the update kernels share (test_ppo_update_gpu, test_minibatch_gpu, test_categorical_gpu): a checker case on the
device, one gradient call into sentinel-filled buffers (pgd_ppo_grad through ctypes here; the categorical module hands in its own call), and
its comparison with the float64 restatement of tests/ppo_ref.py or tests/categorical_ref.py."""
import ctypes as C

import numpy as np

from tests import ppo_ref as rf
from tests.train_util import SENT, ac_nets, dev, six


def shapes(in_dim, out_cols):
    return [(in_dim, 256), (256, ), (256, 256), (256, ), (256, out_cols), (out_cols, )], [(in_dim, 256), (256, ), (256, 256), (256, ), (256, 1), (1, )]


# the per-row arrays of a case: key -> (columns (0: a vector; None: the case's own stride), dtype, what every row outside the case holds).
# A Gaussian case brings `action`, a categorical one `index` (tests/categorical_ref.py): the taken bins, a wild number elsewhere.
ROW_KEYS = dict(x=(None, np.float32, np.nan), action=(2, np.float32, np.nan), index=(2, np.int32, 2 ** 30), logp_old=(0, np.float32, np.nan),
                adv=(0, np.float32, np.nan), ret=(0, np.float32, np.nan))


class Problem:
    """The rollout arrays of a case on the device -- n_rows rows, of which `where` hold the case's rows in minibatch order and every
    other row holds NaN (a wild number in an integer array) in every array -- and a list over them."""
    def __init__(self, case, n_rows=None, where=None, index=None, count=None, n_list=None):
        rows = case["x"].shape[0]
        n_rows = rows if n_rows is None else n_rows
        where = np.arange(rows) if where is None else np.asarray(where)
        full = {}
        for key, (width, dtype, fill) in ROW_KEYS.items():
            if key in case:
                width = case[key].shape[1] if width is None else width
                a = np.full((n_rows, width) if width else (n_rows, ), fill, dtype=dtype)
                a[where] = case[key]
                full[key] = dev(a)
        self.t = full
        self.case, self.n_rows = case, n_rows
        self.index = dev(np.asarray(index, dtype=np.int32)) if index is not None else None
        self.count = dev(np.array([count], dtype=np.int32)) if count is not None else None
        self.n_list = int(n_list if n_list is not None else (len(index) if index is not None else n_rows))
        self.stats_in = dev(case["adv_stats"]) if case["adv_stats"] is not None else None
        self.pw = tuple(dev(w) for w in case["policy"])
        self.vw = tuple(dev(w) for w in case["value"])


def into_sentinels(P, critic, work_floats, call):
    """`call(pg, vg, stats, work)` -- one gradient call of either head, made and synchronised by the caller's closure; its return value
    true: the call was refused, as it was meant to be -- on sentinel-filled gradients and statistics and NaN-filled scratch ->
    dict(stats, policy, value) as numpy (value: the untouched buffers without a critic), and the raw tensors for bit comparisons.
    Every live gradient entry has been written and, without a critic, none of the critic's; a refused call has written nothing (-> None)."""
    import torch
    ps, vs = shapes(P.case["in_dim"], P.case["policy"][4].shape[1])
    pg = [torch.full(s, SENT, dtype=torch.float32, device="cuda") for s in ps]
    vg = [torch.full(s, SENT, dtype=torch.float32, device="cuda") for s in vs]
    stats = torch.full((8, ), SENT, dtype=torch.float32, device="cuda")
    work = torch.full((work_floats, ), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    refused = call(pg, vg, stats, work)
    torch.cuda.synchronize()
    if refused:
        for t in [stats] + pg + vg:
            assert bool((t == SENT).all()), "a refused call wrote"
        return None
    out = dict(stats=stats.cpu().numpy(), policy=[g.cpu().numpy() for g in pg], value=[g.cpu().numpy() for g in vg], raw=[stats] + pg + vg)
    for g in out["policy"] + (out["value"] if critic else []):
        assert not (g == SENT).any(), "a gradient entry was not written"
    if not critic:
        assert all((g == SENT).all() for g in out["value"]), "the critic's gradients were written without a critic"
    return out


def grad(eng, P, start=0, stride=1, rows=None, critic=True, ent_coef=rf.ENT_COEF, short_by=0, shift=0, expect=0):
    """One pgd_ppo_grad through ctypes (into_sentinels).  short_by: bytes taken off work_bytes; shift: floats added to the scratch pointer;
    expect: the status such a call must return, with every output buffer left as it was."""
    from pgdrive_amd import _abi
    k, oc = P.case["in_dim"], P.case["policy"][4].shape[1]
    rows = P.n_list if rows is None else rows
    need = eng.L.pgd_ppo_work_bytes(k, rows, int(critic))
    assert need > 0

    def call(pg, vg, stats, work):
        nets, grads, b = ac_nets(P.pw, P.vw if critic else None, oc), six(_abi.PPOGrads(), pg), _abi.PPOBatch()
        if critic:
            six(grads, vg, "v")
        b.obs, b.action, b.logp_old, b.adv, b.ret = [P.t[q].data_ptr() for q in ("x", "action", "logp_old", "adv", "ret")]
        b.adv_stats = P.stats_in.data_ptr() if P.stats_in is not None else None
        b.index = P.index.data_ptr() if P.index is not None else None
        b.count = P.count.data_ptr() if P.count is not None else None
        b.obs_stride, b.in_dim, b.n_rows, b.n_list, b.start, b.stride, b.rows = P.case["x"].shape[1], k, P.n_rows, P.n_list, start, stride, rows
        hp = _abi.PPOHyper(rf.CLIP, rf.VF_COEF, ent_coef)
        eng._follow_stream()
        rc = eng.L.pgd_ppo_grad(eng.h, C.byref(nets), C.byref(b), C.byref(hp), C.byref(grads), C.c_void_p(stats.data_ptr()),
                                C.c_void_p(work.data_ptr() + 4 * shift), need - short_by)
        assert rc == expect, rc
        eng.sync()
        return bool(expect)

    return into_sentinels(P, critic, (need + 3) // 4 + shift, call)


def check(got, ref, what, live=4, tolerances=rf.tolerances):
    """The gradients and statistics of one call against the float64 reference, under the tolerances of the head's checker; the head's
    columns at or beyond its live width (4, or the categorical head's K) are exactly zero."""
    eg, es = rf.grad_errors(got, ref)
    tol_g, tol_s = tolerances(int(ref["stats"][0]))
    print("%s: gradients %.3f of %.2e, statistics %.3f of %.2e; per slot 1 .. 6: %s" % (
        what, eg / tol_g, tol_g, es / tol_s, tol_s, " ".join("%.2e" % e for e in rf.stat_errors(got, ref))))
    assert eg < tol_g and es < tol_s, (what, eg, tol_g, es, tol_s)
    assert (got["policy"][4][:, live:] == 0).all() and (got["policy"][5][live:] == 0).all(), (what, "unused head columns")
