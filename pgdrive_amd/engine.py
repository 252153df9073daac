"""ctypes binding of libpgdrive_hip.so (C ABI in include/pgdrive_hip.h) + torch buffers for device memory.

PyTorch is plumbing here (device allocation, streams, torch.distributed); all simulation runs in the HIP library.
There is NO CPU fallback: if the HIP library is missing or no GPU is visible, constructing an Engine raises.
"""
import ctypes as C
import os

import numpy as np

from . import _abi
from .build import LIB, build

_LIBH = None

_SIGS = {
    "pgd_obs_dim": (C.c_int, [C.POINTER(_abi.PgdConfig)]),
    "pgd_create": (C.c_int, [C.POINTER(_abi.PgdConfig), C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    "pgd_upload_maps": (C.c_int, [C.c_void_p] + [C.c_void_p, C.c_int] * 6),
    "pgd_upload_scenarios": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "pgd_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "pgd_step": (C.c_int, [C.c_void_p] * 6),
    "pgd_step_packed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pgd_step_n": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pgd_state_dims": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "pgd_get_state": (C.c_int, [C.c_void_p] * 4),
    "pgd_set_state": (C.c_int, [C.c_void_p] * 4),
    "pgd_observe": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pgd_describe_step": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "pgd_forget_rows": (C.c_int, [C.c_void_p]),
    "pgd_mlp_prepared_bytes": (C.c_size_t, [C.c_int]),
    "pgd_mlp_prepare": (C.c_int, [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 6 + [C.c_int, C.c_void_p]),
    "pgd_mlp_policy_prepared": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "pgd_step_geometry": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "pgd_set_step_module": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_int]),
    "pgd_mlp_policy": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_void_p]),
    "pgd_mlp_actor_critic": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(_abi.ActorCritic), C.c_uint32, C.c_uint32,
                                       C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pgd_actor_critic_tick": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pgd_gae": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    "pgd_live_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pgd_rollout_index": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "pgd_mlp_actor_critic_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(_abi.ActorCritic), C.c_uint32, C.c_uint32,
                                            C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pgd_mlp_actor_critic_cat": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(_abi.ActorCritic), C.c_int32, C.c_int32,
                                           C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pgd_mlp_actor_critic_cat_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(_abi.ActorCritic), C.c_int32, C.c_int32,
                                                C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p]),
    "pgd_ppo_cat_work_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "pgd_ppo_grad_cat": (C.c_int, [C.c_void_p, C.POINTER(_abi.ActorCritic), C.POINTER(_abi.PPOBatch), C.POINTER(_abi.PPOHyper),
                                   C.POINTER(_abi.PPOGrads), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "pgd_gae_masked": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p,
                                 C.c_void_p, C.c_void_p]),
    "pgd_ppo_work_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "pgd_ppo_grad": (C.c_int, [C.c_void_p, C.POINTER(_abi.ActorCritic), C.POINTER(_abi.PPOBatch), C.POINTER(_abi.PPOHyper), C.POINTER(_abi.PPOGrads),
                               C.c_void_p, C.c_void_p, C.c_size_t]),
    "pgd_adv_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "pgd_adam": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_float, C.c_float,
                           C.c_float, C.c_float]),
    "pgd_shuffle_index": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "pgd_adam_gated": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_float, C.c_float,
                                 C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]),
    "pgd_mlp_actor_critic_cost": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(_abi.ActorCritic), C.POINTER(_abi.ValueNet),
                                            C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pgd_cost_gae": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_float, C.c_float] +
                     [C.c_void_p] * 6),
    "pgd_lagrange": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_void_p]),
    "pgd_adv_mix": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pgd_ppo_cost_work_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "pgd_ppo_grad_cost": (C.c_int, [C.c_void_p, C.POINTER(_abi.ActorCritic), C.POINTER(_abi.ValueNet), C.POINTER(_abi.PPOBatch),
                                    C.POINTER(_abi.PPOCost), C.POINTER(_abi.PPOHyper), C.POINTER(_abi.PPOGrads), C.POINTER(_abi.ValueGrads),
                                    C.c_void_p, C.c_void_p, C.c_size_t]),
    "pgd_ppo_grad_guided": (C.c_int, [C.c_void_p, C.POINTER(_abi.ActorCritic), C.POINTER(_abi.ValueNet), C.POINTER(_abi.PPOBatch),
                                      C.POINTER(_abi.PPOCost), C.POINTER(_abi.PPOGuide), C.POINTER(_abi.PPOHyper), C.POINTER(_abi.PPOGrads),
                                      C.POINTER(_abi.ValueGrads), C.c_void_p, C.c_void_p, C.c_size_t]),
    "pgd_mlp_terminal_value": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(_abi.ValueNet), C.POINTER(_abi.ValueNet),
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pgd_guardian": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(_abi.ActorCritic), C.POINTER(_abi.GuardianConfig)] +
                     [C.c_void_p] * 6),
    "pgd_gae_bootstrap": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p,
                                    C.c_void_p]),
    "pgd_cost_gae_bootstrap": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_float,
                                         C.c_float] + [C.c_void_p] * 6),
    "pgd_return_norm_work_bytes": (C.c_size_t, [C.c_int]),
    "pgd_return_norm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_double, C.c_float, C.c_uint32,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "pgd_obs_norm_work_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "pgd_obs_norm_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_size_t]),
    "pgd_obs_norm_publish": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p]),
    "pgd_obs_norm_bind": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_float]),
    "pgd_rollout_episodes_work_bytes": (C.c_size_t, [C.c_int]),
    "pgd_rollout_episodes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_uint32] + [C.c_void_p] * 7 + [C.c_size_t]),
    "pgd_step_lane_keep": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_uint32] + [C.c_void_p] * 4),
    "pgd_lane_keep_actions": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_uint32]),
    "pgd_topdown_channels": (C.c_int, [C.POINTER(_abi.TopDownConfig)]),
    "pgd_topdown_enable": (C.c_int, [C.c_void_p, C.POINTER(_abi.TopDownConfig)]),
    "pgd_observe_topdown": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pgd_observe_topdown_u8": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pgd_step_info_enable": (C.c_int, [C.c_void_p, C.POINTER(_abi.StepInfo)]),
    "pgd_step_info_clear_stats": (C.c_int, [C.c_void_p]),
    "pgd_step_info_empty_launch": (C.c_int, [C.c_void_p]),
    "pgd_render_enable": (C.c_int, [C.c_void_p, C.POINTER(_abi.RenderConfig), C.c_void_p]),
    "pgd_render_topdown": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "pgd_render_palette": (C.c_int, [C.c_void_p]),
    "pgd_set_groups": (C.c_int, [C.c_void_p, C.c_int]),
    "pgd_step_group": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 5),
    "pgd_group_stream": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "pgd_group_sync": (C.c_int, [C.c_void_p, C.c_int]),
    "pgd_last_step_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "pgd_profile_begin": (C.c_int, [C.c_void_p, C.c_int]),
    "pgd_profile_begin_strided": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "pgd_enable_step_timing": (C.c_int, [C.c_void_p, C.c_int]),
    "pgd_profile_end": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    "pgd_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pgd_sync": (C.c_int, [C.c_void_p]),
    "pgd_destroy": (C.c_int, [C.c_void_p]),
    "pgd_version": (C.c_char_p, []),
    "pgd_source_sha": (C.c_char_p, []),
    "pgd_plan_arena": (C.c_int, [C.POINTER(C.c_uint64), C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "pgd_gather_create": (C.c_int, [C.c_int] * 6 + [C.POINTER(C.c_void_p)]),
    "pgd_gather_buffer": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "pgd_gather_export": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pgd_gather_connect": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "pgd_gather_push": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "pgd_gather_wait": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "pgd_gather_release": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "pgd_gather_status": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "pgd_gather_mem_kind": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "pgd_gather_destroy": (C.c_int, [C.c_void_p]),
}
EXPORTS = tuple(_SIGS.keys())


def load_library(path=None):
    """dlopen the HIP engine; fails loudly when it has not been built (no fallback path exists)."""
    global _LIBH
    if _LIBH is not None and path is None:
        return _LIBH
    # torch bundles its own HIP runtime: import it first so this library binds to the same libamdhip64 (two runtimes
    # in one process do not see each other's devices / streams)
    import torch  # noqa: F401
    p = path or os.environ.get("PGD_LIB") or LIB  # PGD_LIB: A/B runs of experimental builds (tools/ab.sh)
    if not os.path.exists(p):
        raise RuntimeError(
            "pgdrive_amd: %s is missing — build it with `python -m pgdrive_amd.build` (hipcc, gfx950). "
            "There is no CPU fallback for the step engine." % p
        )
    L = C.CDLL(p)
    for name, (res, args) in _SIGS.items():
        if path is None and os.environ.get("PGD_LIB") and not hasattr(L, name):
            continue  # A/B runs of an OLDER build (tools/ab.sh): entry points it does not have yet are simply absent
        fn = getattr(L, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _LIBH = L
    return L


def _np_p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _p(t):
    """The device pointer of a tensor, as an argument of the C ABI (None: a null pointer)."""
    return None if t is None else C.c_void_p(t.data_ptr())


class PgdError(RuntimeError):
    pass


def _chk(rc, what):
    if rc != 0:
        raise PgdError("%s failed with status %d" % (what, rc))


class PgdArgError(AssertionError):
    """An argument an Engine method refuses before it has called the library.  Raised, never asserted: the checks
    are what stands between a wrong buffer and a kernel, and `python -O` must not remove them."""


def _need(ok, where, wanted):
    """A condition on a call's arguments that is not one tensor's."""
    if not ok:
        raise PgdArgError("%s: %s" % (where, wanted))


def _dev(t, dtype, n=None, where="", name="", at_least=None, contiguous=True, align=0):
    """`t` as a device buffer a kernel may read or write, checked -> `t`.  A cuda tensor of `dtype` (one, a tuple to choose from, or None:
    any) with exactly `n` / at least `at_least` elements (None: not asked), contiguous unless told otherwise, its address a multiple of
    `align` bytes.  `where` and `name`: the method and the argument, for the message."""
    if (t.is_cuda and (t.dtype == dtype or dtype is None or (dtype.__class__ is tuple and t.dtype in dtype)) and
            (n is None or t.numel() == n) and (at_least is None or t.numel() >= at_least) and (not contiguous or t.is_contiguous()) and
            (not align or t.data_ptr() % align == 0)):
        return t
    raise PgdArgError(_refusal(t, dtype, n, where, name, at_least, contiguous, align))


def _refusal(t, dtype, n, where, name, at_least, contiguous, align):
    """The message for a tensor _dev refuses: the method, the argument, what was wanted and what was found."""
    short = lambda d: str(d).replace("torch.", "")
    wanted = "any" if dtype is None else " or ".join(short(d) for d in (dtype if dtype.__class__ is tuple else (dtype, )))
    count = "" if n is None and at_least is None else " of %d elements" % n if at_least is None else " of at least %d elements" % at_least
    found = "%s%s%s%s" % ("" if t.is_cuda else "cpu ", short(t.dtype), ", not contiguous," if contiguous and not t.is_contiguous() else "",
                          " at an address that is not," if align and t.data_ptr() % align else "")
    return "%s: %s: %s%s cuda tensor%s%s wanted, got %s of %d" % (where, name, "contiguous " if contiguous else "", wanted, count,
                                                                  ", %d-byte aligned" % align if align else "", found, t.numel())


def _opt(t, *spec):
    """_dev for an argument that may be None."""
    return None if t is None else _dev(t, *spec)


_SIX = (".w1", ".b1", ".w2", ".b2", ".w3", ".b3")  # the six tensors of a network, as a message names them


class Engine:
    """One simulation handle on one GPU: N envs x (A agents + T traffic slots)."""
    def __init__(self, cfg, bank, scen, device=0, stream=None, lib=None):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("pgdrive_amd.Engine needs a GPU (MI355X); no CPU fallback exists")
        self.torch = torch
        self.L = lib if lib is not None else load_library()  # `lib`: another build of the same ABI (tests: IEEE-math A/B)
        self.cfg = cfg
        self.N, self.A, self.T = cfg.num_envs, cfg.num_agents, cfg.num_traffic
        self.V = self.A + self.T
        self.D = _abi.obs_dim(cfg)
        _need(scen.V == self.V, "Engine", "scenario bank built for V=%d, engine has V=%d" % (scen.V, self.V))
        self.device = torch.device("cuda", device)
        self.bank, self.scen = bank, scen
        h = C.c_void_p()
        torch.cuda.set_device(self.device)
        # the engine enqueues on its own torch stream; step() orders it after / before the caller's current stream
        self.stream = stream if stream is not None else torch.cuda.Stream(device=self.device)
        sptr = C.c_void_p(self.stream.cuda_stream)
        _chk(self.L.pgd_create(C.byref(cfg), device, sptr, C.byref(h)), "pgd_create")
        self.h = h
        _chk(
            self.L.pgd_upload_maps(
                self.h, _np_p(bank.maps), len(bank.maps), _np_p(bank.lanes), len(bank.lanes), _np_p(bank.roads),
                len(bank.roads), _np_p(bank.boxes), len(bank.boxes), _np_p(bank.cell_start), len(bank.cell_start),
                _np_p(bank.cell_items), len(bank.cell_items)
            ), "pgd_upload_maps"
        )
        _chk(self.L.pgd_upload_scenarios(self.h, _np_p(scen.scenarios), len(scen.scenarios), _np_p(scen.spawns)),
             "pgd_upload_scenarios")
        dev = self.device
        self.obs = torch.zeros((self.N, self.A, self.D), dtype=torch.float32, device=dev)
        self.reward = torch.zeros((self.N, self.A), dtype=torch.float32, device=dev)
        self.done = torch.zeros((self.N, self.A), dtype=torch.uint8, device=dev)
        self.flags = torch.zeros((self.N, self.A), dtype=torch.int32, device=dev)
        self._bound_stream = self.stream.cuda_stream  # the stream pgd_create was given
        self._own_ptrs = tuple(C.c_void_p(t.data_ptr()) for t in (self.obs, self.reward, self.done, self.flags))
        self._seen_out = []  # caller-supplied observation tensors of the last steps, kept alive (see step)
        self.step_info = None  # the dict of enable_step_info while the step info is on
        self.n_groups = 1  # env groups of set_groups (1 = none)
        torch.cuda.synchronize(dev)

    def _follow_stream(self):
        """The engine follows the caller's current stream (like a torch op): no events, no cross-stream waits per call; pgd_set_stream
        orders the hand-over when the stream changes.  (Calls on an env group run on the group's stream and do not come here.)"""
        cur = self.torch.cuda.current_stream(self.device).cuda_stream
        if cur != self._bound_stream:
            _chk(self.L.pgd_set_stream(self.h, C.c_void_p(cur)), "pgd_set_stream")
            self._bound_stream = cur

    def _check_actions(self, actions, where="step", name="actions"):
        """An action tensor (or a buffer for one): float32 cuda, contiguous, [N, A, 2], 8-byte aligned (the step kernel reads an agent's
        pair with one 8-byte load; pgd_step* refuse any other pointer with PGD_ERR_ARG: a view that starts at an odd float of its buffer)."""
        if not (actions.is_cuda and actions.dtype == self.torch.float32 and actions.is_contiguous() and actions.numel() == self.N * self.A * 2 and
                actions.data_ptr() % 8 == 0):  # (by hand on the per-step path; _dev words the refusal)
            _dev(actions, self.torch.float32, self.N * self.A * 2, where, name, None, True, 8)

    def _obs_rows(self, o, rows, width, where, name="obs"):
        """Observation rows as a kernel reads them: the 2-D view [rows, >= width] of `o` (rows None: as many as it has), float32 cuda with
        unit column stride; the row stride is free -> the view, its row stride."""
        o2 = o.view(-1, o.shape[-1])
        if not (o2.is_cuda and o2.dtype == self.torch.float32 and o2.stride(1) == 1 and (rows is None or o2.shape[0] == rows) and
                o2.shape[1] >= width):
            raise PgdArgError("%s: %s: float32 cuda rows [%s, >= %d] with unit column stride wanted, got %s%s %s with strides %s" % (
                where, name, "any" if rows is None else rows, width, "" if o2.is_cuda else "cpu ", o2.dtype, tuple(o2.shape), o2.stride()))
        return o2, int(o2.stride(0))

    def _scratch(self, work, need, device, where):
        """A call's scratch: `work` as the caller gave it (any dtype; the library refuses one that is too small), or `need` new bytes -> the
        tensor, its byte count."""
        work = _dev(self.torch.empty(((need + 7) // 8, ), dtype=self.torch.float64, device=device) if work is None else work, None, None, where,
                    "work")
        return work, work.numel() * work.element_size()

    # -- reference surface ------------------------------------------------------------------------------------------
    def reset(self, scen_ids, env_ids=None, out=None):
        """Restart the envs `env_ids` (None: all N, in order) with the scenarios `scen_ids` and write their first rows into `out`
        (default: the engine's own observation buffer, which is returned).  With an id list only the rows of the listed envs are
        written: every other row of the buffer keeps its bytes, e.g. the terminal rows the last step left there."""
        scen_ids = np.ascontiguousarray(scen_ids, dtype=np.int32).reshape(-1)
        env_ids = None if env_ids is None else np.ascontiguousarray(env_ids, dtype=np.int32).reshape(-1)
        if env_ids is not None and len(env_ids) != len(scen_ids):  # (the library reads len(scen_ids) entries of both)
            raise ValueError("reset: %d env ids for %d scenario ids" % (len(env_ids), len(scen_ids)))
        obs = self.obs if out is None else _dev(out, self.torch.float32, self.obs.numel(), "reset", "out")
        self.torch.cuda.synchronize(self.device)
        if obs is not self.obs and self._unseen_rows(obs):
            _chk(self.L.pgd_forget_rows(self.h), "pgd_forget_rows")
        _chk(self.L.pgd_reset(self.h, _np_p(env_ids), _np_p(scen_ids), len(scen_ids), _p(obs)), "pgd_reset")
        self.sync()
        return obs

    def _unseen_rows(self, obs):
        """Is `obs` a caller's observation tensor this multi-agent engine has not seen alive (see step)?  It is kept alive from now on."""
        if self.A > 1 and not any(t is obs for t in self._seen_out):
            self._seen_out.append(obs)
            del self._seen_out[:-4]
            return True
        return False

    def make_outputs(self):
        """A second set of output buffers (double buffering of the per-step gather, pgdrive_amd/dist.py)."""
        t, dev = self.torch, self.device
        return (t.zeros((self.N, self.A, self.D), dtype=t.float32, device=dev),
                t.zeros((self.N, self.A), dtype=t.float32, device=dev),
                t.zeros((self.N, self.A), dtype=t.uint8, device=dev),
                t.zeros((self.N, self.A), dtype=t.int32, device=dev))

    def step(self, actions, want_obs=True, out=None):
        """actions: float32 cuda tensor [N, A, 2] (contiguous). Asynchronous on the engine stream.
        `out` = (obs, reward, done, flags) tensors to write instead of the engine's own buffers.
        The returned obs IS the engine's buffer (or `out[0]`), not a copy.  Multi-agent engines zero the row of a seat that is not
        due ONCE and remember it per buffer (include/pgdrive_hip.h, pgd_step): a caller that edits the returned rows in place
        (normalisation, clamp_, noise) would see its edits persist in the rows of empty seats -- clone first, or create the engine
        with PGD_NO_ROWZ=1 in the environment (the zero rows are then rewritten by every call).  `out` tensors need not be long-lived
        or zero-initialised: a tensor the engine has not seen alive makes it forget its marks (pgd_forget_rows) before the step."""
        self._check_actions(actions)
        if out is None:  # the engine's own output buffers: their addresses never change
            obs, rew, done, flags = self.obs, self.reward, self.done, self.flags
            p_obs, p_rew, p_done, p_flags = self._own_ptrs
        else:
            (obs, rew, done, flags), t, n = out, self.torch, self.N * self.A
            if not (rew.is_cuda and done.is_cuda and flags.is_cuda and rew.dtype == t.float32 and done.dtype == t.uint8 and flags.dtype == t.int32 and
                    rew.numel() == done.numel() == flags.numel() == n and rew.is_contiguous() and done.is_contiguous() and flags.is_contiguous() and
                    (not want_obs or (obs.is_cuda and obs.dtype == t.float32 and obs.numel() == n * self.D and obs.is_contiguous()))):
                [_dev(x, dt, size, "step", "out[%d]" % k) for k, (x, dt, size) in enumerate(  # (by hand above, as _check_actions; _dev words it)
                    ((obs, t.float32, n * self.D), (rew, t.float32, n), (done, t.uint8, n), (flags, t.int32, n))) if k or want_obs]
            p_obs, p_rew, p_done, p_flags = _p(obs), _p(rew), _p(done), _p(flags)
        # The zero-row marks of a multi-agent engine name a buffer by its address: a NEW tensor may sit where a freed one sat
        # (torch's caching allocator; `out=torch.empty(...)` per step) and would inherit "known zero" marks for rows that hold
        # anything.  Tensors seen before are kept alive here (their memory cannot be handed out again); any other tensor makes
        # the engine forget its marks first.  The test is by IDENTITY of the tensor object, not by address, and the
        # rollout collectors rely on that: they pass a fresh view (`obs[t + 1]`) per step, whose address recurs in every rollout
        # while another row was written in between -- keyed by data_ptr, stale marks would get through.
        forget_first = out is not None and want_obs and self._unseen_rows(obs)
        self._follow_stream()
        if forget_first:
            _chk(self.L.pgd_forget_rows(self.h), "pgd_forget_rows")
        _chk(self.L.pgd_step(self.h, _p(actions), p_obs if want_obs else None, p_rew, p_done, p_flags), "pgd_step")
        return obs, rew, done, flags

    def step_packed(self, actions, rows):
        """Like step(), but the env's results go into `rows` [N, >= A*(D+2)] fp32 as [A*D obs | A reward | A done]: the
        row a per-step gather sends (pgdrive_amd/dist.py); `rows` may be a slice of the gather's receive buffer.  The zero-row marks
        of a multi-agent engine name `rows` by address and stride: as for step(out=...), a tensor the engine has not seen alive makes
        it forget its marks first (by identity of the tensor object: pass the same view while its rows are to be trusted)."""
        self._check_actions(actions, "step_packed")
        _dev(rows, self.torch.float32, None, "step_packed", "rows", None, False)
        _need(rows.dim() == 2 and rows.shape[0] == self.N and rows.stride(1) == 1 and rows.stride(0) >= self.A * (self.D + 2), "step_packed",
              "rows: [N, >= A * (D + 2)] with unit column stride wanted")
        forget_first = self._unseen_rows(rows)
        self._follow_stream()
        if forget_first:
            _chk(self.L.pgd_forget_rows(self.h), "pgd_forget_rows")
        p_obs, p_rew, p_done, p_flags = self._own_ptrs
        _chk(self.L.pgd_step_packed(self.h, _p(actions), _p(rows), int(rows.stride(0)), p_rew, p_done, p_flags), "pgd_step_packed")
        return rows, self.reward, self.done, self.flags

    def step_n(self, action_ring, first, n_steps, want_obs=True):
        """n_steps steps of `action_ring` [L, N, A, 2] (step k applies ring[(first + k) % L]) in one call (pgd_step_n): returns
        (obs after the last step or None, reward [n_steps, N, A], done, flags); the intermediate steps skip the observation."""
        t = self.torch
        _dev(action_ring, t.float32, None, "step_n", "action_ring", None, True, 8)  # (alignment: see _check_actions)
        _need(action_ring.dim() == 4 and tuple(action_ring.shape[1:]) == (self.N, self.A, 2), "step_n", "action_ring: [L, N, A, 2] wanted")
        self._follow_stream()
        rew = t.empty((n_steps, self.N, self.A), dtype=t.float32, device=self.obs.device)
        done = t.empty((n_steps, self.N, self.A), dtype=t.uint8, device=self.obs.device)
        flags = t.empty((n_steps, self.N, self.A), dtype=t.int32, device=self.obs.device)
        p_obs = self._own_ptrs[0] if want_obs else None
        _chk(self.L.pgd_step_n(self.h, _p(action_ring), int(action_ring.shape[0]), int(first), int(n_steps), p_obs, _p(rew), _p(done),
                               _p(flags)), "pgd_step_n")
        return (self.obs if want_obs else None), rew, done, flags

    def mlp_prepare(self, weights):
        """The policy network's weights in the split-bf16 kernel's own layout (pgd_mlp_prepare): call once per policy update, hand the
        returned buffer to mlp_policy(prepared=...).  `weights` as for mlp_policy."""
        t = self.torch
        k = int(weights[0].shape[0])
        self._network(weights, k, 2, "mlp_prepare")
        buf = t.empty(int(self.L.pgd_mlp_prepared_bytes(k)), dtype=t.uint8, device=self.device)
        self._follow_stream()
        _chk(self.L.pgd_mlp_prepare(self.h, k, 256, *map(_p, weights), int(weights[4].shape[1]), _p(buf)), "pgd_mlp_prepare")
        buf._pgd_in_dim = k
        return buf

    def specialise(self, wait=True, verbose=False):
        """Build (hipcc, cached) and load a step kernel with THIS engine's configuration compiled in (pgdrive_amd/jit.py):
        configurations the library has no instantiation for then step as fast as the reference's defaults.  wait=False: in a
        background thread, the general kernel steps meanwhile."""
        from . import jit
        return jit.specialise(self, wait=wait, verbose=verbose)

    def describe_step(self):
        """Which step kernel the last step call launched (pgd_describe_step)."""
        buf = C.create_string_buffer(512)
        _chk(self.L.pgd_describe_step(self.h, buf, 512), "pgd_describe_step")
        return buf.value.decode()

    def lane_keep_actions(self, out, tick, obs=None, k_lat=1.0, k_head=2.0, v_target_kmh=30.0, noise=0.05):
        """Scripted lane-keeping actions for the ego from the last observation (pgd_lane_keep_actions): an action stream that
        keeps the ego driving (bench.py --actions expert).  `out` = float32 cuda tensor [N, 1, 2]."""
        _dev(out, self.torch.float32, self.N * 2, "lane_keep_actions", "out")
        o = self.obs if obs is None else _dev(obs, self.torch.float32, None, "lane_keep_actions", "obs", self.N * self.D)
        self._follow_stream()
        _chk(self.L.pgd_lane_keep_actions(self.h, _p(o), _p(out), k_lat, k_head, v_target_kmh, noise, int(tick) & 0xffffffff),
             "pgd_lane_keep_actions")
        return out

    def mlp_policy(self, weights, out, obs=None, group=-1, final_tanh=False, in_dim=None, prepared=None):
        """actions = tanh-MLP(observation rows) in one launch (pgd_mlp_policy; the network of examples/ppo_expert/numpy_expert.py).
        `weights` = (w1 [in, 256], b1, w2 [256, 256], b2, w3 [256, >= 2], b3): contiguous float32 cuda tensors, row-major [in][out].
        `obs`: [rows, stride] float32 cuda (default: the engine's own observation buffer); `out`: float32 cuda [N, A, 2].
        group >= 0: only the rows of that env group, on the group's stream (then `obs` / `out` are still the FULL buffers)."""
        prep = prepared is not None  # split-bf16 kernel on weights prepared by mlp_prepare (`weights` is then ignored)
        k = int(in_dim if in_dim is not None else prepared._pgd_in_dim if prep else weights[0].shape[0])
        o2, stride = self._obs_rows(self.obs if obs is None else obs, self.N * self.A, 0 if prep else k, "mlp_policy")
        self._check_actions(out, "mlp_policy", "out")
        if prep:
            _dev(prepared, self.torch.uint8, None, "mlp_policy", "prepared", int(self.L.pgd_mlp_prepared_bytes(k)))
        else:
            self._network(weights, k, 2, "mlp_policy")
        if group < 0:
            self._follow_stream()
        if prep:
            _chk(self.L.pgd_mlp_policy_prepared(self.h, int(group), _p(o2), stride, k, _p(prepared), int(bool(final_tanh)), _p(out)),
                 "pgd_mlp_policy_prepared")
        else:
            _chk(self.L.pgd_mlp_policy(self.h, int(group), _p(o2), stride, k, 256, *map(_p, weights), int(weights[4].shape[1]),
                                       int(bool(final_tanh)), _p(out)), "pgd_mlp_policy")
        return out

    def _network(self, weights, k, heads, where, name="weights", cols=None):
        """The six tensors of one network checked (float32 cuda, contiguous, [k, 256] / [256, 256] / [256, >= heads], or [256, cols], and
        the biases of their lengths) -> their pointers."""
        w1, b1, w2, b2, w3, b3 = weights
        if not (w3.dim() == 2 and w3.shape[0] == 256 and (w3.shape[1] >= heads if cols is None else w3.shape[1] == cols) and
                w1.shape == (k, 256) and w2.shape == (256, 256)):
            raise PgdArgError("%s: %s: w1 [%d, 256], w2 [256, 256], w3 [256, %s] wanted" % (where, name, k, cols or ">= %d" % heads))
        cols, f32 = int(w3.shape[1]), self.torch.float32
        for w in weights:  # (by hand on the per-step path, as _check_actions; _dev words the refusal below)
            if not (w.is_cuda and w.dtype == f32 and w.is_contiguous()):
                break
        else:
            if b1.numel() == 256 and b2.numel() == 256 and b3.numel() == cols:
                return [w.data_ptr() for w in weights]
        for w, n, part in zip(weights, (k * 256, 256, 65536, 256, 256 * cols, cols), _SIX):
            _dev(w, f32, n, where, name + part)

    def _nets(self, st, policy, value, k, where, name="policy_weights", vname="value_weights"):
        """`st` (ActorCritic of weights, PPOGrads of gradient buffers) with the checked pointers of the policy's six tensors and, unless
        `value` is None, of the critic's."""
        st.w1, st.b1, st.w2, st.b2, st.w3, st.b3 = self._network(policy, k, 4, where, name)
        if value is not None:
            st.vw1, st.vb1, st.vw2, st.vb2, st.vw3, st.vb3 = self._network(value, k, 1, where, vname, 1)
        return st

    def _value_net(self, st, weights, k, where, name):
        """`st` (ValueNet, ValueGrads) with the checked pointers of a critic-shaped network's six tensors."""
        st.w1, st.b1, st.w2, st.b2, st.w3, st.b3 = self._network(weights, k, 1, where, name, 1)
        return st

    def _ac_call(self, where, policy_weights, value_weights, cost_weights, out, per_row, seed, tick, obs, group, deterministic, in_dim, row_list=(),
                 cat=None):
        """The mlp_actor_critic* call pgd_<where>: what they share, checked -- the observation rows, `out`, the `per_row` outputs (logp,
        value, cost_value), the networks (value_weights and cost_weights None: none) --, then the launch on the caller's stream (group < 0);
        `row_list`: the two pointers of mlp_actor_critic_rows' list; `cat`: (bins, action_index, emit_index) of the categorical calls."""
        rows = self.N * self.A
        k = int(in_dim if in_dim is not None else policy_weights[0].shape[0])
        o2, stride = self._obs_rows(self.obs if obs is None else obs, rows, k, where)
        self._check_actions(out, where, "out")
        f32, fn = self.torch.float32, "pgd_" + where
        if cost_weights is not None and value_weights is None:
            raise PgdArgError(where + ": the cost critic comes with a critic")
        for i, v in enumerate(per_row[:3 if value_weights is not None else 1]):  # (no critic: logp alone; by hand, as _check_actions)
            if not (v.is_cuda and v.dtype == f32 and v.is_contiguous() and v.numel() == rows):
                _dev(v, f32, rows, where, ("logp", "value", "cost_value")[i])
        nets = self._nets(_abi.ActorCritic(), policy_weights, value_weights, k, where)
        nets.out_cols = int(policy_weights[4].shape[1])
        cnet = () if cost_weights is None else (C.byref(self._value_net(_abi.ValueNet(), cost_weights, k, where, "cost_weights")), )
        bins, index, mode = (), (), _abi.AC_DETERMINISTIC if deterministic else 0
        if cat is not None:
            bins = _abi.cat_bins(cat[0], where)
            _need(nets.out_cols >= sum(bins), where, "policy_weights: w3 [256, >= %d] wanted for bins %r" % (sum(bins), bins))
            index = (_p(_dev(cat[1], self.torch.int32, 2 * rows, where, "action_index")), )
            mode |= _abi.AC_EMIT_INDEX if cat[2] else 0
        if group < 0:
            self._follow_stream()
        per_row = per_row if value_weights is not None else (per_row[0], None)  # (no critic: a null pointer for `value`)
        _chk(getattr(self.L, fn)(self.h, int(group), _p(o2), stride, k, C.byref(nets), *cnet, *bins, int(seed) & 0xffffffff, int(tick) & 0xffffffff,
                                 mode, *row_list, _p(out), *index, *map(_p, per_row)), fn)

    def _rollout_buffers(self, where, table):
        """The tensors of a rollout call checked: `table` rows are (name, tensor, dtype, extra); the first is the lead, [T, rows...]; extra
        0: T * rows entries, 1: (T + 1) * rows, None: rows; a tensor that is None is allocated (of lead's shape, or [rows]).  Follows the
        caller's stream.  -> T, rows, the tensors."""
        lead = table[0][1]
        T = int(lead.shape[0])
        rows = lead.numel() // max(T, 1)
        out = []
        for name, v, dt, extra in table:
            if v is None:
                v = self.torch.empty(lead.shape if extra == 0 else (rows, ), dtype=dt, device=lead.device)
            out.append(_dev(v, dt, rows if extra is None else (T + extra) * rows, where, name))
        self._follow_stream()
        return T, rows, out

    def mlp_actor_critic(self, policy_weights, value_weights, out, logp, value, seed, tick, obs=None, group=-1, deterministic=False,
                         in_dim=None):
        """A sampled action, its log-probability and the value estimate of every observation row in one launch (pgd_mlp_actor_critic).
        `policy_weights` = (w1 [in, 256], b1, w2 [256, 256], b2, w3 [256, >= 4], b3): the head's columns are mean0, mean1, log_std0,
        log_std1; `value_weights` the same shapes with a head of one column, or None (no critic: `value` is not written and may be None).
        `out` [N, A, 2] (unclipped: step clips), `logp` and `value` [N, A]: float32 cuda.  The noise is a function of (seed, global row,
        tick); `tick` is added to the device counter of actor_critic_tick, if one is set.  deterministic: the action is the mean.
        `obs`, `group`, `in_dim` as for mlp_policy."""
        self._ac_call("mlp_actor_critic", policy_weights, value_weights, None, out, (logp, value), seed, tick, obs, group, deterministic, in_dim)
        return out, logp, value

    def guardian(self, expert_weights, save_level, actions, state, applied, info, seed, tick, prev_flags=None, trace=None, obs=None, group=-1,
                 deterministic=False, immediate=False):
        """The expert guardian in one launch (pgd_guardian; the reference's use_saver / save_level, policy/AI_protect_policy.py), single-agent
        engines: the expert `expert_weights` -- six policy tensors as for mlp_actor_critic, w1 with D rows, or with D + 1 rows for the
        reference's shipped weights (the lateral float is then built by the kernel) -- is evaluated on the observation rows and replaces
        the agent's `actions` [N, 1, 2] where the rule says so.  `state` [N] uint8, in / out: vehicle.takeover; `prev_flags` [N, 1] int32:
        the flags of the previous step, or None; `applied` [N, 1, 2]: what the step is to read (may be `actions` itself); `info` [N] uint8:
        bit 0 takeover, 1 takeover_start, 2 takeover_end; `trace` [N, 4] or None: expert steering, throttle, lateral float, f.  The expert
        samples with (seed, global row, tick + the device counter of actor_critic_tick) unless `deterministic`; `immediate` (not a
        reference behaviour) applies a correction in the step that raises it.  A bound observation normalisation is ignored."""
        t = self.torch
        _need(self.A == 1, "guardian", "the guardian serves single-agent engines")
        o2, stride = self._obs_rows(self.obs if obs is None else obs, self.N, self.D, "guardian")
        self._check_actions(actions, "guardian")
        self._check_actions(applied, "guardian", "applied")
        _dev(state, t.uint8, self.N, "guardian", "state")
        _dev(info, t.uint8, self.N, "guardian", "info")
        _opt(prev_flags, t.int32, self.N, "guardian", "prev_flags")
        _opt(trace, t.float32, 4 * self.N, "guardian", "trace")
        k = int(expert_weights[0].shape[0])
        if k not in (self.D, self.D + 1):
            raise PgdArgError("guardian: the expert takes %d inputs (or %d with the lateral float), not %d" % (self.D, self.D + 1, k))
        nets = self._nets(_abi.ActorCritic(), expert_weights, None, k, "guardian", "expert_weights")
        nets.out_cols = int(expert_weights[4].shape[1])
        mode = (_abi.GUARD_LEGACY_LATERAL if k == self.D + 1 else 0) | (_abi.GUARD_DETERMINISTIC if deterministic else 0) | \
            (_abi.GUARD_IMMEDIATE if immediate else 0)
        cfg = _abi.GuardianConfig(k, float(save_level), int(seed) & 0xffffffff, int(tick) & 0xffffffff, mode)
        if group < 0:
            self._follow_stream()
        _chk(self.L.pgd_guardian(self.h, int(group), _p(o2), stride, C.byref(nets), C.byref(cfg), _p(actions), _p(prev_flags), _p(state),
                                 _p(applied), _p(info), _p(trace)), "pgd_guardian")
        return applied, info

    def actor_critic_tick(self, counter):
        """Give the engine a tick counter in device memory (pgd_actor_critic_tick): a cuda int32 tensor of one element that every later
        mlp_actor_critic launch adds to its `tick` (modulo 2^32) when it RUNS -- what lets a captured rollout draw new noise at every
        replay.  None: back to the argument alone.  The engine keeps the tensor alive."""
        _opt(counter, self.torch.int32, 1, "actor_critic_tick", "counter", None, False)
        _chk(self.L.pgd_actor_critic_tick(self.h, _p(counter)), "pgd_actor_critic_tick")
        self._ac_tick = counter

    def gae(self, reward, value, done, gamma, lam, adv=None, ret=None):
        """Advantages and returns of a rollout (pgd_gae): reward, done (uint8) [T, rows...], value [T + 1, rows...] (the last row is the
        bootstrap), time-major contiguous cuda tensors; a done cuts the episode.  Returns (adv, ret), float32 of reward's shape (`adv`,
        `ret`: buffers to write).  Asynchronous on the caller's current stream."""
        return self._gae("gae", reward, value, done, (), gamma, lam, adv, ret)

    def _gae(self, fn, reward, value, done, term, gamma, lam, adv, ret):
        """gae and gae_bootstrap (`term`: its table row for term_value, or none)."""
        t = self.torch
        T, rows, (*ins, adv, ret) = self._rollout_buffers(fn, (("reward", reward, t.float32, 0), ("value", value, t.float32, 1),
                                                                ("done", done, t.uint8, 0), *term, ("adv", adv, t.float32, 0),
                                                                ("ret", ret, t.float32, 0)))
        _chk(getattr(self.L, "pgd_" + fn)(self.h, *map(_p, ins), T, rows, float(gamma), float(lam), _p(adv), _p(ret)), "pgd_" + fn)
        return adv, ret

    # -- rollouts of multi-agent engines (include/pgdrive_hip.h states the predicates acted / cont / live) -------------------------
    def live_rows(self, flags, done, rows=None, count=None, group=-1):
        """The seat rows that hold an observation an agent will act on, from the flags and dones of the step that wrote it
        (pgd_live_rows): `rows` int32 [N * A] receives their ascending row numbers env * A + seat, `count` int32 [1] their number
        (both cuda; allocated when None).  Entries at and beyond the count are not written.  group >= 0: the rows of that env group, on
        the group's stream (`flags` / `done` are still the full [N, A] tensors).  Three small launches; nothing waits for the device."""
        t = self.torch
        n = self.N * self.A
        rows = t.empty((n, ), dtype=t.int32, device=self.device) if rows is None else rows
        count = t.zeros((1, ), dtype=t.int32, device=self.device) if count is None else count
        _dev(flags, t.int32, n, "live_rows", "flags")
        _dev(done, t.uint8, n, "live_rows", "done")
        lp, cp = self._list_args(rows, count, self._group_rows(group), "live_rows", "rows")
        if group < 0:
            self._follow_stream()
        _chk(self.L.pgd_live_rows(self.h, int(group), _p(flags), _p(done), lp, cp), "pgd_live_rows")
        return rows, count

    def _group_rows(self, group):
        """How many seat rows a call on `group` (< 0: the whole engine) covers: what its row list has to hold."""
        n = self.N * self.A
        return n if group < 0 else n // max(1, int(self.n_groups or 1))

    def rollout_index(self, flags, index=None, count=None):
        """The entries t * rows + r of a time-major flag tensor [T, rows...] at which an agent acted (PGD_F_REPORT), ascending, into
        `index` int32 [T * rows], their number into `count` int32 [1] (pgd_rollout_index): a trainer draws minibatches from
        index[:count].  The first call of a shape allocates scratch and cannot be captured in a graph: call it once before."""
        t = self.torch
        T = int(flags.shape[0])
        rows = flags.numel() // max(T, 1)
        index = t.empty((T * rows, ), dtype=t.int32, device=self.device) if index is None else index
        count = t.zeros((1, ), dtype=t.int32, device=self.device) if count is None else count
        _dev(flags, t.int32, None, "rollout_index", "flags")
        ip, cp = self._list_args(index, count, T * rows, "rollout_index")
        self._follow_stream()
        _chk(self.L.pgd_rollout_index(self.h, _p(flags), T, rows, ip, cp), "pgd_rollout_index")
        return index, count

    def mlp_actor_critic_rows(self, policy_weights, value_weights, rows, count, out, logp, value, seed, tick, obs=None, group=-1,
                              deterministic=False, in_dim=None):
        """mlp_actor_critic over the rows of a list (pgd_mlp_actor_critic_rows): `rows` / `count` as live_rows returns them.  A listed
        row gets bit for bit what mlp_actor_critic gives it; every other row of the range gets action 0, 0, logp 0, value 0 (written by
        this call) and its observation is never used (it may hold NaN).  The other arguments as for mlp_actor_critic."""
        _need(rows is not None and count is not None, "mlp_actor_critic_rows", "rows and count wanted")
        row_list = self._list_args(rows, count, self._group_rows(group), "mlp_actor_critic_rows", "rows")
        self._ac_call("mlp_actor_critic_rows", policy_weights, value_weights, None, out, (logp, value), seed, tick, obs, group, deterministic,
                      in_dim, row_list)
        return out, logp, value

    # -- the categorical head (include/pgdrive_hip.h states the formulas) -------------------------------------------------------------
    def mlp_actor_critic_cat(self, policy_weights, value_weights, bins, out, action_index, logp, value, seed, tick, obs=None, group=-1,
                             deterministic=False, emit_index=False, in_dim=None):
        """mlp_actor_critic with the categorical head (pgd_mlp_actor_critic_cat): `bins` = (ks, kt), 2 <= each, ks + kt <= 16; the policy's
        w3 is [256, >= ks + kt] -- columns 0 .. ks - 1 the steering logits, ks .. ks + kt - 1 the throttle logits.  `action_index` int32
        cuda [N, A, 2] receives the sampled indices, `logp` their log-probability, `value` the critic's output (mlp_actor_critic's bits);
        `out` [N, A, 2] what the step reads: the grid value i * (2 / (K_head - 1)) - 1 for an engine with continuous actions, or, with
        emit_index, the index as a float for an engine with discrete_action.  The draws are mlp_actor_critic's (seed, global row, tick +
        the device counter).  deterministic: the argmax.  The other arguments as for mlp_actor_critic."""
        self._ac_call("mlp_actor_critic_cat", policy_weights, value_weights, None, out, (logp, value), seed, tick, obs, group, deterministic, in_dim,
                      cat=(bins, action_index, emit_index))
        return out, action_index, logp, value

    def mlp_actor_critic_cat_rows(self, policy_weights, value_weights, bins, rows, count, out, action_index, logp, value, seed, tick, obs=None,
                                  group=-1, deterministic=False, emit_index=False, in_dim=None):
        """mlp_actor_critic_cat over the rows of a list (pgd_mlp_actor_critic_cat_rows): `rows` / `count` as live_rows returns them.  A
        listed row gets bit for bit what mlp_actor_critic_cat gives it; every other row of the range gets action 0, 0, index 0, 0, logp 0,
        value 0 and its observation is never used."""
        _need(rows is not None and count is not None, "mlp_actor_critic_cat_rows", "rows and count wanted")
        row_list = self._list_args(rows, count, self._group_rows(group), "mlp_actor_critic_cat_rows", "rows")
        self._ac_call("mlp_actor_critic_cat_rows", policy_weights, value_weights, None, out, (logp, value), seed, tick, obs, group, deterministic,
                      in_dim, row_list, cat=(bins, action_index, emit_index))
        return out, action_index, logp, value

    def ppo_cat_work_bytes(self, in_dim, rows, has_critic=True):
        """The scratch pgd_ppo_grad_cat needs for minibatches of up to `rows` positions (pgd_ppo_cat_work_bytes); 0: the call would refuse
        them."""
        return int(self.L.pgd_ppo_cat_work_bytes(int(in_dim), int(rows), int(bool(has_critic))))

    def ppo_grad_cat(self, policy_weights, value_weights, policy_grads, value_grads, bins, obs, action_index, logp_old, adv, ret, stats, work,
                     start=0, stride=1, rows=None, index=None, count=None, n_list=None, adv_stats=None, clip=0.2, vf_coef=0.5, ent_coef=0.0,
                     in_dim=None):
        """ppo_grad with the categorical head (pgd_ppo_grad_cat): `bins` as for mlp_actor_critic_cat, `action_index` int32 cuda [..., 2] the
        rollout's sampled indices in place of `actions`; `work` of at least ppo_cat_work_bytes(in_dim, rows) bytes.  Every other argument,
        `stats` and the minibatch rule as for ppo_grad."""
        nets, _, b, grads, _ = self._ppo_batch("ppo_grad_cat", (policy_weights, value_weights, None), (policy_grads, value_grads, None), obs, None,
                                               logp_old, adv, ret, None, stats, work, start, stride, rows, index, count, n_list, adv_stats, in_dim,
                                               cat=(bins, action_index))
        ks, kt = _abi.cat_bins(bins, "ppo_grad_cat")
        hp = _abi.PPOHyper(float(clip), float(vf_coef), float(ent_coef))
        _chk(self.L.pgd_ppo_grad_cat(self.h, C.byref(nets), C.byref(b), C.byref(hp), C.byref(grads), ks, kt, _p(action_index), _p(stats), _p(work),
                                     work.numel() * work.element_size()), "pgd_ppo_grad_cat")
        return stats

    def gae_masked(self, reward, value, done, flags, gamma, lam, adv=None, ret=None, mask=None):
        """Advantages and returns of a multi-agent rollout (pgd_gae_masked): as gae(), with the step flags [T, rows...] (int32) deciding
        where an agent acted and whether it continues; rows that did not act get adv = ret = 0 whatever their reward and value hold.
        Returns (adv, ret, mask): mask uint8 of reward's shape, 1 where an agent acted."""
        t = self.torch
        T, rows, (reward, value, done, flags, adv, ret, mask) = self._rollout_buffers(
            "gae_masked", (("reward", reward, t.float32, 0), ("value", value, t.float32, 1), ("done", done, t.uint8, 0), ("flags", flags, t.int32, 0),
                           ("adv", adv, t.float32, 0), ("ret", ret, t.float32, 0), ("mask", mask, t.uint8, 0)))
        _chk(self.L.pgd_gae_masked(self.h, _p(reward), _p(value), _p(done), _p(flags), T, rows, float(gamma), float(lam), _p(adv), _p(ret),
                                   _p(mask)), "pgd_gae_masked")
        return adv, ret, mask

    # -- the PPO update behind a rollout (include/pgdrive_hip.h states the formulas) ---------------------------------------------
    def ppo_work_bytes(self, in_dim, rows, has_critic=True):
        """The scratch pgd_ppo_grad needs for minibatches of up to `rows` positions (pgd_ppo_work_bytes); 0: the call would refuse them."""
        return int(self.L.pgd_ppo_work_bytes(int(in_dim), int(rows), int(bool(has_critic))))

    def _list_args(self, index, count, n_list, where, name="index"):
        """A row list checked: `index` int32 cuda [>= n_list] or None, `count` int32 cuda [1] or None -> their pointers."""
        i32 = self.torch.int32
        return _p(_opt(index, i32, None, where, name, n_list)), _p(_opt(count, i32, 1, where, "count", None, False))

    def adv_stats(self, adv, out=None, index=None, count=None, n_list=None):
        """Population mean and 1 / (std + 1e-8) of the advantages over a row list (pgd_adv_stats) -> `out`, float32 cuda [2].  The list:
        adv.view(-1)[index[q]] for q < count (`index` None: entry q itself; `count` None: n_list; n_list None: every entry of `adv`, or of
        `index`); `count` is read on the device.  No entries: (0, 1)."""
        t = self.torch
        n_list = int((index if index is not None else adv).numel() if n_list is None else n_list)
        _need(0 <= n_list, "adv_stats", "n_list >= 0 wanted")
        _dev(adv, t.float32, None, "adv_stats", "adv", None if index is not None else n_list)
        out = _dev(t.empty((2, ), dtype=t.float32, device=self.device) if out is None else out, t.float32, 2, "adv_stats", "out")
        ip, cp = self._list_args(index, count, n_list, "adv_stats")
        self._follow_stream()
        _chk(self.L.pgd_adv_stats(self.h, _p(adv), ip, cp, n_list, _p(out)), "pgd_adv_stats")
        return out

    def ppo_grad(self, policy_weights, value_weights, policy_grads, value_grads, obs, actions, logp_old, adv, ret, stats, work, start=0, stride=1,
                 rows=None, index=None, count=None, n_list=None, adv_stats=None, clip=0.2, vf_coef=0.5, ent_coef=0.0, in_dim=None):
        """Loss statistics and the gradient of every weight for one minibatch (pgd_ppo_grad).  `obs` [..., D], `actions` [..., 2],
        `logp_old`, `adv`, `ret` [...]: the rollout's tensors, float32 cuda, flattened to rows.  The minibatch: list positions start + i
        stride, i < rows, live below `count` (int32 cuda [1], read on the device; None: n_list; n_list None: every row, or every entry
        of `index`); position q is row index[q] (`index` None: q).  `adv_stats`: the two floats of adv_stats(), or None.  Gradients are
        written into `policy_grads` / `value_grads`, tuples of the weights' shapes (value_weights None: no critic, value_grads ignored);
        `stats` float32 cuda [8] (_abi.PPO_STATS); `work` a cuda tensor of at least ppo_work_bytes(in_dim, rows) bytes.  Asynchronous."""
        nets, _, b, grads, _ = self._ppo_batch("ppo_grad", (policy_weights, value_weights, None), (policy_grads, value_grads, None), obs, actions,
                                               logp_old, adv, ret, None, stats, work, start, stride, rows, index, count, n_list, adv_stats, in_dim)
        hp = _abi.PPOHyper(float(clip), float(vf_coef), float(ent_coef))
        _chk(self.L.pgd_ppo_grad(self.h, C.byref(nets), C.byref(b), C.byref(hp), C.byref(grads), _p(stats), _p(work),
                                 work.numel() * work.element_size()), "pgd_ppo_grad")
        return stats

    def _ppo_batch(self, where, weights, grad_bufs, obs, actions, logp_old, adv, ret, cost_ret, stats, work, start, stride, rows, index, count,
                   n_list, adv_stats, in_dim, cat=None, n_stats=8):
        """What ppo_grad, ppo_grad_cost, ppo_grad_cat and ppo_grad_guided (`n_stats` 12) share, checked: the rollout's tensors, the minibatch, `stats`, `work`, and the networks
        with their gradient buffers -- `weights` and `grad_bufs` are (policy, value or None, cost or None) -> ActorCritic, ValueNet (or None),
        PPOBatch, PPOGrads, ValueGrads (or None).  `cat`: (bins, action_index) of ppo_grad_cat, which reads no `actions`.  Follows the
        caller's stream."""
        t = self.torch
        (pw, vw, cw), (pg, vg, cg) = weights, grad_bufs
        _need(cw is None or vw is not None, where, "the cost critic comes with a critic")
        k = int(in_dim if in_dim is not None else pw[0].shape[0])
        o2, obs_stride = self._obs_rows(obs, None, k, where)
        n_rows = int(o2.shape[0])
        if cat is None:
            _dev(actions, t.float32, 2 * n_rows, where, "actions")
        else:
            _dev(cat[1], t.int32, 2 * n_rows, where, "action_index")
            _need(int(pw[4].shape[1]) >= sum(_abi.cat_bins(cat[0], where)), where, "policy_weights: w3 [256, >= %d] wanted for bins %r" %
                  (sum(cat[0]), cat[0]))
        by_row = (("logp_old", logp_old), ("adv", adv), ("ret", ret), ("cost_ret", cost_ret))
        for name, v in by_row[:2 + (vw is not None) + (cw is not None)]:
            _dev(v, t.float32, n_rows, where, name)
        n_list = int((index.numel() if index is not None else n_rows) if n_list is None else n_list)
        _need(0 <= n_list and (index is not None or n_list <= n_rows), where, "0 <= n_list <= the rows of obs wanted")
        rows = int(max(1, -(-(n_list - int(start)) // int(stride))) if rows is None else rows)
        _need(int(start) >= 0 and int(stride) >= 1 and 1 <= rows <= _abi.PPO_ROWS_MAX, where, "start >= 0, stride >= 1, rows <= PPO_ROWS_MAX wanted")
        _dev(stats, t.float32, n_stats, where, "stats")
        need = self.ppo_cost_work_bytes(k, rows) if cw is not None else (self.ppo_work_bytes if cat is None else self.ppo_cat_work_bytes)(
            k, rows, vw is not None)
        _dev(work, None, None, where, "work", None, True, 16)
        _need(0 < need <= work.numel() * work.element_size(), where, "work: at least %d bytes wanted (0: rows or in_dim out of range)" % need)
        _opt(adv_stats, t.float32, 2, where, "adv_stats")
        nets = self._nets(_abi.ActorCritic(), pw, vw, k, where)
        nets.out_cols = int(pw[4].shape[1])
        grads = self._nets(_abi.PPOGrads(), pg, None if vw is None else vg, k, where, "policy_grads", "value_grads")
        _need(all(g.shape == w.shape for g, w in zip(pg, pw)), where, "policy_grads of the weights' shapes wanted")
        cnet = None if cw is None else self._value_net(_abi.ValueNet(), cw, k, where, "cost_weights")
        cgrads = None if cw is None else self._value_net(_abi.ValueGrads(), cg, k, where, "cost_grads")
        b = _abi.PPOBatch()
        b.obs, b.action, b.logp_old, b.adv = o2.data_ptr(), None if cat is not None else actions.data_ptr(), logp_old.data_ptr(), adv.data_ptr()
        b.ret = ret.data_ptr() if vw is not None else None
        b.adv_stats = adv_stats.data_ptr() if adv_stats is not None else None
        b.index, b.count = self._list_args(index, count, n_list, where)
        b.obs_stride, b.in_dim, b.n_rows, b.n_list, b.start, b.stride, b.rows = obs_stride, k, n_rows, n_list, int(start), int(stride), rows
        self._follow_stream()
        return nets, cnet, b, grads, cgrads

    def adam(self, param, grad, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=0.0):
        """One Adam step on the flat float32 cuda buffer `param` (pgd_adam), `grad`, `m`, `v` of its length; max_grad_norm > 0 clips by the
        global gradient norm first.  `step`: int32 cuda [4], zero before the first step -- entry 0 counts the steps ON THE DEVICE (a
        replayed graph takes the next step), entries 1..3 are the call's record.  Asynchronous."""
        a = self._adam_args("adam", param, grad, m, v, step, lr, betas, eps, max_grad_norm)
        self._follow_stream()
        _chk(self.L.pgd_adam(*a), "pgd_adam")
        return param

    def _adam_args(self, where, param, grad, m, v, step, lr, betas, eps, max_grad_norm):
        """What adam and adam_gated share, checked -> the leading arguments of the C call."""
        t = self.torch
        n = int(param.numel())
        _need(n >= 1, where, "param: at least one element wanted")
        for name, x in (("param", param), ("grad", grad), ("m", m), ("v", v)):
            _dev(x, t.float32, n, where, name)
        _dev(step, t.int32, 4, where, "step")
        return (self.h, _p(param), _p(grad), _p(m), _p(v), n, _p(step), float(lr), float(betas[0]), float(betas[1]), float(eps),
                float(max_grad_norm))

    def shuffle_index(self, index, count, n_list, seed, epoch, epoch_dev=None, out=None):
        """A keyed permutation of a row list (pgd_shuffle_index) -> `out`, int32 cuda [n_list]: out[q] = index[pi(q)] (`index` None: pi(q))
        for q < count (int32 cuda [1], read on the device; None: n_list), pi a bijection of [0, count) drawn from (seed, epoch +
        epoch_dev[0]) -- `epoch_dev` int32 cuda [1] or None: the counter a replayed graph advances.  Entries at and beyond the count keep
        what they held.  `out` must not share memory with `index`.  Asynchronous."""
        t = self.torch
        n_list = int(n_list)
        _need(0 <= n_list <= _abi.PPO_ROWS_MAX and 0 <= int(seed) < 2 ** 32 and 0 <= int(epoch) < 2 ** 32, "shuffle_index",
              "0 <= n_list <= PPO_ROWS_MAX and seed, epoch in [0, 2^32) wanted")
        out = t.empty((n_list, ), dtype=t.int32, device=self.device) if out is None else out
        _dev(out, t.int32, None, "shuffle_index", "out", n_list)
        ip, cp = self._list_args(index, count, n_list, "shuffle_index")
        if index is not None:
            lo, hi = index.data_ptr(), index.data_ptr() + 4 * index.numel()
            _need(out.data_ptr() + 4 * out.numel() <= lo or hi <= out.data_ptr(), "shuffle_index", "`out` overlaps `index`")
        _opt(epoch_dev, t.int32, 1, "shuffle_index", "epoch_dev", None, False)
        self._follow_stream()
        _chk(self.L.pgd_shuffle_index(self.h, ip, cp, n_list, int(seed), int(epoch), _p(epoch_dev), _p(out)), "pgd_shuffle_index")
        return out

    def adam_gated(self, param, grad, m, v, step, lr, gate, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=0.0, lr_scale=None, kl=None,
                   kl_limit=0.0, count_gate=None):
        """adam() behind a gate on the device (pgd_adam_gated).  `gate`: int32 cuda [4] (_abi.ADAM_GATE), zeroed by the caller where an
        update begins.  The call skips -- `param`, `m`, `v` and `step` keep their bytes, gate = (1, ., +1, 1), `count_gate` (int32 cuda [1]
        or None) is zeroed -- when gate[0] is set or `kl` (one float32 cuda, or None) is not <= kl_limit; else it applies adam's step with
        the learning rate lr * lr_scale[0] (`lr_scale`: one float32 cuda, or None) and counts it in gate[1].  Asynchronous."""
        t = self.torch
        a = self._adam_args("adam_gated", param, grad, m, v, step, lr, betas, eps, max_grad_norm)
        _dev(gate, t.int32, 4, "adam_gated", "gate")
        _opt(lr_scale, t.float32, None, "adam_gated", "lr_scale", 1, False, 4)
        _opt(kl, t.float32, None, "adam_gated", "kl", 1, False, 4)
        _opt(count_gate, t.int32, 1, "adam_gated", "count_gate", None, False)
        self._follow_stream()
        _chk(self.L.pgd_adam_gated(*a, _p(lr_scale), _p(kl), float(kl_limit), _p(gate), _p(count_gate)), "pgd_adam_gated")
        return param

    # -- safe RL behind a rollout: the cost side of the loop (include/pgdrive_hip.h states the formulas) ---------------------------
    def mlp_actor_critic_cost(self, policy_weights, value_weights, cost_weights, out, logp, value, cost_value, seed, tick, obs=None, group=-1,
                              deterministic=False, in_dim=None):
        """mlp_actor_critic with a cost critic beside actor and critic in the same launch (pgd_mlp_actor_critic_cost): `cost_weights` has
        the shapes of `value_weights` (both are required), `cost_value` [N, A] float32 cuda receives its output.  Every other argument,
        the noise and the tick rule as for mlp_actor_critic, whose bits `out`, `logp` and `value` are."""
        self._ac_call("mlp_actor_critic_cost", policy_weights, value_weights, cost_weights, out, (logp, value, cost_value), seed, tick, obs, group,
                      deterministic, in_dim)
        return out, logp, value, cost_value

    def cost_gae(self, flags, done, cost_value, costs, gamma, lam, run, cost=None, adv=None, ret=None, ep_sum=None, ep_count=None):
        """The costs of a rollout from its flags, their advantages and returns, and the episode-cost bookkeeping (pgd_cost_gae): flags
        (int32), done (uint8) [T, rows...], cost_value [T + 1, rows...], time-major contiguous cuda tensors; `costs` = (out_of_road,
        crash_vehicle, crash_object); `run` float32 [rows], read and written: the cost of every row's unfinished episode, carried from
        rollout to rollout.  Returns (cost, adv, ret, ep_sum, ep_count): the first three float32 of flags' shape, ep_sum float32 and
        ep_count int32 [rows] -- the episodes that finished in THIS rollout (each a buffer to write, allocated when None).  Asynchronous."""
        return self._cost_gae("cost_gae", flags, done, cost_value, (), costs, gamma, lam, run, cost, adv, ret, ep_sum, ep_count)

    def _cost_gae(self, fn, flags, done, cost_value, term, costs, gamma, lam, run, cost, adv, ret, ep_sum, ep_count):
        """cost_gae and cost_gae_bootstrap (`term`: its table row for term_cost_value, or none)."""
        t = self.torch
        T, rows, (*ins, cost, adv, ret, run, ep_sum, ep_count) = self._rollout_buffers(
            fn, (("flags", flags, t.int32, 0), ("done", done, t.uint8, 0), ("cost_value", cost_value, t.float32, 1), *term,
                 ("cost", cost, t.float32, 0), ("adv", adv, t.float32, 0), ("ret", ret, t.float32, 0), ("run", run, t.float32, None),
                 ("ep_sum", ep_sum, t.float32, None), ("ep_count", ep_count, t.int32, None)))
        c3 = (C.c_float * 3)(*[float(c) for c in costs])
        _chk(getattr(self.L, "pgd_" + fn)(self.h, *map(_p, ins), T, rows, c3, float(gamma), float(lam), _p(cost), _p(adv), _p(ret), _p(run),
                                          _p(ep_sum), _p(ep_count)), "pgd_" + fn)
        return cost, adv, ret, ep_sum, ep_count

    def lagrange(self, ep_sum, ep_count, state, cost_limit, lr, lambda_max=100.0):
        """One step of the Lagrange multiplier from a rollout's finished episodes (pgd_lagrange): `ep_sum` float32, `ep_count` int32 [rows]
        as cost_gae wrote them; `state` float32 cuda [4] (_abi.LAGRANGE_STATE), zero before the first step, updated in place ON THE
        DEVICE: lambda <- clamp(lambda + lr (J_c - cost_limit), 0, lambda_max) with J_c the mean cost of the episodes; no finished
        episode: unchanged.  Asynchronous."""
        t = self.torch
        rows = int(ep_sum.numel())
        _dev(ep_sum, t.float32, None, "lagrange", "ep_sum", 1)
        _dev(ep_count, t.int32, rows, "lagrange", "ep_count")
        _dev(state, t.float32, 4, "lagrange", "state")
        self._follow_stream()
        _chk(self.L.pgd_lagrange(self.h, _p(ep_sum), _p(ep_count), rows, float(cost_limit), float(lr), float(lambda_max), _p(state)),
             "pgd_lagrange")
        return state

    def adv_mix(self, adv, cadv, state, out=None, adv_stats=None, cadv_stats=None):
        """The advantage a PPO-Lagrangian policy sees (pgd_adv_mix): ((adv - m) s - lambda (cadv - m_c)) / (1 + lambda) -> `out`, with
        (m, s) = `adv_stats` and m_c = cadv_stats[0] as adv_stats() wrote them (None: (0, 1) and 0) and lambda = state[0] (lagrange's
        tensor), all read on the device.  `adv`, `cadv`, `out`: float32 cuda of one size.  Asynchronous."""
        t = self.torch
        n = int(adv.numel())
        out = t.empty_like(adv) if out is None else out
        _need(n >= 1, "adv_mix", "adv: at least one element wanted")
        for name, v in (("adv", adv), ("cadv", cadv), ("out", out)):
            _dev(v, t.float32, n, "adv_mix", name)
        _dev(state, t.float32, 4, "adv_mix", "state")
        _opt(adv_stats, t.float32, 2, "adv_mix", "adv_stats")
        _opt(cadv_stats, t.float32, 2, "adv_mix", "cadv_stats")
        self._follow_stream()
        _chk(self.L.pgd_adv_mix(self.h, _p(adv), _p(cadv), n, _p(adv_stats), _p(cadv_stats), _p(state), _p(out)), "pgd_adv_mix")
        return out

    def ppo_cost_work_bytes(self, in_dim, rows):
        """The scratch pgd_ppo_grad_cost needs for minibatches of up to `rows` positions (pgd_ppo_cost_work_bytes); 0: the call would
        refuse them."""
        return int(self.L.pgd_ppo_cost_work_bytes(int(in_dim), int(rows)))

    def ppo_grad_cost(self, policy_weights, value_weights, cost_weights, policy_grads, value_grads, cost_grads, obs, actions, logp_old, adv, ret,
                      cost_ret, stats, work, start=0, stride=1, rows=None, index=None, count=None, n_list=None, adv_stats=None, clip=0.2,
                      vf_coef=0.5, cvf_coef=0.5, ent_coef=0.0, in_dim=None):
        """ppo_grad with the cost critic as a third network (pgd_ppo_grad_cost): `cost_weights` / `cost_grads` of the value network's
        shapes, `cost_ret` its targets by row, `cvf_coef` its loss coefficient; `adv` is normally adv_mix's output (`adv_stats` None).
        `stats` float32 cuda [8] (_abi.PPO_COST_STATS: entry 7 is the cost critic's loss); `work` a cuda tensor of at least
        ppo_cost_work_bytes(in_dim, rows) bytes.  Every other argument as for ppo_grad, whose bits the actor's and the critic's
        gradients and stats[0..6] are.  Asynchronous."""
        nets, cnet, b, grads, cgrads = self._ppo_batch("ppo_grad_cost", (policy_weights, value_weights, cost_weights),
                                                       (policy_grads, value_grads, cost_grads), obs, actions, logp_old, adv, ret, cost_ret, stats,
                                                       work, start, stride, rows, index, count, n_list, adv_stats, in_dim)
        hp = _abi.PPOHyper(float(clip), float(vf_coef), float(ent_coef))
        pc = _abi.PPOCost(cost_ret.data_ptr(), float(cvf_coef))
        _chk(self.L.pgd_ppo_grad_cost(self.h, C.byref(nets), C.byref(cnet), C.byref(b), C.byref(pc), C.byref(hp), C.byref(grads), C.byref(cgrads),
                                      _p(stats), _p(work), work.numel() * work.element_size()), "pgd_ppo_grad_cost")
        return stats

    def ppo_grad_guided(self, policy_weights, value_weights, policy_grads, value_grads, obs, actions, logp_old, adv, ret, stats, work, target,
                        mask=None, mask_bits=1, bc_coef=1.0, keep_surrogate=False, cost_weights=None, cost_grads=None, cost_ret=None, cvf_coef=0.5,
                        start=0, stride=1, rows=None, index=None, count=None, n_list=None, adv_stats=None, clip=0.2, vf_coef=0.5, ent_coef=0.0,
                        in_dim=None):
        """ppo_grad -- with `cost_weights`, `cost_grads`, `cost_ret`: ppo_grad_cost -- that knows which rows an expert overrode
        (pgd_ppo_grad_guided).  `target` float32 cuda [..., 2] or [..., 4] BY ROLLOUT ROW (the stride is its last dimension: 2 for a
        collector's applied_actions, 4 for its guardian_trace, of which columns 0 and 1 are read); `mask` uint8 cuda by row, a row is
        guided where (mask & mask_bits) != 0, None: every live row is.  A guided row drops its clipped surrogate (keep_surrogate: keeps
        it) and adds bc_coef * -logp(target) / n to the loss; critics and the entropy term see every live row.  `stats` float32 cuda
        [12] (_abi.PPO_GUIDED_STATS); `work` as for ppo_grad / ppo_grad_cost.  With no guided row the gradients and stats[0:8] are
        those calls' bits.  Every other argument as for ppo_grad.  Asynchronous."""
        where, t = "ppo_grad_guided", self.torch
        _need(cost_weights is None or (cost_grads is not None and cost_ret is not None), where, "cost_weights come with cost_grads and cost_ret")
        nets, cnet, b, grads, cgrads = self._ppo_batch(where, (policy_weights, value_weights, cost_weights), (policy_grads, value_grads, cost_grads),
                                                       obs, actions, logp_old, adv, ret, cost_ret if cost_weights is not None else None, stats,
                                                       work, start, stride, rows, index, count, n_list, adv_stats, in_dim, n_stats=12)
        ts = int(target.shape[-1]) if target.dim() else 0
        _need(ts in (2, 4), where, "target: a last dimension of 2 or 4 wanted, got shape %r" % (tuple(target.shape), ))
        _dev(target, t.float32, None, where, "target", b.n_rows * ts)
        _opt(mask, t.uint8, None, where, "mask", b.n_rows)
        bc = float(bc_coef)
        _need(0.0 <= bc < float("inf"), where, "bc_coef: a finite number >= 0 wanted, got %r" % (bc_coef, ))
        _need(mask is None or 0 < int(mask_bits) < 256, where, "mask_bits: 1 .. 255 wanted with a mask, got %r" % (mask_bits, ))
        gd = _abi.PPOGuide(target.data_ptr(), None if mask is None else mask.data_ptr(), ts, int(mask_bits) if mask is not None else 0, bc,
                           _abi.GUIDE_KEEP_SURROGATE if keep_surrogate else 0)
        hp = _abi.PPOHyper(float(clip), float(vf_coef), float(ent_coef))
        pc = None if cnet is None else _abi.PPOCost(cost_ret.data_ptr(), float(cvf_coef))
        _chk(self.L.pgd_ppo_grad_guided(self.h, C.byref(nets), None if cnet is None else C.byref(cnet), C.byref(b),
                                        None if pc is None else C.byref(pc), C.byref(gd), C.byref(hp), C.byref(grads),
                                        None if cgrads is None else C.byref(cgrads), _p(stats), _p(work), work.numel() * work.element_size()),
             "pgd_ppo_grad_guided")
        return stats

    # -- GAE that bootstraps through a time limit (include/pgdrive_hip.h states `truncated` and the formulas) ---------------------------
    def mlp_terminal_value(self, value_weights, cost_weights, term_obs, flags, done, term_value, term_cost_value=None, group=-1, in_dim=None):
        """The critic's value of the terminal observation of every env the step truncated, 0 for every other env, in one launch
        (pgd_mlp_terminal_value): `term_obs` [N, >= in_dim] float32 cuda with unit column stride -- step_info["final_observation"] --,
        `flags` (int32) and `done` (uint8) [N] as the step wrote them, `term_value` [N] float32 (written at every row).  `cost_weights`
        (None: no cost critic) has the shapes of `value_weights`; its values go to `term_cost_value` [N].  A truncated row gets the bits
        mlp_actor_critic's `value` has for the same row and weights.  Single-agent engines.  `group`, `in_dim` as for mlp_policy.
        Asynchronous."""
        t = self.torch
        rows = self.N * self.A
        k = int(in_dim if in_dim is not None else value_weights[0].shape[0])
        o2, stride = self._obs_rows(term_obs, rows, k, "mlp_terminal_value", "term_obs")
        _dev(flags, t.int32, rows, "mlp_terminal_value", "flags")
        _dev(done, t.uint8, rows, "mlp_terminal_value", "done")
        _need((cost_weights is None) == (term_cost_value is None), "mlp_terminal_value", "term_cost_value comes with the cost critic")
        _dev(term_value, t.float32, rows, "mlp_terminal_value", "term_value")
        _opt(term_cost_value, t.float32, rows, "mlp_terminal_value", "term_cost_value")
        critic = self._value_net(_abi.ValueNet(), value_weights, k, "mlp_terminal_value", "value_weights")
        cost = None if cost_weights is None else C.byref(self._value_net(_abi.ValueNet(), cost_weights, k, "mlp_terminal_value", "cost_weights"))
        if group < 0:
            self._follow_stream()
        _chk(self.L.pgd_mlp_terminal_value(self.h, int(group), _p(o2), stride, k, C.byref(critic), cost, _p(flags), _p(done), _p(term_value),
                                           _p(term_cost_value)), "pgd_mlp_terminal_value")
        return term_value, term_cost_value

    def gae_bootstrap(self, reward, value, done, term_value, gamma, lam, adv=None, ret=None):
        """gae with the one-step target of a done row taken from `term_value` [T, rows...] (pgd_gae_bootstrap): the critic's value of the
        terminal observation where the episode was truncated, 0 where it terminated, as mlp_terminal_value writes it.  Every other
        argument and the result as for gae."""
        return self._gae("gae_bootstrap", reward, value, done, (("term_value", term_value, self.torch.float32, 0), ), gamma, lam, adv, ret)

    def cost_gae_bootstrap(self, flags, done, cost_value, term_cost_value, costs, gamma, lam, run, cost=None, adv=None, ret=None, ep_sum=None,
                           ep_count=None):
        """cost_gae with the one-step target of a done row taken from `term_cost_value` [T, rows...] (pgd_cost_gae_bootstrap); the costs
        and the books of episode costs are cost_gae's.  Every other argument and the result as for cost_gae."""
        return self._cost_gae("cost_gae_bootstrap", flags, done, cost_value, (("term_cost_value", term_cost_value, self.torch.float32, 0), ), costs,
                              gamma, lam, run, cost, adv, ret, ep_sum, ep_count)

    # -- reward scaling by the running return, in front of GAE (include/pgdrive_hip.h states the rule) -------------------------------------
    def return_norm_work_bytes(self, rows):
        """The scratch pgd_return_norm needs for `rows` rows (pgd_return_norm_work_bytes)."""
        return int(self.L.pgd_return_norm_work_bytes(int(rows)))

    def return_norm_state(self, rows):
        """(carry, record) as pgd_return_norm wants them before its first call: float32 zeros [rows] and the float64 record
        _abi.RETURN_NORM_INIT (count, mean, m2, scale), on the engine's device."""
        t = self.torch
        return (t.zeros((int(rows), ), dtype=t.float32, device=self.device),
                t.tensor(_abi.RETURN_NORM_INIT, dtype=t.float64, device=self.device))

    def return_norm(self, reward, done, gamma, carry, record, flags=None, eps=1e-8, clip=10.0, freeze=False, out=None, work=None):
        """The rewards of a rollout divided by the standard deviation of the running discounted return (pgd_return_norm; the norm_reward
        half of VecNormalize): reward, done (uint8) [T, rows...], time-major contiguous cuda tensors; `flags` (int32, of reward's shape):
        the step flags of a multi-agent rollout -- only rows at which an agent acted are samples, and they alone are scaled (every other
        entry of the result is 0).  `carry` float32 [rows] and `record` float64 [4] (_abi.RETURN_NORM_RECORD) are read and written: the
        discounted return of every row's running episode and the running count, mean, sum of squared deviations and scale; they start as
        return_norm_state() gives them.  The rollout is scaled by the scale that already includes its own samples, then clamped to
        [-clip, clip] (clip <= 0: no clamp).  freeze: carry and record are read, not written.  Returns the scaled rewards, float32 of
        reward's shape (`out`: the buffer to write).  `work`: a cuda tensor of at least return_norm_work_bytes(rows) bytes, allocated when
        None.  Three launches (freeze: one), asynchronous on the caller's current stream."""
        t = self.torch
        T, rows, (reward, done, out, carry) = self._rollout_buffers("return_norm", (
            ("reward", reward, t.float32, 0), ("done", done, t.uint8, 0), ("out", out, t.float32, 0), ("carry", carry, t.float32, None)))
        _opt(flags, t.int32, T * rows, "return_norm", "flags")
        _dev(record, t.float64, 4, "return_norm", "record")
        work, n_bytes = self._scratch(work, self.return_norm_work_bytes(rows), reward.device, "return_norm")
        _chk(self.L.pgd_return_norm(self.h, _p(reward), _p(done), _p(flags), T, rows, float(gamma), float(eps), float(clip),
                                    _abi.RN_FREEZE if freeze else 0, _p(carry), _p(record), _p(out), _p(work), n_bytes), "pgd_return_norm")
        return out

    # -- observation normalisation, fused into the training kernels' row loads (include/pgdrive_hip.h states the rule) -------------------
    def obs_norm_work_bytes(self, in_dim, n_list):
        """The scratch pgd_obs_norm_update needs for a list of up to `n_list` rows of `in_dim` columns (pgd_obs_norm_work_bytes); 0: the
        call would refuse them."""
        return int(self.L.pgd_obs_norm_work_bytes(int(in_dim), int(n_list)))

    def obs_norm_state(self, in_dim=None):
        """(record, table) as the calls want them before the first fold, on the engine's device: float64 zeros [1 + 2 in_dim] (n, the
        column means, the column sums of squared deviations) and the identity table float32 [2, (in_dim + 3) & ~3] (shift | scale)."""
        t = self.torch
        in_dim = self.D if in_dim is None else int(in_dim)
        doubles, shape = _abi.obs_norm_layout(in_dim)
        table = t.zeros(shape, dtype=t.float32, device=self.device)
        table[1] = 1.0
        return t.zeros((doubles, ), dtype=t.float64, device=self.device), table

    def obs_norm_update(self, obs, record, index=None, count=None, n_list=None, in_dim=None, work=None):
        """Fold the first `in_dim` floats (None: the last dimension of `obs`) of every listed row of `obs` [..., stride] (float32 cuda,
        flattened to rows) into `record` (float64 cuda [1 + 2 in_dim]; pgd_obs_norm_update).  The list as for adv_stats: row index[q] for
        q < count (`index` None: row q; `count` int32 cuda [1], read on the device, None: n_list; n_list None: every row, or every entry
        of `index`).  `work`: a cuda tensor of at least obs_norm_work_bytes(in_dim, n_list) bytes, allocated when None.  Two launches,
        asynchronous on the caller's current stream.  Returns `record`."""
        t = self.torch
        _dev(obs, t.float32, None, "obs_norm_update", "obs")
        stride = int(obs.shape[-1])
        in_dim = stride if in_dim is None else int(in_dim)
        n_rows = obs.numel() // stride
        n_list = int((index.numel() if index is not None else n_rows) if n_list is None else n_list)
        _dev(record, t.float64, 1 + 2 * in_dim, "obs_norm_update", "record")
        ip, cp = self._list_args(index, count, n_list, "obs_norm_update")
        work, n_bytes = self._scratch(work, self.obs_norm_work_bytes(in_dim, n_list), obs.device, "obs_norm_update")
        self._follow_stream()
        _chk(self.L.pgd_obs_norm_update(self.h, _p(obs), stride, in_dim, n_rows, ip, cp, n_list, _p(record), _p(work), n_bytes),
             "pgd_obs_norm_update")
        return record

    def obs_norm_publish(self, record, table, eps=1e-8):
        """`record` -> `table` (float32 cuda [2, Dp]: shift = mean, scale = 1 / sqrt(m2 / n + eps); the identity while the record is
        empty; pgd_obs_norm_publish).  One small launch, asynchronous.  Returns `table`."""
        t = self.torch
        in_dim = (record.numel() - 1) // 2
        _dev(record, t.float64, 1 + 2 * in_dim, "obs_norm_publish", "record")
        _dev(table, t.float32, 2 * ((in_dim + 3) & ~3), "obs_norm_publish", "table")
        self._follow_stream()
        _chk(self.L.pgd_obs_norm_publish(self.h, _p(record), in_dim, float(eps), _p(table)), "pgd_obs_norm_publish")
        return table

    def obs_norm_bind(self, table, in_dim=None, clip=10.0):
        """Bind a table (pgd_obs_norm_bind): every later mlp_actor_critic, mlp_actor_critic_rows, mlp_actor_critic_cost,
        mlp_terminal_value, ppo_grad and ppo_grad_cost launch feeds its networks clamp((obs - shift) * scale, -clip, clip), read from the
        table when the launch RUNS; a call of another input width is refused.  None unbinds.  mlp_policy and mlp_policy_prepared ignore
        the binding.  `in_dim` None: the engine's observation width.  The engine keeps the tensor alive."""
        if table is None:
            _chk(self.L.pgd_obs_norm_bind(self.h, None, 0, 0.0), "pgd_obs_norm_bind")
        else:
            in_dim = self.D if in_dim is None else int(in_dim)
            _dev(table, self.torch.float32, 2 * ((in_dim + 3) & ~3), "obs_norm_bind", "table")
            _chk(self.L.pgd_obs_norm_bind(self.h, _p(table), in_dim, float(clip)), "pgd_obs_norm_bind")
        self._obs_norm_table = table

    # -- episode statistics of a rollout (include/pgdrive_hip.h states the rule) ---------------------------------------------------------
    def rollout_episodes_work_bytes(self, rows):
        """The scratch pgd_rollout_episodes needs for `rows` rows (pgd_rollout_episodes_work_bytes)."""
        return int(self.L.pgd_rollout_episodes_work_bytes(int(rows)))

    def rollout_episodes_state(self, rows):
        """(ret_carry, len_carry, record) as pgd_rollout_episodes wants them before its first call: float32 and int32 zeros [rows] and the
        float64 record _abi.ROLLOUT_EPISODES_INIT, on the engine's device."""
        t = self.torch
        return (t.zeros((int(rows), ), dtype=t.float32, device=self.device), t.zeros((int(rows), ), dtype=t.int32, device=self.device),
                t.tensor(_abi.ROLLOUT_EPISODES_INIT, dtype=t.float64, device=self.device))

    def rollout_episodes(self, reward, done, flags, ret_carry, len_carry, record=None, call=None, seats=False, ep_return=None, ep_length=None,
                         work=None):
        """The statistics of the episodes that ended in a rollout (pgd_rollout_episodes; gym's RecordEpisodeStatistics): reward, done
        (uint8) and flags (int32) [T, rows...], time-major contiguous cuda tensors as the step wrote them.  seats: the rows are the seats of
        a multi-agent engine -- only entries at which an agent acted count, and an agent's episode ends at its done or at an env-wide
        restart.  `ret_carry` float32 and `len_carry` int32 [rows] are read and written: the return and the length of every row's
        unfinished episode; they and `record` start as rollout_episodes_state() gives them.  `record` (float64 [16],
        _abi.ROLLOUT_EPISODES) is read and written: the call merged into the running statistics; `call` (float64 [16]) is written: this
        call's own.  `ep_return` float32 / `ep_length` int32 of reward's shape are written when given: the finished episode's return and
        length at the entry where it ended, 0 everywhere else.  `work`: a cuda tensor of at least rollout_episodes_work_bytes(rows) bytes,
        allocated when None.  Two launches, asynchronous on the caller's current stream.  Returns (record, call)."""
        t = self.torch
        where = "rollout_episodes"
        _need(not any(x is None for x in (reward, done, flags, ret_carry, len_carry)), where, "reward, done, flags and both carries wanted")
        T, rows, (reward, done, flags, ret_carry, len_carry) = self._rollout_buffers(
            where, (("reward", reward, t.float32, 0), ("done", done, t.uint8, 0), ("flags", flags, t.int32, 0),
                    ("ret_carry", ret_carry, t.float32, None), ("len_carry", len_carry, t.int32, None)))
        _opt(record, t.float64, len(_abi.ROLLOUT_EPISODES), where, "record")
        _opt(call, t.float64, len(_abi.ROLLOUT_EPISODES), where, "call")
        _opt(ep_return, t.float32, T * rows, where, "ep_return")
        _opt(ep_length, t.int32, T * rows, where, "ep_length")
        work, n_bytes = self._scratch(work, self.rollout_episodes_work_bytes(rows), reward.device, where)
        _chk(self.L.pgd_rollout_episodes(self.h, _p(reward), _p(done), _p(flags), T, rows, _abi.EP_SEATS if seats else 0, _p(ret_carry),
                                         _p(len_carry), _p(record), _p(call), _p(ep_return), _p(ep_length), _p(work), n_bytes),
             "pgd_rollout_episodes")
        return record, call

    def step_lane_keep(self, tick, k_lat=1.0, k_head=2.0, v_target_kmh=30.0, noise=0.05):
        """One closed-loop step under the scripted lane-keeping policy (pgd_step_lane_keep): the policy reads the engine's own
        observation buffer (what the previous step / reset wrote), the step rewrites it -- one launch on engines with one env per
        wave.  Same results as lane_keep_actions(...) followed by step(...)."""
        self._follow_stream()
        p_obs, p_rew, p_done, p_flags = self._own_ptrs
        _chk(self.L.pgd_step_lane_keep(self.h, k_lat, k_head, v_target_kmh, noise, int(tick) & 0xffffffff, p_obs, p_rew, p_done, p_flags),
             "pgd_step_lane_keep")
        return self.obs, self.reward, self.done, self.flags

    # -- top-down observation (obs/top_down_obs_multi_channel.py) -----------------------------------------------------------
    def enable_topdown(self, td_cfg=None, uint8=False):
        """Switch on the bird's-eye observation; `td_cfg` = _abi.make_topdown_config(...).  `uint8`: the engine's own image buffer holds
        bytes in [0, 255] (the reference's rgb_clip=False) instead of float32 in [0, 1]."""
        self.td_cfg = td_cfg or _abi.make_topdown_config()
        _chk(self.L.pgd_topdown_enable(self.h, C.byref(self.td_cfg)), "pgd_topdown_enable")
        R, Cn = self.td_cfg.resolution, self.L.pgd_topdown_channels(C.byref(self.td_cfg))
        self.img = self.torch.zeros((self.N, R, R, Cn), dtype=self.torch.uint8 if uint8 else self.torch.float32, device=self.device)

    def observe_topdown(self, out=None):
        """Image [N, R, R, C] of the present state -- float32 in [0, 1], or bytes in [0, 255] when the buffer (`out`, else the engine's
        own) is a uint8 tensor; call once after every step / reset (it advances the frame history)."""
        img = self.img if out is None else _dev(out, (self.torch.float32, self.torch.uint8), self.img.numel(), "observe_topdown", "out")
        self._follow_stream()
        if img.dtype == self.torch.uint8:
            _chk(self.L.pgd_observe_topdown_u8(self.h, _p(img)), "pgd_observe_topdown_u8")
        else:
            _chk(self.L.pgd_observe_topdown(self.h, _p(img)), "pgd_observe_topdown")
        return img

    # -- step info on the device (pgd_step_info: terminal observation, the reference's info floats, episode statistics) ---------------
    def enable_step_info(self, costs=(1.0, 1.0, 1.0), final_obs=True):
        """Switch on the step info (include/pgdrive_hip.h, pgd_step_info_enable): one more launch per step writes, for every env, the
        reference's info floats, and for every env whose episode ended the terminal row and the episode's statistics; the env is then
        restarted by that launch instead of by the step kernel (same state, reward, done, flags).  `costs` = (out_of_road_cost,
        crash_vehicle_cost, crash_object_cost); final_obs=False: no terminal row (engines whose observation is an image).  Allocates the
        tensors once and returns them as a dict (also `self.step_info`): [N] each, "final_observation" [N, D] or None.  The values of
        a step are valid until the next step; the ep_* statistics accumulate until episode_stats(clear=True)."""
        t = self.torch
        info = {k: t.zeros((self.N, ), dtype=getattr(t, dt), device=self.device) for k, dt in _abi.STEP_INFO_FIELDS.items()}
        info["final_observation"] = t.zeros((self.N, self.D), dtype=t.float32, device=self.device) if final_obs else None
        si = _abi.StepInfo()
        si.out_of_road_cost, si.crash_vehicle_cost, si.crash_object_cost = (float(c) for c in costs)
        for k in _abi.STEP_INFO_FIELDS:
            setattr(si, k, info[k].data_ptr())
        si.final_obs = info["final_observation"].data_ptr() if final_obs else None
        self.torch.cuda.synchronize(self.device)
        _chk(self.L.pgd_step_info_enable(self.h, C.byref(si)), "pgd_step_info_enable")
        self.step_info = info
        return info

    def disable_step_info(self):
        """Back to the plain step (pgd_step_info_enable with NULL): the step kernel restarts finished envs itself again."""
        self.torch.cuda.synchronize(self.device)
        _chk(self.L.pgd_step_info_enable(self.h, None), "pgd_step_info_enable")
        self.step_info = None

    def episode_stats(self, clear=True):
        """The per-env statistics of the episodes that ended since the last clear, reduced with torch (one synchronisation): episodes,
        mean return, mean length, mean cost and the rates of the four outcomes (None where no episode ended)."""
        if self.step_info is None:
            raise PgdError("episode_stats needs enable_step_info")
        s = self.step_info
        self._follow_stream()
        sums = self.torch.stack([s[k].sum(dtype=self.torch.float64) for k in (
            "ep_count", "ep_return_sum", "ep_length_sum", "ep_cost_sum", "ep_arrive", "ep_out_of_road", "ep_crash", "ep_max_step")]).cpu().numpy()
        if clear:
            _chk(self.L.pgd_step_info_clear_stats(self.h), "pgd_step_info_clear_stats")
        n = int(round(float(sums[0])))
        mean = (lambda x: float(x) / n) if n else (lambda x: None)
        return dict(episodes=n, mean_return=mean(sums[1]), mean_length=mean(sums[2]), mean_cost=mean(sums[3]), arrive_rate=mean(sums[4]),
                    out_of_road_rate=mean(sums[5]), crash_rate=mean(sums[6]), max_step_rate=mean(sums[7]))

    # -- top-down scene rendering (env.render(mode="top_down"), obs/top_down_renderer.py) --------------------------------------------
    def enable_render(self, cfg=None):
        """Create the renderer (pgd_render_enable): `cfg` = pgdrive_amd.render.parse_kwargs' settings or a _abi.RenderConfig (None: the
        reference's defaults).  The film of every map is fitted to its road network's bounding box (pgdrive_amd/render.py)."""
        from . import render
        if cfg is None or isinstance(cfg, dict):
            cfg = render.make_config(render.parse_kwargs("top_down", cfg or {}))
        render.check_capacity(cfg.num_stack, self.V)
        geom = np.array([render.film_geometry(d, cfg.film_w, cfg.film_h) for d in self.bank.descs], dtype=np.float64)
        _need(len(geom) == len(self.bank.maps), "enable_render", "one film geometry per map wanted")
        self.render_cfg = cfg
        self.film_geom = geom
        _chk(self.L.pgd_render_enable(self.h, C.byref(cfg), _np_p(np.ascontiguousarray(geom))), "pgd_render_enable")

    def render_topdown(self, env_ids=None, out=None):
        """Frames of the listed envs (None: all) as a cuda uint8 tensor [n, film_h, film_w, 3] (`out`, else a new tensor); appends the
        present state to the envs' trails.  Asynchronous on the engine's stream (the caller's current stream, as for step)."""
        t = self.torch
        ids = None if env_ids is None else np.ascontiguousarray(np.asarray(env_ids, dtype=np.int64).reshape(-1), dtype=np.int32)
        n = self.N if ids is None else len(ids)
        shape = (n, self.render_cfg.film_h, self.render_cfg.film_w, 3)
        out = _dev(t.empty(shape, dtype=t.uint8, device=self.device) if out is None else out, t.uint8, None, "render_topdown", "out")
        _need(tuple(out.shape) == shape, "render_topdown", "out: shape %s wanted, got %s" % (shape, tuple(out.shape)))
        self._follow_stream()
        _chk(self.L.pgd_render_topdown(self.h, _np_p(ids), n, _p(out)), "pgd_render_topdown")
        return out

    def render_palette(self):
        """The ten agent colours (pgd_render_palette): uint8 [10, 3]."""
        p = np.zeros((10, 3), dtype=np.uint8)
        _chk(self.L.pgd_render_palette(_np_p(p)), "pgd_render_palette")
        return p

    # -- asynchronous env groups ----------------------------------------------------------------------------------------
    def set_groups(self, n_groups):
        """Split the envs into `n_groups` equal contiguous groups with their own internal streams (pgd_set_groups)."""
        self.torch.cuda.synchronize(self.device)
        _chk(self.L.pgd_set_groups(self.h, int(n_groups)), "pgd_set_groups")
        self.n_groups = int(n_groups)
        self.group_streams = []
        for g in range(self.n_groups if n_groups > 1 else 0):
            p = C.c_void_p()
            _chk(self.L.pgd_group_stream(self.h, g, C.byref(p)), "pgd_group_stream")
            self.group_streams.append(self.torch.cuda.ExternalStream(p.value, device=self.device))

    def group_slice(self, g):
        n = self.N // self.n_groups
        return slice(g * n, (g + 1) * n)

    def step_group(self, g, actions):
        """Step only the envs of group g, asynchronously on the group's stream; `actions` is the full [N, A, 2] tensor.
        Returns views of the group's rows of the engine's output buffers."""
        self._check_actions(actions, "step_group")
        p_obs, p_rew, p_done, p_flags = self._own_ptrs
        _chk(self.L.pgd_step_group(self.h, int(g), _p(actions), p_obs, p_rew, p_done, p_flags), "pgd_step_group")
        sl = self.group_slice(g)
        return self.obs[sl], self.reward[sl], self.done[sl], self.flags[sl]

    def group_sync(self, g):
        _chk(self.L.pgd_group_sync(self.h, int(g)), "pgd_group_sync")

    def observe(self):
        _chk(self.L.pgd_observe(self.h, _p(self.obs)), "pgd_observe")
        self.sync()
        return self.obs

    def sync(self):
        _chk(self.L.pgd_sync(self.h), "pgd_sync")

    def enable_step_timing(self, on=True):
        _chk(self.L.pgd_enable_step_timing(self.h, int(bool(on))), "pgd_enable_step_timing")

    def last_step_ms(self):
        ms = C.c_float()
        _chk(self.L.pgd_last_step_ms(self.h, C.byref(ms)), "pgd_last_step_ms")
        return ms.value

    def profile_begin(self, capacity, stride=1):
        _chk(self.L.pgd_profile_begin_strided(self.h, int(capacity), int(stride)), "pgd_profile_begin_strided")

    def profile_end(self):
        a, b, n = C.c_float(), C.c_float(), C.c_int()
        _chk(self.L.pgd_profile_end(self.h, C.byref(a), C.byref(b), C.byref(n)), "pgd_profile_end")
        return dict(k_step_ms=a.value, k_observe_ms=b.value, count=n.value)

    # -- checkpoint / resume ------------------------------------------------------------------------------------------
    def get_state(self):
        f = np.zeros((_abi.NF, self.N, self.V), dtype=np.float32)
        i = np.zeros((_abi.NI, self.N, self.V), dtype=np.int32)
        ei = np.zeros((_abi.NEI, self.N), dtype=np.int32)
        _chk(self.L.pgd_get_state(self.h, _np_p(f), _np_p(i), _np_p(ei)), "pgd_get_state")
        return f, i, ei

    def set_state(self, f, i, ei):
        f = np.ascontiguousarray(f, dtype=np.float32)
        i = np.ascontiguousarray(i, dtype=np.int32)
        ei = np.ascontiguousarray(ei, dtype=np.int32)
        _need(f.shape == (_abi.NF, self.N, self.V) and i.shape == (_abi.NI, self.N, self.V), "set_state", "f [NF, N, V] and i [NI, N, V] wanted")
        _chk(self.L.pgd_set_state(self.h, _np_p(f), _np_p(i), _np_p(ei)), "pgd_set_state")

    def close(self):
        t = getattr(self, "_jit_thread", None)
        if t is not None and t.is_alive():  # a run-time kernel still being built (specialise(wait=False))
            t.join(timeout=120)
        if getattr(self, "h", None):
            self.L.pgd_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
