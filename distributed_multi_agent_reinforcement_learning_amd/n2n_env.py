"""`ParticleEnv` (env_n2n): the reference's continuous 2-D pursuit environment batched on the GPU.

Mirrors environment/env_n2n/particle_env.py:105-462 of the reference for N independent environments: `initialize`,
`reset`, `evader_step`, `step`, `get_team_state`, `get_adj_mat`, `get_active` keep their names; tensors carry a leading
environment dimension.  The kinematics / reward / culling / done logic runs in csrc/n2n_env.hip (C ABI include/n2n_env.h),
the reset in the same library's host part with a replica of numpy's legacy generator per environment.
The reference's evader is driven by scipy's SLSQP (eva.py:36-80).  Here the heading command is an input (`evader_step(cmd)`),
or, when none is given, either a simple closed-form rule (head for the target, turn away from the nearest pursuer in sensing
range; `evader="rule"`, the default) or the reference's optimiser itself, Kraft's SLSQP on the GPU (`evader="slsqp"`,
n2n_evader_slsqp in the same library).
"""
import ctypes as C
import math
import os

import numpy as np
import torch

from . import build as _build
from .policy_record import fill_acc, record_opts, rows


class N2nConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("P", "E", "episode_limit", "pad0")] + \
               [(n, C.c_double) for n in ("p_vmax", "e_vmax", "p_sen_range", "p_comm_range", "kill_radius", "ang_lmt", "step_size")]


class N2nState(C.Structure):
    _fields_ = [("N", C.c_int32), ("pad0", C.c_int32)] + [(n, C.c_void_p) for n in ("p", "e", "target", "time_step")]


class N2nObsOut(C.Structure):
    _fields_ = [("p_state", C.c_void_p), ("p_state_stride", C.c_int64), ("e_state", C.c_void_p), ("e_state_stride", C.c_int64),
                ("pp_adj", C.c_void_p), ("pp_adj_stride", C.c_int64), ("pe_adj", C.c_void_p), ("pe_adj_stride", C.c_int64)]


class N2nPolicyIO(C.Structure):
    _fields_ = [(n, t) for k in ("pp_in", "pe_in", "p4", "e4", "e_ref", "live", "pp_adj", "pe_adj") for n, t in ((k, C.c_void_p), (k + "_rs", C.c_int64))]


class N2nGuidanceParams(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("lead", "sep_range", "sep_gain")]


class N2nPolicyAcc(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("done_before", "ended", "captured", "ret", "length")]


class N2nRecordIO(C.Structure):
    _fields_ = [(n, t) for k in ("live", "value", "r", "active", "v", "v_next") for n, t in ((k, C.c_void_p), (k + "_rs", C.c_int64))]


_lib = None


def load_library():
    global _lib
    if _lib is None:
        path = _build.lib_path("libn2n_env.so")
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: build it with __graft_entry__.build(); env_n2n has no CPU fallback")
        L = C.CDLL(path)
        vp = C.c_void_p
        L.n2n_config_check.argtypes = [vp]
        L.n2n_env_load.argtypes = [vp] * 6
        L.n2n_env_observe.argtypes = [vp] * 4
        L.n2n_env_tick.argtypes = [vp] * 9
        L.n2n_resetter_create.argtypes = [vp, C.c_int32, vp]
        L.n2n_resetter_create.restype = vp
        L.n2n_resetter_destroy.argtypes = [vp]
        L.n2n_evader_slsqp.argtypes = [vp] * 4
        L.n2n_evader_slsqp_nit.argtypes = [vp] * 5
        L.n2n_evader_slsqp_host.argtypes = [vp, C.c_int32] + [vp] * 5
        L.n2n_resetter_reset.argtypes = [vp, vp, vp, vp, C.c_int32]
        L.n2n_resetter_state_bytes.argtypes = [vp]
        L.n2n_resetter_state_bytes.restype = C.c_int64
        L.n2n_resetter_get_state.argtypes = [vp, vp]
        L.n2n_resetter_set_state.argtypes = [vp, vp]
        L.n2n_policy_inputs.argtypes = [vp] * 5
        L.n2n_policy_record.argtypes = [vp] * 8
        L.n2n_shaping_begin.argtypes = [vp] * 3 + [C.c_double, vp]
        L.n2n_pursuer_guidance.argtypes = [vp] * 5
        _lib = L
    return _lib


def _check(rc, what):
    if rc != 0:
        extra = " (no placement within N2N_RESET_MAX_DRAWS draws: too many agents for the box at distance 2)" if rc == 30004 else ""
        raise RuntimeError(f"{what} failed with code {rc}{extra}")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class ParticleEnv:
    """cfg values are the reference's hard-coded defaults (particle_env.py:108-121,143-147)."""

    def __init__(self, num_envs=1, seeds=None, device="cuda", p_vmax=0.3, e_vmax=1.0, p_sen_range=3.0, p_comm_range=6.0,
                 kill_radius=0.5, ang_lmt=math.pi / 4, step_size=0.5, episode_limit=100, evader="rule"):
        if evader not in ("rule", "slsqp"):
            raise ValueError(f"evader must be 'rule' or 'slsqp', not {evader!r}")
        self.evader = evader
        self.L = load_library()
        if not torch.cuda.is_available():
            raise RuntimeError("ParticleEnv needs a GPU (MI355X); there is no CPU path")
        self.num_envs = int(num_envs)
        self.device = torch.device(device)
        self.seeds = list(seeds) if seeds is not None else list(range(self.num_envs))
        self.p_obs_dim = self.e_obs_dim = 3
        self.env_name = "ParticleEnvBoundGra"
        self.episode_limit, self.step_size, self.kill_radius = episode_limit, step_size, kill_radius
        self._kw = dict(p_vmax=p_vmax, e_vmax=e_vmax, p_sen_range=p_sen_range, p_comm_range=p_comm_range, kill_radius=kill_radius,
                        ang_lmt=ang_lmt, step_size=step_size)
        self.time_step = 0
        self.n_episode = 0
        self.p_num = self.e_num = None
        self.resetter = None
        self.reward_scale = None
        self.shaping_phi, self.shaping_coef = None, None
        self._guidance_out = None
        self.set_guidance()   # the scripted pursuers' defaults

    def initialize(self, p_num, e_num):
        """particle_env.py:160-162, plus the allocation of the device records"""
        self.p_num, self.e_num = int(p_num), int(e_num)
        c = N2nConfig()
        c.P, c.E, c.episode_limit = self.p_num, self.e_num, self.episode_limit
        for k, v in self._kw.items():
            setattr(c, k, v)
        _check(self.L.n2n_config_check(C.byref(c)), "n2n_config_check")
        self.c = c
        N, dev = self.num_envs, self.device
        self.p = torch.zeros((N, 5, self.p_num), dtype=torch.float64, device=dev)
        self.e = torch.zeros((N, 5, self.e_num), dtype=torch.float64, device=dev)
        self.target = torch.zeros((N, 2), dtype=torch.float64, device=dev)
        self.t_dev = torch.zeros((N,), dtype=torch.int32, device=dev)
        self.st = N2nState()
        self.st.N = N
        self.st.p, self.st.e, self.st.target, self.st.time_step = self.p.data_ptr(), self.e.data_ptr(), self.target.data_ptr(), self.t_dev.data_ptr()
        f = lambda *s: torch.zeros((N, *s), dtype=torch.float32, device=dev)
        self.obs = dict(p_state=f(self.p_num, 3), e_state=f(self.e_num, 3), pp_adj=f(self.p_num, self.p_num), pe_adj=f(self.p_num, self.e_num))
        self.reward_t = f(self.p_num)
        self.active_t = torch.ones((N, self.p_num), dtype=torch.uint8, device=dev)
        self.done_t = torch.zeros((N,), dtype=torch.uint8, device=dev)
        self._cmd_slsqp = torch.zeros((N, self.e_num), dtype=torch.float64, device=dev)  # the kernel's own output buffer
        s = np.ascontiguousarray(self.seeds, np.uint32)
        self.resetter = self.L.n2n_resetter_create(C.byref(c), N, s.ctypes.data_as(C.c_void_p))
        if not self.resetter:
            raise RuntimeError("n2n_resetter_create failed (bad configuration or out of memory)")
        self._obs_struct = N2nObsOut()
        for k, t in self.obs.items():
            setattr(self._obs_struct, k, t.data_ptr())
            setattr(self._obs_struct, k + "_stride", t.stride(0))

    def __del__(self):
        try:
            if self.resetter:
                self.L.n2n_resetter_destroy(self.resetter)
        except Exception:
            pass

    def reset(self, init=None):
        """particle_env.py:200-237.  init = (p [N,P,5], e [N,E,5], target [N,2]) injects recorded initial conditions."""
        N = self.num_envs
        if init is None:
            p = np.empty((N, self.p_num, 5)); e = np.empty((N, self.e_num, 5)); tg = np.empty((N, 2))
            _check(self.L.n2n_resetter_reset(self.resetter, p.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p),
                                             tg.ctypes.data_as(C.c_void_p), min(16, os.cpu_count() or 1)), "n2n_resetter_reset")
        else:
            p, e, tg = (np.ascontiguousarray(a, np.float64) for a in init)
        self.last_init = (p, e, tg)
        _check(self.L.n2n_env_load(C.byref(self.c), C.byref(self.st), p.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p),
                                   tg.ctypes.data_as(C.c_void_p), _stream()), "n2n_env_load")
        torch.cuda.current_stream().synchronize()
        self.time_step = 0
        self.n_episode += 1
        self._cmd = torch.zeros((N, self.e_num), dtype=torch.float64, device=self.device)
        if self.reward_scale is not None:
            self.reward_scale[:, 1 + 2 * self.p_num:].zero_()   # RewardScaling.reset: R; n, mean, S persist
        self.observe()

    def get_resetter_state(self):
        """the reset generators of every environment (include/n2n_env.h n2n_resetter_get_state) as a uint8 array"""
        buf = np.empty(self.L.n2n_resetter_state_bytes(self.resetter), np.uint8)
        _check(self.L.n2n_resetter_get_state(self.resetter, buf.ctypes.data_as(C.c_void_p)), "n2n_resetter_get_state")
        return buf

    def set_resetter_state(self, blob):
        """restores get_resetter_state(); ValueError when the blob comes from another number of environments / agents"""
        buf = np.ascontiguousarray(blob, np.uint8)
        if buf.size != self.L.n2n_resetter_state_bytes(self.resetter):
            raise ValueError("resetter state does not match this number of environments")
        rc = self.L.n2n_resetter_set_state(self.resetter, buf.ctypes.data_as(C.c_void_p))
        if rc != 0:
            raise ValueError(f"resetter state does not match this configuration (n2n_resetter_set_state code {rc})")

    def observe(self):
        _check(self.L.n2n_env_observe(C.byref(self.c), C.byref(self.st), C.byref(self._obs_struct), _stream()), "n2n_env_observe")
        return self.obs

    def get_team_state(self, is_pursuer, rules=False):
        """(N, A, 3) [x, y, phi] of every agent (the reference's rules=False form, :376-384)"""
        return self.obs["p_state"] if is_pursuer else self.obs["e_state"]

    def get_adj_mat(self, which="pp"):
        """:386-397 with the pursuers as observers: 'pp' (communication range) or 'pe' (sensing range)"""
        return self.obs["pp_adj" if which == "pp" else "pe_adj"]

    def get_active(self):
        return self.active_t

    def evader_step(self, cmd=None, nit=None):
        """Sets the evaders' normalised heading command in [-1, 1] for the next step (the reference computes it with SLSQP,
        :179-198).  Without `cmd`, evader="rule": head for the target, but away from the nearest pursuer inside the sensing range;
        evader="slsqp": the reference's SLSQP evader, launched on the current stream without a host synchronisation (it can be
        captured in a graph).  nit, an int32 (N, E) device tensor, receives the SLSQP iterations taken per evader."""
        if cmd is None and self.evader == "slsqp":
            ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None else None)
            if nit is not None:
                assert nit.dtype == torch.int32 and nit.is_contiguous() and nit.numel() == self.num_envs * self.e_num
            _check(self.L.n2n_evader_slsqp_nit(C.byref(self.c), C.byref(self.st), ptr(self._cmd_slsqp), ptr(nit), _stream()),
                   "n2n_evader_slsqp")
            self._cmd = self._cmd_slsqp
            return
        if cmd is None:
            ex, ey = self.e[:, 0], self.e[:, 1]
            to_t = torch.atan2(self.target[:, 1:2] - ey, self.target[:, 0:1] - ex)
            dx, dy = ex[:, :, None] - self.p[:, 0][:, None, :], ey[:, :, None] - self.p[:, 1][:, None, :]
            d = torch.sqrt(dx * dx + dy * dy)
            dmin, imin = d.min(-1)
            away = torch.atan2(torch.gather(dy, 2, imin[..., None])[..., 0], torch.gather(dx, 2, imin[..., None])[..., 0])
            cmd = torch.where(dmin <= self._kw["p_sen_range"], away, to_t) / math.pi
        self._cmd = torch.as_tensor(cmd, dtype=torch.float64, device=self.device).reshape(self.num_envs, self.e_num).contiguous()

    # ---- scripted pursuers (guidance.py) --------------------------------------------------------------------------
    def set_guidance(self, lead=1.0, sep_range=None, sep_gain=1.0):
        """the parameters of guidance_actions (runtime.guidance_lead / guidance_sep_range / guidance_sep_gain): the longest look-ahead in
        the environment's time units, the range inside which team-mates repel (None: 4 x kill_radius) and the weight of that repulsion"""
        g = N2nGuidanceParams()
        g.lead, g.sep_range, g.sep_gain = float(lead), float(4.0 * self.kill_radius if sep_range is None else sep_range), float(sep_gain)
        self.guidance = g

    def guidance_actions(self, out=None):
        """the scripted lead-pursuit action of every pursuer for the current state, (N, P) int32, what step() takes
        (n2n_pursuer_guidance, include/n2n_env.h; specification: tests/guidance_ref.py): one launch, nothing but `out` is written.
        out: a dense device tensor of that shape and type (None: the environment's own, allocated once)."""
        N, P = self.num_envs, self.p_num
        if out is None:
            if self._guidance_out is None:
                self._guidance_out = torch.zeros((N, P), dtype=torch.int32, device=self.device)
            out = self._guidance_out
        assert out.dtype == torch.int32 and out.is_contiguous() and tuple(out.shape) == (N, P) and out.device == self.p.device
        _check(self.L.n2n_pursuer_guidance(C.byref(self.c), C.byref(self.st), C.byref(self.guidance), C.c_void_p(out.data_ptr()), _stream()),
               "n2n_pursuer_guidance")
        return out

    def step(self, action):
        """:164-177 (preceded by the evader's move with the command of evader_step) -> (reward (N,P), done (N,), active (N,P))"""
        a = torch.as_tensor(action, device=self.device).to(torch.int32).reshape(self.num_envs, self.p_num).contiguous()
        ptr = lambda t: C.c_void_p(t.data_ptr())
        _check(self.L.n2n_env_tick(C.byref(self.c), C.byref(self.st), ptr(a), ptr(self._cmd), ptr(self.reward_t), ptr(self.active_t),
                                   ptr(self.done_t), C.byref(self._obs_struct), _stream()), "n2n_env_tick")
        self.time_step += 1
        return self.reward_t, self.done_t, self.active_t

    # ---- MAPPO on env_n2n (n2n_agent.py): one launch before the policy step, one after the tick ------------------------------------
    def new_accumulators(self):
        """zeroed per-environment episode accumulators for policy_record: done_before, ended, captured (uint8), return, length"""
        N, dev = self.num_envs, self.device
        u8 = lambda: torch.zeros(N, dtype=torch.uint8, device=dev)
        return dict(done_before=u8(), ended=u8(), captured=u8(), ret=torch.zeros(N, device=dev), length=torch.zeros(N, device=dev))

    def enable_reward_scaling(self):
        """allocates the RewardScaling state of a training environment (algo.use_reward_scaling): reward_scale (N, 1 + 3P) f64, per
        environment n, mean[P], S[P], R[P] (csrc/reward_scale.hpp); reset() zeroes R, the rest persists over episodes"""
        self.reward_scale = torch.zeros((self.num_envs, 1 + 3 * self.p_num), dtype=torch.float64, device=self.device)
        return self.reward_scale

    def enable_reward_shaping(self, coef):
        """allocates the shaping state of a training environment (algo.reward_shaping: distance): shaping_phi (N, P) f64, the
        potential -coef * (distance to the nearest active evader) of the state the next tick starts from (csrc/reward_shaping.hpp);
        shaping_begin() writes it at every episode start, so nothing of it outlives an episode"""
        self.shaping_coef = float(coef)
        self.shaping_phi = torch.zeros((self.num_envs, self.p_num), dtype=torch.float64, device=self.device)
        return self.shaping_phi

    def shaping_begin(self):
        """after reset(): shaping_phi = the potential of the initial state (n2n_shaping_begin, one launch)"""
        if self.shaping_phi is None:
            raise RuntimeError("shaping_begin() needs enable_reward_shaping() on this environment")
        _check(self.L.n2n_shaping_begin(C.byref(self.c), C.byref(self.st), C.c_void_p(self.shaping_phi.data_ptr()),
                                        C.c_double(self.shaping_coef), _stream()), "n2n_shaping_begin")

    def policy_inputs(self, p4, e4, e_ref, live, pp_adj, pe_adj, done_before=None):
        """the DHGN's fp32 inputs of the current state (n2n_policy_inputs, include/n2n_env.h): p4 (N,P,4), e4 (N,E,4), e_ref (N,4),
        live (N,P), pp_adj (N,P,P), pe_adj (N,P,E), each None (skipped) or a tensor with dense environment rows, e.g. buffer[:, t].
        done_before: the uint8 (N,) accumulator of policy_record (None: no environment is done)."""
        N, P, E = self.num_envs, self.p_num, self.e_num
        io = N2nPolicyIO()
        io.pp_in, io.pp_in_rs = self.obs["pp_adj"].data_ptr(), self.obs["pp_adj"].stride(0)
        io.pe_in, io.pe_in_rs = self.obs["pe_adj"].data_ptr(), self.obs["pe_adj"].stride(0)
        for k, t, shape in (("p4", p4, (N, P, 4)), ("e4", e4, (N, E, 4)), ("e_ref", e_ref, (N, 4)), ("live", live, (N, P)),
                            ("pp_adj", pp_adj, (N, P, P)), ("pe_adj", pe_adj, (N, P, E))):
            ptr, rs = rows(t, shape, k)
            setattr(io, k, ptr)
            setattr(io, k + "_rs", rs)
        if done_before is not None:
            assert done_before.dtype == torch.uint8 and done_before.is_contiguous() and done_before.shape == (N,)
        _check(self.L.n2n_policy_inputs(C.byref(self.c), C.byref(self.st), C.c_void_p(done_before.data_ptr() if done_before is not None else None),
                                        C.byref(io), _stream()), "n2n_policy_inputs")

    def policy_record(self, acc, live, value=None, r=None, active=None, v=None, v_next=None, scale_gamma=None, shaping_gamma=None,
                      team_coef=None):
        """after step(): r = reward * live, active = live, v = value * live (row t of the buffer, None skips), v_next (row t + 1 of v_n)
        zeroed where the pursuer is inactive or its episode ended for a reason other than the time limit; updates the accumulators
        of new_accumulators().  scale_gamma: the discount of the reference's RewardScaling; r is then the scaled reward * live and
        reward_scale (enable_reward_scaling) advances.  shaping_gamma: the discount of the distance shaping; the reward (what
        RewardScaling receives, when both are on) gains gamma Phi' - Phi on live rows and shaping_phi (enable_reward_shaping) advances.
        team_coef: alpha in [0, 1] of the team reward sharing; the reward that enters the row, the shaping and the scaling is
        (1 - alpha) reward + alpha (sum_p reward * live) on live rows; the accumulators keep the raw reward.  Whatever is asked for, it
        is one launch (n2n_policy_record, include/n2n_env.h; the options: include/policy_record.h)."""
        N, P = self.num_envs, self.p_num
        io = N2nRecordIO()
        for k, t in (("live", live), ("value", value), ("r", r), ("active", active), ("v", v), ("v_next", v_next)):
            ptr, rs = rows(t, (N, P), k)
            setattr(io, k, ptr)
            setattr(io, k + "_rs", rs)
        a = fill_acc(N2nPolicyAcc(), acc, N, self.p.device)
        opts = record_opts(self, scale_gamma, shaping_gamma, team_coef)
        _check(self.L.n2n_policy_record(C.byref(self.c), C.byref(self.st), C.c_void_p(self.reward_t.data_ptr()), C.c_void_p(self.done_t.data_ptr()),
                                        C.byref(io), C.byref(a), C.byref(opts) if opts is not None else None, _stream()), "n2n_policy_record")
