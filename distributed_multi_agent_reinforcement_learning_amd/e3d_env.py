"""`ParticleEnv` (env_3d): the reference's continuous 3-D pursuit environment batched on the GPU.

Mirrors environment/env_3d/particle_env.py:76-404 of the reference for N independent environments: `initialize`, `reset`,
`evader_step`, `step`, `get_team_state`, `get_adj_mat`, `get_active` keep their names; tensors carry a leading environment
dimension.  Pursuer actions are continuous, a in [-1, 1]^3 (heading, pitch, speed; Point.step :25-55).  Kinematics / reward /
culling / done run in csrc/e3d_env.hip (C ABI include/e3d_env.h), the reset in the same library's host part with a replica
of numpy's legacy generator per environment.  The reference's evader is driven by scipy's SLSQP (eva.py:87-148): here its
command is an input (`evader_step(cmd)`), or, when none is given, either a closed-form rule (head for the target at full
speed; `evader="rule"`, the default) or the reference's optimiser itself, Kraft's SLSQP on the GPU (`evader="slsqp"`,
e3d_evader_slsqp in the same library).
"""
import ctypes as C
import math
import os

import numpy as np
import torch

from . import build as _build
from .policy_record import fill_acc, record_opts, rows


class E3dConfig(C.Structure):
    _fields_ = [("P", C.c_int32), ("max_step", C.c_int32)] + \
               [(n, C.c_double) for n in ("p_vmax", "e_vmax", "p_sen_range", "p_comm_range", "kill_radius", "ang_lmt", "v_lmt", "step_size")]


class E3dState(C.Structure):
    _fields_ = [("N", C.c_int32), ("pad0", C.c_int32)] + [(n, C.c_void_p) for n in ("p", "e", "target", "time_step")]


class E3dObsOut(C.Structure):
    _fields_ = [("p_state", C.c_void_p), ("p_state_stride", C.c_int64), ("e_state", C.c_void_p), ("e_state_stride", C.c_int64),
                ("pp_adj", C.c_void_p), ("pp_adj_stride", C.c_int64), ("pe_adj", C.c_void_p), ("pe_adj_stride", C.c_int64)]


class E3dGuidanceParams(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("lead", "sep_range", "sep_gain")]


class E3dPolicyAcc(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("done_before", "ended", "captured", "ret", "length")]


class E3dRecordIO(C.Structure):
    _fields_ = [(n, t) for k in ("live", "value", "r", "active", "v", "v_next", "live_next") for n, t in ((k, C.c_void_p), (k + "_rs", C.c_int64))]


_lib = None


def load_library():
    global _lib
    if _lib is None:
        path = _build.lib_path("libe3d_env.so")
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: build it with __graft_entry__.build(); env_3d has no CPU fallback")
        L = C.CDLL(path)
        vp = C.c_void_p
        L.e3d_config_check.argtypes = [vp]
        L.e3d_env_load.argtypes = [vp] * 6
        L.e3d_env_observe.argtypes = [vp] * 4
        L.e3d_env_tick.argtypes = [vp] * 9
        L.e3d_resetter_create.argtypes = [vp, C.c_int32, vp]
        L.e3d_resetter_create.restype = vp
        L.e3d_resetter_destroy.argtypes = [vp]
        L.e3d_evader_slsqp.argtypes = [vp] * 4
        L.e3d_evader_slsqp_nit.argtypes = [vp] * 5
        L.e3d_evader_slsqp_host.argtypes = [vp, C.c_int32] + [vp] * 5
        L.e3d_resetter_reset.argtypes = [vp, vp, vp, vp, C.c_int32]
        L.e3d_resetter_state_bytes.argtypes = [vp]
        L.e3d_resetter_state_bytes.restype = C.c_int64
        L.e3d_resetter_get_state.argtypes = [vp, vp]
        L.e3d_resetter_set_state.argtypes = [vp, vp]
        L.e3d_policy_features.argtypes = [vp] * 6
        L.e3d_policy_features_norm.argtypes = [vp] * 6 + [C.c_double, vp, C.c_int64, vp, vp]
        L.e3d_obs_norm_slots.argtypes = [C.c_int64]
        L.e3d_obs_norm_slots.restype = C.c_int64
        L.e3d_obs_norm_reduce.argtypes = [vp, C.c_int64, vp, vp]
        L.e3d_obs_norm_update.argtypes = [vp, vp, vp, C.c_int64, vp]
        L.e3d_policy_record.argtypes = [vp] * 8
        L.e3d_shaping_begin.argtypes = [vp] * 3 + [C.c_double, vp]
        L.e3d_pursuer_guidance.argtypes = [vp] * 5
        L.e3d_pursuit_features.argtypes = [vp] * 3 + [C.c_int32] + [vp] * 3
        L.e3d_pursuit_features_host.argtypes = [vp, C.c_int32] + [vp] * 6 + [C.c_int32, vp, vp]
        L.e3d_central_features.argtypes = [vp] * 3 + [C.c_int32] + [vp] * 3
        L.e3d_central_features_host.argtypes = [vp, C.c_int32] + [vp] * 6 + [C.c_int32, vp, vp]
        L.gauss_direction_map_host.argtypes = [C.c_int32, vp, vp]
        L.e3d_direction_label_host.argtypes = [C.c_int32, vp, vp]
        _lib = L
    return _lib


def _check(rc, what):
    if rc != 0:
        extra = " (no pursuer placement within E3D_RESET_MAX_DRAWS draws: too many pursuers for the 10^3 box at distance 4)" if rc == 40003 else ""
        raise RuntimeError(f"{what} failed with code {rc}{extra}")


PURSUIT_FEAT = 32                              # E3D_FEAT2: the columns of pursuit_features
EVADER_OBS = ("sensed", "team", "global")      # E3D_EVADER_OBS_SENSED / _TEAM / _GLOBAL = the index
CENTRAL_MATE = 8                               # E3D_CENTRAL_MATE: the columns of one team-mate's slot in central_features' critic row
CENTRAL_MAX_P = 16                             # E3D_CENTRAL_MAX_P


def central_feat(P):
    """E3D_CENTRAL_FEAT(P): the columns of central_features' critic row, the 32 of pursuit_features and a slot per team-mate"""
    return PURSUIT_FEAT + CENTRAL_MATE * (P - 1)


def evader_obs_code(name):
    """the ABI's code of an evader_obs mode given by name; ValueError for a name that is none of EVADER_OBS"""
    if name not in EVADER_OBS:
        raise ValueError(f"evader_obs: {name!r} is not one of {EVADER_OBS}")
    return EVADER_OBS.index(name)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class ParticleEnv:
    """cfg values are the reference's hard-coded defaults (particle_env.py:78-121)."""

    def __init__(self, num_envs=1, seeds=None, device="cuda", p_vmax=0.7, e_vmax=1.0, p_sen_range=3.0, p_comm_range=6.0, kill_radius=0.5,
                 ang_lmt=math.pi / 4, v_lmt=0.4, step_size=0.5, max_step=200, evader="rule"):
        if evader not in ("rule", "slsqp"):
            raise ValueError(f"evader must be 'rule' or 'slsqp', not {evader!r}")
        self.evader = evader
        self.L = load_library()
        if not torch.cuda.is_available():
            raise RuntimeError("ParticleEnv needs a GPU (MI355X); there is no CPU path")
        self.num_envs = int(num_envs)
        self.device = torch.device(device)
        self.seeds = list(seeds) if seeds is not None else list(range(self.num_envs))
        self.p_obs_dim = self.e_obs_dim = 6
        self.state_dim, self.action_dim = 12, 3
        self.env_name = "ParticleEnvBoundGra"
        self.max_step, self.step_size, self.kill_radius = max_step, step_size, kill_radius
        self._kw = dict(p_vmax=p_vmax, e_vmax=e_vmax, p_sen_range=p_sen_range, p_comm_range=p_comm_range, kill_radius=kill_radius,
                        ang_lmt=ang_lmt, v_lmt=v_lmt, step_size=step_size)
        self.time_step = 0
        self.n_episode = 0
        self.p_num = None
        self.e_num = 1
        self.resetter = None
        self.reward_scale = None
        self.shaping_phi, self.shaping_coef = None, None
        self._guidance_out = None
        self.set_guidance()   # the scripted pursuers' defaults

    def initialize(self, p_num):
        """particle_env.py:133-135, plus the allocation of the device records"""
        self.p_num = int(p_num)
        c = E3dConfig()
        c.P, c.max_step = self.p_num, self.max_step
        for k, v in self._kw.items():
            setattr(c, k, v)
        _check(self.L.e3d_config_check(C.byref(c)), "e3d_config_check")
        self.c = c
        N, dev, P = self.num_envs, self.device, self.p_num
        self.p = torch.zeros((N, 7, P), dtype=torch.float64, device=dev)
        self.e = torch.zeros((N, 7), dtype=torch.float64, device=dev)
        self.target = torch.zeros((N, 3), dtype=torch.float64, device=dev)
        self.t_dev = torch.zeros((N,), dtype=torch.int32, device=dev)
        self.st = E3dState()
        self.st.N = N
        self.st.p, self.st.e, self.st.target, self.st.time_step = self.p.data_ptr(), self.e.data_ptr(), self.target.data_ptr(), self.t_dev.data_ptr()
        f = lambda *s: torch.zeros((N, *s), dtype=torch.float32, device=dev)
        self.obs = dict(p_state=f(P, 6), e_state=f(1, 6), pp_adj=f(P, P), pe_adj=f(P, 1))
        self.reward_t = f(P)
        self.active_t = torch.ones((N, P), dtype=torch.uint8, device=dev)
        self.done_t = torch.zeros((N,), dtype=torch.uint8, device=dev)
        self._cmd_slsqp = torch.zeros((N, 3), dtype=torch.float64, device=dev)  # the kernel's own output buffer
        s = np.ascontiguousarray(self.seeds, np.uint32)
        self.resetter = self.L.e3d_resetter_create(C.byref(c), N, s.ctypes.data_as(C.c_void_p))
        if not self.resetter:
            raise RuntimeError("e3d_resetter_create failed (bad configuration or out of memory)")
        self._obs_struct = E3dObsOut()
        for k, t in self.obs.items():
            setattr(self._obs_struct, k, t.data_ptr())
            setattr(self._obs_struct, k + "_stride", t.stride(0))

    def __del__(self):
        try:
            if self.resetter:
                self.L.e3d_resetter_destroy(self.resetter)
        except Exception:
            pass

    def reset(self, init=None):
        """particle_env.py:137-203.  init = (p [N,P,7], e [N,7], target [N,3]) injects recorded initial conditions."""
        N = self.num_envs
        if init is None:
            p = np.empty((N, self.p_num, 7)); e = np.empty((N, 7)); tg = np.empty((N, 3))
            _check(self.L.e3d_resetter_reset(self.resetter, p.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p),
                                             tg.ctypes.data_as(C.c_void_p), min(16, os.cpu_count() or 1)), "e3d_resetter_reset")
        else:
            p, e, tg = (np.ascontiguousarray(a, np.float64) for a in init)
            e = e.reshape(N, 7)
        self.last_init = (p, e, tg)
        _check(self.L.e3d_env_load(C.byref(self.c), C.byref(self.st), p.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p),
                                   tg.ctypes.data_as(C.c_void_p), _stream()), "e3d_env_load")
        torch.cuda.current_stream().synchronize()
        self.time_step = 0
        self.n_episode += 1
        self._cmd = torch.zeros((N, 3), dtype=torch.float64, device=self.device)
        self.active_t.fill_(1)
        if self.reward_scale is not None:
            self.reward_scale[:, 1 + 2 * self.p_num:].zero_()   # RewardScaling.reset: R; n, mean, S persist
        self.observe()

    def get_resetter_state(self):
        """the reset generators of every environment (include/e3d_env.h e3d_resetter_get_state) as a uint8 array"""
        buf = np.empty(self.L.e3d_resetter_state_bytes(self.resetter), np.uint8)
        _check(self.L.e3d_resetter_get_state(self.resetter, buf.ctypes.data_as(C.c_void_p)), "e3d_resetter_get_state")
        return buf

    def set_resetter_state(self, blob):
        """restores get_resetter_state(); ValueError when the blob comes from another number of environments / agents"""
        buf = np.ascontiguousarray(blob, np.uint8)
        if buf.size != self.L.e3d_resetter_state_bytes(self.resetter):
            raise ValueError("resetter state does not match this number of environments")
        rc = self.L.e3d_resetter_set_state(self.resetter, buf.ctypes.data_as(C.c_void_p))
        if rc != 0:
            raise ValueError(f"resetter state does not match this configuration (e3d_resetter_set_state code {rc})")

    def observe(self):
        _check(self.L.e3d_env_observe(C.byref(self.c), C.byref(self.st), C.byref(self._obs_struct), _stream()), "e3d_env_observe")
        return self.obs

    def get_team_state(self, is_pursuer, rules=False):
        """(N, A, 6) [x, y, z, phi, gamma, v] of every agent (the reference's rules=False form, :258-265)"""
        return self.obs["p_state"] if is_pursuer else self.obs["e_state"]

    def get_adj_mat(self, which="pp"):
        """:328-340 with the pursuers as observers: 'pp' (communication range) or 'pe' (sensing range)"""
        return self.obs["pp_adj" if which == "pp" else "pe_adj"]

    def get_active(self):
        return self.active_t

    def evader_step(self, cmd=None, nit=None):
        """Sets the evader's command (heading, pitch, speed) in [-1, 1]^3 for the next step (the reference computes it with
        SLSQP, :354-378).  Without `cmd`, evader="rule": full speed straight at the target; evader="slsqp": the reference's
        SLSQP evader, launched on the current stream without a host synchronisation (it can be captured in a graph).  nit, an
        int32 (N,) device tensor, receives the SLSQP iterations taken per environment."""
        if cmd is None and self.evader == "slsqp":
            ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None else None)
            if nit is not None:
                assert nit.dtype == torch.int32 and nit.is_contiguous() and nit.numel() == self.num_envs
            _check(self.L.e3d_evader_slsqp_nit(C.byref(self.c), C.byref(self.st), ptr(self._cmd_slsqp), ptr(nit), _stream()),
                   "e3d_evader_slsqp")
            self._cmd = self._cmd_slsqp
            return
        if cmd is None:
            d = self.target - self.e[:, :3]
            cmd = torch.stack((torch.atan2(d[:, 1], d[:, 0]) / math.pi, torch.atan2(d[:, 2], torch.hypot(d[:, 0], d[:, 1])) / (math.pi / 2),
                               torch.ones_like(d[:, 0])), -1)
        self._cmd = torch.as_tensor(cmd, dtype=torch.float64, device=self.device).reshape(self.num_envs, 3).contiguous()

    def policy_features(self, actor_feat, critic_feat, norm_state=None, clip=None, live=None, slots=None):
        """the trainer's (N, P, 16) fp32 features of the current state into the two dense tensors (e3d_policy_features,
        include/e3d_env.h): the actor's from its sensed evader and communication neighbours, the critic's from the whole state.
        norm_state (algo.use_obs_norm): the (2, 33) f64 state of obs_norm.ObsNorm; the features are then written normalised under it
        and clipped to +-clip (e3d_policy_features_norm; rows of inactive pursuers stay 0), and, with slots (ObsNorm.slots_for(N P)),
        the same launch adds the sums of the raw features over the rows of the (N, P) mask `live` to them."""
        for t in (actor_feat, critic_feat):
            assert t.dtype == torch.float32 and t.is_contiguous() and t.shape == (self.num_envs, self.p_num, 16) and t.device == self.p.device
        if norm_state is None:
            assert clip is None and live is None and slots is None, "clip, live and slots belong to norm_state"
            _check(self.L.e3d_policy_features(C.byref(self.c), C.byref(self.st), C.byref(self._obs_struct), C.c_void_p(actor_feat.data_ptr()),
                                              C.c_void_p(critic_feat.data_ptr()), _stream()), "e3d_policy_features")
            return actor_feat, critic_feat
        N, P = self.num_envs, self.p_num
        assert norm_state.dtype == torch.float64 and norm_state.is_contiguous() and norm_state.shape == (2, 33) and norm_state.device == self.p.device
        live_ptr, live_rs, slots_ptr = None, 0, None
        if slots is not None:
            n = self.L.e3d_obs_norm_slots(N * P)
            assert slots.dtype == torch.float64 and slots.is_contiguous() and slots.shape == (n, 2, 33) and slots.device == self.p.device
            if live is None:
                raise ValueError("policy_features(slots=...) needs the live mask of the step")
            live_ptr, live_rs = rows(live, (N, P), "live")
            slots_ptr = slots.data_ptr()
        _check(self.L.e3d_policy_features_norm(C.byref(self.c), C.byref(self.st), C.byref(self._obs_struct), C.c_void_p(actor_feat.data_ptr()),
                                               C.c_void_p(critic_feat.data_ptr()), C.c_void_p(norm_state.data_ptr()), C.c_double(float(clip)),
                                               C.c_void_p(live_ptr), C.c_int64(live_rs), C.c_void_p(slots_ptr), _stream()),
               "e3d_policy_features_norm")
        return actor_feat, critic_feat

    def pursuit_features(self, actor_feat, critic_feat, evader_obs="sensed"):
        """the (N, P, 32) fp32 line-of-sight features of the current state into the two dense tensors (algo.e3d_features: pursuit;
        e3d_pursuit_features, include/e3d_env.h; specification: tests/e3d_features_ref.py): own position, heading and speed, the evader
        as direction, range, velocity, closing speed and target offset, the nearest two visible team-mates, the clock.  evader_obs
        says when the ACTOR knows the evader: "sensed" (pe_adj, the rule of policy_features), "team" (some pursuer of its communication
        component senses it) or "global" (always); the critic always does.  One launch; nothing but the two tensors is written."""
        code = evader_obs_code(evader_obs)
        for t in (actor_feat, critic_feat):
            assert t.dtype == torch.float32 and t.is_contiguous() and t.shape == (self.num_envs, self.p_num, PURSUIT_FEAT) and t.device == self.p.device
        _check(self.L.e3d_pursuit_features(C.byref(self.c), C.byref(self.st), C.byref(self._obs_struct), C.c_int32(code),
                                           C.c_void_p(actor_feat.data_ptr()), C.c_void_p(critic_feat.data_ptr()), _stream()), "e3d_pursuit_features")
        return actor_feat, critic_feat

    def central_features(self, actor_feat, critic_feat, evader_obs="sensed"):
        """pursuit_features with the centralised critic row (algo.e3d_critic: central; e3d_central_features, include/e3d_env.h;
        specification: tests/central_critic_ref.py): actor_feat (N, P, 32) is what pursuit_features writes; critic_feat is
        (N, P, central_feat(P)), the 32 critic columns and then, for every active team-mate in the order of distance, its direction,
        range, heading and speed (8 columns; slots past the last team-mate are zero).  P <= CENTRAL_MAX_P.  One launch; nothing but
        the two tensors is written."""
        code = evader_obs_code(evader_obs)
        for t, width in ((actor_feat, PURSUIT_FEAT), (critic_feat, central_feat(self.p_num))):
            assert t.dtype == torch.float32 and t.is_contiguous() and t.shape == (self.num_envs, self.p_num, width) and t.device == self.p.device
        _check(self.L.e3d_central_features(C.byref(self.c), C.byref(self.st), C.byref(self._obs_struct), C.c_int32(code),
                                           C.c_void_p(actor_feat.data_ptr()), C.c_void_p(critic_feat.data_ptr()), _stream()), "e3d_central_features")
        return actor_feat, critic_feat

    # ---- MAPPO on env_3d (e3d_agent.py): the bookkeeping of one lockstep tick, one launch after step() ------------------------------
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
        potential -coef * |pursuer - evader| of the state the next tick starts from (csrc/reward_shaping.hpp); shaping_begin() writes
        it at every episode start, so nothing of it outlives an episode"""
        self.shaping_coef = float(coef)
        self.shaping_phi = torch.zeros((self.num_envs, self.p_num), dtype=torch.float64, device=self.device)
        return self.shaping_phi

    def shaping_begin(self):
        """after reset(): shaping_phi = the potential of the initial state (e3d_shaping_begin, one launch)"""
        if self.shaping_phi is None:
            raise RuntimeError("shaping_begin() needs enable_reward_shaping() on this environment")
        _check(self.L.e3d_shaping_begin(C.byref(self.c), C.byref(self.st), C.c_void_p(self.shaping_phi.data_ptr()),
                                        C.c_double(self.shaping_coef), _stream()), "e3d_shaping_begin")

    def policy_record(self, acc, live, value=None, r=None, active=None, v=None, v_next=None, live_next=None, scale_gamma=None,
                      shaping_gamma=None, team_coef=None):
        """after step(): r = reward * live, active = live, v = value * live (row t of the buffer, None skips), v_next (row t + 1 of v_n)
        zeroed where the pursuer is inactive or its episode ended for a reason other than the time limit, live_next = the next step's
        live mask (may be `live` itself); updates the accumulators of new_accumulators().  scale_gamma: the discount of the reference's
        RewardScaling; r is then the scaled reward * live and reward_scale (enable_reward_scaling) advances.  shaping_gamma: the discount
        of the distance shaping; the reward (what RewardScaling receives, when both are on) gains gamma Phi' - Phi on live rows and
        shaping_phi (enable_reward_shaping) advances.  team_coef: alpha in [0, 1] of the team reward sharing; the reward that enters the
        row, the shaping and the scaling is (1 - alpha) reward + alpha (sum_p reward * live) on live rows; the accumulators keep the raw
        reward.  Whatever is asked for, it is one launch (e3d_policy_record, include/e3d_env.h; the options: include/policy_record.h)."""
        N, P = self.num_envs, self.p_num
        io = E3dRecordIO()
        for k, t in (("live", live), ("value", value), ("r", r), ("active", active), ("v", v), ("v_next", v_next), ("live_next", live_next)):
            ptr, rs = rows(t, (N, P), k)
            setattr(io, k, ptr)
            setattr(io, k + "_rs", rs)
        a = fill_acc(E3dPolicyAcc(), acc, N, self.p.device)
        opts = record_opts(self, scale_gamma, shaping_gamma, team_coef)
        _check(self.L.e3d_policy_record(C.byref(self.c), C.byref(self.st), C.c_void_p(self.reward_t.data_ptr()), C.c_void_p(self.done_t.data_ptr()),
                                        C.byref(io), C.byref(a), C.byref(opts) if opts is not None else None, _stream()), "e3d_policy_record")

    # ---- scripted pursuers (guidance.py) --------------------------------------------------------------------------
    def set_guidance(self, lead=1.0, sep_range=None, sep_gain=1.0):
        """the parameters of guidance_actions (runtime.guidance_lead / guidance_sep_range / guidance_sep_gain): the longest look-ahead in
        the environment's time units, the range inside which team-mates repel (None: 4 x kill_radius) and the weight of that repulsion"""
        g = E3dGuidanceParams()
        g.lead, g.sep_range, g.sep_gain = float(lead), float(4.0 * self.kill_radius if sep_range is None else sep_range), float(sep_gain)
        self.guidance = g

    def guidance_actions(self, out=None):
        """the scripted lead-pursuit action of every pursuer for the current state, (N, P, 3) f64, what step() takes
        (e3d_pursuer_guidance, include/e3d_env.h; specification: tests/guidance_ref.py): one launch, nothing but `out` is written.
        out: a dense device tensor of that shape and type (None: the environment's own, allocated once)."""
        N, P = self.num_envs, self.p_num
        if out is None:
            if self._guidance_out is None:
                self._guidance_out = torch.zeros((N, P, 3), dtype=torch.float64, device=self.device)
            out = self._guidance_out
        assert out.dtype == torch.float64 and out.is_contiguous() and tuple(out.shape) == (N, P, 3) and out.device == self.p.device
        _check(self.L.e3d_pursuer_guidance(C.byref(self.c), C.byref(self.st), C.byref(self.guidance), C.c_void_p(out.data_ptr()), _stream()),
               "e3d_pursuer_guidance")
        return out

    def step(self, action):
        """:205-219 (preceded by the evader's move with the command of evader_step) -> (reward (N,P), done (N,), active (N,P));
        action (N, P, 3) in [-1, 1]"""
        a = torch.as_tensor(action, device=self.device).to(torch.float64).reshape(self.num_envs, self.p_num, 3).contiguous()
        ptr = lambda t: C.c_void_p(t.data_ptr())
        _check(self.L.e3d_env_tick(C.byref(self.c), C.byref(self.st), ptr(a), ptr(self._cmd), ptr(self.reward_t), ptr(self.active_t),
                                   ptr(self.done_t), C.byref(self._obs_struct), _stream()), "e3d_env_tick")
        self.time_step += 1
        return self.reward_t, self.done_t, self.active_t
