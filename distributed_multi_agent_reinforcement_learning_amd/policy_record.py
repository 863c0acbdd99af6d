"""What `ParticleEnv.policy_record` of env_3d and env_n2n share: the reward options record of include/policy_record.h and the argument
checks in front of the one entry point per library (e3d_policy_record, n2n_policy_record)."""
import ctypes as C

import torch


class PolicyRecordOpts(C.Structure):
    """policy_record_opts: rs / phi NULL and team 0 switch RewardScaling, distance shaping and team reward sharing off"""
    _fields_ = [("rs", C.c_void_p), ("phi", C.c_void_p), ("gamma", C.c_double), ("coef", C.c_double), ("alpha", C.c_double),
                ("team", C.c_int32), ("pad0", C.c_int32)]


ACC = (("done_before", torch.uint8), ("ended", torch.uint8), ("captured", torch.uint8), ("ret", torch.float32), ("length", torch.float32))


def rows(t, shape, name):
    """a float32 (N, ...) device tensor whose environment rows are dense (rows may be strided: buffer[:, t]) -> (pointer, row stride)"""
    if t is None:
        return None, 0
    assert t.dtype == torch.float32 and t.is_cuda and tuple(t.shape) == tuple(shape), (name, tuple(t.shape), tuple(shape))
    assert t[0].is_contiguous() and (t.shape[0] == 1 or t.stride(0) >= t[0].numel()), f"{name}: rows must be dense"
    return t.data_ptr(), t.stride(0)


def fill_acc(struct, acc, N, device):
    """the five accumulators of new_accumulators() into a *_policy_acc struct"""
    for k, dt in ACC:
        t = acc[k]
        assert t.dtype == dt and t.is_contiguous() and t.shape == (N,) and t.device == device, k
        setattr(struct, k, t.data_ptr())
    return struct


def record_opts(env, scale_gamma, shaping_gamma, team_coef):
    """the options of one policy_record call from the environment's states: None when all three are off"""
    if scale_gamma is None and shaping_gamma is None and team_coef is None:
        return None
    N, P, dev = env.num_envs, env.p_num, env.p.device
    rs_ptr, phi_ptr, gamma, coef = None, None, 0.0, 0.0
    if scale_gamma is not None:
        rs = env.reward_scale
        if rs is None:
            raise RuntimeError("policy_record(scale_gamma=...) needs enable_reward_scaling() on this environment")
        assert rs.dtype == torch.float64 and rs.is_contiguous() and rs.shape == (N, 1 + 3 * P) and rs.device == dev
        rs_ptr, gamma = rs.data_ptr(), float(scale_gamma)
    if shaping_gamma is not None:
        phi = env.shaping_phi
        if phi is None:
            raise RuntimeError("policy_record(shaping_gamma=...) needs enable_reward_shaping() on this environment")
        if scale_gamma is not None and float(scale_gamma) != float(shaping_gamma):
            raise ValueError("policy_record: scale_gamma and shaping_gamma are one discount (algo.gamma)")
        assert phi.dtype == torch.float64 and phi.is_contiguous() and phi.shape == (N, P) and phi.device == dev
        phi_ptr, gamma, coef = phi.data_ptr(), float(shaping_gamma), env.shaping_coef
    if team_coef is None:
        return PolicyRecordOpts(rs_ptr, phi_ptr, gamma, coef)
    return PolicyRecordOpts(rs_ptr, phi_ptr, gamma, coef, float(team_coef), 1)
