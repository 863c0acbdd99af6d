"""ctypes binding of libpe_env.so (include/pe_env.h) plus the device-resident batched environment.

PyTorch is used for device memory and streams only; the simulation runs in the HIP kernels of csrc/pe_env.hip.
There is no CPU path: importing works anywhere, but constructing a `BatchedEnv` without the built library or a
GPU raises.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import build as _build
from . import tables

MAX_BEAMS = 64
META_INTS = 8
META_T, META_PATH_LEN, META_TAPE_POS, META_COLLISION, META_PATH_CNT, META_ASTAR_EXP, META_STATUS = range(7)


class PeConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("W", "H", "P", "O", "max_steps", "difficulty", "extend_dis", "num_beams",
                                          "lidar_radius", "evader_view", "tape_len", "max_path", "use_reward_norm",
                                          "pad0")] + \
               [(n, C.c_double) for n in ("def_tau", "def_dt", "def_collision_radius", "def_comm_range", "def_sen_range",
                                          "eva_vmax", "eva_tau", "eva_dt", "eva_collision_radius", "resolution")] + \
               [("action_u", (C.c_double * 2) * 9), ("beam_dir", (C.c_double * 2) * MAX_BEAMS)]


class PeState(C.Structure):
    _fields_ = [("N", C.c_int32), ("pad0", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("grid", "bidx", "n_obs", "def_", "eva", "target", "tape", "meta", "path", "rn", "wpw", "raser")]


class PeObsOut(C.Structure):
    _fields_ = [("p_state", C.c_void_p), ("p_state_stride", C.c_int64), ("e_state", C.c_void_p), ("e_state_stride", C.c_int64),
                ("p_adj", C.c_void_p), ("p_adj_stride", C.c_int64), ("e_adj", C.c_void_p), ("e_adj_stride", C.c_int64),
                ("o_adj", C.c_void_p), ("o_adj_stride", C.c_int64), ("o_adj_bits", C.c_void_p), ("o_adj_bits_stride", C.c_int64)]


class PeStepOut(C.Structure):
    _fields_ = [("reward", C.c_void_p), ("reward_stride", C.c_int64), ("reward_raw", C.c_void_p),
                ("reward_raw_stride", C.c_int64), ("done", C.c_void_p)]


class PeHostInit(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("grid", "obs_xy", "n_obs", "def_", "eva", "target", "tape")] + \
               [("reset_rn", C.c_int32), ("pad0", C.c_int32)]


class PeResetParams(C.Structure):
    _fields_ = [("num_blocks", C.c_int32), ("min_dist", C.c_int32), ("center", C.c_double * 2), ("variance", C.c_double),
                ("fixed_grid", C.c_void_p)]


class PeHostInitOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("grid", "obs_xy", "n_obs", "def_", "eva", "target", "tape")]


class PeLaunchPlan(C.Structure):
    """include/pe_env_diag.h pe_launch_plan"""
    _fields_ = [(n, C.c_int32) for n in ("wpb", "lds_per_env", "lds_bytes", "needs_attr", "fast8", "rw_shift")] + \
               [("o4_magic", C.c_uint32)] + [(n, C.c_int32) for n in ("one_load", "grid_copy", "tape_loop")] + \
               [(n, C.c_double) for n in ("inv_def_tau", "inv_eva_tau", "inv_six")]


class PePathfinderParams(C.Structure):
    """include/pe_env.h pe_pathfinder_params"""
    _fields_ = [("lead", C.c_double), ("sep_range", C.c_double), ("clearance", C.c_int32), ("pad0", C.c_int32)]


class PePathfinderDiag(C.Structure):
    """include/pe_env.h pe_pathfinder_diag"""
    _fields_ = [("field", C.c_void_p), ("kstar", C.c_void_p), ("blocked", C.c_void_p)]


class PePathfinderCache(C.Structure):
    """include/pe_env.h pe_pathfinder_cache"""
    _fields_ = [("field", C.c_void_p), ("key", C.c_void_p), ("hits", C.c_void_p)]


class PePathfinderLabel(C.Structure):
    """include/pe_env.h pe_pathfinder_label"""
    _fields_ = [("follow", C.c_void_p), ("action", C.c_void_p), ("a_star", C.c_void_p), ("a_star_env_stride", C.c_int64)]


class PePathfinderTrace(C.Structure):
    """include/pe_env.h pe_pathfinder_trace"""
    _fields_ = [("def_", C.c_void_p), ("def_env_stride", C.c_int64), ("def_tick_stride", C.c_int64),
                ("eva", C.c_void_p), ("eva_env_stride", C.c_int64), ("eva_tick_stride", C.c_int64), ("T", C.c_int32), ("pad0", C.c_int32)]


PATH_MAX_CELLS = 8192
PATH_UNREACHED = 0x7FFFFFFF
STATUS_PATH_CAP = 16


def pathfinder_params(pe_cfg, lead=None, sep_range=None, clearance=None):
    """the pathfinder's parameters with the defaults of include/pe_env.h (lead 0.5, sep_range 2 collision radii, clearance 10)"""
    p = PePathfinderParams()
    p.lead = 0.5 if lead is None else float(lead)
    p.sep_range = 2.0 * pe_cfg.def_collision_radius if sep_range is None else float(sep_range)
    p.clearance = 10 if clearance is None else int(clearance)
    return p


def pathfinder_host(pe_cfg, grid, defs, eva, lead=None, sep_range=None, clearance=None, diag=False):
    """pe_pursuer_pathfinder_host on host arrays laid out like the device records: grid (N, W*H) u8, defs (N, 4, P) f64, eva (N, 4) f64.
    Returns the (N, P) int32 actions, with diag=True also a dict of field (N, W*H) i32, kstar (N, P) i32, blocked (N, P) u16."""
    L = load_library()
    c = pe_cfg
    g = np.ascontiguousarray(grid, np.uint8).reshape(-1, c.W * c.H)
    N = g.shape[0]
    d = np.ascontiguousarray(defs, np.float64).reshape(N, 4, c.P)
    e = np.ascontiguousarray(eva, np.float64).reshape(N, 4)
    prm = pathfinder_params(c, lead, sep_range, clearance)
    actions = np.full((N, c.P), -1, np.int32)
    dg, out = PePathfinderDiag(), None
    if diag:
        out = dict(field=np.zeros((N, c.W * c.H), np.int32), kstar=np.zeros((N, c.P), np.int32), blocked=np.zeros((N, c.P), np.uint16))
        dg.field, dg.kstar, dg.blocked = _np(out["field"]), _np(out["kstar"]), _np(out["blocked"])
    _check(L.pe_pursuer_pathfinder_host(C.byref(c), N, _np(g), _np(d), _np(e), C.byref(prm), _np(actions), C.byref(dg) if diag else None),
           "pe_pursuer_pathfinder_host")
    return (actions, out) if diag else actions


def pathfinder_teach_host(pe_cfg, grid, defs, eva, cache=None, follow=None, action=None, a_star=None, lead=None, sep_range=None, clearance=None,
                          diag=False):
    """pe_pursuer_pathfinder_teach_host on host arrays laid out like pathfinder_host's.  cache: a dict of field (N, W*H) i32, key (N, 2)
    i32 and optionally hits (N,) i32, updated in place; follow (N,) u8 and action (N, P) i32 (in/out); a_star: a float32 array or row
    view whose first axis is the environment and whose last P elements per environment are contiguous.  Returns like pathfinder_host."""
    L = load_library()
    c = pe_cfg
    g = np.ascontiguousarray(grid, np.uint8).reshape(-1, c.W * c.H)
    N = g.shape[0]
    d = np.ascontiguousarray(defs, np.float64).reshape(N, 4, c.P)
    e = np.ascontiguousarray(eva, np.float64).reshape(N, 4)
    prm = pathfinder_params(c, lead, sep_range, clearance)
    actions = np.full((N, c.P), -1, np.int32)
    ca, lb = PePathfinderCache(), PePathfinderLabel()
    if cache is not None:
        for k in ("field", "key", "hits"):
            if cache.get(k) is not None:
                assert cache[k].dtype == np.int32 and cache[k].flags.c_contiguous, k
                setattr(ca, k, _np(cache[k]))
    for k, a, dt in (("follow", follow, np.uint8), ("action", action, np.int32)):
        if a is not None:
            assert a.dtype == dt and a.flags.c_contiguous, k
            setattr(lb, k, _np(a))
    if a_star is not None:
        assert a_star.dtype == np.float32 and a_star.shape[0] == N and a_star.shape[-1] == c.P and a_star.strides[-1] == 4 and a_star.strides[0] % 4 == 0
        lb.a_star, lb.a_star_env_stride = _np(a_star), a_star.strides[0] // 4
    dg, out = PePathfinderDiag(), None
    if diag:
        out = dict(field=np.zeros((N, c.W * c.H), np.int32), kstar=np.zeros((N, c.P), np.int32), blocked=np.zeros((N, c.P), np.uint16))
        dg.field, dg.kstar, dg.blocked = _np(out["field"]), _np(out["kstar"]), _np(out["blocked"])
    _check(L.pe_pursuer_pathfinder_teach_host(C.byref(c), N, _np(g), _np(d), _np(e), C.byref(prm), C.byref(ca) if cache is not None else None,
                                              C.byref(lb), _np(actions), C.byref(dg) if diag else None), "pe_pursuer_pathfinder_teach_host")
    return (actions, out) if diag else actions


def _stride(shape, strides, axis, record):
    """the element stride of `axis`, or one record where the axis has a single entry (its stride then addresses nothing)"""
    return int(strides[axis]) if shape[axis] > 1 else int(record)


def _trace_struct(P, ptr, def_, eva, def_strides, eva_strides):
    """pe_pathfinder_trace over def (N, T, 4, P) and eva (N, T, 4) views whose records are contiguous; strides in elements"""
    N, T = def_.shape[0], def_.shape[1]
    assert tuple(def_.shape) == (N, T, 4, P) and tuple(eva.shape) == (N, T, 4), "trace shapes"
    assert (P == 1 or def_strides[3] == 1) and def_strides[2] == P and eva_strides[2] == 1, "trace records must be contiguous"
    tr = PePathfinderTrace()
    tr.def_, tr.eva, tr.T = ptr(def_), ptr(eva), T
    tr.def_env_stride, tr.def_tick_stride = _stride(def_.shape, def_strides, 0, 4 * P * T), _stride(def_.shape, def_strides, 1, 4 * P)
    tr.eva_env_stride, tr.eva_tick_stride = _stride(eva.shape, eva_strides, 0, 4 * T), _stride(eva.shape, eva_strides, 1, 4)
    return tr


def record_state_host(pe_cfg, defs, eva, def_row, eva_row):
    """pe_env_record_state_host: defs (N, 4, P) and eva (N, 4) f64 copied into the rows def_row (N, 4, P) / eva_row (N, 4), float64 views
    (trace[:, t]) whose records are contiguous; the environment strides are taken from the views."""
    L = load_library()
    c = pe_cfg
    d = np.ascontiguousarray(defs, np.float64).reshape(-1, 4, c.P)
    N = d.shape[0]
    e = np.ascontiguousarray(eva, np.float64).reshape(N, 4)
    assert def_row.dtype == np.float64 and def_row.shape == (N, 4, c.P) and def_row.strides[1:] == (8 * c.P, 8) and def_row.strides[0] % 8 == 0
    assert eva_row.dtype == np.float64 and eva_row.shape == (N, 4) and eva_row.strides[1] == 8 and eva_row.strides[0] % 8 == 0
    _check(L.pe_env_record_state_host(C.byref(c), N, _np(d), _np(e), _np(def_row), _stride(def_row.shape, [v // 8 for v in def_row.strides], 0, 4 * c.P),
                                      _np(eva_row), _stride(eva_row.shape, [v // 8 for v in eva_row.strides], 0, 4)), "pe_env_record_state_host")


def pathfinder_label_episode_host(pe_cfg, grid, trace_def, trace_eva, a_star, builds=None, lead=None, sep_range=None, clearance=None, diag=False):
    """pe_pathfinder_label_episode_host: grid (N, W*H) u8; trace_def (N, T, 4, P) / trace_eva (N, T, 4) f64 and a_star (N, T, P) f32 arrays
    or views with contiguous records, the strides are taken from the views; builds (N,) i32 or None.  Returns a_star, with diag=True also
    the last tick's dict of field / kstar / blocked."""
    L = load_library()
    c = pe_cfg
    g = np.ascontiguousarray(grid, np.uint8).reshape(-1, c.W * c.H)
    N = g.shape[0]
    assert trace_def.dtype == np.float64 and trace_eva.dtype == np.float64 and trace_def.shape[0] == N
    assert all(v % 8 == 0 for v in trace_def.strides + trace_eva.strides)
    tr = _trace_struct(c.P, _np, trace_def, trace_eva, [v // 8 for v in trace_def.strides], [v // 8 for v in trace_eva.strides])
    assert a_star.dtype == np.float32 and a_star.shape == (N, tr.T, c.P) and a_star.strides[2] == 4 and all(v % 4 == 0 for v in a_star.strides)
    if builds is not None:
        assert builds.dtype == np.int32 and builds.shape == (N,) and builds.flags.c_contiguous
    prm = pathfinder_params(c, lead, sep_range, clearance)
    dg, out = PePathfinderDiag(), None
    if diag:
        out = dict(field=np.zeros((N, c.W * c.H), np.int32), kstar=np.zeros((N, c.P), np.int32), blocked=np.zeros((N, c.P), np.uint16))
        dg.field, dg.kstar, dg.blocked = _np(out["field"]), _np(out["kstar"]), _np(out["blocked"])
    a_str = [v // 4 for v in a_star.strides]
    _check(L.pe_pathfinder_label_episode_host(C.byref(c), N, _np(g), C.byref(prm), C.byref(tr), _np(a_star), _stride(a_star.shape, a_str, 0, tr.T * c.P),
                                              _stride(a_star.shape, a_str, 1, c.P), _np(builds) if builds is not None else None,
                                              C.byref(dg) if diag else None), "pe_pathfinder_label_episode_host")
    return (a_star, out) if diag else a_star


FORM_STEP, FORM_OBS, FORM_EVA, FORM_REPLAN = 1, 2, 4, 8
# the launch form of every entry point (pe_env_diag.h); evader_step and tick also exist with FORM_REPLAN
FORMS = dict(observe=FORM_OBS, step=FORM_STEP, step_observe=FORM_STEP | FORM_OBS, evader_step=FORM_EVA, tick=FORM_STEP | FORM_OBS | FORM_EVA,
             evader_step_replan=FORM_EVA | FORM_REPLAN, tick_replan=FORM_STEP | FORM_OBS | FORM_EVA | FORM_REPLAN)


def launch_plan(pe_cfg, form):
    """What the launcher chooses for this configuration and launch form (host only, no GPU): a dict of pe_launch_plan's fields."""
    L = load_library()
    p = PeLaunchPlan()
    _check(L.pe_diag_launch_plan(C.byref(pe_cfg), int(FORMS.get(form, form)), C.byref(p)), "pe_diag_launch_plan")
    return {n: getattr(p, n) for n, _ in PeLaunchPlan._fields_}


EXPORTS = ("pe_config_check", "pe_tick_lds_bytes", "pe_env_load", "pe_env_observe", "pe_evader_step", "pe_env_step",
           "pe_env_demon", "pe_env_tick", "pe_env_step_observe", "pe_astar_batch", "pe_pursuer_pathfinder", "pe_pursuer_pathfinder_host",
           "pe_pursuer_pathfinder_teach", "pe_pursuer_pathfinder_teach_host", "pe_env_record_state", "pe_env_record_state_host",
           "pe_pathfinder_label_episode", "pe_pathfinder_label_episode_host", "pe_error_string")

_lib = None


def lib_path():
    return _build.lib_path("libpe_env.so")


def load_library():
    """Loads libpe_env.so; raises if it has not been built (no fallback exists)."""
    global _lib
    if _lib is None:
        path = lib_path()
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(hipcc --offload-arch=gfx950); the environment has no CPU fallback")
        L = C.CDLL(path)
        vp = C.c_void_p
        L.pe_config_check.argtypes = [vp]
        L.pe_tick_lds_bytes.argtypes = [vp, C.c_int32]
        L.pe_tick_lds_bytes.restype = C.c_int64
        L.pe_env_load.argtypes = [vp, vp, vp, vp]
        L.pe_env_observe.argtypes = [vp, vp, vp, vp]
        L.pe_evader_step.argtypes = [vp, vp, C.c_int32, vp]
        L.pe_env_step.argtypes = [vp, vp, vp, vp, vp]
        L.pe_env_demon.argtypes = [vp, vp, vp, vp, vp]
        L.pe_env_tick.argtypes = [vp, vp, vp, vp, vp, C.c_int32, vp]
        L.pe_env_step_observe.argtypes = [vp, vp, vp, vp, vp, vp]
        L.pe_astar_batch.argtypes = [C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp, C.c_int32, vp]
        L.pe_diag_norm2.argtypes = [C.c_int32, vp, vp, vp, C.c_double, C.c_double, vp]
        L.pe_diag_launch_plan.argtypes = [vp, C.c_int32, vp]
        L.pe_resetter_create.argtypes = [vp, vp, C.c_int32, vp]
        L.pe_resetter_create.restype = vp
        L.pe_resetter_destroy.argtypes = [vp]
        L.pe_resetter_reset.argtypes = [vp, vp, vp, C.c_int32]
        L.pe_resetter_state_bytes.argtypes = [vp]
        L.pe_resetter_state_bytes.restype = C.c_int64
        L.pe_resetter_get_state.argtypes = [vp, vp]
        L.pe_resetter_set_state.argtypes = [vp, vp]
        L.pe_reset_state_bytes.argtypes = [vp, C.c_int32]
        L.pe_reset_state_bytes.restype = C.c_int64
        L.pe_env_reset_seed.argtypes = [vp, C.c_int32, vp, vp, vp]
        L.pe_env_reset.argtypes = [vp, vp, vp, vp, C.c_int32, vp, C.c_int32, vp]
        L.pe_pursuer_pathfinder.argtypes = [vp, vp, vp, vp, vp, vp]
        L.pe_diag_pathfinder_sweeps.argtypes = [vp, vp, vp, vp, vp, vp]
        L.pe_pursuer_pathfinder_host.argtypes = [vp, C.c_int32, vp, vp, vp, vp, vp, vp]
        L.pe_pursuer_pathfinder_teach.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
        L.pe_pursuer_pathfinder_teach_host.argtypes = [vp, C.c_int32, vp, vp, vp, vp, vp, vp, vp, vp]
        L.pe_env_record_state.argtypes = [vp, vp, vp, C.c_int64, vp, C.c_int64, vp]
        L.pe_env_record_state_host.argtypes = [vp, C.c_int32, vp, vp, vp, C.c_int64, vp, C.c_int64]
        L.pe_pathfinder_label_episode.argtypes = [vp, vp, vp, vp, vp, C.c_int64, C.c_int64, vp, vp, vp]
        L.pe_pathfinder_label_episode_host.argtypes = [vp, C.c_int32, vp, vp, vp, vp, C.c_int64, C.c_int64, vp, vp]
        L.pe_error_string.argtypes = [C.c_int]
        L.pe_error_string.restype = C.c_char_p
        _lib = L
    return _lib


STATUS_NAMES = ((1, "target tape exhausted (raise runtime.tape_len)"), (2, "A* iteration cap reached"),
                (4, "stored path tail underflow (raise runtime.max_path)"),
                (8, "episode reset gave up: no valid placement after PE_RESET_MAX_DRAWS draws (map too crowded for this configuration)"),
                (16, "the pathfinder's distance field hit its sweep bound"))


def status_or(meta):
    """bitwise OR over environments of meta[:, PE_META_STATUS] as a 0-d device tensor (no host sync)"""
    st = meta[:, META_STATUS]
    shifts = torch.arange(len(STATUS_NAMES), device=st.device, dtype=st.dtype)
    flags = ((st[:, None] >> shifts) & 1).max(0).values
    return (flags << shifts).sum()


def status_text(bits):
    return "; ".join(n for b, n in STATUS_NAMES if int(bits) & b)


def raser_row_words(O):
    """include/pe_env.h PE_RASER_ROW_WORDS"""
    return (((O + 31) >> 5) + 3) & ~3


def _check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed: {load_library().pe_error_string(rc).decode()} (code {rc})")


def make_pe_config(cfg, tape_len=16, max_path=128):
    """Reference config sections (config.yaml:13-54) -> pe_config."""
    c = PeConfig()
    c.W, c.H = int(cfg.map.map_size[0]), int(cfg.map.map_size[1])
    c.P = int(cfg.env.num_defender)
    c.O = int(cfg.map.num_max_obstacle)
    c.max_steps = int(cfg.env.max_steps)
    c.difficulty = int(cfg.env.difficulty)
    c.extend_dis = int(cfg.attacker.extend_dis)
    c.num_beams = int(cfg.sensor.num_beams)
    c.lidar_radius = int(cfg.sensor.radius)
    c.evader_view = int(cfg.attacker.sen_range)
    c.tape_len = int(tape_len)
    c.max_path = int(max(max_path, c.difficulty + 2))
    c.use_reward_norm = 1 if cfg.algo.use_reward_norm else 0
    c.def_tau, c.def_dt = float(cfg.defender.tau), float(cfg.defender.step_size)
    c.def_collision_radius = float(cfg.defender.collision_radius)
    c.def_comm_range, c.def_sen_range = float(cfg.defender.comm_range), float(cfg.defender.sen_range)
    c.eva_vmax, c.eva_tau, c.eva_dt = float(cfg.attacker.vmax), float(cfg.attacker.tau), float(cfg.attacker.step_size)
    c.eva_collision_radius = float(cfg.attacker.collision_radius)
    c.resolution = float(cfg.map.resolution)
    for k, (ux, uy) in enumerate(tables.action_table(float(cfg.defender.vmax))):
        c.action_u[k][0], c.action_u[k][1] = ux, uy
    for b, (bx, by) in enumerate(tables.beam_table(c.num_beams)):
        c.beam_dir[b][0], c.beam_dir[b][1] = bx, by
    return c


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _np(a):
    return a.ctypes.data_as(C.c_void_p)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class PathfinderCache:
    """The per-environment cached distance field of `BatchedEnv.pathfinder_teach` (include/pe_env.h pe_pathfinder_cache): field (N, W*H)
    i32, key (N, 2) i32 (source cell, -1 = empty; clearance) and hits (N,) i32, counted up by the kernel on every hit."""

    def __init__(self, N, WH, device):
        self.field = torch.zeros((N, WH), dtype=torch.int32, device=device)
        self.key = torch.full((N, 2), -1, dtype=torch.int32, device=device)
        self.hits = torch.zeros((N,), dtype=torch.int32, device=device)
        self.struct = PePathfinderCache()
        self.struct.field, self.struct.key, self.struct.hits = self.field.data_ptr(), self.key.data_ptr(), self.hits.data_ptr()

    def clear(self):
        """empties every key (one device fill, capturable); the fields stay and are never read under an empty key"""
        self.key[:, 0].fill_(-1)


class BatchedEnv:
    """N independent pursuit-evasion environments resident in HBM, stepped by the HIP kernels.

    The tensor attributes are the `pe_state` records of include/pe_env.h; `obs` holds the fp32 observation tensors in
    the reference's layouts (N leading)."""

    def __init__(self, pe_cfg: PeConfig, num_envs: int, device="cuda"):
        self.L = load_library()
        _check(self.L.pe_config_check(C.byref(pe_cfg)), "pe_config_check")
        if not torch.cuda.is_available():
            raise RuntimeError("BatchedEnv needs a GPU (MI355X); there is no CPU path")
        self.c = pe_cfg
        self.N = int(num_envs)
        self.device = torch.device(device)
        c, N, dev = pe_cfg, self.N, self.device
        WH, P = c.W * c.H, c.P
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        self._t = dict(grid=z((N, WH), torch.uint8), bidx=z((N, WH), torch.int16), n_obs=z((N,), torch.int32),
                       defs=z((N, 4, P), torch.float64), eva=z((N, 4), torch.float64), target=z((N, 2), torch.int32),
                       tape=z((N, c.tape_len, 2), torch.int32), meta=z((N, META_INTS), torch.int32),
                       path=z((N, c.max_path, 2), torch.int16), rn=z((N, 1 + 2 * P), torch.float64), wpw=z((N, 16), torch.int32),
                       raser=z((N, WH, raser_row_words(c.O)), torch.int32))
        self.o_state = z((N, c.O, 4), torch.float32)  # boundary obstacles as [x, y, 0, 0] (pursuit_env.py:22-26), padded
        self.st = PeState()
        self.st.N = N
        for name, t in self._t.items():
            setattr(self.st, "def_" if name == "defs" else name, t.data_ptr())
        self.t_host = None  # lockstep time_step known to the host (None: unknown -> always allow replans)
        # replan ticks run the evader's rescan + A* on a second stream so its stragglers overlap the next policy forward
        self.overlap_replan = True
        self._side = torch.cuda.Stream(device=self.device)
        self._ev_obs = torch.cuda.Event()
        self._ev_evader = torch.cuda.Event()
        self._pending = False

    # -- hand-over of Pursuit_Env.reset() results --------------------------------------------------------
    def load(self, init, reset_reward_norm=False):
        self._join()
        """init: dict of host numpy arrays grid [N,W,H] u8, obs_xy [N,O,2] i32 (padded), n_obs [N], defenders [N,P,4] f64,
        evader [N,4] f64, target [N,2] i32, tape [N,tape_len,2] i32."""
        c, N = self.c, self.N
        g = np.ascontiguousarray(init["grid"], np.uint8).reshape(N, c.W * c.H)
        ob = np.ascontiguousarray(init["obs_xy"], np.int32).reshape(N, c.O, 2)
        no = np.ascontiguousarray(init["n_obs"], np.int32).reshape(N)
        if int(no.max()) > c.O:
            raise ValueError(f"an environment has {int(no.max())} boundary obstacles > num_max_obstacle={c.O}")
        d = np.ascontiguousarray(init["defenders"], np.float64).reshape(N, c.P, 4)
        e = np.ascontiguousarray(init["evader"], np.float64).reshape(N, 4)
        tg = np.ascontiguousarray(init["target"], np.int32).reshape(N, 2)
        tp = np.ascontiguousarray(init["tape"], np.int32).reshape(N, c.tape_len, 2)
        h = PeHostInit()
        h.grid, h.obs_xy, h.n_obs, h.def_, h.eva, h.target, h.tape = (_np(g), _np(ob), _np(no), _np(d), _np(e), _np(tg), _np(tp))
        h.reset_rn = 1 if reset_reward_norm else 0
        self._keep = (g, ob, no, d, e, tg, tp)  # the async copies read these host arrays
        with torch.cuda.device(self.device):
            _check(self.L.pe_env_load(C.byref(self.c), C.byref(self.st), C.byref(h), _stream()), "pe_env_load")
            torch.cuda.current_stream().synchronize()
        self._keep = None
        os_ = np.zeros((N, c.O, 4), np.float32)
        os_[:, :, :2] = ob.astype(np.float32)
        valid = np.arange(c.O)[None, :] < no[:, None]
        os_[~valid] = 0.0
        self.o_state.copy_(torch.from_numpy(os_))
        self.t_host = 0

    # -- observation / step entry points -----------------------------------------------------------------
    def new_obs(self, packed=False):
        """fp32 observation tensors in the reference's layouts; packed=True: the LiDAR rows as `o_adj_bits` (N, P, RW) int32
        (bit k of row i = o_adj[i][k]) instead of the (N, P, O) float `o_adj` -- the form the product's rollout consumes."""
        c, N, dev = self.c, self.N, self.device
        f = lambda *s: torch.empty((N, *s), dtype=torch.float32, device=dev)
        obs = dict(p_state=f(c.P, 4), e_state=f(1, 4), p_adj=f(c.P, c.P), e_adj=f(c.P, 1))
        if packed:
            obs["o_adj_bits"] = torch.zeros((N, c.P, raser_row_words(c.O)), dtype=torch.int32, device=dev)
        else:
            obs["o_adj"] = f(c.P, c.O)
        return obs

    @staticmethod
    def _obs_struct(obs):
        o = PeObsOut()
        for k in ("p_state", "e_state", "p_adj", "e_adj", "o_adj", "o_adj_bits"):
            t = obs.get(k) if obs else None
            if t is not None:
                assert t.dtype == (torch.int32 if k == "o_adj_bits" else torch.float32) and t[0].is_contiguous(), k
                setattr(o, k, t.data_ptr())
                setattr(o, k + "_stride", t.stride(0))
        return o

    @staticmethod
    def _step_struct(reward, reward_raw, done):
        s = PeStepOut()
        if reward is not None:
            assert reward.dtype == torch.float32 and reward[0].is_contiguous()
            s.reward, s.reward_stride = reward.data_ptr(), reward.stride(0)
        if reward_raw is not None:
            assert reward_raw.dtype == torch.float32 and reward_raw[0].is_contiguous()
            s.reward_raw, s.reward_raw_stride = reward_raw.data_ptr(), reward_raw.stride(0)
        if done is not None:
            assert done.dtype == torch.uint8 and done.is_contiguous()
            s.done = done.data_ptr()
        return s

    def _may_replan(self):
        return 1 if (self.t_host is None or self.t_host % self.c.difficulty == 0) else 0

    def __getattr__(self, name):
        # state tensors (grid, bidx, n_obs, defs, eva, target, tape, meta, path, rn): reading them orders the caller's stream
        # after an evader step that may still run on the side stream
        t = self.__dict__.get("_t")
        if t is not None and name in t:
            self._join()
            return t[name]
        raise AttributeError(name)

    def _join(self):
        """every entry point that reads or writes environment state first waits for an evader step still in flight"""
        if self._pending:
            torch.cuda.current_stream().wait_event(self._ev_evader)
            self._pending = False
        ev = self.__dict__.get("_ev_reset")
        if ev is not None:      # a device reset issued ahead on the side stream (Pursuit_Env.prefetch_reset)
            torch.cuda.current_stream().wait_event(ev)
            self.__dict__["_ev_reset"] = None

    def observe(self, obs=None):
        self._join()
        obs = obs if obs is not None else self.new_obs()
        o = self._obs_struct(obs)
        _check(self.L.pe_env_observe(C.byref(self.c), C.byref(self.st), C.byref(o), _stream()), "pe_env_observe")
        return obs

    def evader_step(self):
        self._join()
        _check(self.L.pe_evader_step(C.byref(self.c), C.byref(self.st), self._may_replan(), _stream()), "pe_evader_step")

    def step(self, actions, reward=None, reward_raw=None, done=None):
        self._join()
        a = self._actions(actions)
        if reward is None:
            reward = torch.empty((self.N, self.c.P), dtype=torch.float32, device=self.device)
        s = self._step_struct(reward, reward_raw, done)
        _check(self.L.pe_env_step(C.byref(self.c), C.byref(self.st), _ptr(a), C.byref(s), _stream()), "pe_env_step")
        if self.t_host is not None:
            self.t_host += 1
        return reward

    def tick(self, actions, obs, reward, reward_raw=None, done=None):
        """Fused step(actions) -> observe -> attacker_step (one launch)."""
        a = self._actions(actions)
        s = self._step_struct(reward, reward_raw, done)
        o = self._obs_struct(obs)
        self._join()
        if self.t_host is not None:
            self.t_host += 1
        replan = self._may_replan()
        if replan and self.overlap_replan:
            _check(self.L.pe_env_step_observe(C.byref(self.c), C.byref(self.st), _ptr(a), C.byref(s), C.byref(o), _stream()),
                   "pe_env_step_observe")
            self._ev_obs.record(torch.cuda.current_stream())
            self._side.wait_event(self._ev_obs)
            _check(self.L.pe_evader_step(C.byref(self.c), C.byref(self.st), 1, C.c_void_p(self._side.cuda_stream)), "pe_evader_step")
            self._ev_evader.record(self._side)
            self._pending = True
            return
        _check(self.L.pe_env_tick(C.byref(self.c), C.byref(self.st), _ptr(a), C.byref(s), C.byref(o), replan, _stream()), "pe_env_tick")

    def demon(self, out=None):
        """Pursuit_Env.demon (pursuit_env.py:211-229) for every environment -> (N, P) int32 actions (csrc/pe_env.hip k_demon)."""
        self._join()
        if out is None:
            out = torch.empty((self.N, self.c.P), dtype=torch.int32, device=self.device)
        assert out.dtype == torch.int32 and out.is_contiguous() and out.shape == (self.N, self.c.P)
        dirs = (C.c_double * 18)(*[v for cs in tables.action_table(1.0) for v in cs])
        _check(self.L.pe_env_demon(C.byref(self.c), C.byref(self.st), dirs, _ptr(out), _stream()), "pe_env_demon")
        return out

    def pathfinder(self, out=None, lead=None, sep_range=None, clearance=None, diag=False):
        """The scripted path-finding pursuers (include/pe_env.h pe_pursuer_pathfinder) for every environment ->
        (N, P) int32 actions, the tensor `tick` takes; one launch on the current stream, no host read.  diag=True (or a dict of tensors
        to fill) also returns field (N, W*H) i32, kstar (N, P) i32 and blocked (N, P) i16 (bit k: candidate k fails the static-map probe)."""
        self._join()
        c, N = self.c, self.N
        if out is None:
            out = torch.empty((N, c.P), dtype=torch.int32, device=self.device)
        assert out.dtype == torch.int32 and out.is_contiguous() and out.shape == (N, c.P)
        prm = pathfinder_params(c, lead, sep_range, clearance)
        dg = PePathfinderDiag()
        if diag:
            if not isinstance(diag, dict):
                diag = dict(field=torch.empty((N, c.W * c.H), dtype=torch.int32, device=self.device),
                            kstar=torch.empty((N, c.P), dtype=torch.int32, device=self.device),
                            blocked=torch.empty((N, c.P), dtype=torch.int16, device=self.device))
            for k, dt in (("field", torch.int32), ("kstar", torch.int32), ("blocked", torch.int16)):
                t = diag.get(k)
                if t is not None:
                    assert t.dtype == dt and t.is_contiguous(), k
                    setattr(dg, k, t.data_ptr())
        _check(self.L.pe_pursuer_pathfinder(C.byref(c), C.byref(self.st), C.byref(prm), _ptr(out), C.byref(dg) if diag else None, _stream()),
               "pe_pursuer_pathfinder")
        return (out, diag) if diag else out

    def pathfinder_cache(self):
        """a fresh, empty `PathfinderCache` for this batch of environments"""
        return PathfinderCache(self.N, self.c.W * self.c.H, self.device)

    def pathfinder_teach(self, out=None, cache=None, follow=None, action=None, a_star=None, lead=None, sep_range=None, clearance=None, diag=False):
        """The pathfinder as a teacher (include/pe_env.h pe_pursuer_pathfinder_teach): `pathfinder`'s actions from
        one launch that may reuse the distance field of the last launch and writes the imitation labels.  out: (N, P) int32 or None (not
        written); cache: a `pathfinder_cache()` or None; follow (N,) uint8 with action (N, P) int32: the rows of `action` whose follow byte
        is set are overwritten with the teacher's; a_star: float32, every row receives the teacher's action -- a contiguous (N, P) tensor
        or a row view buf[rows, t] of an (N, T, P) one, the stride is taken from the view.
        THE CALLER clears the cache (`cache.clear()`) after anything that writes the grid (`load`, a resetter's `reset`): a key only names
        the evader's cell and the clearance, and nothing here guesses whether the map under it is still the same."""
        self._join()
        c, N = self.c, self.N
        if out is not None:
            assert out.dtype == torch.int32 and out.is_contiguous() and out.shape == (N, c.P)
        prm = pathfinder_params(c, lead, sep_range, clearance)
        lb = PePathfinderLabel()
        if follow is not None:
            assert follow.dtype == torch.uint8 and follow.is_contiguous() and follow.shape == (N,)
            lb.follow = follow.data_ptr()
        if action is not None:
            assert action.dtype == torch.int32 and action.is_contiguous() and action.shape == (N, c.P)
            lb.action = action.data_ptr()
        if a_star is not None:
            assert a_star.dtype == torch.float32 and a_star.shape == (N, c.P) and (c.P == 1 or a_star.stride(1) == 1)
            lb.a_star, lb.a_star_env_stride = a_star.data_ptr(), a_star.stride(0) if N > 1 else c.P
        dg = PePathfinderDiag()
        if diag:
            if not isinstance(diag, dict):
                diag = dict(field=torch.empty((N, c.W * c.H), dtype=torch.int32, device=self.device),
                            kstar=torch.empty((N, c.P), dtype=torch.int32, device=self.device),
                            blocked=torch.empty((N, c.P), dtype=torch.int16, device=self.device))
            for k, dt in (("field", torch.int32), ("kstar", torch.int32), ("blocked", torch.int16)):
                t = diag.get(k)
                if t is not None:
                    assert t.dtype == dt and t.is_contiguous(), k
                    setattr(dg, k, t.data_ptr())
        if cache is not None:
            assert cache.field.shape == (N, c.W * c.H)
        _check(self.L.pe_pursuer_pathfinder_teach(C.byref(c), C.byref(self.st), C.byref(prm), C.byref(cache.struct) if cache is not None else None,
                                                  C.byref(lb), _ptr(out), C.byref(dg) if diag else None, _stream()), "pe_pursuer_pathfinder_teach")
        return (out, diag) if diag else out

    def record_state(self, def_row, eva_row):
        """One tick's row of an episode trace (include/pe_env.h pe_env_record_state): the pursuers' and the evader's records as the next
        step will read them, copied into def_row (N, 4, P) / eva_row (N, 4) float64 -- views trace[:, t] of (N, T, 4, P) / (N, T, 4)
        tensors, the environment strides are taken from the views.  One small launch on the current stream, after the evader step that
        may still run on the side stream (the evader's record is written there)."""
        self._join()
        c, N = self.c, self.N
        assert def_row.dtype == torch.float64 and def_row.shape == (N, 4, c.P) and def_row[0].is_contiguous()
        assert eva_row.dtype == torch.float64 and eva_row.shape == (N, 4) and eva_row[0].is_contiguous()
        _check(self.L.pe_env_record_state(C.byref(c), C.byref(self.st), _ptr(def_row), _stride(def_row.shape, def_row.stride(), 0, 4 * c.P),
                                          _ptr(eva_row), _stride(eva_row.shape, eva_row.stride(), 0, 4), _stream()), "pe_env_record_state")

    def pathfinder_label_episode(self, trace_def, trace_eva, a_star, builds=None, lead=None, sep_range=None, clearance=None, diag=False):
        """The pathfinder's labels for a whole recorded episode in one launch (include/pe_env.h pe_pathfinder_label_episode, DESIGN.md
        section 7p): trace_def (N, T, 4, P) / trace_eva (N, T, 4) float64 as `record_state` filled them, a_star (N, T, P) float32 -- a
        tensor or a view such as buf[rows] whose records are contiguous, the strides are taken from the views; builds (N,) int32 or None:
        the distance fields each environment built.  The grid must still be the episode's (label before the next reset).  diag=True (or
        a dict of tensors to fill) also returns the LAST tick's field / kstar / blocked like `pathfinder`."""
        self._join()
        c, N = self.c, self.N
        assert trace_def.dtype == torch.float64 and trace_eva.dtype == torch.float64 and trace_def.shape[0] == N
        tr = _trace_struct(c.P, _ptr, trace_def, trace_eva, trace_def.stride(), trace_eva.stride())
        assert a_star.dtype == torch.float32 and a_star.shape == (N, tr.T, c.P) and (c.P == 1 or a_star.stride(2) == 1)
        if builds is not None:
            assert builds.dtype == torch.int32 and builds.shape == (N,) and builds.is_contiguous()
        prm = pathfinder_params(c, lead, sep_range, clearance)
        dg = PePathfinderDiag()
        if diag:
            if not isinstance(diag, dict):
                diag = dict(field=torch.empty((N, c.W * c.H), dtype=torch.int32, device=self.device),
                            kstar=torch.empty((N, c.P), dtype=torch.int32, device=self.device),
                            blocked=torch.empty((N, c.P), dtype=torch.int16, device=self.device))
            for k, dt in (("field", torch.int32), ("kstar", torch.int32), ("blocked", torch.int16)):
                t = diag.get(k)
                if t is not None:
                    assert t.dtype == dt and t.is_contiguous(), k
                    setattr(dg, k, t.data_ptr())
        _check(self.L.pe_pathfinder_label_episode(C.byref(c), C.byref(self.st), C.byref(prm), C.byref(tr), _ptr(a_star),
                                                  _stride(a_star.shape, a_star.stride(), 0, tr.T * c.P), _stride(a_star.shape, a_star.stride(), 1, c.P),
                                                  _ptr(builds), C.byref(dg) if diag else None, _stream()), "pe_pathfinder_label_episode")
        return (a_star, diag) if diag else a_star

    def _actions(self, actions):
        if actions.dtype != torch.int32:
            actions = actions.to(torch.int32)
        actions = actions.contiguous()
        assert actions.shape == (self.N, self.c.P) and actions.device.type == "cuda"
        return actions

    # -- host read-back (tests, logging) ---------------------------------------------------------------------
    def defenders_aos(self):
        self._join()
        return self.defs.permute(0, 2, 1).contiguous()  # [N][P][4] like get_state('defender')

    def status(self):
        return self.meta[:, META_STATUS]


def astar_batch(W, H, obs, sg, max_path=256):
    """Diagnostic/test entry: one weighted-A* problem per workgroup. obs [n,(W+1),(H+1)] u8, sg [n,4] int."""
    L = load_library()
    n = obs.shape[0]
    obs_d = torch.as_tensor(np.ascontiguousarray(obs, np.uint8)).cuda()
    sg_d = torch.as_tensor(np.ascontiguousarray(sg, np.int32)).cuda()
    path = torch.zeros((n, max_path, 2), dtype=torch.int16, device="cuda")
    lens = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
    _check(L.pe_astar_batch(W, H, n, _ptr(obs_d), _ptr(sg_d), _ptr(path), _ptr(lens), max_path, _stream()), "pe_astar_batch")
    torch.cuda.synchronize()
    return path.cpu().numpy(), lens.cpu().numpy()


def _reset_params(cfg):
    prm = PeResetParams()
    prm.num_blocks = int(cfg.map.num_obstacle_block)
    prm.min_dist = 4  # pursuit_env.py:71
    prm.center[0], prm.center[1] = float(cfg.map.center[0]), float(cfg.map.center[1])
    prm.variance = float(cfg.map.variance)
    return prm


def _seed_array(seeds):
    s = np.ascontiguousarray(seeds, np.uint64)
    if (s >> np.uint64(32)).any():
        raise ValueError("seeds must fit 32 bits (numpy.random.seed range)")
    return s


class DeviceResetter:
    """Pursuit_Env.reset() on the GPU (csrc/pe_env.hip k_reset): the generator streams of every environment live in device
    memory; same streams, same draws, same results as HostResetter, with no host arrays and no upload."""

    def __init__(self, sim, cfg, seeds, map_bank=0, bank_seed=0):
        """map_bank = B > 0: B maps are generated once (the product's host map generator with seeds bank_seed .. bank_seed + B - 1);
        every reset picks one slot for ALL environments (random.Random(bank_seed).randrange(B), like the older reference driver's
        one `map_info` per node and iteration, MAPPO_parallel_main.py:103-124) and only draws targets / defenders / evader."""
        self.L = load_library()
        self.sim = sim
        self.c = sim.c
        self.N = len(seeds)
        assert self.N == sim.N
        self.prm = _reset_params(cfg)
        self.bank = None
        if map_bank:
            import random as _pyrandom
            gen = HostResetter(sim.c, cfg, [int(bank_seed) + k for k in range(int(map_bank))])
            self.bank = torch.from_numpy(gen.reset()["grid"].reshape(int(map_bank), -1)).to(sim.device).contiguous()   # (B, W*H) u8
            self.bank_rng = _pyrandom.Random(int(bank_seed))
            self.bank_slot = -1
        s = _seed_array(seeds)
        n = self.L.pe_reset_state_bytes(C.byref(self.c), self.N)
        self.state = torch.empty(n, dtype=torch.uint8, device=sim.device)
        with torch.cuda.device(sim.device):
            _check(self.L.pe_env_reset_seed(C.byref(self.c), self.N, _np(s), _ptr(self.state), _stream()), "pe_env_reset_seed")
        self.first = True

    def get_state(self, snapshot=None):
        """the resume-bundle form (host arrays); snapshot: a snapshot_device() result to convert instead of the live state"""
        src = snapshot if snapshot is not None else dict(blob=self.state, first=self.first, bank_rng=self.bank_rng.getstate() if self.bank is not None else None)
        d = dict(blob=src["blob"].cpu().numpy(), first=src["first"], device=True)
        if self.bank is not None:
            d["bank_rng"] = src["bank_rng"]
        return d

    def snapshot_device(self):
        """the generator streams as they stand, kept on the device (no host copy, no synchronisation)"""
        return dict(blob=self.state.clone(), first=self.first, bank_rng=self.bank_rng.getstate() if self.bank is not None else None)

    def set_state(self, state):
        buf = np.ascontiguousarray(state["blob"], np.uint8)
        if not state.get("device") or buf.size != self.state.numel():
            raise ValueError("resetter state does not match this configuration / number of environments / reset mode")
        self.state.copy_(torch.from_numpy(buf))
        self.first = bool(state["first"])
        if self.bank is not None and "bank_rng" in state:
            self.bank_rng.setstate(state["bank_rng"])

    def reset(self, reset_reward_norm=False):
        """Next episode of every environment, in place in the simulator state (reads the finished episode's tape position
        from the device)."""
        self.launch(reset_reward_norm)
        self.check()

    def launch(self, reset_reward_norm=False):
        """the reset kernels on the current stream, no read-back (Pursuit_Env.prefetch_reset issues them on a side stream under the
        PPO update; check() follows when the episode starts)"""
        sim = self.sim
        sim._join()
        if self.bank is not None:
            self.bank_slot = self.bank_rng.randrange(self.bank.shape[0])
            self.prm.fixed_grid = self.bank[self.bank_slot].data_ptr()
        with torch.cuda.device(sim.device):
            _check(self.L.pe_env_reset(C.byref(self.c), C.byref(sim.st), C.byref(self.prm), _ptr(self.state), 1 if self.first else 0,
                                       _ptr(sim.o_state), 1 if reset_reward_norm else 0, _stream()), "pe_env_reset")
        self.first = False
        sim.t_host = 0

    def check(self):
        sim = self.sim
        # one blocking read-back per episode: the largest obstacle count and the sticky kernel status bits (pe_env.h: the
        # finished episode's tape-exhausted / A*-cap / path-underflow bits are carried into the new meta record by the reset)
        worst, bits = torch.stack((sim.n_obs.max(), status_or(sim.meta))).tolist()
        if bits:
            raise RuntimeError("environment kernel status: " + status_text(bits))
        if worst > self.c.O:
            raise ValueError(f"an environment has {worst} boundary obstacles > num_max_obstacle={self.c.O}")


class HostResetter:
    """Host side of Pursuit_Env.reset() for N environments (csrc/pe_reset.cpp): per-environment re-implementations of
    the reference's `random` / `numpy.random` streams, seeded like random.seed(s); np.random.seed(s)."""

    def __init__(self, pe_cfg: PeConfig, cfg, seeds, n_threads=None):
        self.L = load_library()
        self.c = pe_cfg
        self.N = len(seeds)
        prm = _reset_params(cfg)
        s = _seed_array(seeds)
        self.h = self.L.pe_resetter_create(C.byref(pe_cfg), C.byref(prm), self.N, _np(s))
        if not self.h:
            raise RuntimeError("pe_resetter_create failed (bad configuration)")
        world = max(1, int(os.environ.get("LOCAL_WORLD_SIZE", os.environ.get("WORLD_SIZE", "1"))))
        self.n_threads = int(n_threads or max(1, min(16, (os.cpu_count() or 1) // world)))
        self.first = True

    def __del__(self):
        try:
            if self.h:
                self.L.pe_resetter_destroy(self.h)
        except Exception:
            pass

    def get_state(self):
        buf = np.empty(self.L.pe_resetter_state_bytes(self.h), np.uint8)
        _check(self.L.pe_resetter_get_state(self.h, _np(buf)), "pe_resetter_get_state")
        return dict(blob=buf, first=self.first)

    def set_state(self, state):
        buf = np.ascontiguousarray(state["blob"], np.uint8)
        if buf.size != self.L.pe_resetter_state_bytes(self.h):
            raise ValueError("resetter state does not match this configuration / number of environments")
        _check(self.L.pe_resetter_set_state(self.h, _np(buf)), "pe_resetter_set_state")
        self.first = bool(state["first"])

    def reset(self, consumed_targets=None):
        c, N = self.c, self.N
        out = dict(grid=np.empty((N, c.W, c.H), np.uint8), obs_xy=np.empty((N, c.O, 2), np.int32), n_obs=np.empty(N, np.int32),
                   defenders=np.empty((N, c.P, 4), np.float64), evader=np.empty((N, 4), np.float64),
                   target=np.empty((N, 2), np.int32), tape=np.empty((N, c.tape_len, 2), np.int32))
        o = PeHostInitOut()
        o.grid, o.obs_xy, o.n_obs, o.def_, o.eva, o.target, o.tape = (_np(out[k]) for k in
                                                                        ("grid", "obs_xy", "n_obs", "defenders", "evader", "target", "tape"))
        ct = None
        if not self.first:
            if consumed_targets is None:
                raise ValueError("consumed_targets (tape positions of the finished episode) is required after the first reset")
            ct = np.ascontiguousarray(consumed_targets, np.int32)
        _check(self.L.pe_resetter_reset(self.h, _np(ct) if ct is not None else None, C.byref(o), self.n_threads), "pe_resetter_reset")
        self.first = False
        return out
