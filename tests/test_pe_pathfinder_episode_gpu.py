"""The episode labeller (csrc/pe_env.hip k_pathfinder_label_episode and k_record_state) against the per-tick
pathfinder kernel on the same states and against the host twin, bit for bit: labels, builds, the last tick's diag, guard bands, strided
views, refusals, graph replay, and a closed loop labelled afterwards against the per-tick teacher's labels."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import pe_pathfinder_cases as pc
from tests import pe_pathfinder_episode_cases as ec
from tests.test_pe_pathfinder_gpu import _guarded, _guards_intact, _launch as _plain_launch

pytestmark = pytest.mark.gpu
BAD_CONFIG, NULL = 10001, 10002
FILL = dict(a_star=-2.0, builds=-1, trace_def=1e9, trace_eva=1e9, field=-5, kstar=-7, blocked=-9)


class _Rig:
    """a hand-built device state (grid and meta are all the labeller reads of it) and a trace, a_star, builds and diag between guard
    bands; a_star is rows [N:2N] of a (2N, T, P) tensor"""

    def __init__(self, cfg, grid, trace_def, trace_eva):
        from distributed_multi_agent_reinforcement_learning_amd import pe_env
        self.pe_env, self.L, self.cfg = pe_env, pe_env.load_library(), cfg
        N, T, P, WH = trace_eva.shape[0], trace_eva.shape[1], cfg.P, cfg.W * cfg.H
        self.N, self.T, self.P, self.WH = N, T, P, WH
        self.grid_h, self.def_h, self.eva_h = np.ascontiguousarray(grid.reshape(N, WH)), np.ascontiguousarray(trace_def), np.ascontiguousarray(trace_eva)
        self.rec = dict(grid=torch.from_numpy(self.grid_h).cuda(), meta=torch.zeros((N, pe_env.META_INTS), dtype=torch.int32, device="cuda"))
        self.st = pe_env.PeState()
        self.st.N = N
        self.st.grid, self.st.meta = self.rec["grid"].data_ptr(), self.rec["meta"].data_ptr()
        shapes = dict(a_star=((2 * N, T, P), torch.float32), builds=((N,), torch.int32), trace_def=((N, T, 4, P), torch.float64),
                      trace_eva=((N, T, 4), torch.float64), field=((N, WH), torch.int32), kstar=((N, P), torch.int32), blocked=((N, P), torch.int16))
        self.buf, self.t = {}, {}
        for k, (shape, dt) in shapes.items():
            self.buf[k], self.t[k] = _guarded(shape, dt, FILL[k])
        self.t["trace_def"].copy_(torch.from_numpy(self.def_h))
        self.t["trace_eva"].copy_(torch.from_numpy(self.eva_h))
        self.a_rows = self.t["a_star"][N:]

    def trace(self, **over):
        P, T = self.P, self.T
        tr = self.pe_env.PePathfinderTrace()
        tr.def_, tr.def_env_stride, tr.def_tick_stride = self.t["trace_def"].data_ptr(), T * 4 * P, 4 * P
        tr.eva, tr.eva_env_stride, tr.eva_tick_stride, tr.T = self.t["trace_eva"].data_ptr(), T * 4, 4, T
        for k, v in over.items():
            setattr(tr, k, v)
        return tr

    def call(self, kw=None, tr="default", a_star=True, env_stride=None, tick_stride=None, builds=True, diag=True):
        prm = self.pe_env.pathfinder_params(self.cfg, **(kw or {}))
        tr = self.trace() if tr == "default" else tr
        dg = self.pe_env.PePathfinderDiag()
        dg.field, dg.kstar, dg.blocked = (self.t[k].data_ptr() for k in ("field", "kstar", "blocked"))
        return self.L.pe_pathfinder_label_episode(C.byref(self.cfg), C.byref(self.st), C.byref(prm), C.byref(tr) if tr is not None else None,
                                                  C.c_void_p(self.a_rows.data_ptr()) if a_star else None,
                                                  self.T * self.P if env_stride is None else env_stride, self.P if tick_stride is None else tick_stride,
                                                  C.c_void_p(self.t["builds"].data_ptr()) if builds else None, C.byref(dg) if diag else None,
                                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))

    def guards_ok(self):
        return all(_guards_intact(self.buf[k], FILL[k]) for k in self.buf)

    def everything(self):
        return {k: v.clone() for k, v in list(self.buf.items()) + list(self.rec.items())}

    def results(self):
        torch.cuda.synchronize()
        return dict(a_star=self.a_rows.cpu().numpy(), builds=self.t["builds"].cpu().numpy(), field=self.t["field"].cpu().numpy(),
                    kstar=self.t["kstar"].cpu().numpy(), blocked=self.t["blocked"].cpu().numpy().view(np.uint16))


SHAPES = [(5, 7, 2, 1, 1), (5, 7, 9, 67, 7), (40, 40, 8, 5, 12), (64, 64, 16, 3, 6), (90, 91, 16, 2, 4)]
KW = {9: dict(lead=1.5, sep_range=2.5, clearance=37)}


@pytest.mark.parametrize("W,H,P,N,T", SHAPES)
def test_labels_builds_and_diag_equal_the_per_tick_kernel_and_the_host_twin(W, H, P, N, T):
    cfg = pc.pe_config_for(W, H, P)
    grid, trace_def, trace_eva = ec.synthetic(N, W, H, P, T, 1000 * W + P)
    kw = KW.get(P, {})
    rig = _Rig(cfg, grid, trace_def, trace_eva)
    before = rig.everything()
    assert rig.call(kw) == 0
    got = rig.results()
    assert rig.guards_ok()
    for k in ("trace_def", "trace_eva", "grid", "meta"):                     # read only; no build hit the sweep bound
        assert torch.equal(before[k], rig.everything()[k]), k
    assert (rig.t["a_star"][:N] == FILL["a_star"]).all()                     # rows [0:N] of the (2N, T, P) tensor are not the launch's
    # the per-tick kernel on the same state written into the simulator's records, tick by tick
    for t in range(T):
        plain = _plain_launch(cfg, rig.grid_h, trace_def[:, t], trace_eva[:, t], kw)
        assert np.array_equal(got["a_star"][:, t], plain["actions"].astype(np.float32)), t
    for k in ("field", "kstar", "blocked"):                                  # diag is the last tick's
        assert np.array_equal(got[k], plain[k].reshape(got[k].shape)), k
    # the host twin
    want, wb = np.zeros((N, T, P), np.float32), np.zeros(N, np.int32)
    _, wdg = rig.pe_env.pathfinder_label_episode_host(cfg, rig.grid_h, trace_def, trace_eva, want, builds=wb, diag=True, **kw)
    assert np.array_equal(got["a_star"], want) and np.array_equal(got["builds"], wb)
    assert np.array_equal(got["builds"], ec.expected_builds(trace_eva, W, H))
    for k in ("field", "kstar", "blocked"):
        assert np.array_equal(got[k], wdg[k]), k
    # builds NULL and diag NULL: the same labels, nothing else written
    rig.t["a_star"].fill_(FILL["a_star"])
    for k in ("builds", "field", "kstar", "blocked"):
        rig.t[k].fill_(FILL[k])
    assert rig.call(kw, builds=False, diag=False) == 0
    torch.cuda.synchronize()
    assert np.array_equal(rig.a_rows.cpu().numpy(), want) and all((rig.t[k] == FILL[k]).all() for k in ("builds", "field", "kstar", "blocked"))
    assert rig.guards_ok()


def test_strided_trace_views_and_graph_replay_give_the_same_bits():
    """the trace as views of wider tensors through BatchedEnv's wrapper-free entry (tick and environment strides above one record), then the
    launch captured in a graph after one launch outside a capture and replayed"""
    from tests.helpers import no_gc_during_capture
    W, H, P, N, T = 40, 40, 8, 5, 12
    cfg = pc.pe_config_for(W, H, P)
    grid, trace_def, trace_eva = ec.synthetic(N, W, H, P, T, 77)
    rig = _Rig(cfg, grid, trace_def, trace_eva)
    assert rig.call() == 0
    first = rig.results()
    wide_def = torch.full((N + 1, T + 2, 4, P), 1e9, dtype=torch.float64, device="cuda")
    wide_eva = torch.full((N, T + 1, 7), 1e9, dtype=torch.float64, device="cuda")
    vdef, veva = wide_def[:N, 1:T + 1], wide_eva[:, :T, 2:6]
    vdef.copy_(rig.t["trace_def"])
    veva.copy_(rig.t["trace_eva"])
    keep = wide_def.clone(), wide_eva.clone()
    tr = rig.trace(def_=vdef.data_ptr(), def_env_stride=vdef.stride(0), def_tick_stride=vdef.stride(1), eva=veva.data_ptr(),
                   eva_env_stride=veva.stride(0), eva_tick_stride=veva.stride(1))
    rig.t["a_star"].fill_(FILL["a_star"])
    rig.t["builds"].fill_(FILL["builds"])
    assert rig.call(tr=tr) == 0
    second = rig.results()
    for k in first:
        assert np.array_equal(first[k], second[k]), k
    assert torch.equal(keep[0], wide_def) and torch.equal(keep[1], wide_eva) and rig.guards_ok()
    rig.t["a_star"].fill_(FILL["a_star"])
    rig.t["builds"].fill_(FILL["builds"])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with no_gc_during_capture(), torch.cuda.graph(graph):
        assert rig.call() == 0
    graph.replay()
    third = rig.results()
    for k in first:
        assert np.array_equal(first[k], third[k]), k
    assert rig.guards_ok()


def test_every_refused_argument_leaves_all_buffers_untouched():
    W, H, P, N, T = 20, 20, 4, 3, 4
    cfg = pc.pe_config_for(W, H, P)
    rig = _Rig(cfg, *ec.synthetic(N, W, H, P, T, 5))
    before = rig.everything()
    assert rig.call(dict(clearance=1001)) == BAD_CONFIG and rig.call(dict(lead=-1.0)) == BAD_CONFIG      # pathfinder_check
    assert rig.call(tr=rig.trace(T=0)) == BAD_CONFIG and rig.call(tr=rig.trace(T=-1)) == BAD_CONFIG
    assert rig.call(tr=None) == NULL and rig.call(tr=rig.trace(def_=None)) == NULL and rig.call(tr=rig.trace(eva=None)) == NULL
    assert rig.call(a_star=False) == NULL
    assert rig.call(env_stride=P - 1) == BAD_CONFIG and rig.call(tick_stride=P - 1) == BAD_CONFIG
    for k, least in (("def_env_stride", 4 * P), ("def_tick_stride", 4 * P), ("eva_env_stride", 4), ("eva_tick_stride", 4)):
        assert rig.call(tr=rig.trace(**{k: least - 1})) == BAD_CONFIG, k
    grid_ptr, rig.st.grid = rig.st.grid, None
    assert rig.call() == NULL
    rig.st.grid = grid_ptr
    # record_state: NULL rows, strides below one record
    defs, eva = rig.t["trace_def"][:, 0].contiguous(), rig.t["trace_eva"][:, 0].contiguous()
    rig.st.def_, rig.st.eva = defs.data_ptr(), eva.data_ptr()
    row_def, row_eva = rig.t["trace_def"][:, 1], rig.t["trace_eva"][:, 1]
    rec = lambda d=True, e=True, ds=T * 4 * P, es=T * 4: rig.L.pe_env_record_state(
        C.byref(cfg), C.byref(rig.st), C.c_void_p(row_def.data_ptr()) if d else None, ds, C.c_void_p(row_eva.data_ptr()) if e else None, es,
        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rec(d=False) == NULL and rec(e=False) == NULL and rec(ds=4 * P - 1) == BAD_CONFIG and rec(es=3) == BAD_CONFIG
    torch.cuda.synchronize()
    after = rig.everything()
    for k in before:
        assert torch.equal(before[k], after[k]), k
    # what is allowed: row 1 of the trace receives the records through the row's strides, and only row 1
    assert rec() == 0
    torch.cuda.synchronize()
    assert torch.equal(rig.t["trace_def"][:, 1], defs) and torch.equal(rig.t["trace_eva"][:, 1], eva) and rig.guards_ok()
    others = [0, 2, 3]
    assert torch.equal(rig.t["trace_def"][:, others], torch.from_numpy(rig.def_h).cuda()[:, others])
    assert torch.equal(rig.t["trace_eva"][:, others], torch.from_numpy(rig.eva_h).cuda()[:, others])


# ---- closed loop ----------------------------------------------------------------------------------------------------------------------------
def test_closed_loop_trace_labelled_afterwards_equals_the_per_tick_teacher():
    """16 cfg2-like environments driven by the per-tick teacher with its cache, every state recorded through BatchedEnv.record_state just
    before the step: the recorded rows are the simulator's tensors, the episode launch gives the a_star the teacher wrote during the
    loop, and builds is ticks - the cache's hits."""
    from distributed_multi_agent_reinforcement_learning_amd import pe_env
    from distributed_multi_agent_reinforcement_learning_amd.pursuit_env import Pursuit_Env
    from tests.helpers import product_cfg
    N, T = 16, 150
    cfg = product_cfg(8, 40, 40, T=T)
    P = int(cfg.env.num_defender)
    pcfg = pe_env.make_pe_config(cfg, tape_len=int(cfg.runtime.get("tape_len", 16)), max_path=int(cfg.runtime.get("max_path", 128)))
    seeds = [53000 + n for n in range(N)]
    init = pe_env.HostResetter(pcfg, cfg, seeds).reset()
    e = Pursuit_Env(cfg, num_envs=N, seeds=seeds)
    e.reset(init)
    obs = e.sim.new_obs(packed=True)
    e.observe(obs)
    e.attacker_step()
    reward, raw = torch.zeros(N, P, device="cuda"), torch.zeros(N, P, device="cuda")
    actions = torch.zeros(N, P, dtype=torch.int32, device="cuda")
    cache = e.pathfinder_cache()
    buf = torch.full((2 * N, T, P), -2.0, device="cuda")                       # the replay buffer's a_star field; the loop owns rows [N:2N]
    wide_def = torch.full((N, T + 1, 4, P), 1e9, dtype=torch.float64, device="cuda")
    wide_eva = torch.full((N, T, 6), 1e9, dtype=torch.float64, device="cuda")
    trace_def, trace_eva = wide_def[:, 1:], wide_eva[:, :, 1:5]                # strided rows
    for t in range(T):
        e.record_state(trace_def[:, t], trace_eva[:, t])
        if t in (0, 1, 75, T - 1):
            assert torch.equal(trace_def[:, t], e.sim.defs) and torch.equal(trace_eva[:, t], e.sim.eva), t
        e.pathfinder_teach(out=actions, cache=cache, a_star=buf[N:, t])
        e.tick(actions, obs, reward, raw)
    assert (wide_def[:, 0] == 1e9).all() and (wide_eva[:, :, 0] == 1e9).all() and (wide_eva[:, :, 5] == 1e9).all()
    got = torch.full((2 * N, T, P), -2.0, device="cuda")
    builds = torch.full((N,), -1, dtype=torch.int32, device="cuda")
    e.pathfinder_label_episode(trace_def, trace_eva, got[N:], builds=builds)
    torch.cuda.synchronize()
    assert torch.equal(got, buf)
    assert torch.equal(builds, T - cache.hits)
    assert int(e.sim.meta[:, pe_env.META_STATUS].max()) == 0
    print(f"{int(builds.sum())} builds over {N} environments x {T} ticks")
    assert N < int(builds.sum()) < N * T
