"""The teacher launch's host twin (include/pe_env.h pe_pursuer_pathfinder_teach_host) on the CPU: the cached twin driving the C oracle
against the uncached twin every tick, the label outputs, and every refused argument without a write."""
import ctypes as C

import numpy as np
import pytest

from tests import pe_pathfinder_cases as pc

BAD_CONFIG, NULL = 10001, 10002


def _cell(x, y, W, H):
    return min(max(round(x), 0), W - 1) * H + min(max(round(y), 0), H - 1)


@pytest.mark.parametrize("W", [20, 40])
def test_cached_twin_drives_the_oracle_like_the_uncached_one(W):
    """150 ticks of the cached host twin driving the C oracle, 8 environments per map size (the harness of
    test_law_never_proposes_a_move_the_static_probe_rejects): every tick its actions, kstar, blocked and field are the uncached twin's, and
    hits counts exactly the ticks whose evader cell is the previous tick's."""
    from distributed_multi_agent_reinforcement_learning_amd import pe_env
    from tests.helpers import oracle_envs_from_init, product_cfg
    N, P, T = 8, 4, 150
    cfg = product_cfg(P, W, W, T=T, blocks=3 if W == 20 else 5)
    pcfg = pe_env.make_pe_config(cfg)
    init = pe_env.HostResetter(pcfg, cfg, [4200 + n for n in range(N)]).reset()
    _, envs = oracle_envs_from_init(init, P, W, W, T)
    grid = np.ascontiguousarray(init["grid"], np.uint8).reshape(N, W * W)
    cache = dict(field=np.zeros((N, W * W), np.int32), key=np.full((N, 2), -1, np.int32), hits=np.zeros(N, np.int32))
    expect = np.zeros(N, np.int64)
    prev = [None] * N
    for t in range(T):
        for env in envs:
            env.evader_step()
        states = [env.state() for env in envs]
        defs = np.stack([st["defenders"].T for st in states])
        eva = np.stack([st["evader"] for st in states])
        plain, pd = pe_env.pathfinder_host(pcfg, grid, defs, eva, diag=True)
        cached, cd = pe_env.pathfinder_teach_host(pcfg, grid, defs, eva, cache=cache, diag=True)
        assert np.array_equal(cached, plain), t
        for k in ("kstar", "blocked", "field"):
            assert np.array_equal(cd[k], pd[k]), (t, k)
        assert np.array_equal(cache["field"], pd["field"]), t        # hit or miss, the cache now holds this tick's field
        for n in range(N):
            s = _cell(eva[n, 0], eva[n, 1], W, W)
            expect[n] += s == prev[n]
            prev[n] = s
            assert cache["key"][n].tolist() == [s, 10]
        assert np.array_equal(cache["hits"], expect), t
        for n, env in enumerate(envs):
            env.step(cached[n].tolist())
    hits, misses = int(expect.sum()), int(N * T - expect.sum())
    print(f"{W} x {W}: {hits} hits, {misses} misses over {N} environments x {T} ticks")
    assert hits > 0 and misses > N        # both occur, beyond the first tick's misses


def _records(W=5, H=7, P=2, N=3, seed=3):
    cfg = pc.pe_config_for(W, H, P)
    ss = [pc.random_scene(seed + n, W, H, P, 0.15) for n in range(N)]
    return cfg, np.stack([s["grid"] for s in ss]).reshape(N, W * H), np.stack([s["defs"] for s in ss]), np.stack([s["eva"] for s in ss])


def test_labels_follow_mask_and_strided_rows():
    from distributed_multi_agent_reinforcement_learning_amd import pe_env
    cfg, grid, defs, eva = _records(P=3, N=4)
    plain = pe_env.pathfinder_host(cfg, grid, defs, eva)
    buf = np.full((4, 3, 3), -2.0, np.float32)                       # (N, T, P): the launch writes row t = 1 through a view
    action = np.full((4, 3), 7, np.int32)
    follow = np.array([1, 0, 1, 0], np.uint8)
    out = pe_env.pathfinder_teach_host(cfg, grid, defs, eva, follow=follow, action=action, a_star=buf[:, 1])
    assert np.array_equal(out, plain)
    assert np.array_equal(buf[:, 1], plain.astype(np.float32)) and (buf[:, 0] == -2.0).all() and (buf[:, 2] == -2.0).all()
    assert np.array_equal(action[[0, 2]], plain[[0, 2]]) and (action[[1, 3]] == 7).all()
    # nobody follows: action is left alone even when given
    action[:] = 7
    pe_env.pathfinder_teach_host(cfg, grid, defs, eva, action=action)
    assert (action == 7).all()


def test_every_refused_argument_returns_before_a_write():
    from distributed_multi_agent_reinforcement_learning_amd import pe_env
    L = pe_env.load_library()
    cfg, grid, defs, eva = _records()
    N, P, WH = 3, cfg.P, cfg.W * cfg.H
    prm = pe_env.pathfinder_params(cfg)
    bad_prm = pe_env.pathfinder_params(cfg, clearance=1001)
    arrays = dict(field=np.full((N, WH), -5, np.int32), key=np.full((N, 2), -1, np.int32), hits=np.full(N, -6, np.int32),
                  action=np.full((N, P), 7, np.int32), a_star=np.full((N, P), -2.0, np.float32), actions=np.full((N, P), -3, np.int32),
                  follow=np.ones(N, np.uint8))
    before = {k: v.copy() for k, v in arrays.items()}
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(prm=prm, cache=("field", "key", "hits"), follow=True, action=True, stride=P, cfg=cfg):
        ca, lb = pe_env.PePathfinderCache(), pe_env.PePathfinderLabel()
        for k in cache or ():
            setattr(ca, k, ptr(arrays[k]))
        if follow:
            lb.follow = ptr(arrays["follow"])
        if action:
            lb.action = ptr(arrays["action"])
        lb.a_star, lb.a_star_env_stride = ptr(arrays["a_star"]), stride
        return L.pe_pursuer_pathfinder_teach_host(C.byref(cfg), N, ptr(grid), ptr(defs), ptr(eva), C.byref(prm), C.byref(ca) if cache is not None else None,
                                                  C.byref(lb), ptr(arrays["actions"]), None)

    big = pc.pe_config_for(91, 91, 4)
    assert call(prm=bad_prm) == BAD_CONFIG and call(cfg=big) == BAD_CONFIG          # pathfinder_check fails
    assert call(stride=P - 1) == BAD_CONFIG                                         # a_star_env_stride < P with a_star set
    assert call(action=False) == NULL                                               # follow without action
    assert call(cache=("key", "hits")) == NULL and call(cache=("field", "hits")) == NULL and call(cache=()) == NULL
    for k, v in arrays.items():
        assert np.array_equal(v, before[k]), k
    # the device entry refuses the same before any launch: no GPU is touched
    st = pe_env.PeState()
    st.N = N
    lb = pe_env.PePathfinderLabel()
    lb.follow = ptr(arrays["follow"])
    ca = pe_env.PePathfinderCache()
    ca.field = ptr(arrays["field"])
    dev = lambda prm, ca, lb: L.pe_pursuer_pathfinder_teach(C.byref(cfg), C.byref(st), C.byref(prm), ca, lb, None, None, None)
    assert dev(bad_prm, None, None) == BAD_CONFIG and dev(prm, None, C.byref(lb)) == NULL and dev(prm, C.byref(ca), None) == NULL
    lb = pe_env.PePathfinderLabel()
    lb.a_star, lb.a_star_env_stride = ptr(arrays["a_star"]), P - 1
    assert dev(prm, None, C.byref(lb)) == BAD_CONFIG
    # and what is allowed: members that may be NULL (hits, actions, the records themselves), a stride above P
    assert call(cache=("field", "key"), follow=False, action=False, stride=P) == 0
    st0 = pe_env.PeState()      # N = 0 touches nothing
    assert L.pe_pursuer_pathfinder_teach(C.byref(cfg), C.byref(st0), C.byref(prm), None, None, None, None, None) == 0
