"""The pursuit tick kernels (csrc/pe_env.hip) against the C oracle away from the default configuration, bit for bit.

The cases and the oracle's replay live in tests/pe_config_cases.py; tests/test_pe_config_cases_cpu.py shows that each case reaches
the branch it is there for.  Driven like test_env_gpu.test_edge_configurations_match_oracle: load, observe, evader_step, then T
ticks including replans; at every tick all observation tensors, the evader state, path length and stored path tail, tape position,
target, raw and normalised rewards and the defenders' f64 state are compared with np.array_equal.  No tolerance anywhere.
"""
import numpy as np
import pytest
import torch

from tests import pe_config_cases as pc
from tests.helpers import init_from_traces, load_trace, no_gc_during_capture, product_cfg, random_init, trace_files

pytestmark = pytest.mark.gpu

STATUS_TAPE_EXHAUSTED = 1


def _new_obs(env, case):
    c, N = env.c, env.N
    if case.obs == "packed":
        return env.new_obs(packed=True)
    obs = env.new_obs()
    if case.obs == "both":
        obs["o_adj_bits"] = env.new_obs(packed=True)["o_adj_bits"]
    if case.obs == "misaligned":
        flat = torch.zeros(N * c.P * c.O + 4, dtype=torch.float32, device="cuda")
        obs["o_adj"] = flat[1:1 + N * c.P * c.O].view(N, c.P, c.O)
        assert obs["o_adj"].data_ptr() % 16 == 4 and (c.P * c.O * 4) % 16 == 0     # every environment's rows are 4 bytes off
    return obs


def _check_obs(case, got, row, t, RW):
    for n, rec in enumerate(row):
        for key in ("p_state", "e_state", "p_adj", "e_adj"):
            assert np.array_equal(got[key][n], rec[key]), (case.name, key, t, n)
        if "o_adj" in got:
            assert np.array_equal(got["o_adj"][n], rec["o_adj"]), (case.name, "o_adj", t, n)
        if "o_adj_bits" in got:
            assert np.array_equal(got["o_adj_bits"][n], pc.packed_rows(rec["o_adj"], RW)), (case.name, "o_adj_bits", t, n)


def _check_evader(case, env, row, t):
    eva = env.eva.cpu().numpy(); meta = env.meta.cpu().numpy(); tgt = env.target.cpu().numpy(); path = env.path.cpu().numpy()
    for n, rec in enumerate(row):
        assert np.array_equal(eva[n], rec["evader"]), (case.name, "evader", t, n, eva[n], rec["evader"])
        assert meta[n, 1] == rec["path_len"], (case.name, "path_len", t, n, meta[n, 1], rec["path_len"])
        assert meta[n, 2] == rec["tape_pos"], (case.name, "tape_pos", t, n)
        assert np.array_equal(tgt[n], rec["target"]), (case.name, "target", t, n)
        cnt, op = meta[n, 4], rec["path"]
        # the stored tail: path[cnt - 1] is the next waypoint, the oracle keeps the whole path
        assert 1 <= cnt <= min(len(op), case.cfg["max_path"]), (case.name, "path_cnt", t, n)
        assert np.array_equal(path[n, :cnt], op[len(op) - cnt:]), (case.name, "path", t, n)
    return meta


def _check_step(case, env, reward, raw, done, row, t):
    r_raw = raw.cpu().numpy(); r_n = reward.cpu().numpy(); defs = env.defenders_aos().cpu().numpy(); dn = done.cpu().numpy()
    for n, rec in enumerate(row):
        assert np.array_equal(r_raw[n], rec["raw"]), (case.name, "raw reward", t, n)
        assert np.array_equal(r_n[n], rec["norm"]), (case.name, "normalised reward", t, n)
        assert np.array_equal(defs[n], rec["defenders"]), (case.name, "defenders", t, n)
        assert bool(dn[n]) == rec["done"], (case.name, "done", t, n)


def run_case(case, overlap_replan=True, graph=False):
    """One run of a case on the device against the oracle's replay; returns every compared byte of the run (for the rerun)."""
    from distributed_multi_agent_reinforcement_learning_amd import pe_env
    init, actions, ticks = pc.replay(case.name)
    N, P, T = case.N, case.P, case.T
    env = pe_env.BatchedEnv(case.pe_config(), N)
    env.overlap_replan = overlap_replan
    env.load(init, reset_reward_norm=True)
    RW = pe_env.raser_row_words(env.c.O)
    obs = _new_obs(env, case)
    reward = torch.zeros((N, P), dtype=torch.float32, device="cuda")
    raw = torch.zeros((N, P), dtype=torch.float32, device="cuda")
    done = torch.zeros((N,), dtype=torch.uint8, device="cuda")
    trail = []
    graphed = 0
    max_len = 0

    def snap():
        trail.extend(v.cpu().numpy().tobytes() for v in obs.values())
        trail.extend(x.cpu().numpy().tobytes() for x in (env.eva, env.meta, env.target, env.defs, reward, raw))

    if case.mode == "fused":
        env.observe(obs); env.evader_step()
    for t in range(T):
        if case.mode == "split":
            env.observe(obs)
            _check_obs(case, {k: v.cpu().numpy() for k, v in obs.items()}, ticks[t], t, RW)
            env.evader_step()
        else:
            _check_obs(case, {k: v.cpu().numpy() for k, v in obs.items()}, ticks[t], t, RW)
        meta = _check_evader(case, env, ticks[t], t)
        max_len = max(max_len, int(meta[:, 1].max()))
        a = torch.as_tensor(actions[t]).cuda()
        if case.mode == "split" or t == T - 1:      # the last tick without its evader step: the replay ends with the step
            env.step(a, reward, raw, done)
        elif graph and not graphed and (env.t_host + 1) % env.c.difficulty != 0 and t >= 2:
            # the fused non-replan tick, captured and replayed once (the kernel itself ran eagerly on the ticks before)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with no_gc_during_capture(), torch.cuda.graph(g):
                env.tick(a, obs, reward, raw, done)
            g.replay()
            torch.cuda.synchronize()
            graphed += 1
        else:
            env.tick(a, obs, reward, raw, done)
        _check_step(case, env, reward, raw, done, ticks[t], t)
        snap()
    assert graphed == int(graph)
    # status: clean, except the exhausted bit exactly where the oracle's evader arrived more often than the tape is long
    pos = np.asarray([rec["tape_pos"] for rec in ticks[-1]])
    status = env.status().cpu().numpy()
    assert np.array_equal(status, np.where(pos > case.cfg["tape_len"], STATUS_TAPE_EXHAUSTED, 0)), (status, pos)
    if "tape_exhausted" in case.data:
        assert status.any() and not status.all()
    else:
        assert not status.any(), status
    if "path_longer_than_max_path" in case.data:
        assert max_len > case.cfg["max_path"] == env.c.max_path
    return trail


@pytest.mark.parametrize("case", pc.CASES, ids=repr)
def test_case_matches_oracle(case):
    first = run_case(case, graph=case.graph)
    if case.twice:
        # identical bytes on a second run; it takes the replans inside the fused tick (one launch) instead of on the side stream,
        # so pe_env_tick's replan form is held to the same oracle replay
        again = run_case(case, overlap_replan=False)
        assert len(first) == len(again) and all(a == b for a, b in zip(first, again))


@pytest.mark.parametrize("beams,radius", pc.LIDAR_SWEEP)
def test_lidar_full_map_sweep_matches_oracle(beams, radius):
    """k_build_raser at non-default beam counts and radii (1 / odd / PE_MAX_BEAMS beams; radius 0, 1, longer than the map): defenders
    parked on every cell of one 20 x 20 map, one observe launch, rows == the oracle's LiDAR of that cell, both forms of the rows."""
    from distributed_multi_agent_reinforcement_learning_amd import ops, pe_env
    from oracle import pe_oracle
    P, W, H, O = 4, 20, 20, 176
    N = W * H // P
    base = random_init(1, P, W, H, 2, 4, seed=31)
    init = {k: np.repeat(v, N, axis=0) for k, v in base.items()}
    cells = np.arange(N * P)
    frac = np.random.default_rng(2).uniform(0.0, 0.999, (N * P, 2))               # anywhere inside the cell: int() truncates
    init["defenders"][:, :, :2] = (np.stack((cells // H, cells % H), 1) + frac).reshape(N, P, 2)
    cfg = product_cfg(P, W, H, **{"sensor.num_beams": beams, "sensor.radius": radius})
    env = pe_env.BatchedEnv(pe_env.make_pe_config(cfg, tape_len=16, max_path=128), N)
    env.load(init, reset_reward_norm=True)
    k = int(base["n_obs"][0])
    oe = pe_oracle.OracleEnv(pe_oracle.make_config(W=W, H=H, P=P, O=O, num_beams=beams, lidar_radius=radius))
    oe.load(base["grid"][0], base["obs_xy"][0, :k], base["defenders"][0], base["evader"][0], base["target"][0], base["tape"][0])
    want = np.zeros((W * H, O), np.float32)
    for cell in range(W * H):
        want[cell, :k] = oe.lidar_cell(cell // H, cell % H)
    assert want.any() == (radius > 0)
    obs = env.new_obs()
    obs["o_adj_bits"] = env.new_obs(packed=True)["o_adj_bits"]
    env.observe(obs)
    assert np.array_equal(obs["o_adj"].cpu().numpy().reshape(W * H, O), want)
    assert torch.equal(ops.pack_adj_bits(obs["o_adj"]), obs["o_adj_bits"])


def test_device_reset_equals_host_reset_with_a_long_tape_and_more_obstacle_slots():
    """test_env_gpu.test_device_reset_equals_host_reset's assertions at tape_len = 40 (k_reset's tape loop past 32 entries, the tick's
    looped tape copy) and O = 260 (raser rows of 12 words), on a cfg1-sized batch."""
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config
    from distributed_multi_agent_reinforcement_learning_amd.pursuit_env import Pursuit_Env
    from distributed_multi_agent_reinforcement_learning_amd import pe_env
    num_envs = 18
    ov = {"runtime.num_envs": num_envs, "runtime.tape_len": 40, "map.num_max_obstacle": 260}
    eh = Pursuit_Env(baseline_config("cfg1", **ov, **{"runtime.device_reset": False}))
    ed = Pursuit_Env(baseline_config("cfg1", **ov, **{"runtime.device_reset": True}))
    assert isinstance(ed.resetter, pe_env.DeviceResetter) and isinstance(eh.resetter, pe_env.HostResetter)
    assert ed.sim.c.tape_len == 40 and ed.sim.c.O == 260 and ed.sim.tape.shape == (num_envs, 40, 2)
    g = torch.Generator(device="cuda").manual_seed(4)
    P = ed.sim.c.P
    for episode in range(3):
        eh.reset(); ed.reset()
        sh, sd = eh.sim, ed.sim
        for key in ("grid", "bidx", "n_obs", "target", "tape", "eva", "wpw", "raser"):
            assert torch.equal(getattr(sh, key), getattr(sd, key)), (episode, key)
        assert torch.equal(sh.defenders_aos(), sd.defenders_aos()), episode
        assert torch.equal(sh.o_state, sd.o_state), episode
        assert torch.equal(sh.meta, sd.meta), episode
        assert len({t.cpu().numpy().tobytes() for t in sd.tape[:, 32:]}) > 1       # entries past index 32 are drawn, and differ
        oh, od = sh.new_obs(), sd.new_obs()
        rh = torch.zeros(num_envs, P, device="cuda"); rd = torch.zeros_like(rh)
        eh.observe(oh); eh.attacker_step(); ed.observe(od); ed.attacker_step()
        for t in range(60):
            a = torch.randint(0, 9, (num_envs, P), generator=g, device="cuda", dtype=torch.int32)
            eh.tick(a, oh, rh); ed.tick(a, od, rd)
        torch.cuda.synchronize()
        assert torch.equal(sh.meta, sd.meta) and torch.equal(sh.eva, sd.eva)
        assert all(torch.equal(oh[k], od[k]) for k in oh)
        if episode == 0:
            assert int(sh.meta[:, pe_env.META_TAPE_POS].max().item()) > 0   # the rewind path is exercised


@pytest.mark.parametrize("path", trace_files("envcfg_trace_*.npz"), ids=lambda p: p.split("/")[-1][:-4])
def test_config_trace_matches_reference(path):
    """The device against the REFERENCE's own traces recorded off the default configuration (tests/golden/envcfg_trace_*.npz: beam
    count and radius, difficulty, extend_dis, evader view, tau / step size of both sides, communication and sensing range): every
    discrete output and the defenders' f64 state bit for bit, as test_env_gpu.test_trace_parity asserts at the default."""
    from distributed_multi_agent_reinforcement_learning_amd import pe_env
    d = load_trace(path)
    P, W, H, T, k = d["P"], d["W"], d["H"], d["T"], int(d["n_obs"])
    # the product's config.yaml has the reference's keys; make_pe_config converts each value to the field's type
    ov = {str(key): float(v) for keys, vals in (("cfg_keys", "cfg_vals"), ("late_keys", "late_vals")) for key, v in zip(d[keys], d[vals])}
    assert ov
    env = pe_env.BatchedEnv(pe_env.make_pe_config(product_cfg(P, W, H, T, **ov), tape_len=16, max_path=128), 1)
    env.load(init_from_traces([d]), reset_reward_norm=True)
    obs = env.new_obs()
    reward = torch.zeros((1, P), dtype=torch.float32, device="cuda")
    raw = torch.zeros((1, P), dtype=torch.float32, device="cuda")
    off = 0
    for t in range(T):
        env.observe(obs)
        o = {key: v.cpu().numpy()[0] for key, v in obs.items()}
        assert np.array_equal(o["p_state"], d["p_state"][t].astype(np.float32)), t
        assert np.array_equal(o["p_adj"], d["p_adj"][t].astype(np.float32)), t
        assert np.array_equal(o["e_adj"][:, 0], d["e_adj"][t, :, 0].astype(np.float32)), t
        assert np.array_equal(o["o_adj"][:, :k], d["o_adj"][t].astype(np.float32)) and not o["o_adj"][:, k:].any(), t
        env.evader_step()
        meta = env.meta.cpu().numpy()[0]
        L, cnt = int(d["path_len"][t]), int(meta[4])
        assert meta[1] == L, t
        assert np.array_equal(env.path.cpu().numpy()[0, :cnt], d["paths_cat"][off + L - cnt: off + L]), t
        off += L
        env.step(torch.as_tensor(d["action"][t][None]).cuda(), reward, raw)
        assert np.array_equal(raw.cpu().numpy()[0], d["reward"][t].astype(np.float32)), t
        assert np.array_equal(env.defenders_aos().cpu().numpy()[0], d["p_after"][t]), t
        assert np.array_equal(env.target.cpu().numpy()[0], d["target"][t]), t
    assert not env.status().any().item()
    assert int(env.meta[0, 3]) == int(d["collision_flag"]) and int(env.meta[0, 2]) == len(d["tape"])
