"""`algo.critic_team_pool_heads` (DESIGN 7z'): the kernels of csrc/team_pool_heads.hpp against ops.team_pool_formula(heads=H) in f64 on
guarded buffers (the criterion of tests/test_team_pool_gpu.py: err <= 4 x the torch formula's own fp32 error on CPU / GPU + 2e-5
max|reference|), bits, the heads' separation, refusals, and the agents with the key on."""
import functools

import pytest
import torch

from distributed_multi_agent_reinforcement_learning_amd import ops
from tests.test_pool_agg_gpu import FILL, GUARD, _within
from tests.test_team_pool_gpu import BAD_ARG, E, NAMES, _formula, _inputs

pytestmark = pytest.mark.gpu
HS = [2, 4, 8]
KEY, HEADS_KEY = "algo.critic_team_pool", "algo.critic_team_pool_heads"


@functools.lru_cache(maxsize=None)
def _noisy_reference(G, P, mask, H):
    """(the f64 reference, the fp32 formula's distance from it per tensor: the larger of CPU and GPU); once per input set"""
    t, fn = _inputs(G, P, mask), functools.partial(ops.team_pool_formula, heads=H)
    ref = _formula(fn, t, torch.float64, "cpu")
    cpu, gpu = _formula(fn, t, torch.float32, "cpu"), _formula(fn, t, torch.float32, "cuda")
    return ref, [max((a.double() - r).abs().max().item(), (b.double() - r).abs().max().item()) for a, b, r in zip(cpu, gpu, ref)]


def _call(dev, outs, H, max_blocks):
    """both entry points on the device tensors feat, live, score, gate, g -> their return codes"""
    L, (feat, live, score, gate, g), (G, P) = ops.load_library(), dev, dev[0].shape[:2]
    ws = torch.empty(L.team_pool_bwd_workspace(E, max_blocks), dtype=torch.uint8, device="cuda")
    head = (G, P, E, ops._ptr(feat), E, ops._ptr(live), int(live.dtype == torch.uint8), P, ops._ptr(score), ops._ptr(gate))
    rc = (L.team_pool_heads_fwd(*head, ops._ptr(outs[0]), E, H, max_blocks, ops._stream()),
          L.team_pool_heads_bwd(*head, ops._ptr(g), E, ops._ptr(outs[1]), E, ops._ptr(outs[2]), ops._ptr(outs[3]), ops._ptr(ws), H, max_blocks, ops._stream()))
    torch.cuda.synchronize()
    return rc


def _launch(t, H, max_blocks=1, u8=False):
    """both entry points on guarded outputs -> NAMES; the inputs must come back unchanged.  max_blocks 1: five groups are a second trip"""
    dev = [v.cuda() for v in t]
    dev[1] = (dev[1] != 0).to(torch.uint8) if u8 else dev[1]
    before = [v.clone() for v in dev]
    G, P = dev[0].shape[:2]
    bufs = [torch.full((k + 2 * GUARD,), FILL, device="cuda") for k in (G * P * E, G * P * E, E, E)]
    out, d_feat, d_score, d_gate = [b[GUARD:-GUARD] for b in bufs]
    assert _call(dev, (out, d_feat, d_score, d_gate), H, max_blocks) == (0, 0)
    assert all(torch.equal(a, b) for a, b in zip(before, dev)), "an input was written"
    for b, name in zip(bufs, NAMES):
        assert (b[:GUARD] == FILL).all() and (b[-GUARD:] == FILL).all(), f"{name}: a guard band was written"
        assert not (b[GUARD:-GUARD] == FILL).any(), f"{name}: an element was not written"
    return [out.view(G, P, E).clone(), d_feat.view(G, P, E).clone(), d_score.clone(), d_gate.clone()]


@pytest.mark.parametrize("mask", ["all", "one", "random", "none"])
@pytest.mark.parametrize("G", [1, 5])
@pytest.mark.parametrize("P", [1, 2, 8, 9, 17, 64])   # every bucket, one past a bucket, below and above every lane group
@pytest.mark.parametrize("H", HS)
def test_kernels_against_f64(H, P, G, mask):
    t = feat, live, score, gate, g = _inputs(G, P, mask)
    ref, noise = _noisy_reference(G, P, mask, H)
    got = _launch(t, H, u8=(P, G, mask) == (9, 5, "random"))
    _within(got, ref, noise, f"H{H} P{P} G{G} {mask}", NAMES)
    if mask == "one":
        # ds = w (a - e) of the only live row is 0 exactly; with the others' rows zero and gate one every other row of out is c = that row
        assert (got[2] == 0).all(), "one live row: d_score is not exactly 0"
        f1 = feat * live.unsqueeze(-1)
        out, alive = _launch((f1, live, score, torch.ones(E), g), H)[0].cpu(), f1[live != 0]
        assert all(torch.equal(out[k, i], alive[k]) for k in range(G) for i in range(P) if live[k, i] == 0), "c is not the live row to the bit"
    if mask == "random" and G == 5:
        assert all(torch.equal(x, y) for x, y in zip(got, _launch(t, H))), "two runs differ"
        alone = _launch((feat[:1], live[:1], score, gate, g[:1]), H)
        assert torch.equal(alone[0][0], got[0][0]) and torch.equal(alone[1][0], got[1][0]), "group 0 depends on its launch"


@pytest.mark.parametrize("P", [9, 64])
@pytest.mark.parametrize("H", HS)
def test_a_score_in_head_0_leaves_the_other_heads_at_the_live_mean(H, P):
    """unless a butterfly crosses a lane-group boundary"""
    feat, live, score, _, g = _inputs(5, P, "random")
    D = E // H
    t = (feat, live, torch.cat([score[:D], torch.zeros(E - D)]), torch.ones(E), g)
    on = (live != 0).double().unsqueeze(-1)
    ref = (feat.double() + (feat.double() * on).sum(1, keepdim=True) / on.sum(1, keepdim=True).clamp_min(1))[..., D:]
    fn = functools.partial(ops.team_pool_formula, heads=H)
    noise = max((fn(*[v.to(dev) for v in t[:4]]).cpu().double()[..., D:] - ref).abs().max().item() for dev in ("cpu", "cuda"))
    _within([_launch(t, H)[0][..., D:]], [ref], [noise], f"H{H} P{P} heads 1 .. {H - 1}", ["out"])


@pytest.mark.parametrize("heads", [0, 1, 3, 16])
def test_other_head_counts_are_refused_without_a_write(heads):
    outs = [torch.full((k,), FILL, device="cuda") for k in (3 * 4 * E, 3 * 4 * E, E, E)]
    assert _call([v.cuda() for v in _inputs(3, 4, "all")], outs, heads, 0) == (BAD_ARG, BAD_ARG)
    assert all((o == FILL).all() for o in outs), f"heads={heads}: an output was written"


CFG = {"e3d": ("cfg5", {"runtime.num_envs": 16, "env.max_steps": 10, "env.num_defender": 3, "runtime.e3d_evader": "rule"}),
       "n2n": ("cfg4_n2n", {"runtime.num_envs": 8, "env.max_steps": 10, "runtime.n2n_evader": "rule"})}


def _trainer(kind, heads=4):   # None: the off-agent; 1: the pool with the key absent
    from distributed_multi_agent_reinforcement_learning_amd import e3d_agent, n2n_agent
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config
    keys = {} if heads is None else {KEY: "attention"} if heads == 1 else {KEY: "attention", HEADS_KEY: heads}
    cfg = baseline_config(CFG[kind][0], **CFG[kind][1], **{"algo.epochs": 2}, **keys)
    return (e3d_agent.E3dTrainer if kind == "e3d" else n2n_agent.N2nTrainer)(cfg, num_eval_envs=4, eval_every=1)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("kind", list(CFG))
def test_agent_starts_as_the_off_agent_trains_resumes_and_refuses_other_files(kind, tmp_path):
    on, off = _trainer(kind), _trainer(kind, None)
    critic = on.agent.critic
    assert list(critic.state_dict())[-3:] == ["team_pool.score", "team_pool.gate", "team_pool.heads"] and int(critic.team_pool.heads) == 4
    buf_on, buf_off = on.agent.explore_env(on.env)[1], off.agent.explore_env(off.env)[1]
    assert buf_on.keys() == buf_off.keys() and all(torch.equal(buf_on[k], buf_off[k]) for k in buf_on), "gate = 0 is not the off-agent"
    on.iterate(), on.iterate()
    sd = critic.state_dict()
    assert all(torch.isfinite(v).all() for v in sd.values()) and sd["team_pool.score"].abs().max() > 0, "two iterations leave score at zero"
    path, again = str(tmp_path / "resume.pt"), _trainer(kind)   # a resume after iteration 2 continues bit for bit
    on.save_resume(path), on.iterate(), again.load_resume(path), again.iterate()
    assert all(torch.equal(x, y) for x, y in zip(critic.state_dict().values(), again.agent.critic.state_dict().values()))
    # files of one head, of two heads and of the off-agent are refused by name, and so is this agent's file by each of them
    on.agent.save_model(str(tmp_path / "h4"))
    for heads, key in ((1, HEADS_KEY), (2, HEADS_KEY), (None, KEY)):
        other = _trainer(kind, heads)
        other.agent.save_model(str(tmp_path / "other"))
        for load in (lambda: other.load_resume(path), lambda: other.agent.load_model(str(tmp_path / "h4")), lambda: on.agent.load_model(str(tmp_path / "other"))):
            with pytest.raises(ValueError, match=key):
                load()
