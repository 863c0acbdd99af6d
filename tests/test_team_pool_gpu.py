"""`algo.critic_team_pool`: the kernels of csrc/team_pool.hpp against tests/team_pool_ref.py in f64 on guarded buffers
(criterion of tests/test_pool_agg_gpu.py: err <= 4 x the torch formula's own fp32 error on CPU / GPU + 2e-5 max|reference|), bits,
refusals, and the agents with the key on."""
import ctypes as C
import functools

import pytest
import torch

from distributed_multi_agent_reinforcement_learning_amd import ops
from tests import team_pool_ref
from tests.test_pool_agg_gpu import FILL, GUARD, _within

pytestmark = pytest.mark.gpu
E, BAD_ARG = 128, 20001
NAMES = ("out", "d_feat", "d_score", "d_gate")
PS = [1, 2, 8, 9, 16, 17, 33, 64]      # the bucket edges and one past each
GS = [1, 5, 67]                        # 67: no multiple of the four waves, more than one workgroup at max_blocks 8
MASKS = ["all", "one", "random", "none"]


@functools.lru_cache(maxsize=None)
def _inputs(G, P, mask, scale=1.0):
    """-> feat, live, score, gate, g (CPU fp32); random: a fully dead group (the second) among live ones"""
    rn = functools.partial(torch.randn, generator=torch.manual_seed(1000 * G + P))
    feat, g, score, gate = rn(G, P, E), rn(G, P, E), scale * 0.2 * rn(E), 0.5 * rn(E)
    live = torch.zeros(G, P)
    if mask == "all":
        live[:] = 1
    elif mask == "one":
        live[torch.arange(G), torch.arange(G) % P] = 1
    elif mask == "random":
        live = (torch.rand(G, P, generator=torch.manual_seed(G + P)) < 0.6).float()
        live[0, 0] = 1
        live[1 % G] = 0
    return feat, live, score, gate, g


def _formula(fn, t, dtype, device):
    feat, live, score, gate, g = [v.to(device=device, dtype=dtype, copy=True) for v in t]   # (the cached inputs stay as they are)
    feat, score, gate = feat.requires_grad_(), score.requires_grad_(), gate.requires_grad_()
    out = fn(feat, live, score, gate)
    leaves = (feat, score, gate)           # (nobody live anywhere: the reference never touches score)
    return [out.detach().cpu()] + [torch.zeros_like(x).cpu() if v is None else v.cpu() for v, x in zip(torch.autograd.grad(out, leaves, g, allow_unused=True), leaves)]


@functools.lru_cache(maxsize=None)
def _noisy_reference(G, P, mask, scale=1.0):
    """(the f64 reference, the fp32 formula's distance from it per tensor: the larger of CPU and GPU); once per input set"""
    t = _inputs(G, P, mask, scale)
    ref = _formula(team_pool_ref.team_pool, t, torch.float64, "cpu")
    cpu, gpu = _formula(ops.team_pool_formula, t, torch.float32, "cpu"), _formula(ops.team_pool_formula, t, torch.float32, "cuda")
    return ref, [max((a.double() - r).abs().max().item(), (b.double() - r).abs().max().item()) for a, b, r in zip(cpu, gpu, ref)]


def _launch(t, max_blocks=8, u8=False):
    """both entry points on guarded outputs -> NAMES; the inputs must come back unchanged"""
    L = ops.load_library()
    feat, live, score, gate, g = [v.cuda() for v in t]
    live = (live != 0).to(torch.uint8) if u8 else live
    before = [v.clone() for v in (feat, live, score, gate, g)]
    G, P = feat.shape[:2]
    bufs = [torch.full((k + 2 * GUARD,), FILL, device="cuda") for k in (G * P * E, G * P * E, E, E)]
    out, d_feat, d_score, d_gate = [b[GUARD:-GUARD] for b in bufs]
    ws = torch.empty(L.team_pool_bwd_workspace(E, max_blocks), dtype=torch.uint8, device="cuda")
    head = (G, P, E, ops._ptr(feat), E, ops._ptr(live), int(u8), P, ops._ptr(score), ops._ptr(gate))
    assert L.team_pool_fwd(*head, ops._ptr(out), E, max_blocks, ops._stream()) == 0
    assert L.team_pool_bwd(*head, ops._ptr(g), E, ops._ptr(d_feat), E, ops._ptr(d_score), ops._ptr(d_gate), ops._ptr(ws), max_blocks, ops._stream()) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, (feat, live, score, gate, g))), "an input was written"
    for b, name in zip(bufs, NAMES):
        assert (b[:GUARD] == FILL).all() and (b[-GUARD:] == FILL).all(), f"{name}: a guard band was written"
        assert not (b[GUARD:-GUARD] == FILL).any(), f"{name}: an element was not written"
    return [out.view(G, P, E).clone(), d_feat.view(G, P, E).clone(), d_score.clone(), d_gate.clone()]


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("P", PS)
def test_kernels_against_f64(P, G, mask):
    ref, noise = _noisy_reference(G, P, mask)
    _within(_launch(_inputs(G, P, mask), u8=(P + G) % 2 == 1), ref, noise, f"P{P} G{G} {mask}", NAMES)


@pytest.mark.parametrize("P", [8, 33])
def test_scores_of_a_thousand_stay_finite_and_within_the_bound(P):
    t = _inputs(5, P, "random", 400.0)     # |s| = 400 * 0.2 * |N(0, 128)|: up to about 1e3
    assert (t[0] @ t[2]).abs().max() > 5e2
    ref, noise = _noisy_reference(5, P, "random", 400.0)
    _within(_launch(t), ref, noise, f"P{P} large scores", NAMES)


@pytest.mark.parametrize("P", [2, 9, 64])
def test_exact_cases_and_bits(P):
    feat, live, score, gate, g = _inputs(67, P, "random")
    assert torch.equal(_launch((feat, live, score, torch.zeros(E), g))[0].cpu(), feat), "gate = 0: out is not feat to the bit"
    # one live pursuer, the others' rows zero, gate one: every other row of out is c, which must be the live row to the bit
    _, one, *_ = _inputs(67, P, "one")
    f1 = feat * one.unsqueeze(-1)
    out = _launch((f1, one, score, torch.ones(E), g))[0].cpu()
    alive = f1[one != 0]
    assert all(torch.equal(out[k, i], alive[k]) for k in range(67) for i in range(P) if one[k, i] == 0)
    # two runs; groups 0, 1 and 66 launched alone
    a, b = _launch((feat, live, score, gate, g)), _launch((feat, live, score, gate, g))
    assert all(torch.equal(x, y) for x, y in zip(a, b)), "two runs differ"
    for k in (0, 1, 66):
        alone = _launch((feat[k:k + 1], live[k:k + 1], score, gate, g[k:k + 1]))
        assert torch.equal(alone[0][0], a[0][k]) and torch.equal(alone[1][0], a[1][k]), f"group {k} depends on its launch"


@pytest.mark.parametrize("what,change", [("P=0", dict(P=0)), ("P=65", dict(P=65)), ("E=64", dict(E=64)), ("feat NULL", dict(feat=None)),
                                         ("G=0", dict(G=0))], ids=lambda v: v if isinstance(v, str) else "")
def test_refusals_leave_the_outputs_untouched(what, change):
    L, G, P = ops.load_library(), 3, 4
    feat, live, score, gate, g = [v.cuda() for v in _inputs(G, P, "all")]
    outs = [torch.full((k,), FILL, device="cuda") for k in (G * P * E, G * P * E, E, E)]
    ws = torch.empty(L.team_pool_bwd_workspace(E, 0), dtype=torch.uint8, device="cuda")
    a = {**dict(G=G, P=P, E=E, feat=feat), **change}
    head = (a["G"], a["P"], a["E"], ops._ptr(a["feat"]), E, ops._ptr(live), 0, P, ops._ptr(score), ops._ptr(gate))
    rc_f = L.team_pool_fwd(*head, ops._ptr(outs[0]), E, 0, ops._stream())
    rc_b = L.team_pool_bwd(*head, ops._ptr(g), E, ops._ptr(outs[1]), E, ops._ptr(outs[2]), ops._ptr(outs[3]), ops._ptr(ws), 0, ops._stream())
    torch.cuda.synchronize()
    assert rc_f == rc_b == (0 if what == "G=0" else BAD_ARG), (what, rc_f, rc_b)
    assert all((o == FILL).all() for o in outs), f"{what}: an output was written"


CFG = {"e3d": ("cfg5", {"runtime.num_envs": 8, "env.max_steps": 10, "env.num_defender": 3, "runtime.e3d_evader": "rule"}),
       "n2n": ("cfg4_n2n", {"runtime.num_envs": 8, "env.max_steps": 10, "runtime.n2n_evader": "rule"}),
       "n2n17": ("cfg4_n2n", {"runtime.num_envs": 8, "env.max_steps": 10, "runtime.n2n_evader": "rule", "env.num_defender": 17, "algo.large_teams": True})}


def _trainer(kind, on=True):
    from distributed_multi_agent_reinforcement_learning_amd import e3d_agent, n2n_agent
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config
    cfg = baseline_config(CFG[kind][0], **CFG[kind][1], **{"algo.epochs": 2}, **({"algo.critic_team_pool": "attention"} if on else {}))
    return (e3d_agent.E3dTrainer if kind == "e3d" else n2n_agent.N2nTrainer)(cfg, num_eval_envs=4, eval_every=1)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("kind", list(CFG))
def test_agent_starts_as_the_off_agent_trains_and_refuses_the_other_setting(kind, tmp_path):
    on, off = _trainer(kind), _trainer(kind, on=False)
    critic = on.agent.critic
    assert list(critic.state_dict())[-2:] == ["team_pool.score", "team_pool.gate"] and on.agent.ac_parameters[-1] is critic.team_pool.gate
    calls = ops.team_pool_calls
    buf_on, buf_off = on.agent.explore_env(on.env)[1], off.agent.explore_env(off.env)[1]
    T = buf_on["r"].shape[1]
    assert ops.team_pool_calls == calls + T + 1, "one launch a tick and one for the bootstrap value"
    assert buf_on.keys() == buf_off.keys() and all(torch.equal(buf_on[k], buf_off[k]) for k in buf_on), "gate = 0 is not the off-agent"
    on.iterate()
    gs, gg = critic.team_pool.score.grad, critic.team_pool.gate.grad
    assert torch.isfinite(gs).all() and torch.isfinite(gg).all() and gg.abs().max() > 0
    # random parameters: the rollout's values are the update forward's on the live rows, within the agents' own 1e-4
    with torch.no_grad():
        critic.team_pool.score.copy_(0.3 * torch.randn(E)), critic.team_pool.gate.copy_(0.3 * torch.randn(E))
    buf = on.agent.explore_env(on.env)[1]
    N = on.env.num_envs
    values = (on.agent.sequence_forward(buf["feat_a"], buf["feat_c"], N, T, live=buf["active"]) if kind == "e3d"
              else on.agent.sequence_forward(buf, 0, N))[1]
    live = buf["active"] == 1
    err = (values.detach() - buf["v_n"][:, :T])[live].abs().max().item()
    print(f"{kind}: live rows {int(live.sum())} of {live.numel()}, value error {err:.3e}")
    assert live.sum() > 0 and err <= 1e-4
    # save / load round-trips; a file of the other setting is refused by name
    path = str(tmp_path / "resume.pt")
    on.save_resume(path), on.agent.save_model(str(tmp_path / "on")), off.agent.save_model(str(tmp_path / "off"))
    again = _trainer(kind)
    again.agent.load_model(str(tmp_path / "on"))
    assert all(torch.equal(x, y) for x, y in zip(critic.state_dict().values(), again.agent.critic.state_dict().values()))
    again.load_resume(path)
    for load in (lambda: off.load_resume(path), lambda: off.agent.load_model(str(tmp_path / "on")), lambda: on.agent.load_model(str(tmp_path / "off"))):
        with pytest.raises(ValueError, match="algo.critic_team_pool"):
            load()
