"""The flagship learner (MAPPO / Trainer) and the env_3d / env_n2n learners (ParticleMAPPO / ParticleTrainer) share ONE set of option
validators (options.py), ONE imitation schedule, optimiser schedule and phase step (imitation.py) and ONE read-back at the end of
train() (readback.py).  The ValueError texts are the ones the per-feature parsers had before they were folded.  No GPU needed."""
import math
import types

import pytest
import torch

from distributed_multi_agent_reinforcement_learning_amd import imitation, kickstart, minibatch_steps, options, pursuit_imitation, readback
from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config
from distributed_multi_agent_reinforcement_learning_amd.mappo import MAPPO
from distributed_multi_agent_reinforcement_learning_amd.particle_agent import BcSums, ParticleMAPPO

NAN = float("nan")


# ---- sharing by identity --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["set_lr", "reset_optimizer", "lr_decay"])
def test_both_agents_have_the_same_optimiser_schedule(name):
    assert getattr(MAPPO, name) is getattr(ParticleMAPPO, name) is getattr(imitation.OptimizerSchedule, name)


def test_the_flagship_options_are_imitation_options():
    o = pursuit_imitation.pursuit_imitation_options(baseline_config("cfg2", **{"algo.pathfinder_bc_iterations": 2}))
    assert isinstance(o, imitation.ImitationOptions) and o.on and o.cache is True
    assert isinstance(imitation.imitation_options(baseline_config("cfg5")), imitation.ImitationOptions)
    assert pursuit_imitation.schedule is imitation.schedule
    assert pursuit_imitation.check_iterations_entry is imitation.check_iterations_entry
    assert pursuit_imitation.follow_count is imitation.follow_count


def test_the_per_module_validators_are_the_shared_ones():
    assert imitation.real is kickstart.real is options.real
    assert imitation.count is kickstart.count is options.count
    assert imitation.flag is pursuit_imitation.flag is minibatch_steps.flag is options.flag
    assert readback.BcSums is BcSums
    for mod in (imitation, kickstart, pursuit_imitation, minibatch_steps):
        assert not hasattr(mod, "_real") and not hasattr(mod, "_flag")


# ---- message parity: the texts of the parsers before they shared their validators, as literals ---------------------------------------------
def _number_cases(key, low, low_text, real_text=" is not a finite number"):
    """a key that wants a number: a bool, a string, nan, and one value out of its range"""
    return [(key, True, f"{key}: True{real_text}"), (key, "half", f"{key}: 'half'{real_text}"), (key, NAN, f"{key}: nan{real_text}"),
            (key, low, f"{key}: {low}{low_text}")]


def _integer_cases(key):
    return _number_cases(key, -1, " is not an integer >= 0", " is not an integer >= 0") + [(key, 1.5, f"{key}: 1.5 is not an integer >= 0")]


def _flag_cases(key):
    """a key that wants true or false: a number, a string, nan"""
    return [(key, 1, f"{key}: 1 is not true or false"), (key, "yes", f"{key}: 'yes' is not true or false"),
            (key, NAN, f"{key}: nan is not true or false")]


def _schedule_cases(prefix):
    return (_integer_cases(prefix + "iterations") + _number_cases(prefix + "beta", 1.5, " is not in [0, 1]")
            + _number_cases(prefix + "beta", -0.25, " is not in [0, 1]")[3:] + _number_cases(prefix + "beta_decay", 0.0, " is not in (0, 1]")
            + _number_cases(prefix + "beta_decay", 1.5, " is not in (0, 1]")[3:] + _number_cases(prefix + "lr", 0.0, " is not > 0")
            + [(prefix + "lr", 0, f"{prefix}lr: 0.0 is not > 0")])     # an integer is shown as the float it became


PARSERS = {
    "bc": ("cfg5", imitation.imitation_options,
           _schedule_cases("algo.bc_") + _number_cases("algo.bc_target_bound", 1.0, " is not in (0, 1)")
           + _number_cases("algo.bc_target_bound", 0.0, " is not in (0, 1)")[3:] + _flag_cases("algo.bc_fit_std") + _flag_cases("algo.bc_heading_wrap")),
    "pathfinder_bc": ("cfg2", pursuit_imitation.pursuit_imitation_options,
                      _schedule_cases("algo.pathfinder_bc_") + _flag_cases("runtime.pathfinder_cache")
                      + [("runtime.pathfinder_cache", None, "runtime.pathfinder_cache: None is not true or false")]),
    "bc_coef": ("cfg4_n2n", kickstart.kickstart_options,
                _number_cases("algo.bc_coef", -0.5, " is not >= 0") + _number_cases("algo.bc_coef_decay", 0.0, " is not in (0, 1]")
                + _number_cases("algo.bc_coef_decay", 1.5, " is not in (0, 1]")[3:] + _integer_cases("algo.bc_coef_iterations")),
    "minibatch_steps": ("cfg5", minibatch_steps.minibatch_steps_options, _flag_cases("algo.minibatch_steps")),
}
PARITY = [(which, key, value, text) for which, (_, _, cases) in PARSERS.items() for key, value, text in cases]


@pytest.mark.parametrize("which,key,value,text", PARITY, ids=[f"{k}={v!r}" for _, k, v, _ in PARITY])
def test_the_error_texts_are_the_parsers_own(which, key, value, text):
    name, parse, _ = PARSERS[which]
    with pytest.raises(ValueError) as e:
        parse(baseline_config(name, **{key: value}))
    assert str(e.value) == text


def test_the_literal_texts_spelled_out():
    """a few of PARITY's texts in full, so that a slip in the helpers above cannot hide one in the package"""
    texts = {(k, repr(v)): t for _, k, v, t in PARITY}
    assert texts["algo.bc_iterations", "True"] == "algo.bc_iterations: True is not an integer >= 0"
    assert texts["algo.pathfinder_bc_iterations", "'half'"] == "algo.pathfinder_bc_iterations: 'half' is not an integer >= 0"
    assert texts["algo.bc_beta", "nan"] == "algo.bc_beta: nan is not a finite number"
    assert texts["algo.pathfinder_bc_beta", "1.5"] == "algo.pathfinder_bc_beta: 1.5 is not in [0, 1]"
    assert texts["algo.pathfinder_bc_beta_decay", "0.0"] == "algo.pathfinder_bc_beta_decay: 0.0 is not in (0, 1]"
    assert texts["algo.bc_lr", "0"] == "algo.bc_lr: 0.0 is not > 0"
    assert texts["algo.bc_target_bound", "1.0"] == "algo.bc_target_bound: 1.0 is not in (0, 1)"
    assert texts["algo.bc_coef", "-0.5"] == "algo.bc_coef: -0.5 is not >= 0"
    assert texts["algo.bc_coef_decay", "True"] == "algo.bc_coef_decay: True is not a finite number"
    assert texts["algo.bc_coef_iterations", "-1"] == "algo.bc_coef_iterations: -1 is not an integer >= 0"
    assert texts["runtime.pathfinder_cache", "'yes'"] == "runtime.pathfinder_cache: 'yes' is not true or false"
    assert texts["algo.minibatch_steps", "1"] == "algo.minibatch_steps: 1 is not true or false"


def test_resume_entry_texts():
    agent = types.SimpleNamespace(imitation=imitation.imitation_options(baseline_config("cfg5", **{"algo.bc_iterations": 2})),
                                  pathfinder_bc=pursuit_imitation.pursuit_imitation_options(baseline_config("cfg2")))
    imitation.check_entry(agent, 2, "bundle b")
    pursuit_imitation.check_entry(agent, None, "bundle b")
    with pytest.raises(ValueError) as e:
        imitation.check_entry(agent, None, "bundle b")
    assert str(e.value) == "bundle b was written with algo.bc_iterations: 0, this agent has algo.bc_iterations: 2"
    with pytest.raises(ValueError) as e:
        pursuit_imitation.check_entry(agent, 3, "bundle b")
    assert str(e.value) == "bundle b was written with algo.pathfinder_bc_iterations: 3, this agent has algo.pathfinder_bc_iterations: 0"


def test_follow_mask():
    for beta, n in ((0.0, 16), (0.5, 16), (1.0, 16), (0.26, 16), (0.5, 5)):
        m = imitation.follow_mask(beta, n, "cpu")
        k = imitation.follow_count(beta, n)
        assert m.dtype == torch.uint8 and m.shape == (n,) and m.tolist() == [1] * k + [0] * (n - k)


# ---- the read-back ----------------------------------------------------------------------------------------------------------------------------
class _Part:
    def __init__(self, values, log, reduce=True):
        self.sums = torch.tensor(values, dtype=torch.float64)
        self.allreduce = (lambda t: log.append(t)) if reduce else None


@pytest.fixture
def host_reads(monkeypatch):
    """counts the tensors that go to the host: every Tensor.tolist / .cpu / .item / .numpy call"""
    calls = []
    for name in ("tolist", "cpu", "item", "numpy"):
        orig = getattr(torch.Tensor, name)
        monkeypatch.setattr(torch.Tensor, name, lambda self, *a, _o=orig, _n=name, **k: (calls.append((_n, self)), _o(self, *a, **k))[1])
    return calls


def test_read_back_groups_reduces_each_part_once_and_reads_once(host_reads):
    log = []
    big = 2 ** 24 + 1                                   # an integer count that float32 cannot hold
    third = float(torch.tensor(1.0 / 3.0, dtype=torch.float32).double())
    host_reads.clear()
    a = _Part([1.5, -2.0], log)
    b = _Part([0.1, 0.2, 0.3], log, reduce=False)
    c = _Part([float(i) + 1e-9 for i in range(8)], log)
    scalars = (0.25, torch.tensor(1.0 / 3.0, dtype=torch.float32), torch.tensor(big, dtype=torch.int64), -7.0)
    out = readback.read_back(scalars, a, None, b, (torch.tensor(big + 2, dtype=torch.int64),), c)
    assert len(log) == 2 and log[0] is a.sums and log[1] is c.sums           # once each, on its own tensor, in the order added
    assert [None if g is None else len(g) for g in out] == [4, 2, None, 3, 1, 8]
    assert out[0] == [0.25, third, float(big), -7.0] and out[4] == [float(big + 2)]
    assert out[1] == [1.5, -2.0] and out[3] == [0.1, 0.2, 0.3] and out[5] == [float(i) + 1e-9 for i in range(8)]
    assert all(type(v) is float for g in out if g is not None for v in g)
    assert int(out[0][2]) == big and int(out[4][0]) == big + 2
    assert len(host_reads) == 1 and host_reads[0][0] == "tolist" and host_reads[0][1].dtype == torch.float64


def test_read_back_with_every_feature_off_calls_nothing_else(host_reads):
    out = readback.read_back((0.5, torch.tensor(2.0 ** -30, dtype=torch.float64)), None, None, None, None)
    assert out == [[0.5, 2.0 ** -30], None, None, None, None]
    assert len(host_reads) == 1
    (vals,) = readback.read_back((1.0, 2.0))
    assert vals == [1.0, 2.0]


def test_update_diag_read_keeps_its_return_value():
    from distributed_multi_agent_reinforcement_learning_amd.update_diag import LOG_KEYS, UpdateDiag, derive
    log = []
    d = UpdateDiag("cpu")
    d.allreduce = log.append
    d.begin()
    d.sums.copy_(torch.tensor([10.0, 0.5, 2.0, 7.0, 3.0, 4.0, 1.0, 10.5], dtype=torch.float64))
    want = derive(d.sums.tolist())
    vals, out = d.read(torch.tensor(0.125, dtype=torch.float64), 3.0)
    assert vals == [0.125, 3.0] and len(log) == 1 and log[0] is d.sums
    assert tuple(out) == LOG_KEYS and math.isnan(out.pop("grad_norm")) and out == want     # no norm was noted
    d.note_grad_norm(torch.tensor(2.5))
    assert d.read(1.0)[1]["grad_norm"] == 2.5 and d.last_sums == d.sums.tolist()


# ---- the phase step ---------------------------------------------------------------------------------------------------------------------------
class _Agent:
    def __init__(self):
        self.calls = []

    def set_lr(self, lr):
        self.calls.append(("set_lr", lr))

    def reset_optimizer(self, total_steps):
        self.calls.append(("reset_optimizer", total_steps))


def test_phase_step_over_a_two_iteration_phase():
    K = 2
    o = imitation.ImitationOptions(K, 0.8, 0.5, 1e-3)
    for k in range(K + 2):
        agent = _Agent()
        got = imitation.phase_step(agent, o, k, 1000 + k)
        if k < K:
            assert got == (True, 0.8 * 0.5 ** k) and agent.calls == [("set_lr", 1e-3)]
        elif k == K:
            assert got == (False, None) and agent.calls == [("reset_optimizer", 1000 + K)]
        else:
            assert got == (False, None) and agent.calls == []


def test_phase_step_with_the_feature_off_touches_nothing():
    agent = _Agent()
    o = imitation.ImitationOptions(0, 1.0, 1.0, 1e-3)
    assert [imitation.phase_step(agent, o, k, 5) for k in range(4)] == [(False, None)] * 4 and agent.calls == []


def test_reset_optimizer_clears_adam_and_returns_to_the_schedule():
    class Agent(imitation.OptimizerSchedule):
        lr, max_train_steps, use_lr_decay = 0.01, 1000, True

    agent = Agent()
    w = torch.nn.Parameter(torch.ones(3))
    agent.ac_optimizer = torch.optim.Adam([w], lr=agent.lr)
    w.grad = torch.ones(3)
    agent.ac_optimizer.step()
    agent.set_lr(0.5)
    agent.reset_optimizer(250)
    st = agent.ac_optimizer.state[w]
    assert float(st["step"]) == 0 and not st["exp_avg"].any() and not st["exp_avg_sq"].any()
    assert agent.ac_optimizer.param_groups[0]["lr"] == 0.01 * (1 - 250 / 1000) and agent.total_step == 250
    agent.use_lr_decay = False
    agent.set_lr(0.5)
    agent.reset_optimizer(500)
    assert agent.ac_optimizer.param_groups[0]["lr"] == 0.01
