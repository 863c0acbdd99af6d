"""The env_3d and env_n2n learners share ONE update loop, trainer and result normaliser (particle_agent.py): the agent modules inherit
them and override none, so an option written into the shared core reaches both.  No GPU needed."""
import pytest
import torch

from distributed_multi_agent_reinforcement_learning_amd.e3d_agent import E3dMAPPO, E3dTrainer
from distributed_multi_agent_reinforcement_learning_amd.n2n_agent import N2nMAPPO, N2nTrainer
from distributed_multi_agent_reinforcement_learning_amd.particle_agent import ParticleMAPPO, ParticleTrainer, episode_triple
from distributed_multi_agent_reinforcement_learning_amd.trainer import ParticleRunState


@pytest.mark.parametrize("name", ["__init__", "train", "lr_decay", "explore_env", "_state"])
def test_the_agents_inherit_the_update_loop(name):
    assert getattr(E3dMAPPO, name) is getattr(N2nMAPPO, name) is getattr(ParticleMAPPO, name)


@pytest.mark.parametrize("name", ["__init__", "iterate", "evaluate", "baseline", "make_eval_env", "last_breakdown_ms", "save_resume",
                                  "load_resume", "record_evaluation"])
def test_the_trainers_inherit_the_trainer(name):
    base = ParticleRunState if name in ("save_resume", "load_resume", "record_evaluation") else ParticleTrainer
    assert getattr(E3dTrainer, name) is getattr(N2nTrainer, name) is getattr(base, name)


def test_each_trainer_names_its_agent_and_environment():
    from distributed_multi_agent_reinforcement_learning_amd import e3d_agent, n2n_agent
    assert E3dTrainer.agent_cls is E3dMAPPO and E3dTrainer.make_env is e3d_agent.make_env and not E3dTrainer.log_breakdown
    assert N2nTrainer.agent_cls is N2nMAPPO and N2nTrainer.make_env is n2n_agent.make_env and N2nTrainer.log_breakdown


def test_the_base_agent_has_the_defaults_the_run_protocol_reads():
    agent = ParticleMAPPO.__new__(ParticleMAPPO)
    assert agent.obs_norm is None and agent.policy_meta() is None and agent.check_policy_meta({"gauss_std": "state"}, "a file") is None
    assert N2nMAPPO.policy_meta is ParticleMAPPO.policy_meta and N2nMAPPO.check_policy_meta is ParticleMAPPO.check_policy_meta
    assert E3dMAPPO.policy_meta is not ParticleMAPPO.policy_meta and E3dMAPPO.check_policy_meta is not ParticleMAPPO.check_policy_meta


def test_episode_triple_of_a_tuple_and_of_an_accumulator_dict():
    ret = torch.tensor([1.5, -2.0, 0.25, 7.0, -0.5])
    length = torch.tensor([12.0, 3.0, 12.0, 7.0, 1.0])
    flag = torch.tensor([1, 0, 0, 1, 1], dtype=torch.uint8)
    acc = dict(done_before=torch.ones(5), ended=torch.zeros(5), captured=flag, ret=ret, length=length)
    given = (ret, flag != 0, length)
    from_tuple, from_dict = episode_triple(given), episode_triple(acc)
    assert from_tuple is given                                       # env_3d's triple passes through
    assert len(from_dict) == 3 and from_dict[1].dtype == torch.bool
    for a, b in zip(from_tuple, from_dict):
        assert a.dtype == b.dtype and torch.equal(a, b)
    # the capture rate does not depend on which form the flag had
    assert from_dict[1].float().mean().item() == flag.float().mean().item() == pytest.approx(0.6)
