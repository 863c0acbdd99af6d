"""`algo.large_teams`: the key's parsing and the env_n2n learner's refusals around teams above 16 pursuers."""
import pytest


def _options(**ov):
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config
    from distributed_multi_agent_reinforcement_learning_amd.n2n_agent import N2nMAPPO
    cfg = baseline_config("cfg4_n2n", **ov)
    N2nMAPPO._options(N2nMAPPO.__new__(N2nMAPPO), cfg)
    return cfg


def test_the_key_defaults_to_false_and_parses():
    assert _options().algo.large_teams is False
    for P in (17, 64):
        assert _options(**{"env.num_defender": P, "algo.large_teams": True}).algo.large_teams is True
    assert _options(**{"env.num_defender": 17, "algo.large_teams": True, "algo.fcra_aggregator": "att"}).env.num_defender == 17


@pytest.mark.parametrize("ov,match", [({"env.num_defender": 17}, "env.num_defender.*algo.large_teams"),
                                      ({"env.num_defender": 65, "algo.large_teams": True}, "env.num_defender"),
                                      ({"env.num_defender": 17, "algo.large_teams": True, "algo.fcra_aggregator": "pool"}, "algo.fcra_aggregator"),
                                      ({"env.num_defender": 17, "algo.large_teams": True, "algo.embedding_dim": 64}, "algo.embedding_dim")])
def test_refusals_name_their_keys(ov, match):
    with pytest.raises(ValueError, match=match):
        _options(**ov)
