"""CPU-side checks of the flagship's imitation warm start (algo.pathfinder_bc_iterations): the option validators,
what MAPPO keeps refusing, and the teacher launch's C boundary against the ctypes declarations."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

from tests.conftest import ROOT


def _options(**ov):
    from distributed_multi_agent_reinforcement_learning_amd import pursuit_imitation as pi
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config
    return pi.pursuit_imitation_options(baseline_config("cfg2", **ov))


def test_defaults():
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config
    o = _options()
    assert (o.iterations, o.beta, o.beta_decay, o.cache, o.on) == (0, 1.0, 1.0, True, False)
    assert o.lr == float(baseline_config("cfg2").algo.lr)
    o = _options(**{"algo.pathfinder_bc_iterations": 3, "algo.lr": 0.002})
    assert o.on and o.iterations == 3 and o.lr == 0.002          # pathfinder_bc_lr defaults to algo.lr
    o = _options(**{"algo.pathfinder_bc_iterations": 3, "algo.pathfinder_bc_lr": 1e-4, "algo.pathfinder_bc_beta": 0.0,
                    "algo.pathfinder_bc_beta_decay": 0.5, "runtime.pathfinder_cache": False})
    assert (o.lr, o.beta, o.beta_decay, o.cache) == (1e-4, 0.0, 0.5, False)


def test_beta_at_and_follow_count():
    from distributed_multi_agent_reinforcement_learning_amd import pursuit_imitation as pi
    o = _options(**{"algo.pathfinder_bc_iterations": 4, "algo.pathfinder_bc_beta": 0.8, "algo.pathfinder_bc_beta_decay": 0.5})
    assert [o.beta_at(k) for k in range(3)] == [0.8, 0.4, 0.2]
    assert _options().beta_at(7) == 1.0
    assert [pi.follow_count(b, 16) for b in (0.0, 0.5, 1.0, 0.26)] == [0, 8, 16, 4]


BAD = [("algo.pathfinder_bc_iterations", v) for v in (-1, 1.5, True, "3", None)] + \
      [("algo.pathfinder_bc_beta", v) for v in (-0.1, 1.1, float("nan"), float("inf"), True, "half")] + \
      [("algo.pathfinder_bc_beta_decay", v) for v in (0.0, -0.5, 1.01, float("nan"), False, "slow")] + \
      [("algo.pathfinder_bc_lr", v) for v in (0.0, -1e-3, float("inf"), float("nan"), True, "small")] + \
      [("runtime.pathfinder_cache", v) for v in (0, 1, "true", None, 0.5)]


@pytest.mark.parametrize("key,value", BAD)
def test_bad_values_raise_and_name_the_key(key, value):
    with pytest.raises(ValueError, match=re.escape(key) + r"\b"):
        _options(**{key: value})


@pytest.mark.parametrize("key,value", [("algo.pathfinder_bc_beta", 0), ("algo.pathfinder_bc_beta", 1), ("algo.pathfinder_bc_beta_decay", 1),
                                       ("algo.pathfinder_bc_beta_decay", 1e-9), ("algo.pathfinder_bc_lr", 1e-9), ("algo.pathfinder_bc_iterations", 0)])
def test_edges_of_the_domains_pass(key, value):
    _options(**{key: value})


def test_trainer_validates_before_building_anything():
    from distributed_multi_agent_reinforcement_learning_amd import trainer
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config
    for key, bad in (("algo.pathfinder_bc_beta", 2.0), ("algo.pathfinder_bc_iterations", -3), ("runtime.pathfinder_cache", "yes")):
        with pytest.raises(ValueError, match=re.escape(key)):
            trainer.train_agent_multiprocessing(baseline_config("cfg1", **{key: bad}), max_iterations=1)
    with pytest.raises(ValueError, match="runtime.pathfinder_clearance"):      # the teacher's parameters, once the phase is on
        trainer.train_agent_multiprocessing(baseline_config("cfg1", **{"algo.pathfinder_bc_iterations": 1, "runtime.pathfinder_clearance": 1001}),
                                            max_iterations=1)


@pytest.mark.parametrize("name", ["cfg1", "cfg2", "cfg3"])
def test_mappo_still_refuses_the_particle_keys(name):
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config
    from distributed_multi_agent_reinforcement_learning_amd.mappo import MAPPO
    with pytest.raises(ValueError, match="algo.bc_iterations"):
        MAPPO(baseline_config(name, **{"algo.bc_iterations": 2}), 8, 4, "Learner")
    with pytest.raises(ValueError, match=r"algo\.bc_coef "):
        MAPPO(baseline_config(name, **{"algo.bc_coef": 0.5}), 8, 4, "Learner")
    with pytest.raises(ValueError, match="algo.pathfinder_bc_beta"):          # the new keys: refused before anything is built
        MAPPO(baseline_config(name, **{"algo.pathfinder_bc_beta": -1}), 8, 4, "Learner")


def test_resume_entry_check_names_the_key():
    import types
    from distributed_multi_agent_reinforcement_learning_amd import pursuit_imitation as pi
    agent = types.SimpleNamespace(pathfinder_bc=_options(**{"algo.pathfinder_bc_iterations": 2}))
    pi.check_entry(agent, 2, "bundle")
    for theirs in (None, 3):
        with pytest.raises(ValueError, match="algo.pathfinder_bc_iterations"):
            pi.check_entry(agent, theirs, "bundle")
    pi.check_entry(types.SimpleNamespace(pathfinder_bc=_options()), None, "bundle")


# ---- the C boundary ---------------------------------------------------------------------------------------------------------------------
def _header():
    return open(os.path.join(ROOT, "include", "pe_env.h")).read()


def test_symbols_are_exported():
    from distributed_multi_agent_reinforcement_learning_amd import pe_env
    L = pe_env.load_library()
    for name in ("pe_pursuer_pathfinder_teach", "pe_pursuer_pathfinder_teach_host"):
        assert hasattr(L, name) and name in pe_env.EXPORTS


def test_struct_layouts_match_header():
    from distributed_multi_agent_reinforcement_learning_amd import pe_env
    fields = [("pe_pathfinder_cache", pe_env.PePathfinderCache, ("field", "key", "hits")),
              ("pe_pathfinder_label", pe_env.PePathfinderLabel, ("follow", "action", "a_star", "a_star_env_stride"))]
    prints = "".join(f'printf("%zu ", sizeof({s}));' + "".join(f'printf("%zu ", offsetof({s}, {f}));' for f in fs) for s, _, fs in fields)
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "pe_env.h"\nint main(){' + prints + 'return 0;}\n'
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), os.path.join(td, "s.c"), "-o", os.path.join(td, "s")])
        out = [int(v) for v in subprocess.check_output([os.path.join(td, "s")]).decode().split()]
    mine = []
    for _, cls, fs in fields:
        assert tuple(n for n, _ in cls._fields_) == fs
        mine += [C.sizeof(cls)] + [getattr(cls, f).offset for f in fs]
    assert out == mine
    assert out[0] == 24 and out[4] == 32
    assert pe_env.PePathfinderLabel.a_star_env_stride.size == 8


def test_prototypes_match_the_ctypes_declarations():
    """the header's parameter lists, reduced to pointer / int32, against argtypes; and the header compiles against the very calls the
    binding makes (a C compiler checks the types of a call through the prototype)"""
    from distributed_multi_agent_reinforcement_learning_amd import pe_env
    L = pe_env.load_library()
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in ("pe_pursuer_pathfinder_teach", "pe_pursuer_pathfinder_teach_host"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        kinds = [C.c_void_p if "*" in p else C.c_int32 for p in params]
        assert all("*" in p or p.startswith("int32_t ") for p in params)
        assert list(getattr(L, name).argtypes) == kinds, name
    src = ('#include "pe_env.h"\nint f(const pe_config *c, const pe_state *s, const pe_pathfinder_params *p, const pe_pathfinder_cache *ca,\n'
           '      const pe_pathfinder_label *lb, int32_t *a, const pe_pathfinder_diag *d, void *q, const uint8_t *g, const double *x) {\n'
           '  int (*dev)(const pe_config *, const pe_state *, const pe_pathfinder_params *, const pe_pathfinder_cache *, const pe_pathfinder_label *,\n'
           '             int32_t *, const pe_pathfinder_diag *, void *) = pe_pursuer_pathfinder_teach;\n'
           '  int (*host)(const pe_config *, int32_t, const uint8_t *, const double *, const double *, const pe_pathfinder_params *,\n'
           '              const pe_pathfinder_cache *, const pe_pathfinder_label *, int32_t *, const pe_pathfinder_diag *) = pe_pursuer_pathfinder_teach_host;\n'
           '  return dev(c, s, p, ca, lb, a, d, q) + host(c, 1, g, x, x, p, ca, lb, a, d);\n}\n')
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "p.c"), "w").write(src)
        subprocess.check_call(["gcc", "-Wall", "-Werror", "-c", "-I" + os.path.join(ROOT, "include"), os.path.join(td, "p.c"), "-o", os.path.join(td, "p.o")])
