"""CPU-side checks of teacher-regularised PPO on the flagship (algo.pathfinder_bc_coef): the option validators and
defaults, the lambda schedule, what MAPPO keeps refusing, the resume-entry check, and the episode labeller's C boundary against the ctypes
declarations."""
import ctypes as C
import os
import re
import subprocess
import tempfile
import types

import pytest

from tests.conftest import ROOT


def _options(**ov):
    from distributed_multi_agent_reinforcement_learning_amd import pursuit_imitation as pi
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config
    return pi.pursuit_kickstart_options(baseline_config("cfg2", **ov))


def test_defaults_and_overrides():
    from distributed_multi_agent_reinforcement_learning_amd import pursuit_imitation as pi
    o = _options()
    assert (o.coef, o.decay, o.iterations, o.on, o.key) == (0.0, 1.0, 0, False, "algo.pathfinder_bc_coef")
    assert o.labeller == pi.DEFAULT_LABELLER and pi.DEFAULT_LABELLER in pi.LABELLERS == ("episode", "tick")
    o = _options(**{"algo.pathfinder_bc_coef": 2, "algo.pathfinder_bc_coef_decay": 0.5, "algo.pathfinder_bc_coef_iterations": 3,
                    "runtime.pathfinder_labeller": "episode"})
    assert (o.coef, o.decay, o.iterations, o.on, o.labeller) == (2.0, 0.5, 3, True, "episode")
    assert o.entry() == (2.0, 0.5, 3)
    assert _options(**{"runtime.pathfinder_labeller": "tick"}).labeller == "tick"
    # the env_3d / env_n2n keys are another feature's: they do not switch this one on
    assert not _options(**{"algo.bc_coef": 1.0}).on


def test_coef_at_before_the_phase_at_the_cut_off_and_past_it():
    o = _options(**{"algo.pathfinder_bc_coef": 2.0, "algo.pathfinder_bc_coef_decay": 0.5, "algo.pathfinder_bc_coef_iterations": 3})
    assert [o.coef_at(j) for j in (-1, 0, 1, 2, 3, 4)] == [0.0, 2.0, 1.0, 0.5, 0.0, 0.0]
    o = _options(**{"algo.pathfinder_bc_coef": 1.0, "algo.pathfinder_bc_coef_decay": 0.9})          # no cut-off
    assert o.coef_at(-1) == 0.0 and o.coef_at(0) == 1.0 and o.coef_at(1) == 0.9 and o.coef_at(50) == 0.9 ** 50 > 0.0
    assert [_options().coef_at(j) for j in (-1, 0, 1)] == [0.0, 0.0, 0.0]


BAD = [("algo.pathfinder_bc_coef", v) for v in (-0.1, float("nan"), float("inf"), True, "1", None)] + \
      [("algo.pathfinder_bc_coef_decay", v) for v in (0.0, -0.5, 1.01, float("nan"), False, "slow")] + \
      [("algo.pathfinder_bc_coef_iterations", v) for v in (-1, 1.5, True, "3", None)] + \
      [("runtime.pathfinder_labeller", v) for v in ("launch", "", "Episode", 1, True, None)]


@pytest.mark.parametrize("key,value", BAD)
def test_bad_values_raise_and_name_the_key(key, value):
    with pytest.raises(ValueError, match=re.escape(key) + r"\b"):
        _options(**{key: value})


@pytest.mark.parametrize("key,value", [("algo.pathfinder_bc_coef", 0), ("algo.pathfinder_bc_coef", 1e9), ("algo.pathfinder_bc_coef_decay", 1),
                                       ("algo.pathfinder_bc_coef_decay", 1e-9), ("algo.pathfinder_bc_coef_iterations", 0)])
def test_edges_of_the_domains_pass(key, value):
    _options(**{key: value})


def test_the_particle_trainers_keys_read_as_before():
    from distributed_multi_agent_reinforcement_learning_amd import kickstart as ks
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config
    o = ks.kickstart_options(baseline_config("cfg2", **{"algo.bc_coef": 0.5, "algo.bc_coef_decay": 0.25, "algo.pathfinder_bc_coef": 3.0}))
    assert (o.coef, o.decay, o.iterations, o.key) == (0.5, 0.25, 0, "algo.bc_coef")
    with pytest.raises(ValueError, match=r"algo\.bc_coef_decay\b"):
        ks.kickstart_options(baseline_config("cfg2", **{"algo.bc_coef_decay": 0.0}))


def test_trainer_validates_before_building_anything():
    from distributed_multi_agent_reinforcement_learning_amd import trainer
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config
    for key, bad in (("algo.pathfinder_bc_coef", -1.0), ("algo.pathfinder_bc_coef_decay", 2.0), ("algo.pathfinder_bc_coef_iterations", -3),
                     ("runtime.pathfinder_labeller", "both")):
        with pytest.raises(ValueError, match=re.escape(key)):
            trainer.train_agent_multiprocessing(baseline_config("cfg1", **{key: bad}), max_iterations=1)
    with pytest.raises(ValueError, match="runtime.pathfinder_clearance"):      # the teacher's parameters, once the feature is on
        trainer.train_agent_multiprocessing(baseline_config("cfg1", **{"algo.pathfinder_bc_coef": 1.0, "runtime.pathfinder_clearance": 1001}),
                                            max_iterations=1)


@pytest.mark.parametrize("name", ["cfg1", "cfg2", "cfg3"])
def test_mappo_validates_first_and_still_refuses_the_particle_keys(name):
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config
    from distributed_multi_agent_reinforcement_learning_amd.mappo import MAPPO
    with pytest.raises(ValueError, match=r"algo\.bc_coef "):
        MAPPO(baseline_config(name, **{"algo.bc_coef": 0.5}), 8, 4, "Learner")
    with pytest.raises(ValueError, match=r"algo\.bc_coef "):                 # ... also beside the flagship's own key
        MAPPO(baseline_config(name, **{"algo.bc_coef": 0.5, "algo.pathfinder_bc_coef": 0.5}), 8, 4, "Learner")
    with pytest.raises(ValueError, match="algo.bc_iterations"):
        MAPPO(baseline_config(name, **{"algo.bc_iterations": 2, "algo.pathfinder_bc_coef": 0.5}), 8, 4, "Learner")
    for key, bad in (("algo.pathfinder_bc_coef", -1), ("algo.pathfinder_bc_coef_decay", 0), ("algo.pathfinder_bc_coef_iterations", 1.5),
                     ("runtime.pathfinder_labeller", "gpu")):
        with pytest.raises(ValueError, match=re.escape(key)):                 # refused before anything is built (no GPU is asked for)
            MAPPO(baseline_config(name, **{key: bad}), 8, 4, "Learner")


def test_resume_entry_check_in_both_directions():
    from distributed_multi_agent_reinforcement_learning_amd import pursuit_imitation as pi
    on = types.SimpleNamespace(pathfinder_kick=_options(**{"algo.pathfinder_bc_coef": 1.0, "algo.pathfinder_bc_coef_decay": 0.9}))
    off = types.SimpleNamespace(pathfinder_kick=_options())
    pi.check_coef_entry(on, (1.0, 0.9, 0), "bundle")
    pi.check_coef_entry(on, [1.0, 0.9, 0], "bundle")             # a bundle's tuple may come back as a list
    pi.check_coef_entry(off, None, "bundle")
    for agent, theirs in ((on, None), (on, (0.5, 0.9, 0)), (on, (1.0, 1.0, 0)), (on, (1.0, 0.9, 4)), (off, (1.0, 0.9, 0))):
        with pytest.raises(ValueError, match=r"algo\.pathfinder_bc_coef\b"):
            pi.check_coef_entry(agent, theirs, "bundle")
    # the env_3d / env_n2n check keeps naming its own key
    from distributed_multi_agent_reinforcement_learning_amd import kickstart as ks
    with pytest.raises(ValueError, match=r"algo\.bc_coef: 0 \(off\)"):
        ks.check_entry(types.SimpleNamespace(kick=ks.KickstartOptions(1.0, 1.0, 0)), None, "bundle")


def test_the_buffer_has_the_label_field_when_either_key_is_on():
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config
    from distributed_multi_agent_reinforcement_learning_amd.mappo import ReplayBuffer
    want = (({}, False), ({"algo.pathfinder_bc_coef": 0.5}, True), ({"algo.pathfinder_bc_iterations": 1}, True),
            ({"algo.pathfinder_bc_coef": 0.0, "algo.pathfinder_bc_coef_decay": 0.5, "runtime.pathfinder_labeller": "episode"}, False))
    for ov, labelled in want:
        assert ReplayBuffer(baseline_config("cfg1", **ov), 4, "cpu").labelled == labelled, ov


# ---- the C boundary ---------------------------------------------------------------------------------------------------------------------
NAMES = ("pe_env_record_state", "pe_env_record_state_host", "pe_pathfinder_label_episode", "pe_pathfinder_label_episode_host")


def test_symbols_are_exported():
    from distributed_multi_agent_reinforcement_learning_amd import pe_env
    L = pe_env.load_library()
    for name in NAMES:
        assert hasattr(L, name) and name in pe_env.EXPORTS


def test_trace_struct_layout_matches_header():
    from distributed_multi_agent_reinforcement_learning_amd import pe_env
    header = ("def", "def_env_stride", "def_tick_stride", "eva", "eva_env_stride", "eva_tick_stride", "T", "pad0")
    prints = 'printf("%zu ", sizeof(pe_pathfinder_trace));' + "".join(f'printf("%zu ", offsetof(pe_pathfinder_trace, {f}));' for f in header)
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "pe_env.h"\nint main(){' + prints + 'return 0;}\n'
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), os.path.join(td, "s.c"), "-o", os.path.join(td, "s")])
        out = [int(v) for v in subprocess.check_output([os.path.join(td, "s")]).decode().split()]
    cls = pe_env.PePathfinderTrace
    assert tuple(n for n, _ in cls._fields_) == ("def_",) + header[1:]
    assert out == [C.sizeof(cls)] + [getattr(cls, n).offset for n, _ in cls._fields_]
    assert out[0] == 56 and cls.T.size == 4 and cls.def_env_stride.size == 8


def test_prototypes_match_the_ctypes_declarations():
    """the header's parameter lists, reduced to pointer / int32 / int64, against argtypes; and the header compiles against the very calls
    the binding makes (a C compiler checks the types of a call through the prototype)"""
    from distributed_multi_agent_reinforcement_learning_amd import pe_env
    L = pe_env.load_library()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pe_env.h")).read(), flags=re.S)
    for name in NAMES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        assert all("*" in p or p.startswith(("int32_t ", "int64_t ")) for p in params)
        kinds = [C.c_void_p if "*" in p else (C.c_int64 if p.startswith("int64_t ") else C.c_int32) for p in params]
        assert list(getattr(L, name).argtypes) == kinds, name
    src = ('#include "pe_env.h"\nint f(const pe_config *c, const pe_state *s, const pe_pathfinder_params *p, const pe_pathfinder_trace *tr,\n'
           '      float *a, int32_t *b, const pe_pathfinder_diag *d, void *q, const uint8_t *g, const double *x, double *y) {\n'
           '  int (*dev)(const pe_config *, const pe_state *, const pe_pathfinder_params *, const pe_pathfinder_trace *, float *, int64_t, int64_t,\n'
           '             int32_t *, const pe_pathfinder_diag *, void *) = pe_pathfinder_label_episode;\n'
           '  int (*host)(const pe_config *, int32_t, const uint8_t *, const pe_pathfinder_params *, const pe_pathfinder_trace *, float *, int64_t,\n'
           '              int64_t, int32_t *, const pe_pathfinder_diag *) = pe_pathfinder_label_episode_host;\n'
           '  int (*rec)(const pe_config *, const pe_state *, double *, int64_t, double *, int64_t, void *) = pe_env_record_state;\n'
           '  int (*rech)(const pe_config *, int32_t, const double *, const double *, double *, int64_t, double *, int64_t) = pe_env_record_state_host;\n'
           '  return dev(c, s, p, tr, a, 1, 1, b, d, q) + host(c, 1, g, p, tr, a, 1, 1, b, d) + rec(c, s, y, 1, y, 1, q) + rech(c, 1, x, x, y, 1, y, 1);\n}\n')
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "p.c"), "w").write(src)
        subprocess.check_call(["gcc", "-Wall", "-Werror", "-c", "-I" + os.path.join(ROOT, "include"), os.path.join(td, "p.c"), "-o", os.path.join(td, "p.o")])
