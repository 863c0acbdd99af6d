"""CPU checks of the SLSQP evader (csrc/slsqp_box.hpp): the new entry points are declared and exported, and the library's host
path -- the kernels' own solver and objectives compiled for the CPU -- reproduces the reference's eva.e_f commands."""
import os
import re

import numpy as np
import pytest

from tests import evader_cases as ec
from tests.conftest import ROOT

NEW = {"n2n_env.h": ("libn2n_env.so", ("n2n_evader_slsqp", "n2n_evader_slsqp_nit", "n2n_evader_slsqp_host")),
       "e3d_env.h": ("libe3d_env.so", ("e3d_evader_slsqp", "e3d_evader_slsqp_nit", "e3d_evader_slsqp_host"))}


def _lib(name):
    import ctypes
    from distributed_multi_agent_reinforcement_learning_amd import build
    path = build.build_lib(name)
    assert path and os.path.exists(path)
    return ctypes.CDLL(path)


@pytest.mark.parametrize("header", sorted(NEW))
def test_evader_symbols_declared_and_exported(header):
    libname, names = NEW[header]
    txt = open(os.path.join(ROOT, "include", header)).read()
    lib = _lib(libname)
    for n in names:
        assert re.search(r"\bint\s+" + n + r"\s*\(", txt), f"{n} is not declared in include/{header}"
        assert hasattr(lib, n), f"{libname} does not export {n}"
    # the device entry point has the issue's signature: (cfg, st, double *e_cmd, void *stream)
    m = re.search(r"int\s+" + names[0] + r"\s*\(([^)]*)\)", txt)
    assert [a.strip().split()[-1].lstrip("*") for a in m.group(1).split(",")] == ["cfg", "st", "e_cmd", "stream"]


def test_n2n_host_evader_matches_reference():
    from distributed_multi_agent_reinforcement_learning_amd import n2n_env
    L = n2n_env.load_library()
    groups = ec.n2n_groups()
    n, hit, worst = ec.n2n_check(groups, [ec.n2n_host(L, g)[0] for g in groups])
    assert n > 2000
    assert hit >= 0.97 * n, (hit, n)
    assert worst <= 1e-3, worst


def test_e3d_host_evader_matches_reference():
    from distributed_multi_agent_reinforcement_learning_amd import e3d_env
    L = e3d_env.load_library()
    groups = ec.e3d_groups()
    n, hit = ec.e3d_check(groups, [ec.e3d_host(L, g)[0] for g in groups])
    assert n > 2000
    assert hit >= 0.90 * n, (hit, n)


def test_host_evader_edge_cases():
    """no pursuer in range: the n2n objective is the target term alone, so the heading points at the target (up to ftol);
    uncalled evaders get 0; the iteration count stays within scipy's limit"""
    from distributed_multi_agent_reinforcement_learning_amd import n2n_env
    L = n2n_env.load_library()
    cfg = np.asarray([0.3, 1.0, 3.0, 6.0, 0.5, np.pi / 4, 0.5])
    P, E = 4, 2
    p = np.zeros((1, 5, P)); p[0, 0] = 50.0; p[0, 1] = 50.0; p[0, 3] = 0.3; p[0, 4] = 1.0
    e = np.zeros((1, 5, E)); e[0, :, 0] = (5.0, 5.0, 0.0, 1.0, 1.0); e[0, :, 1] = (5.0, 5.0, 0.0, 1.0, 0.0)
    tg = np.array([[5.0, 15.0]])
    cmd, nit = ec.n2n_host(L, dict(cfg=cfg, P=P, E=E, p=p, e=e, target=tg))
    assert abs(cmd[0, 0] - 0.5) < 1e-3 and cmd[0, 1] == 0.0
    assert 1 <= nit[0, 0] <= 100 and nit[0, 1] == 0
