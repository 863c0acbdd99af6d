"""CPU-side checks of the C ABI of team reward sharing: the two exports, their declarations, and the argument checks that return before
anything is launched -- the null checks with the codes of the sibling entry point (*_policy_record_shaped) and a bad alpha with the
library's bad-config code."""
import ctypes as C
import os

import pytest

from tests.conftest import ROOT

CASES = [("e3d_env.h", "libe3d_env.so", "e3d", 40001, 40002), ("n2n_env.h", "libn2n_env.so", "n2n", 30001, 30002)]
VP, D = C.c_void_p, C.c_double


def _lib(libname):
    from distributed_multi_agent_reinforcement_learning_amd import build
    path = build.build_lib(libname)
    assert path and os.path.exists(path)
    return C.CDLL(path)


def _mirrors(pre):
    if pre == "e3d":
        from distributed_multi_agent_reinforcement_learning_amd import e3d_env as m
        return m.E3dConfig, m.E3dState, m.E3dRecordIO, m.E3dPolicyAcc
    from distributed_multi_agent_reinforcement_learning_amd import n2n_env as m
    return m.N2nConfig, m.N2nState, m.N2nRecordIO, m.N2nPolicyAcc


@pytest.mark.parametrize("header,libname,pre,bad,null", CASES)
def test_export_is_declared_in_the_header(header, libname, pre, bad, null):
    assert hasattr(_lib(libname), f"{pre}_policy_record_team")
    txt = " ".join(open(os.path.join(ROOT, "include", header)).read().split())
    assert (f"int {pre}_policy_record_team(const {pre}_config *cfg, const {pre}_state *st, const float *reward, const uint8_t *done, "
            f"const {pre}_record_io *io, const {pre}_policy_acc *acc, double alpha, double *phi, double coef, double gamma, double *rs, "
            f"void *stream);") in txt
    assert f"#define {pre.upper()}_ERR_BAD_CONFIG {bad}" in txt and f"#define {pre.upper()}_ERR_NULL {null}" in txt


@pytest.mark.parametrize("header,libname,pre,bad,null", CASES)
def test_null_pointers_and_bad_alpha_return_the_abi_errors(header, libname, pre, bad, null):
    """every check sits before the launch, so it runs without a device: an empty batch (N = 0) with good arguments returns 0"""
    L = _lib(libname)
    team, shaped = getattr(L, f"{pre}_policy_record_team"), getattr(L, f"{pre}_policy_record_shaped")
    team.argtypes = [VP] * 6 + [D, VP, D, D, VP, VP]
    shaped.argtypes = [VP] * 7 + [D, D, VP, VP]
    Cfg, St, IO, Acc = _mirrors(pre)
    cfg, st, io, acc = Cfg(), St(), IO(), Acc()
    cfg.P = 3
    if pre == "e3d":
        cfg.max_step = 10
    else:
        cfg.E, cfg.episode_limit = 2, 10
    cfg.p_vmax, cfg.kill_radius = 0.5, 0.5
    f32, u8, f64 = (C.c_float * 16)(), (C.c_uint8 * 16)(), (C.c_double * 64)()
    ptr = lambda a: C.cast(a, VP)
    io.live = ptr(f32).value
    for k in ("done_before", "ended", "captured"):
        setattr(acc, k, ptr(u8).value)
    acc.ret = acc.length = ptr(f32).value
    head = [C.byref(cfg), C.byref(st), ptr(f32), ptr(u8), C.byref(io), C.byref(acc)]

    def call(alpha=0.5, phi=None, rs=None, **swap):
        a = list(head)
        for k, v in swap.items():
            a[int(k[1:])] = v
        return team(*a, alpha, phi, 0.1, 0.99, rs, None)

    assert st.N == 0
    for phi in (None, ptr(f64)):
        for rs in (None, ptr(f64)):
            for alpha in (0.0, 0.25, 1.0):
                assert call(alpha, phi, rs) == 0
    for k in range(6):                                             # the codes of the sibling, argument by argument
        a = list(head); a[k] = None
        assert call(**{f"a{k}": None}) == shaped(*a, ptr(f64), 0.1, 0.99, None, None) == null, k
    for field in ("live", "done_before", "ended", "captured", "ret", "length"):
        io2, acc2 = IO.from_buffer_copy(io), Acc.from_buffer_copy(acc)
        setattr(io2 if field == "live" else acc2, field, None)
        a = list(head); a[4], a[5] = C.byref(io2), C.byref(acc2)
        assert call(a4=a[4], a5=a[5]) == shaped(*a, ptr(f64), 0.1, 0.99, None, None) == null, field
    io2 = IO.from_buffer_copy(io)
    io2.v = ptr(f32).value                                         # v without value
    assert call(a4=C.byref(io2)) == null
    for alpha in (-0.1, -1e-300, 1.0000000000000002, 1.5, float("inf"), -float("inf"), float("nan")):
        for phi in (None, ptr(f64)):
            for rs in (None, ptr(f64)):
                assert call(alpha, phi, rs) == bad, alpha
    cfg.P = 0                                                      # the configuration check, as in the sibling
    assert call() == shaped(*head, ptr(f64), 0.1, 0.99, None, None) == bad
