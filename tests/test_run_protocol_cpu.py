"""CPU side of the env_3d / env_n2n run protocol: the host resetters' state blobs (n2n_resetter_* / e3d_resetter_* through ctypes),
the main flags that drive resume / evaluation, the atomic bundle write and the evaluation record with its best checkpoint."""
import ctypes as C
import math
import os

import numpy as np
import pytest

HEADER = 16                      # u32 tag, i32 N, P, E
RECORD = 624 * 4 + 4 + 4 + 8     # MT19937 key, position, has_gauss, gauss


def _n2n(P, E=1):
    from distributed_multi_agent_reinforcement_learning_amd import build, n2n_env
    build.build_lib("libn2n_env.so")
    L = n2n_env.load_library()
    c = n2n_env.N2nConfig()
    c.P, c.E, c.episode_limit = P, E, 100
    for k, v in dict(p_vmax=0.3, e_vmax=1.0, p_sen_range=3.0, p_comm_range=6.0, kill_radius=0.5, ang_lmt=math.pi / 4, step_size=0.5).items():
        setattr(c, k, v)
    shapes = lambda N: ((N, P, 5), (N, E, 5), (N, 2))
    return L, "n2n", c, shapes, 30003


def _e3d(P, E=1):
    from distributed_multi_agent_reinforcement_learning_amd import build, e3d_env
    build.build_lib("libe3d_env.so")
    L = e3d_env.load_library()
    c = e3d_env.E3dConfig()
    c.P, c.max_step = P, 200
    for k, v in dict(p_vmax=0.7, e_vmax=1.0, p_sen_range=3.0, p_comm_range=6.0, kill_radius=0.5, ang_lmt=math.pi / 4, v_lmt=0.4,
                     step_size=0.5).items():
        setattr(c, k, v)
    shapes = lambda N: ((N, P, 7), (N, 7), (N, 3))
    return L, "e3d", c, shapes, 40004


ENVS = {"n2n": _n2n, "e3d": _e3d}


class Resetter:
    def __init__(self, L, pre, c, shapes, seeds):
        self.L, self.pre, self.shapes, self.N = L, pre, shapes, len(seeds)
        s = np.ascontiguousarray(seeds, np.uint32)
        self.h = getattr(L, f"{pre}_resetter_create")(C.byref(c), self.N, s.ctypes.data_as(C.c_void_p))
        assert self.h

    def __del__(self):
        getattr(self.L, f"{self.pre}_resetter_destroy")(self.h)

    def reset(self):
        out = [np.empty(s) for s in self.shapes(self.N)]
        rc = getattr(self.L, f"{self.pre}_resetter_reset")(self.h, *(a.ctypes.data_as(C.c_void_p) for a in out), 4)
        assert rc == 0
        return out

    def get(self):
        buf = np.empty(getattr(self.L, f"{self.pre}_resetter_state_bytes")(self.h), np.uint8)
        assert getattr(self.L, f"{self.pre}_resetter_get_state")(self.h, buf.ctypes.data_as(C.c_void_p)) == 0
        return buf

    def set(self, buf):
        return getattr(self.L, f"{self.pre}_resetter_set_state")(self.h, np.ascontiguousarray(buf).ctypes.data_as(C.c_void_p))


@pytest.mark.parametrize("env", ["n2n", "e3d"])
def test_resetter_state_restores_the_streams(env):
    L, pre, c, shapes, _ = ENVS[env](4)
    a = Resetter(L, pre, c, shapes, list(range(11, 27)))
    a.reset()
    blob = a.get()
    assert blob.size == HEADER + 16 * RECORD
    assert blob[:HEADER].view(np.int32)[1:].tolist() == [16, 4, 1]
    has_gauss = blob[HEADER:].reshape(16, RECORD)[:, 624 * 4 + 4:624 * 4 + 8].copy().view(np.int32)[:, 0]
    if env == "e3d":   # normal(size 3) draws leave a cached normal behind in some environments (env_n2n draws pairs: never)
        assert set(has_gauss.tolist()) == {0, 1}
    want = [a.reset(), a.reset()]
    b = Resetter(L, pre, c, shapes, list(range(500, 516)))
    b.reset()
    assert b.set(blob) == 0
    got = [b.reset(), b.reset()]
    for w, g in zip(want, got):
        for x, y in zip(w, g):
            assert x.tobytes() == y.tobytes()
    assert b.get().tobytes() == a.get().tobytes()


@pytest.mark.parametrize("env", ["n2n", "e3d"])
def test_resetter_state_rejects_a_foreign_blob(env):
    L, pre, c4, shapes4, bad = ENVS[env](4)
    _, _, c5, shapes5, _ = ENVS[env](5)
    r = Resetter(L, pre, c4, shapes4, [1, 2, 3])
    before = r.get()
    other_p = Resetter(L, pre, c5, shapes5, [1, 2, 3]).get()
    assert other_p.size == before.size and r.set(other_p) == bad
    other_n = Resetter(L, pre, c4, shapes4, [1, 2, 3, 4]).get()
    assert r.set(other_n) == bad
    tagged = before.copy()
    tagged[0] ^= 1
    assert r.set(tagged) == bad
    torn = before.copy()
    torn[HEADER + 2 * RECORD + 624 * 4:HEADER + 2 * RECORD + 624 * 4 + 4] = np.frombuffer(np.int32(625).tobytes(), np.uint8)
    assert r.set(torn) == bad
    assert r.get().tobytes() == before.tobytes()       # a rejected blob leaves every stream as it was
    if env == "n2n":                                    # E is part of the header too
        _, _, c_e2, shapes_e2, _ = ENVS[env](4, 2)
        assert r.set(Resetter(L, pre, c_e2, shapes_e2, [1, 2, 3]).get()) == bad


def _main_calls(monkeypatch):
    from distributed_multi_agent_reinforcement_learning_amd import main as m
    calls = []
    for name in ("train_e3d", "train_n2n", "train_agent_multiprocessing"):
        monkeypatch.setattr(m, name, lambda cfg, _n=name, **kw: calls.append((_n, kw)))
    monkeypatch.setattr(m, "evaluate_saved", lambda cls, cfg, cwd, n: calls.append(("evaluate", cls.__name__, cwd, n)))
    return m, calls


@pytest.mark.parametrize("config,target", [("cfg5", "train_e3d"), ("cfg4_n2n", "train_n2n"), ("cfg2", "train_agent_multiprocessing")])
def test_main_resume_flags_reach_every_trainer(monkeypatch, config, target):
    m, calls = _main_calls(monkeypatch)
    m.main(["--config", config, "--iterations", "3", "--save-resume", "/ckpt/a", "--resume", "/ckpt/b"])
    assert calls[-1] == (target, dict(max_iterations=3, num_eval_envs=64, eval_every=1, save_resume="/ckpt/a", resume="/ckpt/b"))
    m.main(["--config", config, "--iterations", "3"])
    assert calls[-1] == (target, dict(max_iterations=3, num_eval_envs=64, eval_every=1))   # no flags: today's call


def test_main_evaluate_routes_and_refuses_pursuit(monkeypatch):
    m, calls = _main_calls(monkeypatch)
    m.main(["--config", "cfg5", "--evaluate", "/w", "--eval-envs", "8"])
    m.main(["--config", "cfg4_n2n", "--evaluate", "/v"])
    assert calls == [("evaluate", "E3dTrainer", "/w", 8), ("evaluate", "N2nTrainer", "/v", 64)]
    with pytest.raises(SystemExit):
        m.main(["--config", "cfg3", "--evaluate", "/w"])
    assert len(calls) == 2


class _FakeTrainer:
    rank = 3

    def __init__(self):
        self.written = []

    def save_resume(self, path):
        assert not os.path.exists(path)
        open(path, "wb").write(b"bundle %d" % len(self.written))
        self.written.append(path)


def test_save_resume_atomic_replaces_the_bundle(tmp_path):
    from distributed_multi_agent_reinforcement_learning_amd.trainer import resume_path, save_resume_atomic
    tr = _FakeTrainer()
    d = str(tmp_path / "ckpt")
    save_resume_atomic(tr, d)
    save_resume_atomic(tr, d)
    assert resume_path(d, 3) == os.path.join(d, "resume_rank3.pt")
    assert sorted(os.listdir(d)) == ["resume_rank3.pt"]             # the temporary files were renamed into place
    assert open(resume_path(d, 3), "rb").read() == b"bundle 1"
    assert all(p != resume_path(d, 3) for p in tr.written)


class _FakeAgent:
    def __init__(self):
        self.saved = []
        self.weights = 0

    def save_model(self, cwd, best=False):
        self.saved.append((cwd, best, self.weights))


def test_record_evaluation_rows_and_best_rule(tmp_path):
    from distributed_multi_agent_reinforcement_learning_amd.trainer import ParticleRunState
    tr = ParticleRunState()
    tr.agent, tr.recorder, tr.best_eval_return = _FakeAgent(), [], -float("inf")
    cwd = str(tmp_path / "run")
    for k, r in enumerate([1.0, 0.5, 1.0, 2.0, -1.0]):
        tr.agent.weights, tr.eval_return_std = k, 0.25 * k
        tr.record_evaluation(dict(total_steps=100 * (k + 1), eval_return=r, mean_return=-r, critic_loss=k + 0.5, actor_loss=-k), cwd)
    rec = np.load(os.path.join(cwd, "recorder.npy"))
    assert rec.shape == (5, 6)
    assert rec[:, 0].tolist() == [100, 200, 300, 400, 500] and rec[:, 2].tolist() == [0, 0.25, 0.5, 0.75, 1.0]
    assert rec[3].tolist() == [400, 2.0, 0.75, -2.0, 3.5, -3]
    assert tr.agent.saved == [(cwd, True, 0), (cwd, True, 2), (cwd, True, 3)]   # ties count as "not worse" (main.py:139-156)
    assert os.path.exists(os.path.join(cwd, "learning_curve.jpg"))
