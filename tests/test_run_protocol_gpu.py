"""Run protocol of the env_3d (cfg5) and env_n2n (cfg4_n2n) trainers on the MI355X: a resume bundle continues the run bit for bit,
every evaluation is recorded with a best checkpoint, `main --evaluate` reproduces a trainer's evaluation of saved weights, and
`main --save-resume` / `--resume` continue a command-line run like an uninterrupted one."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

N_ENVS, N_EVAL = 16, 8
CONFIG = {"e3d": "cfg5", "n2n": "cfg4_n2n"}
TIMING = ("seconds", "rollout_ms", "update_ms")


def _cfg(env, save_cwd, num_envs=N_ENVS):
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config
    return baseline_config(CONFIG[env], **{"runtime.num_envs": num_envs, "algo.save_cwd": str(save_cwd)})


def _trainer(env, cfg, **kw):
    if env == "e3d":
        from distributed_multi_agent_reinforcement_learning_amd.e3d_agent import E3dTrainer as T
    else:
        from distributed_multi_agent_reinforcement_learning_amd.n2n_agent import N2nTrainer as T
    return T(cfg, **kw)


def _train(env):
    if env == "e3d":
        from distributed_multi_agent_reinforcement_learning_amd.e3d_agent import train_e3d as f
    else:
        from distributed_multi_agent_reinforcement_learning_amd.n2n_agent import train_n2n as f
    return f


def _final_files(env, cwd, best=False):
    sfx = "_best" if best else ""
    names = [f"e3d_state_dicts{sfx}.pt"] if env == "e3d" else [f"n2n_actor{sfx}.pth", f"n2n_critic{sfx}.pth"]
    return [os.path.join(cwd, n) for n in names]


def _saved_weights(env, cwd, best=False):
    files = _final_files(env, cwd, best)
    if env == "e3d":
        sd = torch.load(files[0], map_location="cpu")
        return sd["actor"], sd["critic"]
    return tuple(torch.load(f, map_location="cpu") for f in files)


def _assert_state_dicts_equal(got, want):
    assert list(got) == list(want)
    for k in want:
        assert torch.equal(got[k].cpu(), want[k].cpu()), k


@pytest.mark.timeout(600)
@pytest.mark.parametrize("env", ["e3d", "n2n"])
def test_resume_bundle_continues_the_run_bit_for_bit(tmp_path, env):
    cfg = _cfg(env, tmp_path / "model")
    a = _trainer(env, cfg, num_eval_envs=N_EVAL, eval_every=1)
    a.iterate(); a.iterate()
    a.save_resume(str(tmp_path / "resume.pt"))
    _, log_a = a.iterate()
    b = _trainer(env, cfg, num_eval_envs=N_EVAL, eval_every=1)
    b.load_resume(str(tmp_path / "resume.pt"))
    assert b.iteration == 2 and b.total_steps == 2 * N_ENVS * int(cfg.env.max_steps)
    _, log_b = b.iterate()
    assert (b.total_steps, b.iteration) == (a.total_steps, a.iteration)
    assert a.agent.ac_optimizer.param_groups[0]["lr"] == b.agent.ac_optimizer.param_groups[0]["lr"]
    _assert_state_dicts_equal(b.agent.actor.state_dict(), a.agent.actor.state_dict())
    _assert_state_dicts_equal(b.agent.critic.state_dict(), a.agent.critic.state_dict())
    assert torch.equal(a.agent._state(a.env).counter, b.agent._state(b.env).counter)
    assert int(a.agent._state(a.env).counter.item()) > 0
    for k in ("p", "e", "target"):
        assert torch.equal(getattr(a.env, k), getattr(b.env, k)), k
    assert a.env.n_episode == b.env.n_episode == 3
    assert log_a["mean_return"] == log_b["mean_return"]
    assert log_a["eval_return"] == log_b["eval_return"]          # the evaluation environments continue their own seeds
    c = _trainer(env, _cfg(env, tmp_path / "model", N_ENVS // 2), num_eval_envs=N_EVAL)
    with pytest.raises(ValueError, match="num_envs"):
        c.load_resume(str(tmp_path / "resume.pt"))


@pytest.fixture(scope="module", params=["e3d", "n2n"])
def trained(request, tmp_path_factory):
    """train_e3d / train_n2n for 3 iterations, evaluating after each, into a fresh save_cwd"""
    env = request.param
    cwd = tmp_path_factory.mktemp(f"run_{env}")
    cfg = _cfg(env, cwd)
    tr = _train(env)(cfg, max_iterations=3, num_eval_envs=N_EVAL, eval_every=1)
    return env, cfg, str(cwd), tr


@pytest.mark.timeout(600)
def test_recorder_and_best_checkpoint(trained):
    env, cfg, cwd, tr = trained
    rec = np.load(os.path.join(cwd, "recorder.npy"))
    assert rec.shape == (3, 6) and np.all(np.diff(rec[:, 0]) > 0)
    assert rec[:, 0].tolist() == [k * N_ENVS * int(cfg.env.max_steps) for k in (1, 2, 3)]
    assert np.all(np.isfinite(rec)) and np.all(rec[:, 2] >= 0)
    assert os.path.exists(os.path.join(cwd, "learning_curve.jpg"))
    final_a, final_c = _saved_weights(env, cwd)                  # today's final files, today's names
    _assert_state_dicts_equal(final_a, tr.agent.actor.state_dict())
    _assert_state_dicts_equal(final_c, tr.agent.critic.state_dict())
    best = 0                                                      # the last evaluation that was not worse than every earlier one
    for k in range(1, 3):
        if rec[k, 1] >= rec[:k, 1].max():
            best = k
    # the same run again (evaluations included: they advance the critic's spectral-norm vectors), stopped at the best iteration
    again = _trainer(env, cfg, num_eval_envs=N_EVAL, eval_every=1)
    for k in range(best + 1):
        _, log = again.iterate()
        assert log["eval_return"] == rec[k, 1] and log["mean_return"] == rec[k, 3]
        assert log["critic_loss"] == rec[k, 4] and log["actor_loss"] == rec[k, 5] and again.eval_return_std == rec[k, 2]
    best_a, best_c = _saved_weights(env, cwd, best=True)
    _assert_state_dicts_equal(best_a, again.agent.actor.state_dict())
    _assert_state_dicts_equal(best_c, again.agent.critic.state_dict())
    # load_model reads both kinds of files back
    fresh = _trainer(env, cfg, num_eval_envs=N_EVAL)
    fresh.agent.load_model(cwd, best=True)
    _assert_state_dicts_equal(fresh.agent.actor.state_dict(), again.agent.actor.state_dict())
    fresh.agent.load_model(cwd)
    _assert_state_dicts_equal(fresh.agent.critic.state_dict(), tr.agent.critic.state_dict())


def _main(args, timeout=600):
    """python -m ...main ARGS in a child process -> its JSON lines"""
    out = subprocess.run([sys.executable, "-m", "distributed_multi_agent_reinforcement_learning_amd.main", *args], cwd=ROOT,
                         capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr[-4000:]
    return [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")]


@pytest.mark.timeout(600)
def test_main_evaluate_matches_the_trainer(trained):
    env, cfg, cwd, _ = trained
    lines = _main(["--config", CONFIG[env], "--evaluate", cwd, "--eval-envs", str(N_EVAL), f"runtime.num_envs={N_ENVS}",
                   f"algo.save_cwd={cwd}"])
    assert len(lines) == 1 and set(lines[0]) == {"eval_return", "eval_capture_rate", "eval_episode_length"}
    tr = _trainer(env, cfg, num_eval_envs=N_EVAL)
    tr.agent.load_model(cwd)
    assert lines[0] == tr.evaluate()


@pytest.mark.timeout(900)
@pytest.mark.parametrize("env", ["e3d", "n2n"])
def test_main_resume_continues_like_one_run(tmp_path, env):
    base = ["--config", CONFIG[env], "--eval-envs", str(N_EVAL)]
    ckpt, resumed, straight = tmp_path / "ckpt", tmp_path / "resumed", tmp_path / "straight"
    ov = lambda cwd: [f"runtime.num_envs={N_ENVS}", f"algo.save_cwd={cwd}"]     # the overrides go last (one positional list)
    first = _main(base + ["--iterations", "2", "--save-resume", str(ckpt)] + ov(resumed))
    assert len(first) == 2 and os.listdir(ckpt) == ["resume_rank0.pt"]
    second = _main(base + ["--iterations", "3", "--resume", str(ckpt)] + ov(resumed))
    whole = _main(base + ["--iterations", "3"] + ov(straight))
    assert len(second) == 1 and len(whole) == 3
    drop = lambda log: {k: v for k, v in log.items() if k not in TIMING}
    assert drop(second[-1]) == drop(whole[-1])
    assert drop(first[-1]) == drop(whole[1])
    assert np.array_equal(np.load(resumed / "recorder.npy"), np.load(straight / "recorder.npy"))   # the record carries over
    for got, want in zip(_saved_weights(env, str(resumed)), _saved_weights(env, str(straight))):
        _assert_state_dicts_equal(got, want)


@pytest.mark.timeout(600)
def test_pursuit_loop_writes_and_reads_resume_bundles(tmp_path):
    """--save-resume / --resume on the pursuit loop: Trainer.save_resume after every iteration, Trainer.load_resume before the first"""
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config
    from distributed_multi_agent_reinforcement_learning_amd.trainer import train_agent_multiprocessing
    cfg = baseline_config("cfg1", **{"env.max_steps": 10, "runtime.num_envs": 8, "algo.save_cwd": str(tmp_path / "model")})
    ckpt = str(tmp_path / "ckpt")
    a = train_agent_multiprocessing(cfg, max_iterations=2, num_eval_envs=4, async_eval=False, save_resume=ckpt)
    assert a.iteration == 2 and os.listdir(ckpt) == ["resume_rank0.pt"]
    b = train_agent_multiprocessing(cfg, max_iterations=3, num_eval_envs=4, async_eval=False, resume=ckpt)
    assert b.iteration == 3 and b.total_steps == 3 * (a.total_steps // 2)
