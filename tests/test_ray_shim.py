"""ray_shim ("a thin .remote / ray.get shim keeps main.py's loop text runnable").

The constructs main.py:41-172 uses -- remote actors and functions, ObjectRef arguments, ray.get / ray.wait, background actors --
on the shim.  The GPU suite runs the training loop built on them with the real Learner / Worker / EvaluatorProc
(tests/test_runner_gpu.py)."""
import threading
import time

import pytest

from distributed_multi_agent_reinforcement_learning_amd import ray_shim as ray


def test_refs_wait_and_background_actor():
    class Slow:
        def __init__(self, delay):
            self.delay = delay
            self.calls = []

        def work(self, x):
            time.sleep(self.delay)
            self.calls.append((x, threading.current_thread().name))
            return x * 2

        def boom(self):
            raise ValueError("inside the actor")

    A = ray.remote(Slow)
    inline = A.remote(0.0)
    r = inline.work.remote(ray.put(21))                      # ObjectRef arguments are resolved
    assert ray.get(r) == 42 and ray.get([r, r]) == [42, 42] and ray.get(7) == 7
    bad = inline.boom.remote()                               # the error surfaces at get()
    with pytest.raises(ValueError):
        ray.get(bad)
    bg = A.options(resources={"node_0": 0.001}, background=True).remote(0.15)
    t0 = time.monotonic()
    refs = [bg.work.remote(k) for k in range(3)]             # returns at once
    assert time.monotonic() - t0 < 0.1
    ready, rest = ray.wait(refs, num_returns=1, timeout=0.01)
    assert ready == [] and len(rest) == 3
    ready, rest = ray.wait(refs, num_returns=1, timeout=2.0)
    assert len(ready) == 1 and ready[0] is refs[0] and len(rest) == 2   # an actor runs its calls in submission order
    assert ray.get(refs) == [0, 2, 4]
    with pytest.raises(ValueError):
        ray.get(bg.boom.remote())
    assert ray.get(bg.work.remote(ray.put(5))) == 10
    with pytest.raises(TypeError):
        bg.work(1)
    bg._shutdown()

    @ray.remote(num_cpus=1)
    def f(a, b=1):
        return a + b
    assert ray.get(f.remote(1, b=ray.put(2))) == 3
