"""A2C env-steps/s of `a2c.learn`'s update loop on the device env (runner.run() -> Model.train_rollout(), the loop body of
baselines_amd/a2c/a2c.py:learn), nsteps = 5:

  atari   NatureCNN  N = 16, 4096
  mujoco  2x64 MLP   N = 1024

  python scripts/a2c_rate.py [updates]          -> one JSON line per configuration

Each configuration: warm-up updates (graph captures included), then `updates` timed updates between device
synchronisations; the median shader clock sampled with `rocm-smi --showclocks` while the timed region runs.
"""
import json
import re
import subprocess
import sys
import threading
import time

import torch

sys.path.insert(0, __file__.rsplit('/', 2)[0])
from baselines_amd.a2c import Model, Runner                                         # noqa: E402
from baselines_amd.common import set_global_seeds                                   # noqa: E402
from baselines_amd.common.policies import build_policy                              # noqa: E402
from baselines_amd.common.vec_env.synthetic_vec_env import SyntheticVecEnv          # noqa: E402

CONFIGS = [('atari', 'cnn', 16), ('atari', 'cnn', 4096), ('mujoco', 'mlp', 1024)]
T = 5


class ClockSampler(object):
    def __init__(self, period=0.3):
        self.period, self.samples, self._stop = period, [], threading.Event()
        self._t = threading.Thread(target=self._run, daemon=True)

    def _run(self):
        while not self._stop.is_set():
            try:
                out = subprocess.run(['rocm-smi', '--showclocks'], capture_output=True, text=True, timeout=5).stdout
                m = re.search(r'sclk clock level:\s*\d+:\s*\((\d+)Mhz\)', out)
                if m:
                    self.samples.append(int(m.group(1)))
            except Exception:
                pass
            self._stop.wait(self.period)

    def __enter__(self):
        self._t.start()
        return self

    def __exit__(self, *a):
        self._stop.set()
        self._t.join()

    def median(self):
        s = sorted(self.samples)
        return s[len(s) // 2] if s else None


def rate(kind, net, N, updates, warmup=5):
    set_global_seeds(0)
    env = SyntheticVecEnv(kind, N, seed=1)
    model = Model(policy=build_policy(env, net), env=env, nsteps=T, total_timesteps=int(1e9))
    runner = Runner(env, model, nsteps=T, gamma=0.99, return_host=False)
    runner.returns_by_model = True
    for _ in range(warmup):
        runner.run()
        model.train_rollout(runner)
    torch.cuda.synchronize()
    with ClockSampler() as clk:
        t0 = time.perf_counter()
        for _ in range(updates):
            runner.run()
            stats = model.train_rollout(runner)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    assert torch.isfinite(stats).all()
    return dict(kind=kind, network=net, num_envs=N, nsteps=T, updates=updates, ms_per_update=1e3 * dt / updates,
                env_steps_per_s=updates * N * T / dt, sclk_mhz_median=clk.median(),
                rollout_graph=bool(runner._graph), step_graph=isinstance(model._a2c_graph, dict))


def main():
    updates = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    torch.cuda.set_device(0)
    for kind, net, N in CONFIGS:
        print(json.dumps(rate(kind, net, N, updates)), flush=True)


if __name__ == '__main__':
    main()
