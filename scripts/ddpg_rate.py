"""DDPG on the device env at the reference's default hyperparameters (2 x 64 tanh, batch 64, 100 rollout + 50 train steps
per cycle, adaptive-param_0.2 noise):

  env-steps/s of `ddpg.learn`'s cycle loop   Pendulum-shaped (3/1, N = 1), HalfCheetah-shaped (17/6, N = 1 and 64),
                                             the `mujoco` preset (376/17, N = 64)
  time of one train step, three ways         the fused kernel (one launch, eager, back to back), the captured 50-step
                                             cycle / 50, the same step written as torch ops on the GPU (autograd)

  python scripts/ddpg_rate.py [epochs]          -> one JSON line per configuration

Times are host wall clock around work that ends in a device synchronisation, after a warm-up; the median shader clock is
sampled with `rocm-smi --showclocks` during the timed region.
"""
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit('/', 2)[0])
sys.path.insert(0, __file__.rsplit('/', 1)[0])
from a2c_rate import ClockSampler                                                   # noqa: E402
from baselines_amd import logger                                                    # noqa: E402
from baselines_amd.common.vec_env.synthetic_vec_env import SyntheticVecEnv          # noqa: E402
from baselines_amd.ddpg import ddpg as ddpg_mod                                     # noqa: E402

CONFIGS = [(3, 1, 1), (17, 6, 1), (17, 6, 64), (376, 17, 64)]      # ob_dim, nact, num_envs


def learn_rate(D, A, N, cycles):
    env = SyntheticVecEnv('mujoco', N, seed=1, ob_shape=(D,), nact=A)
    ddpg_mod.learn('mlp', env, seed=0, total_timesteps=200, nb_epoch_cycles=2)          # warm-up (code objects, captures)
    torch.cuda.synchronize()
    with ClockSampler() as clk:
        t0 = time.perf_counter()
        ddpg_mod.learn('mlp', env, seed=0, total_timesteps=cycles * 100, nb_epoch_cycles=cycles)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    return dict(what='learn', ob_dim=D, nact=A, num_envs=N, cycles=cycles, env_steps_per_s=cycles * 100 * N / dt,
                s_per_cycle=dt / cycles, sclk_mhz_median=clk.median())


def torch_step(p, o0, a, r, o1, d, gamma=0.99, l2=1e-2, tau=0.01, lr=(1e-4, 1e-3), t=1):
    """the same train step (no pop-art, no clip) as torch ops: target, both losses, autograd, MpiAdam, soft update"""
    def mlp(w, x, out_tanh):
        h = torch.tanh(x @ w[0] + w[1])
        h = torch.tanh(h @ w[2] + w[3])
        y = h @ w[4] + w[5]
        return torch.tanh(y) if out_tanh else y
    with torch.no_grad():
        q1 = mlp(p['tc'], torch.cat([o1, mlp(p['ta'], o1, True)], -1), False)
        tq = r + (1 - d) * gamma * q1
    qc = mlp(p['c'], torch.cat([o0, a], -1), False)
    cl = torch.mean((qc - tq) ** 2) + l2 * (p['c'][0].square().sum() + p['c'][2].square().sum()) / 2
    cconst = [x.detach() for x in p['c']]
    al = -torch.mean(mlp(cconst, torch.cat([o0, mlp(p['a'], o0, True)], -1), False))
    ga = torch.autograd.grad(al, p['a'])
    gc = torch.autograd.grad(cl, p['c'])
    with torch.no_grad():
        for key, gs, k in (('a', ga, 0), ('c', gc, 1)):
            alpha = lr[k] * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
            for w, g, m, v in zip(p[key], gs, p['m' + key], p['v' + key]):
                m.mul_(0.9).add_(0.1 * g)
                v.mul_(0.999).add_(0.001 * g * g)
                w.add_(-alpha * m / (v.sqrt() + 1e-8))
        for key in ('a', 'c'):
            for w, tw in zip(p[key], p['t' + key]):
                tw.mul_(1 - tau).add_(tau * w)
    return cl, al


def step_times(D, A, reps=200):
    from baselines_amd.ddpg.ddpg_learner import DDPG
    from baselines_amd.ddpg.memory import Memory
    from baselines_amd.ddpg.models import Actor, Critic
    np.random.seed(0)
    B = 64
    mem = Memory(10000, (A,), (D,))
    agent = DDPG(Actor(A, network='mlp'), Critic(network='mlp'), mem, (D,), (A,), batch_size=B, critic_l2_reg=1e-2,
                 tau=0.01)
    agent.initialize()
    rng = np.random.RandomState(1)
    n = 2000
    agent.store_transition(rng.randn(n, D).astype(np.float32), rng.uniform(-1, 1, (n, A)).astype(np.float32),
                           rng.randn(n).astype(np.float32), rng.randn(n, D).astype(np.float32), rng.rand(n) < 0.05)
    idx = torch.from_numpy(rng.randint(n - 2, size=B)).cuda()
    losses = torch.zeros(2, device='cuda')
    agent.neg_alpha.copy_(torch.from_numpy(agent.next_alphas()))

    def timed(fn, k):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / k

    fused = timed(lambda: agent.train_step_dev(idx, agent.neg_alpha, losses, soft_update=True), reps)
    cyc = ddpg_mod._TrainCycle(agent, 50)
    cyc.idx.copy_(idx.view(1, -1).expand(50, -1))
    cyc.alpha.copy_(agent.neg_alpha.view(1, 2).expand(50, 2))
    cycle = timed(lambda: cyc.run(False), max(reps // 50, 4)) / 50
    # torch composition on the same shapes
    dev = 'cuda'
    tens = lambda *s: (torch.randn(*s, device=dev) * 0.1)
    shapes_a = [(D, 64), (64,), (64, 64), (64,), (64, A), (A,)]
    shapes_c = [(D + A, 64), (64,), (64, 64), (64,), (64, 1), (1,)]
    p = {'a': [tens(*s).requires_grad_() for s in shapes_a], 'c': [tens(*s).requires_grad_() for s in shapes_c]}
    p['ta'] = [x.detach().clone() for x in p['a']]
    p['tc'] = [x.detach().clone() for x in p['c']]
    for k in ('a', 'c'):
        p['m' + k] = [torch.zeros_like(x) for x in p[k]]
        p['v' + k] = [torch.zeros_like(x) for x in p[k]]
    o0, o1, a = tens(B, D), tens(B, D), tens(B, A)
    r, d = tens(B, 1), torch.zeros(B, 1, device=dev)
    torch_t = timed(lambda: torch_step(p, o0, a, r, o1, d), reps // 4)
    return dict(what='train_step', ob_dim=D, nact=A, batch=B, fused_kernel_us=1e6 * fused, captured_cycle_per_step_us=1e6 * cycle,
                torch_ops_us=1e6 * torch_t)


def main():
    cycles = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    torch.cuda.set_device(0)
    logger.configure(format_strs=[])
    for D, A in ((3, 1), (17, 6), (376, 17)):
        print(json.dumps(step_times(D, A)), flush=True)
    for D, A, N in CONFIGS:
        print(json.dumps(learn_rate(D, A, N, cycles)), flush=True)


if __name__ == '__main__':
    main()
