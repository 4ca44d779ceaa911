"""GPU: DDPG's HIP kernels (csrc/ddpg.hip) against the float64 / float32 restatement of ddpg_learner.py in
tests/_ddpg_oracle.py, the bit-exact replay store, the act side with each noise kind, parameter noise, the captured train
cycle against the same cycle run eagerly, and `learn` on the device env against `learn` on its host twin."""
import json
import os

import numpy as np
import pytest
import torch

from baselines_amd import _lib
from baselines_amd.ddpg import ddpg as ddpg_mod
from baselines_amd.ddpg.ddpg_learner import DDPG
from baselines_amd.ddpg.memory import Memory
from baselines_amd.ddpg.models import Actor, Critic
from baselines_amd.ddpg.noise import AdaptiveParamNoiseSpec, NormalActionNoise, OrnsteinUhlenbeckActionNoise

from tests._ddpg_oracle import Oracle, oracle_learn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.environ.get('MRL_DDPG_REPORT')        # optional: append the measured error table (jsonl) here


def make_agent(D, A, H, L, act='tanh', ln=False, B=64, popart=False, norm_ret=False, clip=None, l2=1e-2, limit=4096,
               n=None, param_noise=None, action_noise=None, seed=0):
    np.random.seed(seed)
    torch.manual_seed(seed)
    mem = Memory(limit, (A,), (D,))
    kw = dict(network='mlp', num_layers=L, num_hidden=H, activation=act, layer_norm=ln)
    agent = DDPG(Actor(A, **kw), Critic(**kw), mem, (D,), (A,), gamma=0.99, tau=0.01, normalize_returns=norm_ret,
                 enable_popart=popart, batch_size=B, critic_l2_reg=l2, clip_norm=clip, param_noise=param_noise,
                 action_noise=action_noise)
    agent.initialize()
    rng = np.random.RandomState(seed + 1)
    n = n or max(3 * B, 300)
    for c0 in range(0, n, 250):
        m = min(250, n - c0)
        agent.store_transition((rng.randn(m, D) * 1.5 + 0.3).astype(np.float32), rng.uniform(-1, 1, (m, A)).astype(np.float32),
                               rng.randn(m).astype(np.float32), (rng.randn(m, D) * 1.5 + 0.3).astype(np.float32),
                               rng.rand(m) < 0.1)
    return agent


def snapshot(agent):
    f = lambda t: t.detach().cpu().numpy().copy()
    return dict(actor=f(agent.actor_params), critic=f(agent.critic_params), target_actor=f(agent.target_actor_params),
                target_critic=f(agent.target_critic_params), actor_m=f(agent.actor_m), actor_v=f(agent.actor_v),
                critic_m=f(agent.critic_m), critic_v=f(agent.critic_v), obs_rms=f(agent.obs_rms.buf),
                ret_rms=f(agent.ret_rms.buf), actor_t=agent.actor_t, critic_t=agent.critic_t)


def load(agent, snap):
    for k in ('actor', 'critic', 'target_actor', 'target_critic', 'actor_m', 'actor_v', 'critic_m', 'critic_v'):
        getattr(agent, k + ('_params' if k in ('actor', 'critic', 'target_actor', 'target_critic') else '')).copy_(
            torch.from_numpy(np.asarray(snap[k], np.float32)))
    agent.obs_rms.buf.copy_(torch.from_numpy(np.asarray(snap['obs_rms'])))
    agent.ret_rms.buf.copy_(torch.from_numpy(np.asarray(snap['ret_rms'])))
    agent.actor_t, agent.critic_t = snap['actor_t'], snap['critic_t']


def batch(agent, idx):
    m = agent.memory
    rows = (m.observations0.start + idx) % m.limit
    g = lambda r: r.data.cpu().numpy()[rows]
    return g(m.observations0), g(m.actions), g(m.rewards).reshape(-1), g(m.observations1), g(m.terminals1).reshape(-1)


def oracle(agent, snap, dtype):
    return Oracle(agent.actor, agent.critic, activation=agent.actor.activation,
                  normalize_observations=agent.normalize_observations, normalize_returns=agent.normalize_returns,
                  popart=agent.enable_popart, gamma=agent.gamma, tau=agent.tau, critic_l2_reg=agent.critic_l2_reg,
                  clip_norm=agent.clip_norm, actor_lr=agent.actor_lr, critic_lr=agent.critic_lr, dtype=dtype, flat=snap)


def device_step(agent, idx):
    dev = agent.device
    grads = torch.zeros(agent.Pa + agent.Pc, dtype=torch.float32, device=dev)
    losses = torch.zeros(2, dtype=torch.float32, device=dev)
    agent.neg_alpha.copy_(torch.from_numpy(agent.next_alphas()))
    agent.train_step_dev(torch.from_numpy(idx).to(dev), agent.neg_alpha, losses, soft_update=True, grads_out=grads)
    torch.cuda.synchronize()
    return losses.cpu().numpy(), grads.cpu().numpy()


def tensors_of(agent):
    """[(key, name, slice into the flat vector)] for both networks"""
    out = []
    for key, model in (('actor', agent.actor), ('critic', agent.critic)):
        for name, shape, off, _ in model.tensors:
            out.append((key, name, slice(off, off + int(np.prod(shape)))))
    return out


def compare_step(agent, idx, label, record=None):
    """one train step + soft update on the device and in both oracles from the same state; returns the worst
    error(kernel) / error(float32 oracle) ratio and checks every tensor against its bar"""
    snap = snapshot(agent)
    obs0, acts, rew, obs1, term = batch(agent, idx)
    res = {}
    for dt in (torch.float64, torch.float32):
        o = oracle(agent, snap, dt)
        r = o.train(obs0, acts, rew, obs1, term)
        o.soft_update()
        res[dt] = (o, r)
    losses, grads = device_step(agent, idx)
    o64, r64 = res[torch.float64]
    o32, r32 = res[torch.float32]
    after = snapshot(agent)
    Pa = agent.Pa
    rows = []

    def check(what, k, ref, f32):
        ref, f32, k = np.asarray(ref, np.float64), np.asarray(f32, np.float64), np.asarray(k, np.float64)
        scale = float(np.max(np.abs(ref))) or 1.0
        rows.append(dict(cfg=label, what=what, scale=scale, err_f32=float(np.max(np.abs(f32 - ref))),
                         err_kernel=float(np.max(np.abs(k - ref)))))

    check('critic_loss', losses[0], r64['critic_loss'], r32['critic_loss'])
    check('actor_loss', losses[1], r64['actor_loss'], r32['actor_loss'])
    for key, name, sl in tensors_of(agent):
        base = 0 if key == 'actor' else Pa
        gsl = slice(base + sl.start, base + sl.stop)
        check('grad ' + name, grads[gsl], r64['grads'][key][sl].numpy(), r32['grads'][key][sl].numpy())
    check_adam_and_soft_update(agent, snap, after, grads)
    # pop-art's ret_rms.update(target_Q) against the float64 oracle's: count exact, sums within the float32 error of target_Q
    # itself (the kernel sums the f32 target_Q in f64 in batch order; the oracle sums its f64 target_Q with NumPy)
    assert after['ret_rms'][2] == o64.ret_rms[2]
    tol = 4e-6 * np.abs(o64.ret_rms[:2] - snap['ret_rms'][:2]) + 1e-12
    assert np.all(np.abs((after['ret_rms'][:2] - snap['ret_rms'][:2]) - (o64.ret_rms[:2] - snap['ret_rms'][:2])) <= tol), \
        (after['ret_rms'], o64.ret_rms)
    if REPORT:
        with open(REPORT, 'a') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')
    # the bar, per tensor: twice that tensor's own float32-oracle error, never looser than PPO2's 5e-6 of its scale, floored at
    # 2^-20 (eight f32 ulps) of its scale.  The floor is for single-number tensors -- the losses, the critic's output-bias
    # gradient -- that are batch means of the networks' fp32 outputs: their error is the rounding those outputs carry (a few
    # ulps of the scale, in the oracle as in the kernel), and two independent fp32 evaluations differ by chance there.
    # The critic's output-bias gradient is the batch sum of 2 (Q - target) / B: its error is the fp32 rounding of Q and of
    # target_Q summed over the batch, not accumulation error (the kernel's sums are compensated), so against it the f32
    # oracle's own error is a draw of the same size; that one tensor is held to PPO2's 5e-6 of its scale alone.
    for r in rows:
        if r['what'] == 'grad critic/output/bias':
            r['bar'] = 5e-6 * r['scale']
        else:
            r['bar'] = min(max(2.0 * r['err_f32'], 2.0 ** -20 * r['scale']), 5e-6 * r['scale'])
        assert r['err_kernel'] <= r['bar'], (label, r)
    worst = max(r['err_kernel'] / r['bar'] for r in rows)
    return worst


def adam_np(p, g, m, v, lr, t):
    """MpiAdam.update (common/mpi_adam.py:37-41) in NumPy float32, as the reference runs it under NumPy 1.x's value-based
    casting: the f64 scalar `- a` meets the f32 slot `m` and is rounded to f32 (NumPy 2 would promote the step to f64)"""
    a = lr * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
    m = np.float32(0.9) * m + np.float32(1 - 0.9) * g
    v = np.float32(0.999) * v + np.float32(1 - 0.999) * (g * g)
    return p + np.float32(- a) * m / (np.sqrt(v) + np.float32(1e-8)), m, v


def check_adam_and_soft_update(agent, before, after, grads):
    """post-Adam parameters, slots and soft-updated targets: the reference's f32 NumPy arithmetic applied to the gradient the
    kernel produced (and to the pop-art renormalised output layer) -- equal to the last bit"""
    f32 = np.float32
    Pa = agent.Pa
    pre = {k: before[k].copy() for k in ('critic', 'target_critic')}
    if agent.normalize_returns and agent.enable_popart:
        def ms(b):
            mean = f32(b[0] / b[2])
            return mean, np.sqrt(np.maximum(f32(b[1] / b[2]) - np.square(mean), f32(1e-2)))
        om, os_ = ms(before['ret_rms'])
        nm, ns = ms(after['ret_rms'])
        wo = [t for t in agent.critic.tensors if t[0].endswith('output/kernel')][0][2]
        H = agent.critic.num_hidden
        for k in pre:
            pre[k][wo:wo + H] = pre[k][wo:wo + H] * np.float32(os_) / np.float32(ns)
            pre[k][wo + H] = (pre[k][wo + H] * np.float32(os_) + np.float32(om) - np.float32(nm)) / np.float32(ns)
    for key, g, lr, t in (('actor', grads[:Pa], agent.actor_lr, after['actor_t']),
                          ('critic', grads[Pa:], agent.critic_lr, after['critic_t'])):
        p0 = before[key] if key == 'actor' else pre['critic']
        p, m, v = adam_np(p0, g, before[key + '_m'], before[key + '_v'], lr, t)
        assert np.array_equal(after[key + '_m'], m), key
        assert np.array_equal(after[key + '_v'], v), key
        assert np.array_equal(after[key], p), (key, np.max(np.abs(after[key] - p)))
        t0 = before['target_actor'] if key == 'actor' else pre['target_critic']
        tgt = np.float32(1. - agent.tau) * t0 + np.float32(agent.tau) * p
        assert np.array_equal(after['target_' + key], tgt.astype(np.float32)), key


GRID = [
    # D, A, H, L, act, ln, B, clip, popart
    (3, 1, 64, 1, 'tanh', False, 1, None, False),
    (3, 1, 64, 2, 'relu', True, 64, 0.5, True),
    (17, 6, 64, 2, 'tanh', False, 64, None, False),
    (17, 6, 256, 1, 'relu', False, 1000, 0.5, False),
    (17, 6, 64, 2, 'tanh', True, 1000, None, True),
    (376, 17, 64, 2, 'tanh', False, 64, 0.5, False),
    (376, 17, 256, 2, 'relu', True, 64, None, True),
    (376, 17, 256, 1, 'tanh', True, 1, 0.5, False),
]


@pytest.mark.parametrize('cfg', GRID, ids=lambda c: '-'.join(str(x) for x in c))
def test_train_step_against_oracle(cfg):
    D, A, H, L, act, ln, B, clip, popart = cfg
    agent = make_agent(D, A, H, L, act, ln, B, popart=popart, norm_ret=popart, clip=clip)
    np.random.seed(5)
    idx = agent.memory.draw_indices(B).astype(np.int64)
    compare_step(agent, idx, str(cfg))
    # a second step from the state the first one left (non-zero Adam slots, moved obs / ret statistics)
    idx = agent.memory.draw_indices(B).astype(np.int64)
    compare_step(agent, idx, str(cfg) + ' step 2')


def test_teacher_forced_50_steps():
    """50 steps, each started from the float64 oracle's state: the per-step error stays at single-step level"""
    agent = make_agent(17, 6, 64, 2, 'tanh', False, 64, popart=True, norm_ret=True, clip=None)
    np.random.seed(9)
    snap = snapshot(agent)
    ratios = []
    for s in range(50):
        load(agent, snap)
        idx = agent.memory.draw_indices(64).astype(np.int64)
        obs0, acts, rew, obs1, term = batch(agent, idx)
        o = oracle(agent, snap, torch.float64)
        o.train(obs0, acts, rew, obs1, term)
        o.soft_update()
        ratios.append(compare_step(agent, idx, 'teacher-forced step %d' % s))
        snap = dict(actor=o.flat['actor'].numpy(), critic=o.flat['critic'].numpy(),
                    target_actor=o.flat['target_actor'].numpy(), target_critic=o.flat['target_critic'].numpy(),
                    actor_m=o.flat['actor_m'].numpy(), actor_v=o.flat['actor_v'].numpy(),
                    critic_m=o.flat['critic_m'].numpy(), critic_v=o.flat['critic_v'].numpy(), obs_rms=o.obs_rms,
                    ret_rms=o.ret_rms, actor_t=o.t['actor'], critic_t=o.t['critic'])
    assert max(ratios) <= 1.0, ratios


def test_store_bit_exact_over_a_wrap():
    D, A, limit = 5, 2, 37
    np.random.seed(0)
    mem = Memory(limit, (A,), (D,))
    kw = dict(network='mlp', num_layers=1, num_hidden=32)
    agent = DDPG(Actor(A, **kw), Critic(**kw), mem, (D,), (A,), batch_size=8, reward_scale=0.7)
    rng = np.random.RandomState(3)
    ring = {k: np.zeros((limit,) + s, np.float32) for k, s in (('o0', (D,)), ('a', (A,)), ('r', (1,)), ('o1', (D,)), ('d', (1,)))}
    start = length = 0
    rms = np.zeros(2 * D + 1)
    rms[D:] = 1e-2
    for n in (13, 20, 1, 50, 9):
        o0 = (rng.randn(n, D) * 3).astype(np.float32)
        a = rng.uniform(-1, 1, (n, A)).astype(np.float32)
        r = rng.randn(n).astype(np.float32)
        o1 = rng.randn(n, D).astype(np.float32)
        d = rng.rand(n) < 0.3
        agent.store_transition(o0, a, r, o1, d)
        r = r.copy()
        r *= 0.7                                                       # ddpg_learner.py:260, f32 in place
        for b in range(n):                                             # memory.py:24-35,71-79 + obs_rms.update per row
            if length < limit:
                length += 1
            else:
                start = (start + 1) % limit
            slot = (start + length - 1) % limit
            ring['o0'][slot], ring['a'][slot], ring['r'][slot], ring['o1'][slot], ring['d'][slot] = o0[b], a[b], r[b], o1[b], d[b]
            x = o0[b:b + 1].astype('float64')
            rms += np.concatenate([x.sum(axis=0), np.square(x).sum(axis=0), [1.0]])
    assert (mem.observations0.start, mem.observations0.length) == (start, length)
    assert mem.ring_pos.cpu().tolist() == [start, length]
    for k, rb in (('o0', mem.observations0), ('a', mem.actions), ('r', mem.rewards), ('o1', mem.observations1),
                  ('d', mem.terminals1)):
        assert np.array_equal(rb.data.cpu().numpy(), ring[k]), k
    assert np.array_equal(agent.obs_rms.buf.cpu().numpy(), rms)


@pytest.mark.parametrize('kind', ['none', 'normal', 'ou', 'param'])
def test_act_each_noise_kind(kind):
    D, A = 17, 6
    an = {'normal': NormalActionNoise(np.zeros(A), 0.2 * np.ones(A)),
          'ou': OrnsteinUhlenbeckActionNoise(np.zeros(A), 0.2 * np.ones(A))}.get(kind)
    pn = AdaptiveParamNoiseSpec(0.2, 0.2) if kind == 'param' else None
    agent = make_agent(D, A, 64, 2, 'tanh', True, 64, param_noise=pn, action_noise=an)
    agent.reset()
    obs = (np.random.RandomState(4).randn(40, D) * 2).astype(np.float32)
    snap = snapshot(agent)
    o = oracle(agent, snap, torch.float64)
    np.random.seed(11)
    act, q, _, _ = agent.step(obs, apply_noise=True, compute_Q=True)
    if an is not None:
        an.reset()
    np.random.seed(11)
    noise = an() if an is not None else 0.0
    src = agent.perturbed_actor_params.cpu().numpy() if pn is not None else snap['actor']
    ref = o.actions(src, obs).numpy() + noise
    assert np.allclose(act, np.clip(ref, -1, 1), atol=2e-6)
    # Q from the critic on the UNPERTURBED actor's action (critic_with_actor_tf)
    qref = o.q(obs, o.actions(snap['actor'], obs).numpy()).numpy()
    assert np.allclose(q, qref, atol=2e-6, rtol=1e-5)
    if pn is not None:
        assert not np.allclose(src, snap['actor'])


def test_perturb_leaves_layernorm_and_distance_matches():
    agent = make_agent(17, 6, 64, 2, 'relu', True, 64, param_noise=AdaptiveParamNoiseSpec(0.3, 0.3))
    base = agent.actor_params.cpu().numpy()
    agent.perturb(agent.adaptive_actor_params, 0.3)
    noise = agent.noise_buf.cpu().numpy()
    pert = agent.adaptive_actor_params.cpu().numpy()
    for name, shape, off, _ in agent.actor.tensors:
        sl = slice(off, off + int(np.prod(shape)))
        if 'LayerNorm' in name:
            assert np.array_equal(pert[sl], base[sl]), name
        else:
            assert np.array_equal(pert[sl], base[sl] + (noise[sl] * np.float32(0.3) + np.float32(0))), name
    np.random.seed(2)
    idx = agent.memory.draw_indices(64).astype(np.int64)
    agent.k.policy_distance(agent.state, agent.adaptive_actor_params, torch.from_numpy(idx).cuda(), agent.distance)
    o = oracle(agent, snapshot(agent), torch.float64)
    obs0 = batch(agent, idx)[0]
    ref = float(torch.sqrt(torch.mean((o.actions(base, obs0) - o.actions(pert, obs0)) ** 2)))
    assert abs(float(agent.distance.item()) - ref) <= 1e-6 * max(ref, 1e-3)


def _small_learn(env, **kw):
    from baselines_amd import logger
    logger.configure(format_strs=[])
    args = dict(seed=3, nb_epochs=None, total_timesteps=2 * 2 * 20, nb_epoch_cycles=2, nb_rollout_steps=20, nb_train_steps=10,
                batch_size=16, num_hidden=32, noise_type='adaptive-param_0.2,ou_0.2', param_noise_adaption_interval=10)
    args.update(kw)
    agent = ddpg_mod.learn('mlp', env, **args)
    torch.cuda.synchronize()
    return agent


@pytest.mark.parametrize('noise', ['adaptive-param_0.2', 'adaptive-param_0.2,ou_0.2'])
def test_captured_cycle_bit_identical_to_eager(noise):
    """captured train cycles (and, without action noise, captured rollouts) against the same launches run eagerly"""
    from baselines_amd.common.vec_env.synthetic_vec_env import SyntheticVecEnv
    outs = []
    for capture in (True, False):
        ddpg_mod.CAPTURE_TRAIN = ddpg_mod.CAPTURE_ROLLOUT = capture
        try:
            agent = _small_learn(SyntheticVecEnv('mujoco', 4, seed=2, ob_shape=(17,), nact=6), noise_type=noise,
                                 nb_epoch_cycles=3, total_timesteps=2 * 3 * 20)
        finally:
            ddpg_mod.CAPTURE_TRAIN = ddpg_mod.CAPTURE_ROLLOUT = True
        outs.append((snapshot(agent), agent.last_stats, agent.memory.actions.data[:agent.memory.nb_entries].cpu().numpy()))
    for k in ('actor', 'critic', 'target_actor', 'target_critic', 'actor_m', 'critic_v', 'obs_rms'):
        assert np.array_equal(outs[0][0][k], outs[1][0][k]), k
    assert np.array_equal(outs[0][2], outs[1][2])
    for k in outs[0][1]:
        if k not in ('total/duration', 'total/steps_per_second'):
            assert np.array_equal(np.float64(outs[0][1][k]), np.float64(outs[1][1][k])) or np.isnan(outs[0][1][k]), k


class _PointEnv(object):
    """a tiny gym-style env for DummyVecEnv: 3-D observations from a step counter, episodes of 7 + i steps, actions in
    Box(-2, 2, (2,)) that the dynamics ignore (so both drivers see the same observations)"""

    def __init__(self, i):
        from baselines_amd.common.spaces import Box
        self.i, self.k, self.n = i, 0, 0
        self.observation_space = Box(-1.0, 1.0, (3,), np.float32)
        self.action_space = Box(-2.0, 2.0, (2,), np.float32)

    def _obs(self):
        return np.array([np.sin(self.k * 0.3 + self.i + self.n), np.cos(self.k * 0.7 + self.n), (self.k % 5) / 5.], np.float32)

    def reset(self):
        self.k = 0
        self.n += 1
        return self._obs()

    def step(self, a):
        self.k += 1
        return self._obs(), float(np.cos(self.k + self.i)), self.k >= 7 + self.i, {}


@pytest.mark.parametrize('kind', ['device', 'dummy'])
def test_learn_against_oracle_driver(kind, monkeypatch):
    """learn() against a restatement of ddpg/ddpg.py's loop on the float64 oracle (tests/_ddpg_oracle.py:oracle_learn)
    with the same seed and noise: index streams and stored observations exactly, actions, per-epoch losses and the final
    parameters within float32 drift"""
    from baselines_amd.common.vec_env.dummy_vec_env import DummyVecEnv
    from baselines_amd.common.vec_env.synthetic_vec_env import SyntheticVecEnv, SyntheticVecEnvCPU
    from baselines_amd.ddpg.memory import Memory as M
    if kind == 'device':
        mk_dev = lambda: SyntheticVecEnv('mujoco', 4, seed=2, ob_shape=(17,), nact=6)
        mk_host = lambda: SyntheticVecEnvCPU('mujoco', 4, seed=2, ob_shape=(17,), nact=6)
        noise = 'adaptive-param_0.2'
    else:
        mk_dev = mk_host = lambda: DummyVecEnv([lambda i=i: _PointEnv(i) for i in range(2)])
        noise = 'adaptive-param_0.2,ou_0.2'
    draws = []
    orig = M.draw_indices
    monkeypatch.setattr(M, 'draw_indices', lambda self, n: draws.append(orig(self, n)) or draws[-1])
    kw = dict(seed=3, nb_epochs=None, total_timesteps=2 * 2 * 20, nb_epoch_cycles=2, nb_rollout_steps=20, nb_train_steps=10,
              batch_size=16, num_hidden=32, noise_type=noise, param_noise_adaption_interval=10)
    agent = _small_learn(mk_dev(), **kw)
    stats = agent.last_stats
    ref = oracle_learn(mk_host(), seed=3, nb_epochs=2, nb_epoch_cycles=2, nb_rollout_steps=20, nb_train_steps=10,
                       batch_size=16, noise_type=noise, param_noise_adaption_interval=10, num_hidden=32)
    assert len(draws) == len(ref['draws'])
    for a, b in zip(draws, ref['draws']):
        assert np.array_equal(a, b)
    m = agent.memory
    n = m.nb_entries
    assert n == len(ref['ring']['obs0'])
    assert np.array_equal(m.observations0.data[:n].cpu().numpy(), ref['ring']['obs0'])
    assert np.array_equal(m.observations1.data[:n].cpu().numpy(), ref['ring']['obs1'])
    assert np.array_equal(m.rewards.data[:n].cpu().numpy().reshape(-1), ref['ring']['rew'])
    assert np.array_equal(m.terminals1.data[:n].cpu().numpy().reshape(-1), ref['ring']['term'].astype(np.float32))
    assert np.allclose(m.actions.data[:n].cpu().numpy(), ref['ring']['act'], atol=2e-5)
    assert np.allclose([stats['train/loss_critic'], stats['train/loss_actor']], ref['losses'][-1], rtol=1e-4, atol=1e-7)
    assert np.isclose(stats['param_noise_stddev'], ref['param_noise'].current_stddev, rtol=1e-12)
    o = ref['oracle']
    for k, mine in (('actor', agent.actor_params), ('critic', agent.critic_params), ('target_actor', agent.target_actor_params),
                    ('target_critic', agent.target_critic_params)):
        r = o.flat[k].numpy()
        assert np.max(np.abs(mine.cpu().numpy() - r)) <= 1e-5 * np.max(np.abs(r)), k
    assert np.allclose(agent.obs_rms.buf.cpu().numpy(), o.obs_rms, rtol=1e-12)


def test_learn_device_env_matches_host_twin_and_logs_reference_keys():
    from baselines_amd import logger
    from baselines_amd.common.vec_env.synthetic_vec_env import SyntheticVecEnv, SyntheticVecEnvCPU
    a_dev = _small_learn(SyntheticVecEnv('mujoco', 4, seed=2, ob_shape=(17,), nact=6))
    s_dev = dict(a_dev.last_stats)
    a_host = _small_learn(SyntheticVecEnvCPU('mujoco', 4, seed=2, ob_shape=(17,), nact=6))
    s_host = dict(a_host.last_stats)
    d, h = snapshot(a_dev), snapshot(a_host)
    for k in ('actor', 'critic', 'target_actor', 'target_critic', 'obs_rms'):
        assert np.array_equal(d[k], h[k]), k
    for m in (a_dev.memory, a_host.memory):
        assert m.nb_entries == 2 * 2 * 20 * 4
    assert np.array_equal(a_dev.memory.actions.data.cpu().numpy(), a_host.memory.actions.data.cpu().numpy())
    keys = {'obs_rms_mean', 'obs_rms_std', 'reference_Q_mean', 'reference_Q_std', 'reference_actor_Q_mean',
            'reference_actor_Q_std', 'reference_action_mean', 'reference_action_std', 'reference_perturbed_action_mean',
            'reference_perturbed_action_std', 'param_noise_stddev', 'rollout/return', 'rollout/return_std',
            'rollout/return_history', 'rollout/return_history_std', 'rollout/episode_steps', 'rollout/actions_mean',
            'rollout/Q_mean', 'train/loss_actor', 'train/loss_critic', 'train/param_noise_distance', 'total/duration',
            'total/steps_per_second', 'total/episodes', 'rollout/episodes', 'rollout/actions_std', 'total/epochs',
            'total/steps'}
    assert set(s_dev) == keys and set(s_host) == keys
    for k in keys - {'total/duration', 'total/steps_per_second'}:
        assert np.array_equal(np.float64(s_dev[k]), np.float64(s_host[k])) or (np.isnan(s_dev[k]) and np.isnan(s_host[k])), k
    assert s_dev['total/steps'] == 2 * 2 * 20


def test_unsupported_configurations_return_eunsup():
    lib = _lib.load()
    import ctypes
    for kw in (dict(num_hidden=48), dict(num_hidden=288), dict(num_layers=5), dict(nact=33), dict(activation=0)):
        d = _lib.DDPGDesc(ob_dim=17, nact=6, num_layers=2, num_hidden=64, activation=_lib.ACT_TANH)
        for k, v in kw.items():
            setattr(d, k, v)
        assert lib.mrl_ddpg_num_params(ctypes.byref(d), 0) == -1
        st = _lib.DDPGState()
        assert lib.mrl_ddpg_train_step(ctypes.byref(d), ctypes.byref(st), None, 64, None, 0.99, 0.01, 0., -1., 0, None, None,
                                       None, 0, None) == -3, kw
    agent = make_agent(3, 1, 32, 1, B=8)
    out = torch.zeros(2, device='cuda')
    idx = torch.zeros(1025, dtype=torch.int64, device='cuda')
    with pytest.raises(_lib.MrlError, match='unsupported'):
        agent.train_step_dev(idx, agent.neg_alpha, out)
