"""CPU: DDPG's host-side pieces against tests/golden/ddpg.npz (written from the reference's own ddpg/memory.py and
ddpg/noise.py by scripts/make_golden_ddpg.py): ring indexing over a wrap, the Memory.sample index stream, the noise
sequences, param-noise adaptation; noise_type parsing; variable names, shapes and TF order; init distributions; and
`learn` refusing what the device path does not support."""
import os

import numpy as np
import pytest
import torch

from baselines_amd.ddpg.memory import Memory, RingBuffer
from baselines_amd.ddpg.models import Actor, Critic
from baselines_amd.ddpg.noise import (AdaptiveParamNoiseSpec, NormalActionNoise, OrnsteinUhlenbeckActionNoise,
                                      parse_noise_type)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ddpg.npz')


@pytest.fixture(scope='module')
def g():
    return np.load(GOLDEN)


def test_ring_buffer_over_a_wrap(g):
    rb = RingBuffer(7, (3,), device='cpu')
    for i, v in enumerate(g['ring_values']):
        rb.append(v)
        assert (rb.start, rb.length) == tuple(g['ring_pos'][i])
        assert np.array_equal(rb.data.numpy(), g['ring_data'][i])
    with pytest.raises(KeyError):
        rb[7]


def test_memory_sample_index_stream_and_rows(g):
    np.random.seed(int(g['mem_sample_seed']))
    mem = Memory(limit=50, action_shape=(2,), observation_shape=(4,), device='cpu')
    for k, (n_app, stop) in enumerate(((30, 30), (30, 60), (20, 80))):
        for i in range(stop - n_app, stop):
            mem.append(g['mem_obs0'][i], g['mem_act'][i], g['mem_rew'][i], g['mem_obs1'][i], g['mem_term'][i])
        idx = mem.draw_indices(16)                            # randint(nb_entries - 2): the reference's quirk
        assert np.array_equal(idx, g['mem_idx'][k])
        assert idx.max() < mem.nb_entries - 2
        rows = (mem.observations0.start + idx) % mem.limit
        got = np.concatenate([mem.observations0.data.numpy()[rows], mem.actions.data.numpy()[rows],
                              mem.rewards.data.numpy()[rows], mem.observations1.data.numpy()[rows],
                              mem.terminals1.data.numpy()[rows]], axis=1)
        assert np.array_equal(got, g['mem_batches'][k])
        assert mem.ring_pos.tolist() == [mem.observations0.start, mem.nb_entries]


def test_noise_sequences(g):
    np.random.seed(3)
    nn = NormalActionNoise(mu=np.zeros(3), sigma=0.2 * np.ones(3))
    assert np.array_equal(np.stack([nn() for _ in range(10)]), g['normal_seq'])
    np.random.seed(4)
    ou = OrnsteinUhlenbeckActionNoise(mu=np.zeros(3), sigma=0.3 * np.ones(3))
    seq = []
    for i in range(25):
        if i in (10, 17):
            ou.reset()
        seq.append(ou())
    assert np.array_equal(np.stack(seq), g['ou_seq'])
    spec = AdaptiveParamNoiseSpec(initial_stddev=0.2, desired_action_stddev=0.2)
    traj = []
    for d in g['adapt_distances']:
        spec.adapt(d)
        traj.append(spec.current_stddev)
    assert np.array_equal(np.array(traj), g['adapt_stddev'])
    assert spec.get_stats() == {'param_noise_stddev': traj[-1]}


def test_noise_type_parsing():
    an, pn = parse_noise_type('adaptive-param_0.2', 3)
    assert an is None and pn.initial_stddev == 0.2 and pn.desired_action_stddev == 0.2
    an, pn = parse_noise_type('normal_0.1, adaptive-param_0.3', 2)
    assert isinstance(an, NormalActionNoise) and np.array_equal(an.sigma, [0.1, 0.1]) and pn.current_stddev == 0.3
    an, pn = parse_noise_type('ou_0.5', 4)
    assert isinstance(an, OrnsteinUhlenbeckActionNoise) and pn is None and an.mu.shape == (4,)
    assert parse_noise_type('none', 2) == (None, None)
    assert parse_noise_type(None, 2) == (None, None)
    with pytest.raises(RuntimeError, match='unknown noise type'):
        parse_noise_type('gauss_0.2', 2)


def test_variable_names_shapes_and_order():
    a = Actor(6, network='mlp', num_layers=2, num_hidden=64, layer_norm=True).build(17)
    assert [(n, s) for n, s, _, _ in a.tensors] == [
        ('actor/mlp_fc0/w', (17, 64)), ('actor/mlp_fc0/b', (64,)), ('actor/LayerNorm/beta', (64,)),
        ('actor/LayerNorm/gamma', (64,)), ('actor/mlp_fc1/w', (64, 64)), ('actor/mlp_fc1/b', (64,)),
        ('actor/LayerNorm_1/beta', (64,)), ('actor/LayerNorm_1/gamma', (64,)), ('actor/dense/kernel', (64, 6)),
        ('actor/dense/bias', (6,))]
    assert a.perturbable_vars == [v for v in a.vars if 'LayerNorm' not in v]
    c = Critic(network='mlp', num_layers=1, num_hidden=32).build(3, 1)
    assert [(n, s) for n, s, _, _ in c.tensors] == [
        ('critic/mlp_fc0/w', (4, 32)), ('critic/mlp_fc0/b', (32,)), ('critic/output/kernel', (32, 1)),
        ('critic/output/bias', (1,))]
    assert c.output_vars == ['critic/output/kernel', 'critic/output/bias']
    offs = [o for _, _, o, _ in c.tensors]
    assert offs == [0, 128, 160, 192] and c.num_params == 193


def test_init_distributions():
    np.random.seed(0)
    a = Actor(6, network='mlp', num_layers=2, num_hidden=64, layer_norm=True).build(17)
    p = a.unflatten(a.init_params())
    w0 = p['actor/mlp_fc0/w'].astype(np.float64)
    assert np.allclose(w0 @ w0.T, 2.0 * np.eye(17), atol=1e-5)                       # ortho_init(sqrt 2)
    w1 = p['actor/mlp_fc1/w'].astype(np.float64)
    assert np.allclose(w1.T @ w1, 2.0 * np.eye(64), atol=1e-5)
    k = p['actor/dense/kernel']
    assert np.abs(k).max() <= 3e-3 and np.abs(k).max() > 2e-3 and abs(k.mean()) < 1e-3
    for n in ('actor/mlp_fc0/b', 'actor/LayerNorm/beta', 'actor/dense/bias'):
        assert not p[n].any(), n
    assert np.all(p['actor/LayerNorm_1/gamma'] == 1.0)
    np.random.seed(0)
    first = a.init_params()
    np.random.seed(0)
    assert np.array_equal(first, Actor(6, network='mlp', num_layers=2, num_hidden=64, layer_norm=True).build(17).init_params())


def test_learn_refuses_unsupported_configurations(monkeypatch):
    from baselines_amd.ddpg import ddpg as D
    from baselines_amd.common.vec_env.synthetic_vec_env import SyntheticVecEnvCPU
    env = SyntheticVecEnvCPU('mujoco', 2, ob_shape=(5,), nact=2)
    with pytest.raises(NotImplementedError, match='mlp'):
        Actor(2, network='cnn')
    with pytest.raises(ValueError):
        Actor(2, network='mlp', activation='sigmoid')

    class TwoRanks(object):
        def Get_size(self):
            return 2
    monkeypatch.setattr(D, 'default_comm', lambda: TwoRanks())
    with pytest.raises(NotImplementedError, match='multi-rank'):
        D.learn('mlp', env, total_timesteps=100)
