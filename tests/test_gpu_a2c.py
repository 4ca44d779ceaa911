"""GPU: A2C (baselines_amd.a2c) -- the n-step returns kernel, clip + RMSProp, the A2C head gradients on every head-kernel
path, learn() end to end, the captured returns + train-step graph, checkpoints and the refusal of a communicator.
References: tests/golden/a2c.npz (the reference's Runner.run), tests/_a2c_oracle.py (float64 returns, float32 RMSProp, the
A2C loss on oracle.ppo2_torch.OracleModel)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests._a2c_oracle import A2COracle, nstep_returns, rmsprop_step

pytestmark = pytest.mark.gpu


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------- 1. returns kernel
def test_nstep_returns_bit_identical_to_reference(golden_dir):
    from baselines_amd import ops
    g = np.load(os.path.join(golden_dir, 'a2c.npz'))
    for name in g['cases']:
        f = lambda k: g['%s/%s' % (name, k)]
        T, N = f('in_rewards').shape
        ret = ops.nstep_returns(dev(f('in_rewards')), dev(f('in_dones')), dev(f('in_last_values')),
                                dev(f('in_last_dones')), float(f('gamma'))).cpu().numpy()
        ref = f('out_returns').reshape(N, T).swapaxes(0, 1)
        assert np.array_equal(u32(ret), u32(ref)), name


@pytest.mark.parametrize('T', [1, 5, 128])
def test_nstep_returns_vs_float64_restatement(T):
    from baselines_amd import ops
    rng = np.random.RandomState(T)
    for N in (1, 63, 64, 65, 4096):
        rew = (3 * rng.randn(T, N)).astype(np.float32)
        rew[rng.rand(T, N) < 0.05] = -0.0
        dones = (rng.rand(T, N) < 0.1).astype(np.uint8)
        lv = rng.randn(N).astype(np.float32)
        ld = (rng.rand(N) < 0.3).astype(np.uint8)
        out = torch.full((T, N), np.nan, dtype=torch.float32, device='cuda')
        ops.nstep_returns(dev(rew), dev(dones), dev(lv), dev(ld), 0.99, out=out)
        assert np.array_equal(u32(out.cpu().numpy()), u32(nstep_returns(rew, dones, lv, ld, 0.99))), (T, N)


# ---------------------------------------------------------------------------------------------------- 2. clip + RMSProp
def _rms_bufs(P, seed):
    rng = np.random.RandomState(seed)
    p = rng.randn(P).astype(np.float32)
    grads = [(0.3 * rng.randn(P)).astype(np.float32) for _ in range(3)]
    return p, grads


def test_rmsprop_unclipped_bit_identical():
    from baselines_amd import _lib, ops
    P = 1031                                    # not a multiple of 4 or 256: the vector body and the tail both run
    p, grads = _rms_bufs(P, 0)
    ms, mom = np.ones(P, np.float32), np.zeros(P, np.float32)
    dp, dms, dmom = dev(p), dev(ms), dev(mom)
    scratch = torch.empty(int(_lib.load().mrl_adam_scratch_bytes(P)), dtype=torch.uint8, device='cuda')
    lr_dev = dev(np.array([7e-4], np.float32))
    for k, g in enumerate(grads):
        dg = dev(g)
        if k == 1:                              # the device-scalar form gives the same bits
            ops.rmsprop_clip_step(dp, dg, dms, dmom, 0.0, 0.99, 0.0, 1e-5, None, scratch, lr_dev=lr_dev)
        else:
            ops.rmsprop_clip_step(dp, dg, dms, dmom, 7e-4, 0.99, 0.0, 1e-5, None, scratch)
        rmsprop_step(p, g, ms, mom, 7e-4, 0.99, 0.0, 1e-5, None)
        assert np.array_equal(u32(dp.cpu().numpy()), u32(p)), k
        assert np.array_equal(u32(dms.cpu().numpy()), u32(ms)), k
        assert np.array_equal(u32(dmom.cpu().numpy()), u32(mom)), k


def test_rmsprop_clipped_within_one_ulp():
    from baselines_amd import _lib, ops
    P = 1031
    p, grads = _rms_bufs(P, 1)
    ms, mom = np.ones(P, np.float32), np.zeros(P, np.float32)
    dp, dms, dmom = dev(p), dev(ms), dev(mom)
    scratch = torch.empty(int(_lib.load().mrl_adam_scratch_bytes(P)), dtype=torch.uint8, device='cuda')
    gn_d = torch.zeros(1, dtype=torch.float32, device='cuda')
    dg = dev(grads[0])
    ops.rmsprop_clip_step(dp, dg, dms, dmom, 7e-4, 0.99, 0.0, 1e-5, 0.5, scratch, gnorm_out=gn_d)
    gc, gn = rmsprop_step(p, grads[0], ms, mom, 7e-4, 0.99, 0.0, 1e-5, 0.5)
    assert gn > 0.5                             # the clip is active
    assert abs(float(gn_d.item()) - float(gn)) <= 1e-6 * float(gn)
    # the clipped gradient within 1 ulp; the update from it within a few ulp of the restatement's
    np.testing.assert_array_less(np.abs(dg.cpu().numpy() - gc), np.spacing(np.abs(gc)) * 1.0001 + 1e-30)
    np.testing.assert_allclose(dp.cpu().numpy(), p, rtol=0, atol=4 * np.spacing(np.abs(p)).max())


# ---------------------------------------------------------------------------------------------------- 3. gradients
GRAD_CASES = {
    # name: (env kind, network, value_network, env kwargs, T, N)
    'cartpole_mlp_generic': ('cartpole', 'mlp', None, {}, 5, 8),
    'mujoco_mlp_copy': ('mujoco', 'mlp', 'copy', {}, 5, 6),
    'atari_cnn_wave2_nact6': ('atari', 'cnn', None, {}, 5, 4),
    'atari_cnn_wave_nact8': ('atari', 'cnn', None, dict(nact=8), 5, 4),
    'lstm_vector_env': ('cartpole', 'lstm', None, dict(ob_shape=(12,)), 5, 6),
}


def _model(kind, net, vn, env_kw, N, T, seed=0, **model_kw):
    from baselines_amd.a2c import Model
    from baselines_amd.common import set_global_seeds
    from baselines_amd.common.policies import build_policy
    from baselines_amd.common.vec_env.synthetic_vec_env import SyntheticVecEnv
    env = SyntheticVecEnv(kind, N, seed=3, **env_kw)
    set_global_seeds(seed)
    kw = dict(nlstm=32) if net == 'lstm' else {}
    policy = build_policy(env, net, value_network=vn, **kw)
    model = Model(policy=policy, env=env, nsteps=T, **model_kw)
    return env, model


def _oracle(env, model, net, vn, dtype, params=None):
    kw = dict(nlstm=32) if net == 'lstm' else {}
    om = A2COracle(network=net, ob_shape=env.observation_space.shape, ob_dtype=env.observation_space.dtype,
                   pd_kind=model.pd_kind, nact=model.nact, value_network=vn, ent_coef=0.01, vf_coef=0.5,
                   max_grad_norm=0.5, dtype=dtype, params=params, **kw)
    return om


def _params_dict(model):
    flat = model.get_flat_params()
    return {t['name']: flat[t['offset']:t['offset'] + t['size']].reshape(t['shape']) for t in model.dm.tensors}


@pytest.mark.parametrize('name', list(GRAD_CASES))
def test_a2c_gradient_vs_fp64_oracle(name):
    kind, net, vn, env_kw, T, N = GRAD_CASES[name]
    env, model = _model(kind, net, vn, env_kw, N, T)
    om = _oracle(env, model, net, vn, torch.float64, params=_params_dict(model))
    B = N * T
    rng = np.random.RandomState(5)
    shape = env.observation_space.shape
    if env.observation_space.dtype == np.uint8:
        obs = rng.randint(0, 256, (B,) + shape).astype(np.uint8)
    else:
        obs = rng.randn(B, *shape).astype(np.float32)
    if model.pd_kind == 'categorical':
        actions = rng.randint(0, model.nact, B)
        d_act = dev(actions.astype(np.int32))
    else:
        actions = rng.randn(B, model.nact).astype(np.float32)
        d_act = dev(actions)
    rewards, values = (2 * rng.randn(B)).astype(np.float32), rng.randn(B).astype(np.float32)
    grads = torch.empty(model.dm.P, dtype=torch.float32, device='cuda')
    stats = torch.empty(3, dtype=torch.float32, device='cuda')
    states = masks = None
    d_m = d_s = None
    nseq = 0
    if model.recurrent:                          # env-major rows: N whole trajectories of T steps, dones inside
        masks = rng.rand(B) < 0.25
        states = (0.5 * rng.randn(N, model.dm.state_size)).astype(np.float32)
        d_m, d_s, nseq = dev(masks.view(np.uint8)), dev(states), N
    model.dm.grad_a2c(model.params, dev(obs), d_act, dev(rewards), dev(values), d_m, d_s, nseq, None, B, 1, 1, 0.01, 0.5,
                      grads, stats)
    s64, g64 = om.a2c_grads(obs, rewards, actions, values, states=states, masks=masks)
    g_d = grads.cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(stats.cpu().numpy(), np.array(s64), rtol=1e-5, atol=1e-5)
    # the PPO2 bar (test_gpu_benched_shapes.py); recurrent nets: the bar of test_gpu_lstm.py (gates through T steps)
    bar = 5e-5 if model.recurrent else 5e-6
    scale = np.abs(g64).max()
    for t in model.dm.tensors:
        sl = slice(t['offset'], t['offset'] + t['size'])
        tol = bar * max(np.abs(g64[sl]).max(), 1e-3 * scale)
        assert np.abs(g_d[sl] - g64[sl]).max() <= tol, (name, t['name'], np.abs(g_d[sl] - g64[sl]).max(), tol)


# ---------------------------------------------------------------------------------------------------- 4. learn()
@pytest.mark.parametrize('kind', ['cartpole', 'atari'])
def test_learn_vs_oracle_replay(kind, monkeypatch):
    from baselines_amd.a2c import a2c as A
    from baselines_amd.a2c.utils import schedules
    from baselines_amd.common.vec_env.synthetic_vec_env import SyntheticVecEnv
    N, T, U = 8, 5, 3
    net = 'cnn' if kind == 'atari' else 'mlp'
    rec = []
    orig = A.Model.train_rollout

    def recording(self, runner, lr=None):
        ro = runner.rollout
        if not rec:
            rec.append(dict(params0=self.get_flat_params()))
        r = dict(obs=ro.obs.cpu().numpy(), act=ro.actions.cpu().numpy(), rew=ro.rewards.cpu().numpy(),
                 val=ro.values.cpu().numpy(), dones=ro.dones.cpu().numpy(), lv=runner.last_values.cpu().numpy(),
                 ld=runner._dones_dev.cpu().numpy())
        out = orig(self, runner, lr)
        r.update(ret=ro.returns.cpu().numpy(), stats=out.cpu().numpy(), lr=self.last_lr)
        rec.append(r)
        return out

    monkeypatch.setattr(A.Model, 'train_rollout', recording)
    env = SyntheticVecEnv(kind, N, seed=11)
    total = U * N * T
    model = A.learn(network=net, env=env, seed=0, nsteps=T, total_timesteps=total, log_interval=1)
    assert len(rec) == U + 1
    # initial parameters: the oracle's draw of the same seed (ortho_init order, a2c/utils.py:20-35)
    np.random.seed(0)
    om = _oracle(env, model, net, None, torch.float64)
    np.testing.assert_array_equal(om.flat_params().astype(np.float32), rec[0]['params0'])
    for u, r in enumerate(rec[1:], 1):
        assert r['lr'] == np.float32(7e-4 * schedules['linear']((u * N * T - 1) / total)), u
        ret = nstep_returns(r['rew'], r['dones'], r['lv'], r['ld'], 0.99)
        assert np.array_equal(u32(r['ret']), u32(ret)), u
        em = lambda x: np.ascontiguousarray(x.swapaxes(0, 1)).reshape((N * T,) + x.shape[2:])     # time-major -> env-major
        st = om.a2c_train(r['lr'], em(r['obs']), None, em(ret), em(r['dones']), em(r['act']).astype(np.int64), em(r['val']))
        np.testing.assert_allclose(r['stats'], np.array(st), rtol=1e-5, atol=1e-5)
    # RMSProp steps of ~ lr * g / sqrt(ms ~ 1) do not amplify round-off the way Adam's sign-like steps do
    np.testing.assert_allclose(model.get_flat_params(), om.flat_params(), rtol=0, atol=2e-6)


# ---------------------------------------------------------------------------------------------------- 5. captured graph
def test_captured_step_replays_like_eager(monkeypatch):
    from baselines_amd.a2c import Runner
    results = []
    for graph in ('1', '0'):
        monkeypatch.setenv('MRL_A2C_GRAPH', graph)
        env, model = _model('cartpole', 'mlp', None, {}, 8, 5)
        runner = Runner(env, model, nsteps=5, gamma=0.99, return_host=False)
        runner.returns_by_model = True
        stats = []
        for _ in range(4):
            runner.run()
            stats.append(model.train_rollout(runner).cpu().numpy())
        if graph == '1':
            assert isinstance(model._a2c_graph, dict), 'the step graph was not captured'
        else:
            assert model._a2c_graph is None
        results.append((model.get_flat_params(), model.rms_ms.cpu().numpy(), np.stack(stats),
                        runner.rollout.returns.cpu().numpy()))
    for a, b in zip(*results):
        assert np.array_equal(u32(a), u32(b))


# ---------------------------------------------------------------------------------------------------- 6. checkpoints
def test_save_load_roundtrip(tmp_path):
    from baselines_amd.a2c import Runner, learn
    env, model = _model('cartpole', 'mlp', None, {}, 4, 5)
    runner = Runner(env, model, nsteps=5, gamma=0.99, return_host=True)
    obs, states, rewards, masks, actions, values, _ = runner.run()
    pl, vl, ent = model.train(obs, states, rewards, masks, actions, values)
    assert np.isfinite([pl, vl, ent]).all()
    path = str(tmp_path / 'a2c.joblib')
    model.save(path)
    import joblib
    d = joblib.load(path)
    assert 'a2c_model/pi/w:0' in d and 'a2c_model/pi/w/RMSProp:0' in d and 'a2c_model/pi/w/RMSProp_1:0' in d
    _, other = _model('cartpole', 'mlp', None, {}, 4, 5, seed=1)
    assert not np.array_equal(other.get_flat_params(), model.get_flat_params())
    other.load(path)
    for a, b in ((other.params, model.params), (other.rms_ms, model.rms_ms), (other.rms_mom, model.rms_mom)):
        assert np.array_equal(u32(a.cpu().numpy()), u32(b.cpu().numpy()))
    built = learn(network='mlp', env=env, seed=3, nsteps=5, total_timesteps=0, load_path=path)
    assert np.array_equal(built.get_flat_params(), model.get_flat_params())
    assert built._a2c_calls == 0


# ---------------------------------------------------------------------------------------------------- 7. no communicator
def test_communicator_refused():
    from baselines_amd.a2c import Runner
    env, model = _model('cartpole', 'mlp', None, {}, 4, 5)
    runner = Runner(env, model, nsteps=5, gamma=0.99, return_host=False)
    runner.run()
    fake = ctypes.c_void_p(64)                   # never dereferenced: the A2C entries refuse any attached communicator
    model.attach_comm(fake, 1.0)
    try:
        with pytest.raises(NotImplementedError, match='communicator'):
            model.train_rollout(runner)
        torch.cuda.synchronize()
    finally:
        model.attach_comm(None, 1.0)
    model.train_rollout(runner)
    torch.cuda.synchronize()
