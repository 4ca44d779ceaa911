"""A2C with the reference's protocol (a2c/a2c.py:18-232):

    Model(policy, env, nsteps, ent_coef=0.01, vf_coef=0.5, max_grad_norm=0.5, lr=7e-4, alpha=0.99, epsilon=1e-5,
          total_timesteps=int(80e6), lrschedule='linear')
    .train(obs, states, rewards, masks, actions, values) -> (policy_loss, value_loss, policy_entropy)
    .step  .value  .initial_state  .save(path)  .load(path)
    learn(network, env, seed=None, nsteps=5, total_timesteps=int(80e6), vf_coef=0.5, ent_coef=0.01, max_grad_norm=0.5,
          lr=7e-4, lrschedule='linear', epsilon=1e-5, alpha=0.99, gamma=0.99, log_interval=100, load_path=None,
          **network_kwargs) -> model

The act side, the parameter buffers and their initialisation are PPO2's Model (same policies, same ortho_init draws);
the learner is one C call, mrl_model_train_step_a2c: gradient of the A2C loss over the whole nenv*nsteps batch ->
clip_by_global_norm -> TF-1 RMSProp.  On the device fast path (`train_rollout`) the returns kernel and that step are
captured once per rollout shape as a hipGraph and replayed every update; the learning rate lives in a device scalar.
"""
import os
import time
from collections import deque

import numpy as np
import torch

from .. import _lib, logger
from ..common import explained_variance, set_global_seeds
from ..common.math_util import safemean
from ..common.policies import build_policy
from ..ppo2.model import Model as _PPO2Model
from .runner import Runner
from .utils import Scheduler

_SCOPE = 'a2c_model/'


def checkpoint_to_flat(loaded, tensors):
    """Host-only half of `Model.load`: maps what `joblib.load` returned from a checkpoint written by the reference's
    `save_variables` (tf_util.py:345-355) onto the flat parameter / RMSProp-slot buffers.

    tensors: [(tf_variable_name, shape, offset, size)] in variable-creation order, names under `a2c_model/`.
    loaded:  * dict {var.name: ndarray} -- `a2c_model/.../w:0`, `.../w/RMSProp:0` (ms), `.../w/RMSProp_1:0` (momentum);
               parameters are required, optimizer slots optional (tf_util.py:367-369 assigns by name);
             * list (legacy format, tf_util.py:362-366) -- the n model variables, then (ms, momentum) for each variable in
               turn (RMSProp has no beta powers): 3n arrays; a list of only the n model variables is accepted too; any
               other length fails with the reference's message.
    Returns {'params' | 'ms' | 'mom': [(offset, flat float32 array)]}."""
    out = {'params': [], 'ms': [], 'mom': []}

    def put(key, t, arr):
        name, shape, off, size = t
        a = np.asarray(arr, np.float32)
        flat_ok = a.ndim == 1 and len([d for d in shape if d != 1]) <= 1
        if a.size != size or (tuple(a.shape) != tuple(shape) and not flat_ok and a.ndim != 0):
            raise ValueError('checkpoint variable %s has shape %s, the model expects %s' % (name, a.shape, tuple(shape)))
        out[key].append((off, a.reshape(-1)))

    n = len(tensors)
    if isinstance(loaded, list):
        if len(loaded) not in (n, 3 * n):
            raise ValueError('number of variables loaded mismatches len(variables)')           # tf_util.py:363's message
        for t, a in zip(tensors, loaded[:n]):
            put('params', t, a)
        if len(loaded) > n:
            for i, t in enumerate(tensors):
                put('ms', t, loaded[n + 2 * i])
                put('mom', t, loaded[n + 1 + 2 * i])
        return out
    for t in tensors:
        put('params', t, loaded[t[0] + ':0'])          # KeyError for a missing model variable, like tf_util.py:369
        if t[0] + '/RMSProp:0' in loaded:
            put('ms', t, loaded[t[0] + '/RMSProp:0'])
        if t[0] + '/RMSProp_1:0' in loaded:
            put('mom', t, loaded[t[0] + '/RMSProp_1:0'])
    return out


def a2c_name(ppo2_name):
    """the model's TF variable name under the A2C scope (a2c.py:42 tf.variable_scope('a2c_model'))"""
    return _SCOPE + ppo2_name.split('/', 1)[1]


class Model(_PPO2Model):
    loss_names = ['policy_loss', 'value_loss', 'policy_entropy']
    stock_act_side = True          # PPO2's act side unchanged: the runner may capture its rollout as a graph

    def __init__(self, policy, env=None, nsteps=5, ent_coef=0.01, vf_coef=0.5, max_grad_norm=0.5, lr=7e-4, alpha=0.99,
                 epsilon=1e-5, total_timesteps=int(80e6), lrschedule='linear', *, ob_space=None, ac_space=None,
                 nenvs=None, chunk=None, device=None):
        ob_space = ob_space if ob_space is not None else env.observation_space
        ac_space = ac_space if ac_space is not None else env.action_space
        nenvs = int(nenvs if nenvs is not None else env.num_envs)
        super().__init__(policy=policy, ob_space=ob_space, ac_space=ac_space, nbatch_act=nenvs,
                         nbatch_train=nenvs * nsteps, nsteps=nsteps, ent_coef=ent_coef, vf_coef=vf_coef,
                         max_grad_norm=max_grad_norm, chunk=chunk, device=device)
        if self.multi:
            raise NotImplementedError('A2C has no multi-rank path (the reference\'s a2c.py has none either)')
        self.nenvs = nenvs
        # tf.train.RMSPropOptimizer(learning_rate=LR, decay=alpha, epsilon=epsilon) (a2c.py:83): the `rms` slot starts at
        # ONES, `momentum` at zeros.  They live in the buffers PPO2's Model allocates for its Adam slots.
        self.rms_ms = self.adam_m.fill_(1.0)
        self.rms_mom = self.adam_v.zero_()
        self.alpha, self.epsilon, self.momentum = np.float32(alpha), np.float32(epsilon), np.float32(0.0)
        self.lr = Scheduler(v=lr, nvalues=total_timesteps, schedule=lrschedule)
        self._lr_dev = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._a2c_stats = torch.zeros(3, dtype=torch.float32, device=self.device)
        self._a2c_graph = None
        self._a2c_calls = 0
        self.last_lr = None

    # ------------------------------------------------------------------ learner
    def _check(self, rc, what):
        if rc == -3 and getattr(self, '_comm_attached', False):
            raise NotImplementedError('%s: A2C does not run with a communicator attached (no multi-rank A2C)' % what)
        _lib.check(rc, what)

    def attach_comm(self, native_comm, rank_weight=1.0):
        """Attach an RCCL communicator to the device model.  Allowed by the layout object, refused by every A2C step."""
        self.dm.attach_comm(native_comm, rank_weight)
        self._comm_attached = bool(native_comm)

    def _train_step(self, obs, actions, returns, values, masks, states, nseq, idx, B, T, N, lr, lr_dev, stats):
        mgn = -1.0 if self.max_grad_norm is None else float(self.max_grad_norm)
        lib = _lib.load()
        self._check(lib.mrl_model_train_step_a2c(
            self.dm.handle, _lib.ptr(self.params), _lib.ptr(self.grads), _lib.ptr(self.rms_ms), _lib.ptr(self.rms_mom),
            _lib.ptr(obs), _lib.ptr(actions), _lib.ptr(returns), _lib.ptr(values), _lib.ptr(masks), _lib.ptr(states),
            int(nseq), _lib.ptr(idx), int(B), int(T), int(N), self.ent_coef, self.vf_coef, float(lr), _lib.ptr(lr_dev),
            float(self.alpha), float(self.momentum), float(self.epsilon), mgn, _lib.ptr(stats), _lib.ptr(self._gnorm),
            _lib.ptr(self.dm.workspace), self.dm.workspace.numel(), self.dm.chunk, _lib.stream_ptr()),
            'mrl_model_train_step_a2c')

    def _next_lr(self, nbatch):
        """a2c.py:94-95: Scheduler.value() once per sample, the last value fed as the f32 LR placeholder"""
        self.last_lr = np.float32(self.lr.advance(nbatch))
        return self.last_lr

    def train(self, obs, states, rewards, masks, actions, values):
        """Reference signature (a2c.py:88-109): env-major arrays of the whole batch (host NumPy or device tensors).
        Returns (policy_loss, value_loss, policy_entropy) as Python floats."""
        obs = self._to_dev_obs(obs)
        B = obs.shape[0]
        lr = self._next_lr(B)
        act = self._field(actions, self.dm.action_dtype)
        ret, val = (self._field(x, torch.float32) for x in (rewards, values))
        stats = torch.empty(3, dtype=torch.float32, device=self.device)
        m8 = st = None
        nseq = 0
        if self.recurrent:              # a2c.py:98-100: td_map[S] = states, td_map[M] = masks
            assert states is not None, 'recurrent policy: train(obs, states, ...)'
            nseq = np.asarray(states).shape[0] if not isinstance(states, torch.Tensor) else states.shape[0]
            m8, st = self._dev_mask(masks, B), self._dev_state(states, nseq)
        self._train_step(obs, act, ret, val, m8, st, nseq, None, B, 1, 1, lr, None, stats)
        self._a2c_calls += 1
        return tuple(float(x) for x in stats.cpu().numpy())

    def _env_major_idx(self, T, N):
        key = ('a2c_idx', T, N)
        t = self._rings.get(key)
        if t is None:
            t = self._rings[key] = torch.arange(N * T, dtype=torch.int64, device=self.device)
        return t

    def train_rollout(self, runner, lr=None):
        """Device fast path of one update: the n-step returns of the runner's resident rollout (written to ro.returns) and the
        train step on all of it, without a host round trip.  Returns a device tensor [3] (pg_loss, vf_loss, entropy).
        Feedforward policies run both as ONE captured hipGraph (captured on the second call, again when a buffer moves),
        reading the learning rate from a device scalar.  lr: the f32 step size (None: the schedule's next value)."""
        ro = runner.rollout
        T, N = ro.T, ro.N
        lr = self._next_lr(T * N) if lr is None else np.float32(lr)
        self._lr_dev.fill_(float(lr))
        if self.recurrent:
            # whole trajectories of all N envs (a2c.py:98-100): env-major indices, masks = dones entering, states before
            ops_returns(ro, runner)
            idx = self._env_major_idx(T, N)
            st = runner._mb_states
            st = st if isinstance(st, torch.Tensor) else self._dev_state(st, N)
            self._train_step(ro.obs, ro.actions, ro.returns, ro.values, ro.dones, st.contiguous(), N, idx, T * N, T, N,
                             lr, None, self._a2c_stats)
            self._a2c_calls += 1
            return self._a2c_stats.clone()
        graphable = (self._a2c_calls > 0 and not _lib.prof_enabled() and self._a2c_graph is not False
                     and os.environ.get('MRL_A2C_GRAPH', '1') != '0')
        if not graphable:
            self._a2c_eager(ro, runner, lr)
            self._a2c_calls += 1
            return self._a2c_stats.clone()
        g = self._a2c_graph
        lv = runner.last_values
        key = (T, N, float(runner.gamma), ro.obs.data_ptr(), ro.actions.data_ptr(), ro.rewards.data_ptr(),
               ro.returns.data_ptr(), ro.values.data_ptr(), ro.dones.data_ptr(), runner._dones_dev.data_ptr(),
               self.dm.workspace.data_ptr(), self.dm.chunk)
        if g is None or g['key'] != key:
            try:
                g = self._a2c_graph = self._capture_a2c(key, ro, runner)
            except Exception as exc:                     # capture unsupported here: eager steps from now on
                import warnings
                warnings.warn('A2C step graph capture failed (%s); using eager steps' % (exc,))
                self._a2c_graph = False
                torch.cuda.synchronize()
                return self.train_rollout(runner, lr)
        g['lastv'].copy_(lv)
        g['graph'].replay()
        self._a2c_calls += 1
        return self._a2c_stats.clone()

    def _a2c_eager(self, ro, runner, lr, lastv=None, lr_dev=None):
        ops_returns(ro, runner, lastv)
        self._train_step(ro.obs, ro.actions, ro.returns, ro.values, None, None, 0, None, ro.T * ro.N, ro.T, ro.N,
                         lr, lr_dev, self._a2c_stats)

    def _capture_a2c(self, key, ro, runner):
        lastv = torch.zeros(ro.N, dtype=torch.float32, device=self.device)
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with _lib.capture_graph(graph):
            self._a2c_eager(ro, runner, 0.0, lastv=lastv, lr_dev=self._lr_dev)
        return dict(key=key, graph=graph, lastv=lastv)

    # ------------------------------------------------------------------ checkpoints
    def _a2c_named(self, flat):
        host = flat.detach().cpu().numpy()
        return {a2c_name(t['name']): host[t['offset']:t['offset'] + t['size']].reshape(t['shape']).copy()
                for t in self.dm.tensors}

    def save(self, save_path):
        """joblib dict {tf_variable_name: ndarray} over all global variables -- parameters and RMSProp slots
        (tf_util.py:345-355)."""
        import joblib
        d = {}
        for k, v in self._a2c_named(self.params).items():
            d[k + ':0'] = v
        for k, v in self._a2c_named(self.rms_ms).items():
            d[k + '/RMSProp:0'] = v
        for k, v in self._a2c_named(self.rms_mom).items():
            d[k + '/RMSProp_1:0'] = v
        dirname = os.path.dirname(save_path)
        if dirname:
            os.makedirs(dirname, exist_ok=True)
        joblib.dump(d, save_path)

    def load(self, load_path):
        """tf_util.py:357-372 -- dict by name, legacy list by position (see `checkpoint_to_flat`)."""
        import joblib
        loaded = joblib.load(os.path.expanduser(load_path))
        tensors = [(a2c_name(t['name']), tuple(t['shape']), t['offset'], t['size']) for t in self.dm.tensors]
        out = checkpoint_to_flat(loaded, tensors)
        for dst, key in ((self.params, 'params'), (self.rms_ms, 'ms'), (self.rms_mom, 'mom')):
            host = dst.detach().cpu().numpy()
            for off, arr in out[key]:
                host[off:off + arr.size] = arr
            dst.copy_(torch.from_numpy(host))


def ops_returns(ro, runner, lastv=None):
    """the runner's n-step returns into ro.returns (mrl_nstep_returns)"""
    from .. import ops
    lv = runner.last_values if lastv is None else lastv
    ops.nstep_returns(ro.rewards, ro.dones, lv, runner._dones_dev, runner.gamma, out=ro.returns)


def learn(network, env, seed=None, nsteps=5, total_timesteps=int(80e6), vf_coef=0.5, ent_coef=0.01, max_grad_norm=0.5,
          lr=7e-4, lrschedule='linear', epsilon=1e-5, alpha=0.99, gamma=0.99, log_interval=100, load_path=None,
          **network_kwargs):
    """a2c.py:119-232 on the device path: rollout (graph-replayed on the device env) -> returns + train step (one
    replayed graph).  Loss statistics are read back only on the updates that log."""
    set_global_seeds(seed)
    nenvs = env.num_envs
    policy = build_policy(env, network, **network_kwargs)
    model = Model(policy=policy, env=env, nsteps=nsteps, ent_coef=ent_coef, vf_coef=vf_coef, max_grad_norm=max_grad_norm,
                  lr=lr, alpha=alpha, epsilon=epsilon, total_timesteps=total_timesteps, lrschedule=lrschedule)
    if load_path is not None:
        model.load(load_path)
    runner = Runner(env, model, nsteps=nsteps, gamma=gamma, return_host=False)
    runner.returns_by_model = True
    epinfobuf = deque(maxlen=100)
    nbatch = nenvs * nsteps
    tstart = time.time()
    for update in range(1, int(total_timesteps) // nbatch + 1):
        obs, states, rewards, masks, actions, values, epinfos = runner.run()
        epinfobuf.extend(epinfos)
        stats = model.train_rollout(runner)
        nseconds = time.time() - tstart
        fps = int((update * nbatch) / nseconds)
        if update % log_interval == 0 or update == 1:
            policy_loss, value_loss, policy_entropy = stats.cpu().numpy().tolist()
            ev = explained_variance(values.to_numpy(), rewards.to_numpy())
            logger.logkv('nupdates', update)
            logger.logkv('total_timesteps', update * nbatch)
            logger.logkv('fps', fps)
            logger.logkv('policy_entropy', float(policy_entropy))
            logger.logkv('value_loss', float(value_loss))
            logger.logkv('explained_variance', float(ev))
            logger.logkv('eprewmean', safemean([epinfo['r'] for epinfo in epinfobuf]))
            logger.logkv('eplenmean', safemean([epinfo['l'] for epinfo in epinfobuf]))
            logger.dumpkvs()
    return model
