"""DDPG agent with the reference's protocol (ddpg/ddpg_learner.py:65-396):

    DDPG(actor, critic, memory, observation_shape, action_shape, param_noise=None, action_noise=None, gamma=0.99,
         tau=0.001, normalize_returns=False, enable_popart=False, normalize_observations=True, batch_size=128,
         observation_range=(-5., 5.), action_range=(-1., 1.), return_range=(-inf, inf), critic_l2_reg=0.,
         actor_lr=1e-4, critic_lr=1e-3, clip_norm=None, reward_scale=1.)
    .initialize(sess=None)  .step(obs, apply_noise=True, compute_Q=True) -> (action, q, None, None)
    .store_transition(obs0, action, reward, obs1, terminal1)  .train() -> (critic_loss, actor_loss)
    .update_target_net()  .adapt_param_noise() -> distance  .get_stats() -> dict  .reset()

Where the reference builds a TF graph, this object owns flat f32 device buffers (actor, critic, their targets, the two
param-noise copies, the MpiAdam slots, obs_rms / ret_rms in f64) and drives the HIP kernels of csrc/ddpg.hip:
mrl_ddpg_train_step (the whole train() in one launch, update_target_net fused on the learn path), mrl_ddpg_act,
mrl_ddpg_store, mrl_ddpg_perturb, mrl_ddpg_policy_distance.  Observations and actions may be host NumPy arrays (host
VecEnvs; results come back as NumPy) or device tensors (the device env; results stay on the device).
TF's random_normal for the parameter perturbations is replaced by a torch device generator seeded from torch's seed."""
import ctypes

import numpy as np
import torch

from .. import _lib, ops


class RunningMeanStdDev(object):
    """common/mpi_running_mean_std.py on the device: f64 [2*n + 1] = runningsum | runningsumsq | count, epsilon 1e-2"""

    def __init__(self, n, device, epsilon=1e-2):
        self.n = n
        self.buf = torch.zeros(2 * n + 1, dtype=torch.float64, device=device)
        self.buf[n:] = epsilon

    def mean_std(self):
        """(mean, std) as the reference's graph computes them: f64 sums, f32 cast, std = sqrt(max(sumsq/count - mean^2, 1e-2))"""
        b = self.buf.cpu().numpy()
        n = self.n
        mean = (b[:n] / b[2 * n]).astype(np.float32)
        std = np.sqrt(np.maximum((b[n:2 * n] / b[2 * n]).astype(np.float32) - np.square(mean), np.float32(1e-2)))
        return mean, std


class DDPG(object):
    def __init__(self, actor, critic, memory, observation_shape, action_shape, param_noise=None, action_noise=None,
                 gamma=0.99, tau=0.001, normalize_returns=False, enable_popart=False, normalize_observations=True,
                 batch_size=128, observation_range=(-5., 5.), action_range=(-1., 1.), return_range=(-np.inf, np.inf),
                 critic_l2_reg=0., actor_lr=1e-4, critic_lr=1e-3, clip_norm=None, reward_scale=1.):
        if tuple(observation_range) != (-5., 5.) or tuple(action_range) != (-1., 1.) or \
                tuple(return_range) != (-np.inf, np.inf):
            raise NotImplementedError('DDPG on the device path keeps the reference\'s observation_range (-5, 5), '
                                      'action_range (-1, 1) and return_range (-inf, inf)')
        if len(observation_shape) != 1 or len(action_shape) != 1:
            raise NotImplementedError('DDPG on the device path takes 1-D Box observations and actions')
        self.gamma = gamma
        self.tau = tau
        self.memory = memory
        self.normalize_observations = normalize_observations
        self.normalize_returns = normalize_returns
        self.action_noise = action_noise
        self.param_noise = param_noise
        self.action_range = action_range
        self.return_range = return_range
        self.observation_range = observation_range
        self.actor = actor.build(observation_shape[0])
        self.critic = critic.build(observation_shape[0], action_shape[0])
        self.actor_lr = actor_lr
        self.critic_lr = critic_lr
        self.clip_norm = clip_norm
        self.enable_popart = enable_popart
        self.reward_scale = reward_scale
        self.batch_size = batch_size
        self.stats_sample = None
        self.critic_l2_reg = critic_l2_reg
        self.initial_state = None
        self.ob_dim, self.nb_actions = int(observation_shape[0]), int(action_shape[0])
        if (actor.num_layers, actor.num_hidden, actor.activation, actor.layer_norm) != \
                (critic.num_layers, critic.num_hidden, critic.activation, critic.layer_norm):
            raise NotImplementedError('actor and critic must share one mlp configuration on the device path')
        if not 1 <= batch_size <= 1024:
            raise NotImplementedError('batch_size must be in 1..1024 on the device path')
        self.k = ops.DDPGKernels(ob_dim=self.ob_dim, nact=self.nb_actions, num_layers=actor.num_layers,
                                 num_hidden=actor.num_hidden, activation=actor.activation, layer_norm=actor.layer_norm,
                                 normalize_observations=normalize_observations, normalize_returns=normalize_returns,
                                 popart=enable_popart, max_batch=batch_size, device=memory.ring_pos.device)
        assert self.k.Pa == actor.num_params and self.k.Pc == critic.num_params
        dev = self.device = memory.ring_pos.device
        f32 = dict(dtype=torch.float32, device=dev)
        self.Pa, self.Pc = self.k.Pa, self.k.Pc
        self.actor_params = torch.zeros(self.Pa, **f32)
        self.critic_params = torch.zeros(self.Pc, **f32)
        self.target_actor_params = torch.zeros(self.Pa, **f32)
        self.target_critic_params = torch.zeros(self.Pc, **f32)
        self.perturbed_actor_params = torch.zeros(self.Pa, **f32)           # param_noise_actor
        self.adaptive_actor_params = torch.zeros(self.Pa, **f32)            # adaptive_param_noise_actor
        self.actor_m, self.actor_v = torch.zeros(self.Pa, **f32), torch.zeros(self.Pa, **f32)
        self.critic_m, self.critic_v = torch.zeros(self.Pc, **f32), torch.zeros(self.Pc, **f32)
        self.actor_t = self.critic_t = 0
        self.obs_rms = RunningMeanStdDev(self.ob_dim, dev)
        self.ret_rms = RunningMeanStdDev(1, dev)
        self.neg_alpha = torch.zeros(2, **f32)
        self.losses = torch.zeros(2, **f32)
        self.distance = torch.zeros(1, **f32)
        self.noise_buf = torch.zeros(self.Pa, **f32)
        self.gen = torch.Generator(device=dev)
        self.gen.manual_seed(torch.initial_seed())
        self.state = _lib.DDPGState()
        for name, t in (('actor', self.actor_params), ('critic', self.critic_params),
                        ('target_actor', self.target_actor_params), ('target_critic', self.target_critic_params),
                        ('actor_m', self.actor_m), ('actor_v', self.actor_v), ('critic_m', self.critic_m),
                        ('critic_v', self.critic_v), ('obs_rms', self.obs_rms.buf), ('ret_rms', self.ret_rms.buf)):
            setattr(self.state, name, t.data_ptr())
        memory.state_fields(self.state)

    # ---- variables ---------------------------------------------------------------------------------------------------
    def variables(self):
        """[(TF variable name, device tensor view)] in the reference's creation order (ddpg_learner.py:100-150)"""
        out = [('obs_rms/runningsum', self.obs_rms.buf[:self.ob_dim]),
               ('obs_rms/runningsumsq', self.obs_rms.buf[self.ob_dim:2 * self.ob_dim]),
               ('obs_rms/count', self.obs_rms.buf[2 * self.ob_dim])]
        if self.normalize_returns:
            out += [('ret_rms/runningsum', self.ret_rms.buf[0]), ('ret_rms/runningsumsq', self.ret_rms.buf[1]),
                    ('ret_rms/count', self.ret_rms.buf[2])]
        nets = [('actor', self.actor, self.actor_params), ('critic', self.critic, self.critic_params),
                ('target_actor', self.actor, self.target_actor_params),
                ('target_critic', self.critic, self.target_critic_params)]
        if self.param_noise is not None:
            nets += [('param_noise_actor', self.actor, self.perturbed_actor_params),
                     ('adaptive_param_noise_actor', self.actor, self.adaptive_actor_params)]
        for scope, model, flat in nets:
            for name, shape, off, _ in model.tensors:
                out.append((scope + name[len(model.name):], flat[off:off + int(np.prod(shape))].view(shape)))
        return out

    def initialize(self, sess=None):
        """global_variables_initializer (actor, then critic, from the NumPy stream; models.py) + target_init_updates"""
        self.actor_params.copy_(torch.from_numpy(self.actor.init_params()))
        self.critic_params.copy_(torch.from_numpy(self.critic.init_params()))
        self.target_actor_params.copy_(self.actor_params)
        self.target_critic_params.copy_(self.critic_params)
        self.perturbed_actor_params.copy_(self.actor_params)
        self.adaptive_actor_params.copy_(self.actor_params)

    # ---- acting ------------------------------------------------------------------------------------------------------
    def _dev(self, x, dtype=torch.float32):
        if isinstance(x, torch.Tensor):
            return x.to(device=self.device, dtype=dtype).contiguous()
        return torch.as_tensor(np.asarray(x), dtype=dtype).to(self.device)

    def act_into(self, obs, actions_out, q_out, apply_noise=True, noise=None):
        """device-side step(): obs f32 [n, ob_dim] device; noise: device f64 [nact] or None"""
        pert = self.perturbed_actor_params if (self.param_noise is not None and apply_noise) else None
        self.k.act(self.state, obs, perturbed=pert, noise=noise, actions_out=actions_out, q_out=q_out)

    def step(self, obs, apply_noise=True, compute_Q=True):
        host = not isinstance(obs, torch.Tensor)
        o = self._dev(obs).reshape(-1, self.ob_dim)
        n = o.shape[0]
        actions = torch.empty((n, self.nb_actions), dtype=torch.float32, device=self.device)
        q = torch.empty(n, dtype=torch.float32, device=self.device) if compute_Q else None
        noise = None
        if self.action_noise is not None and apply_noise:
            nz = np.asarray(self.action_noise(), dtype=np.float64)
            assert nz.shape == (self.nb_actions,)
            noise = torch.from_numpy(nz).to(self.device)
        self.act_into(o, actions, q, apply_noise, noise)
        if q is not None:
            q = q.view(n, 1)
        if host:
            actions = actions.cpu().numpy()
            q = q.cpu().numpy() if q is not None else None
        return actions, q, None, None

    def store_transition(self, obs0, action, reward, obs1, terminal1):
        o0 = self._dev(obs0).reshape(-1, self.ob_dim)
        n = o0.shape[0]
        a = self._dev(action).reshape(n, self.nb_actions)
        r = self._dev(reward).reshape(n)
        o1 = self._dev(obs1).reshape(n, self.ob_dim)
        d = self._dev(terminal1, torch.uint8).reshape(n)
        self.k.store(self.state, o0, a, r, o1, d, self.reward_scale)
        self.memory.advance(n)

    # ---- training ----------------------------------------------------------------------------------------------------
    @staticmethod
    def _neg_alpha(lr, t):
        # MpiAdam.update, common/mpi_adam.py:37-41: a in f64, `(- a) * self.m` rounds -a to f32
        a = lr * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
        return np.float32(-a)

    def next_alphas(self):
        """advance both MpiAdam step counters by one update; -> f32 [2] (-a_actor, -a_critic)"""
        self.actor_t += 1
        self.critic_t += 1
        return np.array([self._neg_alpha(self.actor_lr, self.actor_t), self._neg_alpha(self.critic_lr, self.critic_t)],
                        np.float32)

    def train_step_dev(self, idx_dev, neg_alpha_dev, losses_out, soft_update=False, grads_out=None):
        self.k.train_step(self.state, idx_dev, neg_alpha_dev, self.gamma, self.tau, self.critic_l2_reg, self.clip_norm,
                          soft_update, losses_out, grads_out)

    def train(self):
        idx = torch.from_numpy(self.memory.draw_indices(self.batch_size).astype(np.int64)).to(self.device)
        self.neg_alpha.copy_(torch.from_numpy(self.next_alphas()))
        self.train_step_dev(idx, self.neg_alpha, self.losses)
        cl, al = self.losses.cpu().numpy()
        return cl, al

    def update_target_net(self):
        self.k.soft_update(self.state, self.tau)

    # ---- parameter noise ---------------------------------------------------------------------------------------------
    def perturb(self, out, stddev):
        torch.randn(self.Pa, generator=self.gen, out=self.noise_buf)
        self.k.perturb(self.actor_params, out, self.noise_buf, np.float32(stddev))

    def adapt_param_noise_dev(self, idx_dev):
        """perturb_adaptive_policy_ops + adaptive_policy_distance on the batch idx_dev; distance left in self.distance"""
        self.perturb(self.adaptive_actor_params, self.param_noise.current_stddev)
        self.k.policy_distance(self.state, self.adaptive_actor_params, idx_dev, self.distance)

    def adapt_param_noise(self):
        if self.param_noise is None:
            return 0.
        idx = torch.from_numpy(self.memory.draw_indices(self.batch_size).astype(np.int64)).to(self.device)
        self.adapt_param_noise_dev(idx)
        mean_distance = float(self.distance.item())
        self.param_noise.adapt(mean_distance)
        return mean_distance

    def reset(self):
        if self.action_noise is not None:
            self.action_noise.reset()
        if self.param_noise is not None:
            self.perturb(self.perturbed_actor_params, self.param_noise.current_stddev)

    # ---- statistics --------------------------------------------------------------------------------------------------
    def get_stats(self):
        """ddpg_learner.py:319-360, on a sample fixed at the first call"""
        if self.stats_sample is None:
            self.stats_sample = self.memory.sample(batch_size=self.batch_size)
        obs0 = self.stats_sample['obs0'].contiguous()
        acts = self.stats_sample['actions'].contiguous()
        n = obs0.shape[0]
        q_ref = torch.empty(n, dtype=torch.float32, device=self.device)
        q_act = torch.empty(n, dtype=torch.float32, device=self.device)
        a_ref = torch.empty((n, self.nb_actions), dtype=torch.float32, device=self.device)
        self.k.act(self.state, obs0, actions_in=acts, q_out=q_ref)
        self.k.act(self.state, obs0, actions_out=a_ref, q_out=q_act)
        names, values = [], []
        if self.normalize_returns:
            m, s = self.ret_rms.mean_std()
            names += ['ret_rms_mean', 'ret_rms_std']
            values += [m[0], s[0]]
        if self.normalize_observations:
            m, s = self.obs_rms.mean_std()
            names += ['obs_rms_mean', 'obs_rms_std']
            values += [np.mean(m), np.mean(s)]
        q_ref, q_act, a_ref = q_ref.cpu().numpy(), q_act.cpu().numpy(), a_ref.cpu().numpy()
        names += ['reference_Q_mean', 'reference_Q_std', 'reference_actor_Q_mean', 'reference_actor_Q_std',
                  'reference_action_mean', 'reference_action_std']
        values += [np.mean(q_ref), np.std(q_ref), np.mean(q_act), np.std(q_act), np.mean(a_ref), np.std(a_ref)]
        if self.param_noise:
            a_p = torch.empty((n, self.nb_actions), dtype=torch.float32, device=self.device)
            self.k.act(self.state, obs0, perturbed=self.perturbed_actor_params, actions_out=a_p)
            a_p = a_p.cpu().numpy()
            names += ['reference_perturbed_action_mean', 'reference_perturbed_action_std']
            values += [np.mean(a_p), np.std(a_p)]
        stats = dict(zip(names, values))
        if self.param_noise is not None:
            stats = {**stats, **self.param_noise.get_stats()}
        return stats
