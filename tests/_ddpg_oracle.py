"""Restatement of ddpg/ddpg_learner.py's graph in torch (CPU) at a chosen dtype, for the DDPG tests.

float64: the reference's arithmetic without rounding noise; float32: the same graph in the reference's own precision, whose
distance to float64 sets the bars the HIP kernels are held to.  References are to the reference's baselines/ tree."""
import numpy as np
import torch


def mlp_fwd(p, model, x, act, out_act):
    """common/models.py:75-103 body + the final dense layer (ddpg/models.py:27-51); p: {name: tensor}"""
    pre = model.name
    h = x
    for i in range(model.num_layers):
        h = h @ p['%s/mlp_fc%d/w' % (pre, i)] + p['%s/mlp_fc%d/b' % (pre, i)]
        if model.layer_norm:
            ln = 'LayerNorm' if i == 0 else 'LayerNorm_%d' % i
            mu = h.mean(-1, keepdim=True)
            var = ((h - mu) ** 2).mean(-1, keepdim=True)
            h = (h - mu) * torch.rsqrt(var + 1e-12) * p['%s/%s/gamma' % (pre, ln)] + p['%s/%s/beta' % (pre, ln)]
        h = torch.tanh(h) if act == 'tanh' else torch.relu(h)
    final = 'dense' if 'actor' in pre else 'output'
    y = h @ p['%s/%s/kernel' % (pre, final)] + p['%s/%s/bias' % (pre, final)]
    return torch.tanh(y) if out_act else y


def rms_mean_std(buf, n, dtype):
    """common/mpi_running_mean_std.py:29-30 (f64 sums -> f32 mean, std)"""
    b = np.asarray(buf, np.float64)
    mean = (b[:n] / b[2 * n]).astype(np.float32)
    std = np.sqrt(np.maximum((b[n:2 * n] / b[2 * n]).astype(np.float32) - np.square(mean), np.float32(1e-2)))
    if dtype == torch.float64:          # the exact form of the same quantities
        mean = b[:n] / b[2 * n]
        std = np.sqrt(np.maximum(b[n:2 * n] / b[2 * n] - np.square(mean), 1e-2))
    return torch.tensor(mean, dtype=dtype), torch.tensor(std, dtype=dtype)


class Oracle(object):
    """state: flat actor / critic / target parameters, MpiAdam m, v, t per net, obs_rms / ret_rms f64 buffers"""

    def __init__(self, actor, critic, *, activation, normalize_observations, normalize_returns, popart, gamma, tau,
                 critic_l2_reg, clip_norm, actor_lr, critic_lr, dtype, flat):
        self.actor, self.critic, self.act = actor, critic, activation
        self.norm_obs, self.norm_ret, self.popart = normalize_observations, normalize_returns, popart
        self.gamma, self.tau, self.l2, self.clip = gamma, tau, critic_l2_reg, clip_norm
        self.lr = {'actor': actor_lr, 'critic': critic_lr}
        self.dtype = dtype
        t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
        self.flat = {k: t(flat[k]) for k in ('actor', 'critic', 'target_actor', 'target_critic', 'actor_m', 'actor_v',
                                               'critic_m', 'critic_v')}
        self.obs_rms = np.array(flat['obs_rms'], np.float64)
        self.ret_rms = np.array(flat['ret_rms'], np.float64)
        self.t = {'actor': int(flat['actor_t']), 'critic': int(flat['critic_t'])}

    def params(self, key, model, requires_grad=False):
        f = self.flat[key]
        out = {}
        for name, shape, off, _ in model.tensors:
            v = f[off:off + int(np.prod(shape))].reshape(shape).clone()
            out[name] = v.requires_grad_(requires_grad)
        return out

    def norm_obs_(self, x):
        """ddpg_learner.py:104-107"""
        x = torch.tensor(np.asarray(x), dtype=self.dtype)
        if self.norm_obs:
            m, s = rms_mean_std(self.obs_rms, self.actor.ob_dim, self.dtype)
            x = (x - m) / (s + 1e-8)
        return torch.clamp(x, -5., 5.)

    def ret_stats(self):
        if not self.norm_ret:
            return torch.tensor(0., dtype=self.dtype), torch.tensor(1., dtype=self.dtype)
        m, s = rms_mean_std(self.ret_rms, 1, self.dtype)
        return m[0], s[0]

    def train(self, obs0, actions, rewards, obs1, terminals1):
        """ddpg_learner.py:268-309 + MpiAdam; returns dict(critic_loss, actor_loss, grads={'actor', 'critic'} flat)"""
        dt = self.dtype
        o0, o1 = self.norm_obs_(obs0), self.norm_obs_(obs1)
        acts = torch.tensor(np.asarray(actions), dtype=dt)
        r = torch.tensor(np.asarray(rewards), dtype=dt).reshape(-1, 1)
        d = torch.tensor(np.asarray(terminals1), dtype=dt).reshape(-1, 1)
        ta, tc = self.params('target_actor', self.actor), self.params('target_critic', self.critic)
        m0, s0 = self.ret_stats()
        with torch.no_grad():
            a1 = mlp_fwd(ta, self.actor, o1, self.act, True)
            q1 = mlp_fwd(tc, self.critic, torch.cat([o1, a1], -1), self.act, False)
            target_q = r + (1. - d) * self.gamma * (q1 * s0 + m0 if self.norm_ret else q1)      # :134-135
        if self.norm_ret and self.popart:                                                          # :217-236, :279-292
            x = target_q.double().numpy().reshape(-1)
            self.ret_rms += np.array([x.sum(), np.square(x).sum(), len(x)])
            m1, s1 = self.ret_stats()
            H = self.critic.num_hidden
            for key in ('critic', 'target_critic'):
                f = self.flat[key]
                wo = [t for t in self.critic.tensors if t[0].endswith('output/kernel')][0][2]
                f[wo:wo + H] = f[wo:wo + H] * s0 / s1
                f[wo + H] = (f[wo + H] * s0 + m0 - m1) / s1
            m0, s0 = m1, s1
        pa = self.params('actor', self.actor, True)
        pc = self.params('critic', self.critic, True)
        # critic loss (:198-213)
        qn = mlp_fwd(pc, self.critic, torch.cat([o0, acts], -1), self.act, False)
        tn = (target_q - m0) / (s0 + 1e-8) if self.norm_ret else target_q
        critic_loss = torch.mean((qn - tn) ** 2)
        if self.l2 > 0:
            for i in range(self.critic.num_layers):
                critic_loss = critic_loss + self.l2 * torch.sum(pc['critic/mlp_fc%d/w' % i] ** 2) / 2
        # actor loss (:186): the critic's current (pre-update) parameters, gradient only into the actor
        pc_const = {k: v.detach() for k, v in pc.items()}
        a0 = mlp_fwd(pa, self.actor, o0, self.act, True)
        qa = mlp_fwd(pc_const, self.critic, torch.cat([o0, a0], -1), self.act, False)
        actor_loss = -torch.mean(qa * s0 + m0 if self.norm_ret else qa)
        grads = {}
        for key, model, p, loss in (('actor', self.actor, pa, actor_loss), ('critic', self.critic, pc, critic_loss)):
            names = [t[0] for t in model.tensors]
            gs = torch.autograd.grad(loss, [p[n] for n in names])
            flat = []
            for g in gs:
                g = g.detach().reshape(-1)
                if self.clip is not None:                                  # tf.clip_by_norm per variable (flatgrad)
                    g = g * self.clip / torch.clamp(torch.sqrt(torch.sum(g * g)), min=self.clip)
                flat.append(g)
            grads[key] = torch.cat(flat)
        for key in ('actor', 'critic'):                                    # MpiAdam.update (mpi_adam.py:38-41)
            self.t[key] += 1
            t = self.t[key]
            a = self.lr[key] * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
            g = grads[key]
            m = 0.9 * self.flat[key + '_m'] + (1 - 0.9) * g
            v = 0.999 * self.flat[key + '_v'] + (1 - 0.999) * (g * g)
            self.flat[key + '_m'], self.flat[key + '_v'] = m, v
            self.flat[key] = self.flat[key] + (-a) * m / (torch.sqrt(v) + 1e-8)
        return dict(critic_loss=float(critic_loss.detach()), actor_loss=float(actor_loss.detach()), grads=grads)

    def soft_update(self):
        """get_target_updates (:36-47)"""
        for k in ('actor', 'critic'):
            self.flat['target_' + k] = (1. - self.tau) * self.flat['target_' + k] + self.tau * self.flat[k]

    def actions(self, flat_actor, obs):
        p = self.params_from(flat_actor, self.actor)
        return mlp_fwd(p, self.actor, self.norm_obs_(obs), self.act, True)

    def q(self, obs, actions):
        o = self.norm_obs_(obs)
        a = torch.tensor(np.asarray(actions), dtype=self.dtype)
        q = mlp_fwd(self.params('critic', self.critic), self.critic, torch.cat([o, a], -1), self.act, False)
        m, s = self.ret_stats()
        return q * s + m if self.norm_ret else q

    def params_from(self, flat, model):
        f = torch.tensor(np.asarray(flat), dtype=self.dtype)
        return {name: f[off:off + int(np.prod(shape))].reshape(shape) for name, shape, off, _ in model.tensors}


def oracle_learn(env, *, seed, nb_epochs, nb_epoch_cycles, nb_rollout_steps, nb_train_steps, batch_size, noise_type,
                 param_noise_adaption_interval, num_hidden, gamma=0.99, tau=0.01, critic_l2_reg=1e-2, actor_lr=1e-4,
                 critic_lr=1e-3, reward_scale=1.0):
    """ddpg/ddpg.py:47-200 restated on the float64 Oracle with a host ring (memory.py) and host obs_rms, drawing from
    np.random in the reference's order.  Initial parameters come from the package's models (the documented NumPy-stream
    init); the parameter-space noise from a torch device generator seeded like the agent's (it stands in for TF's
    random_normal in both).  Returns index streams, the ring, last-cycle losses per epoch and the final state."""
    from baselines_amd.common import set_global_seeds
    from baselines_amd.ddpg.models import Actor, Critic
    from baselines_amd.ddpg.noise import parse_noise_type
    set_global_seeds(seed)
    A, D = env.action_space.shape[-1], env.observation_space.shape[0]
    actor = Actor(A, network='mlp', num_hidden=num_hidden).build(D)
    critic = Critic(network='mlp', num_hidden=num_hidden).build(D, A)
    action_noise, param_noise = parse_noise_type(noise_type, A)
    gen = torch.Generator(device='cuda')
    gen.manual_seed(torch.initial_seed())
    pa = actor.init_params()
    pc = critic.init_params()
    rms = np.zeros(2 * D + 1)
    rms[D:] = 1e-2
    flat = dict(actor=pa, critic=pc, target_actor=pa.copy(), target_critic=pc.copy(), actor_m=np.zeros_like(pa),
                actor_v=np.zeros_like(pa), critic_m=np.zeros_like(pc), critic_v=np.zeros_like(pc), obs_rms=rms,
                ret_rms=np.array([0., 1e-2, 1e-2]), actor_t=0, critic_t=0)
    o = Oracle(actor, critic, activation='tanh', normalize_observations=True, normalize_returns=False, popart=False,
               gamma=gamma, tau=tau, critic_l2_reg=critic_l2_reg, clip_norm=None, actor_lr=actor_lr, critic_lr=critic_lr,
               dtype=torch.float64, flat=flat)
    ring = dict(obs0=[], act=[], rew=[], obs1=[], term=[])
    draws, losses = [], []
    perturbed = None

    def perturb(stddev):
        n = torch.randn(actor.num_params, generator=gen, device='cuda').cpu().numpy()
        out = o.flat['actor'].numpy().astype(np.float32).copy()
        for name, shape, off, _ in actor.tensors:
            if 'LayerNorm' not in name:
                sl = slice(off, off + int(np.prod(shape)))
                out[sl] = out[sl] + (n[sl] * np.float32(stddev))
        return out

    def reset():
        nonlocal perturbed
        if action_noise is not None:
            action_noise.reset()
        if param_noise is not None:
            perturbed = perturb(param_noise.current_stddev)

    def draw():
        idx = np.random.randint(len(ring['obs0']) - 2, size=batch_size)
        draws.append(idx)
        return idx

    max_action = env.action_space.high
    reset()
    obs = env.reset()
    nenvs = obs.shape[0]
    stats_drawn = False
    for epoch in range(nb_epochs):
        for cycle in range(nb_epoch_cycles):
            if nenvs > 1:
                reset()
            for _ in range(nb_rollout_steps):
                src = perturbed if param_noise is not None else o.flat['actor'].numpy()
                action = o.actions(src, np.asarray(obs, np.float32)).numpy().astype(np.float32)
                if action_noise is not None:
                    action = (action + action_noise()).astype(np.float32)
                action = np.clip(action, -1., 1.)
                new_obs, r, done, _ = env.step(max_action * action)
                r = np.asarray(r, np.float32) * np.float32(reward_scale)
                for b in range(nenvs):
                    for k, v in (('obs0', obs[b]), ('act', action[b]), ('rew', r[b]), ('obs1', new_obs[b]), ('term', done[b])):
                        ring[k].append(np.asarray(v, np.float32))
                    x = np.asarray(obs[b:b + 1], np.float64)
                    o.obs_rms += np.concatenate([x.sum(axis=0), np.square(x).sum(axis=0), [1.0]])
                obs = new_obs
                if nenvs == 1 and done[0]:
                    reset()
            cyc = []
            for t_train in range(nb_train_steps):
                if len(ring['obs0']) >= batch_size and t_train % param_noise_adaption_interval == 0 and param_noise is not None:
                    idx = draw()
                    adaptive = perturb(param_noise.current_stddev)
                    obs0 = np.stack(ring['obs0'])[idx]
                    d = torch.sqrt(torch.mean((o.actions(o.flat['actor'].numpy(), obs0) - o.actions(adaptive, obs0)) ** 2))
                    param_noise.adapt(float(d))
                idx = draw()
                g = lambda k: np.stack(ring[k])[idx]
                r = o.train(g('obs0'), g('act'), g('rew'), g('obs1'), g('term'))
                o.soft_update()
                cyc.append((r['critic_loss'], r['actor_loss']))
        losses.append(np.mean(np.array(cyc), axis=0))
        if not stats_drawn:                       # get_stats fixes its sample at the first call (ddpg_learner.py:320-323)
            draw()
            stats_drawn = True
    return dict(draws=draws, ring={k: np.stack(v) for k, v in ring.items()}, losses=np.array(losses), oracle=o,
                param_noise=param_noise)
