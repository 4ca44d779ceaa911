"""Test helper (no tests here): host restatements of the A2C pieces the device path is checked against.

  * nstep_returns       a2c/runner.py:58-71 + a2c/utils.py:147-153 in float64 (the reference's Python floats), f32 store;
  * rmsprop_step        TF 1.x ApplyRMSProp after clip_by_global_norm (a2c.py:76-86), float32 NumPy;
  * A2COracle           oracle.ppo2_torch.OracleModel with the A2C loss (a2c.py:57-68) and that optimizer.
"""
import numpy as np
import torch

from oracle.ppo2_torch import OracleModel


def nstep_returns(rewards, dones, last_values, last_dones, gamma):
    """rewards f32 [T][N], dones [T][N] entering each step, last_values f32 [N], last_dones [N] -> f32 [T][N]"""
    rewards = np.asarray(rewards, np.float32)
    T, N = rewards.shape
    if not gamma > 0.0:
        return rewards.copy()
    dones = np.asarray(dones).astype(bool)
    done_after = np.concatenate([dones[1:], np.asarray(last_dones, bool)[None]], 0)
    out = np.empty((T, N), np.float32)
    g = np.float64(gamma)
    r = np.zeros(N, np.float64)
    boot = ~np.asarray(last_dones, bool)
    rb = np.asarray(last_values, np.float32).astype(np.float64) + (g * r) * 1.0
    r = np.where(boot, rb, r)
    for t in range(T - 1, -1, -1):
        r = rewards[t].astype(np.float64) + (g * r) * (1.0 - done_after[t].astype(np.float64))
        out[t] = r.astype(np.float32)
    return out


def clip_by_global_norm(g, max_grad_norm):
    """f32 gradient, f64 norm (as the device reduction), scale = c * min(1/gn, 1/c) in f32"""
    g = np.asarray(g, np.float32)
    if max_grad_norm is None or max_grad_norm < 0:
        return g, None
    gn = np.float32(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
    c = np.float32(max_grad_norm)
    scale = c * np.minimum(np.float32(1) / gn, np.float32(1) / c)
    return g * scale, gn


def rmsprop_step(p, g, ms, mom, lr, decay=0.99, momentum=0.0, eps=1e-5, max_grad_norm=None):
    """in place on f32 arrays p, ms, mom; returns (clipped g, global norm)"""
    f = np.float32
    g, gn = clip_by_global_norm(g, max_grad_norm)
    ms += (g * g - ms) * (f(1) - f(decay))
    mom[...] = mom * f(momentum) + (f(lr) * g) / np.sqrt(ms + f(eps))
    p -= mom
    return g, gn


class A2COracle(OracleModel):
    loss_names = ['policy_loss', 'value_loss', 'policy_entropy']

    def __init__(self, **kw):
        self.alpha, self.rms_eps = kw.pop('alpha', 0.99), kw.pop('epsilon', 1e-5)
        super().__init__(**kw)
        self.ms = {k: torch.ones_like(self.p[k]) for k in self.names}
        self.mom = {k: torch.zeros_like(self.p[k]) for k in self.names}

    def a2c_loss(self, obs, rewards, actions, values, states=None, masks=None):
        dt = self.dtype
        R = torch.as_tensor(np.asarray(rewards)).to(dt)
        ADV = torch.as_tensor(np.asarray(rewards, np.float32) - np.asarray(values, np.float32)).to(dt)   # a2c.py:93
        A = torch.as_tensor(np.asarray(actions))
        if self.pd_kind in ('gaussian', 'bernoulli'):
            A = A.to(dt)
        if self.recurrent:
            pi, vpred = self.forward(obs, states, masks, nenv=np.asarray(states).shape[0])
        else:
            pi, vpred = self.forward(obs)
        pg_loss = (ADV * self._neglogp(pi, A)).mean()
        entropy = self._entropy(pi).mean()
        vf_loss = ((R - vpred) ** 2).mean()
        loss = pg_loss - entropy * self.ent_coef + vf_loss * self.vf_coef
        return loss, [pg_loss, vf_loss, entropy]

    def a2c_grads(self, obs, rewards, actions, values, states=None, masks=None):
        for t in self.p.values():
            t.grad = None
        loss, stats = self.a2c_loss(obs, rewards, actions, values, states, masks)
        loss.backward()
        flat = torch.cat([(torch.zeros_like(self.p[k]) if self.p[k].grad is None else self.p[k].grad).reshape(-1)
                          for k in self.names])
        return [float(s.detach()) for s in stats], flat.detach().numpy()

    def flat_slots(self):
        cat = lambda d: np.concatenate([d[k].numpy().reshape(-1) for k in self.names])
        return cat(self.ms), cat(self.mom)

    def a2c_train(self, lr, obs, states, rewards, masks, actions, values):
        """Model.train (a2c.py:88-109) in f32: gradient, clip_by_global_norm, RMSProp"""
        stats, flat = self.a2c_grads(obs, rewards, actions, values, states, masks)
        p = self.flat_params().astype(np.float32)
        ms, mom = self.flat_slots()
        rmsprop_step(p, flat.astype(np.float32), ms, mom, lr, self.alpha, 0.0, self.rms_eps, self.max_grad_norm)
        off = 0
        with torch.no_grad():
            for k in self.names:
                n = self.p[k].numel()
                sh = self.p[k].shape
                self.p[k].copy_(torch.from_numpy(p[off:off + n].reshape(sh)))
                self.ms[k].copy_(torch.from_numpy(ms[off:off + n].reshape(sh)))
                self.mom[k].copy_(torch.from_numpy(mom[off:off + n].reshape(sh)))
                off += n
        return stats
