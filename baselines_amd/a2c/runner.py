"""A2C rollout collector with the reference's contract (a2c/runner.py:7-76):

    Runner(env, model, nsteps=5, gamma=0.99).run()
        -> (obs, states, rewards, masks, actions, values, epinfos)
    rewards are the n-step discounted returns bootstrapped from V(s_T); masks are the done flags ENTERING each step;
    the array fields are env-major flat [N*T, ...] (index i = e*T + t).

The rollout paths are PPO2's (device env with the graph-replayed rollout, host-env bridge, eager host env): this class
only replaces GAE by the n-step returns kernel (mrl_nstep_returns, bit-exact vs runner.py:58-71) and hands back the A2C
tuple.  `return_host=True`: fresh host arrays like the reference's; otherwise `RolloutField` views of the resident HBM
rollout (overwritten by the next run()).
"""
import numpy as np

from .. import ops
from ..ppo2.runner import Runner as _PPO2Runner, RolloutField


class Runner(_PPO2Runner):
    def __init__(self, env, model, nsteps=5, gamma=0.99, return_host=None):
        super().__init__(env=env, model=model, nsteps=nsteps, gamma=gamma, lam=None, return_host=return_host)
        # set by learn(): the model's captured train step computes the returns itself (Model.train_rollout), so run()
        # leaves ro.returns to it
        self.returns_by_model = False
        self.last_values = None

    def run(self):
        ro = self.rollout
        if self.device_env and self.fast_step:
            last_values, epinfos = self._run_device_env(ro)
        else:
            last_values, epinfos = self._run_host_env(ro)
        self.last_values = last_values
        if not self.returns_by_model:
            ops.nstep_returns(ro.rewards, ro.dones, last_values, self._dones_dev, self.gamma, out=ro.returns)
        T, N = ro.T, ro.N
        act_dtype = {'categorical': np.int64, 'multicategorical': np.int32}.get(ro.pd_kind, np.float32)
        obs, rewards, masks, actions, values = (
            RolloutField(ro.obs, T, N, self._ob_np), RolloutField(ro.returns, T, N, np.float32),
            RolloutField(ro.dones, T, N, np.bool_), RolloutField(ro.actions, T, N, act_dtype),
            RolloutField(ro.values, T, N, np.float32))
        if self.return_host:
            obs, rewards, masks, actions, values = (f.to_numpy() for f in (obs, rewards, masks, actions, values))
        states = self._mb_states if self.recurrent else self.states
        if self.recurrent and self._states_dev is not None:
            self.states = self._states_dev
            if self.return_host:
                states = states.cpu().numpy()
        return obs, states, rewards, masks, actions, values, epinfos
