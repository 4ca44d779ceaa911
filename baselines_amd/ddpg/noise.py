"""Exploration noise with the reference's surface and NumPy draws (ddpg/noise.py): the same `np.random` calls in the same
order, so a seeded run reproduces the reference's noise sequence exactly."""
import numpy as np


class AdaptiveParamNoiseSpec(object):
    def __init__(self, initial_stddev=0.1, desired_action_stddev=0.1, adoption_coefficient=1.01):
        self.initial_stddev = initial_stddev
        self.desired_action_stddev = desired_action_stddev
        self.adoption_coefficient = adoption_coefficient
        self.current_stddev = initial_stddev

    def adapt(self, distance):
        # shrink the perturbation when the policy moved further than desired, grow it otherwise
        if distance > self.desired_action_stddev:
            self.current_stddev /= self.adoption_coefficient
        else:
            self.current_stddev *= self.adoption_coefficient

    def get_stats(self):
        return {'param_noise_stddev': self.current_stddev}

    def __repr__(self):
        return 'AdaptiveParamNoiseSpec(initial_stddev={}, desired_action_stddev={}, adoption_coefficient={})'.format(
            self.initial_stddev, self.desired_action_stddev, self.adoption_coefficient)


class ActionNoise(object):
    def reset(self):
        pass


class NormalActionNoise(ActionNoise):
    def __init__(self, mu, sigma):
        self.mu = mu
        self.sigma = sigma

    def __call__(self):
        return np.random.normal(self.mu, self.sigma)

    def __repr__(self):
        return 'NormalActionNoise(mu={}, sigma={})'.format(self.mu, self.sigma)


class OrnsteinUhlenbeckActionNoise(ActionNoise):
    """Euler-Maruyama step of an Ornstein-Uhlenbeck process: x += theta (mu - x) dt + sigma sqrt(dt) N(0, 1)"""

    def __init__(self, mu, sigma, theta=.15, dt=1e-2, x0=None):
        self.theta = theta
        self.mu = mu
        self.sigma = sigma
        self.dt = dt
        self.x0 = x0
        self.reset()

    def __call__(self):
        drift = self.theta * (self.mu - self.x_prev) * self.dt
        x = self.x_prev + drift + self.sigma * np.sqrt(self.dt) * np.random.normal(size=self.mu.shape)
        self.x_prev = x
        return x

    def reset(self):
        self.x_prev = np.zeros_like(self.mu) if self.x0 is None else self.x0

    def __repr__(self):
        return 'OrnsteinUhlenbeckActionNoise(mu={}, sigma={})'.format(self.mu, self.sigma)


def parse_noise_type(noise_type, nb_actions):
    """ddpg/ddpg.py:71-88: a comma list of 'none', 'adaptive-param_<s>', 'normal_<s>', 'ou_<s>' -> (action_noise, param_noise)"""
    action_noise = None
    param_noise = None
    if noise_type is None:
        return action_noise, param_noise
    for current in noise_type.split(','):
        current = current.strip()
        if current == 'none':
            continue
        if 'adaptive-param' in current:
            _, stddev = current.split('_')
            param_noise = AdaptiveParamNoiseSpec(initial_stddev=float(stddev), desired_action_stddev=float(stddev))
        elif 'normal' in current:
            _, stddev = current.split('_')
            action_noise = NormalActionNoise(mu=np.zeros(nb_actions), sigma=float(stddev) * np.ones(nb_actions))
        elif 'ou' in current:
            _, stddev = current.split('_')
            action_noise = OrnsteinUhlenbeckActionNoise(mu=np.zeros(nb_actions), sigma=float(stddev) * np.ones(nb_actions))
        else:
            raise RuntimeError('unknown noise type "{}"'.format(current))
    return action_noise, param_noise
