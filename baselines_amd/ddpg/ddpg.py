"""DDPG driver with the reference's signature, defaults and logger keys (ddpg/ddpg.py:21-275).

On a device-resident env (SyntheticVecEnv) observations, actions, rewards and dones never leave the device inside a cycle:
every rollout step is mrl_ddpg_act -> env step -> mrl_ddpg_store, and the cycle's train steps (with their param-noise
adaptation and soft target updates) are one captured hipGraph of one mrl_ddpg_train_step launch per step, replayed every
cycle with the cycle's batch indices and Adam step sizes drawn on the host up front, in the reference's np.random order,
and copied once.  With nenvs > 1 and no action noise (the default 'adaptive-param_0.2') nothing in the rollout depends on a
host value, so the cycle's rollout steps are a second captured graph.  Losses, actions, Q values and finished episodes are
read back when the epoch logs.  Action noise is drawn on the host per step (the reference's np.random stream), and with
nenvs == 1 the reference resets the agent on every done, so those rollouts launch eagerly (the latter reads the done flag
back every step).  Host VecEnvs run through the same objects eagerly.
"""
import os
import pickle
import time
from collections import deque

import numpy as np
import torch

from .. import _lib, logger
from ..common import set_global_seeds
from ..common.dist import default_comm
from .ddpg_learner import DDPG
from .memory import Memory
from .models import Actor, Critic
from .noise import parse_noise_type

CAPTURE_TRAIN = True      # replay each cycle's train steps from a captured graph (False: the same launches, eagerly)
CAPTURE_ROLLOUT = True    # the same for the rollout steps of a device env (nenvs > 1, no action noise)


class _RolloutCycle(object):
    """nb_rollout_steps of act -> env step -> store (ddpg.py:125-161) on fixed device buffers: obs [T+1, N, D] (slot 0 = the
    observation entering the cycle), actions, Q, rewards, dones and finished-episode statistics per step.  Runs eagerly the
    first time, is captured as a graph the second time and replayed afterwards; the host only advances the ring mirror."""

    def __init__(self, agent, env, T):
        self.agent, self.env, self.T = agent, env, T
        N, D, A = env.num_envs, agent.ob_dim, agent.nb_actions
        dev = agent.device
        f32 = dict(dtype=torch.float32, device=dev)
        self.obs = torch.zeros((T + 1, N, D), **f32)
        self.actions = torch.zeros((T, N, A), **f32)
        self.q = torch.zeros((T, N), **f32)
        self.rew = torch.zeros((T, N), **f32)
        self.done = torch.zeros((T, N), dtype=torch.uint8, device=dev)
        self.fin_r = torch.zeros((T, N), **f32)
        self.fin_l = torch.zeros((T, N), dtype=torch.int32, device=dev)
        self.scale = None
        self.graph = None
        self.runs = 0

    def _launch(self):
        a = self.agent
        for t in range(self.T):
            a.act_into(self.obs[t], self.actions[t], self.q[t], True, None)
            act = self.actions[t] if self.scale is None else self.actions[t] * self.scale
            _, _, _, info = self.env.step_into(act, obs_out=self.obs[t + 1], rew_out=self.rew[t], done_out=self.done[t])
            self.fin_r[t].copy_(info['fin_r'])
            self.fin_l[t].copy_(info['fin_l'])
            a.k.store(a.state, self.obs[t], self.actions[t], self.rew[t], self.obs[t + 1], self.done[t], a.reward_scale)
        self.obs[0].copy_(self.obs[self.T])

    def run(self):
        if not CAPTURE_ROLLOUT or self.runs == 0:
            self._launch()
        else:
            if self.graph is None:
                self.agent.k.frozen = True
                self.graph = torch.cuda.CUDAGraph()
                with _lib.capture_graph(self.graph):
                    self._launch()
            self.graph.replay()
        self.runs += 1
        self.agent.memory.advance(self.T * self.env.num_envs)


class _TrainCycle(object):
    """The nb_train_steps train steps of one cycle (ddpg.py:175-185) as launches on fixed device buffers: per step the
    batch indices and the two Adam step sizes; the param-noise distance at step 0 when the cycle adapts.  Captured as a
    graph at its first use per `adapt` flag, replayed afterwards."""

    def __init__(self, agent, nb_train_steps):
        self.agent = agent
        self.S = nb_train_steps
        dev = agent.device
        B = agent.batch_size
        self.idx = torch.zeros((self.S, B), dtype=torch.int64, device=dev)
        self.adapt_idx = torch.zeros(B, dtype=torch.int64, device=dev)
        self.alpha = torch.zeros((self.S, 2), dtype=torch.float32, device=dev)
        self.losses = torch.zeros((self.S, 2), dtype=torch.float32, device=dev)
        self.graphs = {}

    def _launch(self, adapt):
        a = self.agent
        if adapt:
            a.k.policy_distance(a.state, a.adaptive_actor_params, self.adapt_idx, a.distance)
        for s in range(self.S):
            a.train_step_dev(self.idx[s], self.alpha[s], self.losses[s], soft_update=True)

    def run(self, adapt):
        if not CAPTURE_TRAIN:
            self._launch(adapt)
            return
        g = self.graphs.get(adapt)
        if g is None:
            self._launch(adapt)                        # warm-up outside the capture (first cycle runs eagerly)
            g = torch.cuda.CUDAGraph()
            self.graphs[adapt] = (g, False)
            return
        graph, captured = g
        if not captured:
            # capturing launches nothing: capture, then replay once as this cycle's launch
            self.agent.k.frozen = True
            with _lib.capture_graph(graph):
                self._launch(adapt)
            self.graphs[adapt] = (graph, True)
        graph.replay()


def learn(network, env,
          seed=None,
          total_timesteps=None,
          nb_epochs=None,
          nb_epoch_cycles=20,
          nb_rollout_steps=100,
          reward_scale=1.0,
          render=False,
          render_eval=False,
          noise_type='adaptive-param_0.2',
          normalize_returns=False,
          normalize_observations=True,
          critic_l2_reg=1e-2,
          actor_lr=1e-4,
          critic_lr=1e-3,
          popart=False,
          gamma=0.99,
          clip_norm=None,
          nb_train_steps=50,
          nb_eval_steps=100,
          batch_size=64,
          tau=0.01,
          eval_env=None,
          param_noise_adaption_interval=50,
          **network_kwargs):
    comm = default_comm()
    if comm is not None and comm.Get_size() > 1:
        raise NotImplementedError('DDPG has no multi-rank path here (the reference\'s MpiAdam all-reduce is not built)')
    set_global_seeds(seed)

    if total_timesteps is not None:
        assert nb_epochs is None
        nb_epochs = int(total_timesteps) // (nb_epoch_cycles * nb_rollout_steps)
    else:
        nb_epochs = 500
    rank = 0

    nb_actions = env.action_space.shape[-1]
    assert (np.abs(env.action_space.low) == env.action_space.high).all()  # symmetric actions

    memory = Memory(limit=int(1e6), action_shape=env.action_space.shape, observation_shape=env.observation_space.shape)
    critic = Critic(network=network, **network_kwargs)
    actor = Actor(nb_actions, network=network, **network_kwargs)
    action_noise, param_noise = parse_noise_type(noise_type, nb_actions)

    max_action = env.action_space.high
    logger.info('scaling actions by {} before executing in env'.format(max_action))

    agent = DDPG(actor, critic, memory, env.observation_space.shape, env.action_space.shape,
                 gamma=gamma, tau=tau, normalize_returns=normalize_returns, normalize_observations=normalize_observations,
                 batch_size=batch_size, action_noise=action_noise, param_noise=param_noise, critic_l2_reg=critic_l2_reg,
                 actor_lr=actor_lr, critic_lr=critic_lr, enable_popart=popart, clip_norm=clip_norm,
                 reward_scale=reward_scale)
    logger.info('Using agent with the following configuration:')
    logger.info(str(agent.__dict__.items()))

    eval_episode_rewards_history = deque(maxlen=100)
    episode_rewards_history = deque(maxlen=100)
    agent.initialize()
    agent.reset()

    device_env = bool(getattr(env, 'device_resident', False))
    obs = env.reset()
    if eval_env is not None:
        eval_obs = eval_env.reset()
    nenvs = obs.shape[0]
    dev = agent.device
    # one workspace for every launch of the run: graphs capture its address
    agent.k.reserve(min(1024, max(batch_size, nenvs, eval_obs.shape[0] if eval_env is not None else 0)))
    unit_scale = bool(np.all(np.asarray(max_action) == 1.0))
    max_action_dev = torch.as_tensor(np.asarray(max_action, np.float32)).to(dev)

    episode_reward = np.zeros(nenvs, dtype=np.float32)
    episode_step = np.zeros(nenvs, dtype=int)
    episodes = 0
    t = 0
    start_time = time.time()

    epoch_episode_rewards = []
    epoch_episode_steps = []
    epoch_actions = []           # host arrays (the device path appends device tensors and moves them at log time)
    epoch_qs = []
    epoch_episodes = 0
    # one train cycle's worth of adaptation + train steps captured together (only when it adapts at most at step 0)
    cycle = _TrainCycle(agent, nb_train_steps) if param_noise_adaption_interval >= nb_train_steps else None
    pending_distance = False
    fin = []                     # device path: (done, fin_r, fin_l) per step, resolved at log time
    last_losses = None
    epoch_adaptive_distances = []
    rollout = None
    if device_env and nenvs > 1 and action_noise is None and not render:
        rollout = _RolloutCycle(agent, env, nb_rollout_steps)
        rollout.obs[0].copy_(obs)
        if not unit_scale:
            rollout.scale = max_action_dev

    def resolve_episodes():
        nonlocal episodes, epoch_episodes
        for done_d, fr, fl in fin:
            done_h, fr_h, fl_h = done_d.cpu().numpy(), fr.cpu().numpy(), fl.cpu().numpy()
            for d in range(len(done_h)):
                if done_h[d]:
                    epoch_episode_rewards.append(fr_h[d])
                    episode_rewards_history.append(fr_h[d])
                    epoch_episode_steps.append(int(fl_h[d]))
                    epoch_episodes += 1
                    episodes += 1
        fin.clear()

    def finish_adapt():
        nonlocal pending_distance
        if pending_distance:
            distance = float(agent.distance.item())
            agent.param_noise.adapt(distance)
            epoch_adaptive_distances.append(distance)
            pending_distance = False

    for epoch in range(nb_epochs):
        for cycle_i in range(nb_epoch_cycles):
            finish_adapt()
            if nenvs > 1:
                agent.reset()
            if rollout is not None:
                rollout.run()
                t += nb_rollout_steps
                epoch_actions.append(rollout.actions.clone())
                epoch_qs.append(rollout.q.clone())
                fin.append((rollout.done.clone().reshape(-1), rollout.fin_r.clone().reshape(-1),
                            rollout.fin_l.clone().reshape(-1)))
                obs = rollout.obs[0]
            for t_rollout in range(nb_rollout_steps if rollout is None else 0):
                if device_env:
                    action = torch.empty((nenvs, nb_actions), dtype=torch.float32, device=dev)
                    q = torch.empty(nenvs, dtype=torch.float32, device=dev)
                    noise = None
                    if action_noise is not None:
                        noise = torch.from_numpy(np.asarray(action_noise(), np.float64)).to(dev)
                    agent.act_into(obs, action, q, True, noise)
                    new_obs, r, done, info = env.step_into(action if unit_scale else action * max_action_dev)
                    t += 1
                    epoch_actions.append(action)
                    epoch_qs.append(q)
                    agent.store_transition(obs, action, r, new_obs, done)
                    obs = new_obs
                    fin.append((done, info['fin_r'], info['fin_l']))
                    if nenvs == 1 and bool(done[0].item()):
                        agent.reset()
                    continue
                action, q, _, _ = agent.step(obs, apply_noise=True, compute_Q=True)
                if rank == 0 and render:
                    env.render()
                new_obs, r, done, info = env.step(max_action * action)
                t += 1
                if rank == 0 and render:
                    env.render()
                episode_reward += r
                episode_step += 1
                epoch_actions.append(action)
                epoch_qs.append(q)
                agent.store_transition(obs, action, r, new_obs, done)
                obs = new_obs
                for d in range(len(done)):
                    if done[d]:
                        epoch_episode_rewards.append(episode_reward[d])
                        episode_rewards_history.append(episode_reward[d])
                        epoch_episode_steps.append(episode_step[d])
                        episode_reward[d] = 0.
                        episode_step[d] = 0
                        epoch_episodes += 1
                        episodes += 1
                        if nenvs == 1:
                            agent.reset()

            # Train.
            epoch_adaptive_distances = []
            if cycle is not None:
                adapt = param_noise is not None and memory.nb_entries >= batch_size
                if adapt:                          # the adaptation batch is drawn before the first train batch
                    cycle.adapt_idx.copy_(torch.from_numpy(memory.draw_indices(batch_size).astype(np.int64)))
                    agent.perturb(agent.adaptive_actor_params, param_noise.current_stddev)
                idx = np.stack([memory.draw_indices(batch_size) for _ in range(nb_train_steps)]).astype(np.int64)
                alpha = np.stack([agent.next_alphas() for _ in range(nb_train_steps)])
                cycle.idx.copy_(torch.from_numpy(idx))
                cycle.alpha.copy_(torch.from_numpy(alpha))
                cycle.run(adapt)
                pending_distance = adapt
                if param_noise is None and memory.nb_entries >= batch_size:
                    epoch_adaptive_distances.append(0.)          # adapt_param_noise() returns 0. without param noise
                last_losses = cycle.losses
            else:
                losses = []
                for t_train in range(nb_train_steps):
                    if memory.nb_entries >= batch_size and t_train % param_noise_adaption_interval == 0:
                        epoch_adaptive_distances.append(agent.adapt_param_noise())
                    idx = torch.from_numpy(memory.draw_indices(batch_size).astype(np.int64)).to(dev)
                    agent.neg_alpha.copy_(torch.from_numpy(agent.next_alphas()))
                    out = torch.empty(2, dtype=torch.float32, device=dev)
                    agent.train_step_dev(idx, agent.neg_alpha, out, soft_update=True)
                    losses.append(out)
                last_losses = torch.stack(losses) if losses else None

            # Evaluate.
            eval_episode_rewards = []
            eval_qs = []
            if eval_env is not None:
                nenvs_eval = eval_obs.shape[0]
                eval_episode_reward = np.zeros(nenvs_eval, dtype=np.float32)
                for t_rollout in range(nb_eval_steps):
                    eval_action, eval_q, _, _ = agent.step(eval_obs, apply_noise=False, compute_Q=True)
                    if isinstance(eval_action, torch.Tensor):
                        eval_action, eval_q = eval_action.cpu().numpy(), eval_q.cpu().numpy()
                    eval_obs, eval_r, eval_done, eval_info = eval_env.step(max_action * eval_action)
                    if isinstance(eval_r, torch.Tensor):
                        eval_r, eval_done = eval_r.cpu().numpy(), eval_done.cpu().numpy()
                    if render_eval:
                        eval_env.render()
                    eval_episode_reward += eval_r
                    eval_qs.append(eval_q)
                    for d in range(len(eval_done)):
                        if eval_done[d]:
                            eval_episode_rewards.append(eval_episode_reward[d])
                            eval_episode_rewards_history.append(eval_episode_reward[d])
                            eval_episode_reward[d] = 0.0

        mpi_size = 1
        finish_adapt()
        resolve_episodes()
        # device entries: [N, A] / [N] per eager step, [T, N, A] / [T, N] per captured cycle -> one host array per step
        host_actions, host_qs = [], []
        for a in epoch_actions:
            a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
            host_actions.extend(list(a) if a.ndim == 3 else [a])
        for q in epoch_qs:
            if isinstance(q, torch.Tensor):
                q = q.cpu().numpy()
                host_qs.extend([x.reshape(-1, 1) for x in q] if q.ndim == 2 else [q.reshape(-1, 1)])
            else:
                host_qs.append(q)
        epoch_actions[:], epoch_qs[:] = host_actions, host_qs
        lh = last_losses.cpu().numpy() if last_losses is not None else np.zeros((0, 2), np.float32)
        epoch_critic_losses, epoch_actor_losses = list(lh[:, 0]), list(lh[:, 1])

        # Log stats.
        duration = time.time() - start_time
        stats = agent.get_stats()
        combined_stats = stats.copy()
        combined_stats['rollout/return'] = np.mean(epoch_episode_rewards)
        combined_stats['rollout/return_std'] = np.std(epoch_episode_rewards)
        combined_stats['rollout/return_history'] = np.mean(episode_rewards_history)
        combined_stats['rollout/return_history_std'] = np.std(episode_rewards_history)
        combined_stats['rollout/episode_steps'] = np.mean(epoch_episode_steps)
        combined_stats['rollout/actions_mean'] = np.mean(epoch_actions)
        combined_stats['rollout/Q_mean'] = np.mean(epoch_qs)
        combined_stats['train/loss_actor'] = np.mean(epoch_actor_losses)
        combined_stats['train/loss_critic'] = np.mean(epoch_critic_losses)
        combined_stats['train/param_noise_distance'] = np.mean(epoch_adaptive_distances)
        combined_stats['total/duration'] = duration
        combined_stats['total/steps_per_second'] = float(t) / float(duration)
        combined_stats['total/episodes'] = episodes
        combined_stats['rollout/episodes'] = epoch_episodes
        combined_stats['rollout/actions_std'] = np.std(epoch_actions)
        if eval_env is not None:
            combined_stats['eval/return'] = eval_episode_rewards
            combined_stats['eval/return_history'] = np.mean(eval_episode_rewards_history)
            combined_stats['eval/Q'] = eval_qs
            combined_stats['eval/episodes'] = len(eval_episode_rewards)

        # the reference takes the first element of every value (ddpg.py:249); an empty list logs nan instead of raising
        combined_stats_sums = np.array([np.array(x).flatten()[0] if np.size(x) else np.nan for x in combined_stats.values()])
        combined_stats = {k: v / mpi_size for (k, v) in zip(combined_stats.keys(), combined_stats_sums)}
        combined_stats['total/epochs'] = epoch + 1
        combined_stats['total/steps'] = t

        for key in sorted(combined_stats.keys()):
            logger.record_tabular(key, combined_stats[key])
        if rank == 0:
            logger.dump_tabular()
        logger.info('')
        logdir = logger.get_dir()
        if rank == 0 and logdir:
            if hasattr(env, 'get_state'):
                with open(os.path.join(logdir, 'env_state.pkl'), 'wb') as f:
                    pickle.dump(env.get_state(), f)
            if eval_env and hasattr(eval_env, 'get_state'):
                with open(os.path.join(logdir, 'eval_env_state.pkl'), 'wb') as f:
                    pickle.dump(eval_env.get_state(), f)

    agent.last_stats = combined_stats
    return agent
