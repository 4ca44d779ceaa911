"""Replay memory of DDPG on the device (ddpg/memory.py).  The rows live in f32 device rings; the ring's (start, length) is
kept both on the host (for index drawing) and in a device int64 [2] that the HIP kernels read and advance (mrl_ddpg_store
appends, mrl_ddpg_train_step gathers at (start + idx) % limit).  `sample` draws its indices with the reference's
`np.random.randint(nb_entries - 2, size=batch_size)` -- the `- 2` included."""
import numpy as np
import torch

from .. import _lib, ops


class RingBuffer(object):
    def __init__(self, maxlen, shape, dtype='float32', device=None):
        assert np.dtype(dtype) == np.float32, 'the device ring holds float32 rows'
        self.maxlen = int(maxlen)
        self.start = 0
        self.length = 0
        self.shape = tuple(shape)
        self.data = torch.zeros((self.maxlen,) + self.shape, dtype=torch.float32, device=device or 'cuda')

    def __len__(self):
        return self.length

    def __getitem__(self, idx):
        if idx < 0 or idx >= self.length:
            raise KeyError()
        return self.data[(self.start + idx) % self.maxlen]

    def get_batch(self, idxs):
        """rows at (start + idxs) % maxlen (host index array) -> device tensor [len(idxs), *shape]"""
        rows = torch.from_numpy((self.start + np.asarray(idxs, dtype=np.int64)) % self.maxlen).to(self.data.device)
        return ops.gather_rows(self.data.view((1, self.maxlen) + self.shape), rows, 1, self.maxlen)

    def _advance(self, n):
        """host mirror of n appends (memory.py:24-35)"""
        tot = self.length + n
        self.start = (self.start + max(0, tot - self.maxlen)) % self.maxlen
        self.length = min(tot, self.maxlen)

    def append(self, v):
        self._advance(1)
        self.data[(self.start + self.length - 1) % self.maxlen] = torch.as_tensor(np.asarray(v, np.float32)).to(self.data.device)


def array_min2d(x):
    return x if x.dim() >= 2 else x.reshape(-1, 1)


class Memory(object):
    def __init__(self, limit, action_shape, observation_shape, device=None):
        if torch.device(device or 'cuda').type == 'cuda':
            _lib.require_gpu()          # a CPU Memory only serves host-side bookkeeping tests; sample() needs the device
        self.limit = int(limit)
        self.observations0 = RingBuffer(limit, shape=observation_shape, device=device)
        self.actions = RingBuffer(limit, shape=action_shape, device=device)
        self.rewards = RingBuffer(limit, shape=(1,), device=device)
        self.terminals1 = RingBuffer(limit, shape=(1,), device=device)
        self.observations1 = RingBuffer(limit, shape=observation_shape, device=device)
        self.ring_pos = torch.zeros(2, dtype=torch.int64, device=self.observations0.data.device)   # (start, length)

    @property
    def _rings(self):
        return (self.observations0, self.actions, self.rewards, self.terminals1, self.observations1)

    def draw_indices(self, batch_size):
        """the reference's draw: always leaves room for a following element (memory.py:52-53)"""
        return np.random.randint(self.nb_entries - 2, size=batch_size)

    def sample(self, batch_size):
        batch_idxs = self.draw_indices(batch_size)
        return {
            'obs0': array_min2d(self.observations0.get_batch(batch_idxs)),
            'obs1': array_min2d(self.observations1.get_batch(batch_idxs)),
            'rewards': array_min2d(self.rewards.get_batch(batch_idxs)),
            'actions': array_min2d(self.actions.get_batch(batch_idxs)),
            'terminals1': array_min2d(self.terminals1.get_batch(batch_idxs)),
        }

    def append(self, obs0, action, reward, obs1, terminal1, training=True):
        if not training:
            return
        self.observations0.append(obs0)
        self.actions.append(action)
        self.rewards.append(reward)
        self.observations1.append(obs1)
        self.terminals1.append(terminal1)
        self._sync_pos()

    def advance(self, n):
        """host bookkeeping after a device append of n rows (mrl_ddpg_store advanced ring_pos itself)"""
        for r in self._rings:
            r._advance(n)

    def _sync_pos(self):
        self.ring_pos.copy_(torch.tensor([self.observations0.start, self.observations0.length], dtype=torch.int64))

    def state_fields(self, st):
        """fill the ring part of an mrl_ddpg_state"""
        st.obs0 = self.observations0.data.data_ptr()
        st.actions = self.actions.data.data_ptr()
        st.rewards = self.rewards.data.data_ptr()
        st.obs1 = self.observations1.data.data_ptr()
        st.terminals1 = self.terminals1.data.data_ptr()
        st.ring_pos = self.ring_pos.data_ptr()
        st.limit = self.limit

    @property
    def nb_entries(self):
        return len(self.observations0)
