"""
TEST INFRASTRUCTURE ONLY.  Generates tests/golden/ddpg.npz from the REFERENCE's own DDPG replay memory and noise code
(read from a reference checkout, never copied; not run on GPU machines and imported by no test).  baselines/ddpg/memory.py
and baselines/ddpg/noise.py are NumPy-only and are imported as they stand:

  * RingBuffer contents, start and length after every append across a wrap at limit 7;
  * Memory.sample: the np.random.randint(nb_entries - 2, size) index streams of a seeded run and the batches they gather,
    before and after the ring wraps;
  * NormalActionNoise and OrnsteinUhlenbeckActionNoise sequences from a fixed seed, with resets in between;
  * an AdaptiveParamNoiseSpec.adapt trajectory over a fixed list of distances.

Run:  python scripts/make_golden_ddpg.py     (BASELINES_REFERENCE: path of the reference checkout)
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle import make_golden as MG   # noqa: E402

REF = MG.REF
OUT = os.path.join(ROOT, 'tests', 'golden', 'ddpg.npz')


def _load(name):
    spec = importlib.util.spec_from_file_location('ref_ddpg_' + name, os.path.join(REF, 'baselines', 'ddpg', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    memory, noise = _load('memory'), _load('noise')
    out = {}
    # RingBuffer across a wrap
    rb = memory.RingBuffer(7, shape=(3,))
    vals = np.arange(12 * 3, dtype=np.float32).reshape(12, 3) * 0.5 - 4
    data, pos = [], []
    for v in vals:
        rb.append(v)
        data.append(rb.data.copy())
        pos.append((rb.start, rb.length))
    out['ring_values'] = vals
    out['ring_data'] = np.stack(data)
    out['ring_pos'] = np.array(pos, np.int64)
    # Memory.sample streams and batches (limit 50, obs 4, action 2), before and after the wrap
    np.random.seed(17)
    mem = memory.Memory(limit=50, action_shape=(2,), observation_shape=(4,))
    rng = np.random.RandomState(5)
    rows = dict(obs0=rng.randn(80, 4).astype(np.float32), act=rng.uniform(-1, 1, (80, 2)).astype(np.float32),
                rew=rng.randn(80).astype(np.float32), obs1=rng.randn(80, 4).astype(np.float32), term=rng.rand(80) < 0.2)
    for k, v in rows.items():
        out['mem_' + k] = v
    idx_streams, batches = [], []
    for n_app, stop in ((30, 30), (30, 60), (20, 80)):
        for i in range(stop - n_app, stop):
            mem.append(rows['obs0'][i], rows['act'][i], rows['rew'][i], rows['obs1'][i], rows['term'][i])
        state = np.random.get_state()
        idx_streams.append(np.random.randint(mem.nb_entries - 2, size=16))
        np.random.set_state(state)
        b = mem.sample(16)
        batches.append(np.concatenate([b['obs0'], b['actions'], b['rewards'], b['obs1'], b['terminals1']], axis=1))
    out['mem_sample_seed'] = np.array(17)
    out['mem_idx'] = np.stack(idx_streams)
    out['mem_batches'] = np.stack(batches)
    # action noise sequences with resets
    np.random.seed(3)
    nn = noise.NormalActionNoise(mu=np.zeros(3), sigma=0.2 * np.ones(3))
    out['normal_seq'] = np.stack([nn() for _ in range(10)])
    np.random.seed(4)
    ou = noise.OrnsteinUhlenbeckActionNoise(mu=np.zeros(3), sigma=0.3 * np.ones(3))
    seq = []
    for i in range(25):
        if i in (10, 17):
            ou.reset()
        seq.append(ou())
    out['ou_seq'] = np.stack(seq)
    # adaptive parameter noise
    spec = noise.AdaptiveParamNoiseSpec(initial_stddev=0.2, desired_action_stddev=0.2)
    dists = np.array([0.1, 0.3, 0.25, 0.19, 0.2, 0.21, 0.05, 0.5])
    traj = []
    for d in dists:
        spec.adapt(d)
        traj.append(spec.current_stddev)
    out['adapt_distances'] = dists
    out['adapt_stddev'] = np.array(traj)
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, sorted(out))


if __name__ == '__main__':
    main()
