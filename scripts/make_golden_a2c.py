"""
TEST INFRASTRUCTURE ONLY.  Generates tests/golden/a2c.npz from the REFERENCE's own A2C code (read from a reference
checkout, never copied; not run on GPU machines and imported by no test):

  * baselines/a2c/utils.py imports tensorflow at module level, so the three pure-Python pieces the A2C runner and model
    use -- ``discount_with_dones``, the schedule functions + ``schedules`` table and ``Scheduler`` -- are cut out of the
    file with ``ast`` and exec'd unmodified into a stub ``baselines.a2c.utils`` module;
  * baselines/a2c/runner.py is then imported as it stands and its ``Runner.run()`` is driven by the replay env / model
    stubs of oracle/make_golden.py (imported, not edited): n-step returns with bootstrap (runner.py:49-75);
  * the learning rate ``Scheduler`` yields per update (a2c.py:94-95: value() once per sample, the last one is used).

Run:  python scripts/make_golden_a2c.py     (BASELINES_REFERENCE: path of the reference checkout)
"""
import ast
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle import make_golden as MG   # noqa: E402

REF = MG.REF
OUT = os.path.join(ROOT, 'tests', 'golden', 'a2c.npz')
NEEDED = ('discount_with_dones', 'constant', 'linear', 'middle_drop', 'double_linear_con', 'double_middle_drop',
          'schedules', 'Scheduler')


def _stub_a2c_utils():
    src = open(os.path.join(REF, 'baselines', 'a2c', 'utils.py')).read()
    tree = ast.parse(src)
    keep = []
    for node in tree.body:
        names = ([node.name] if isinstance(node, (ast.FunctionDef, ast.ClassDef)) else
                 [t.id for t in node.targets if isinstance(t, ast.Name)] if isinstance(node, ast.Assign) else [])
        if any(n in NEEDED for n in names):
            keep.append(node)
    mod = types.ModuleType('baselines.a2c.utils')
    exec(compile(ast.Module(body=keep, type_ignores=[]), 'baselines/a2c/utils.py', 'exec'), mod.__dict__)
    assert all(hasattr(mod, n) for n in NEEDED)
    return mod


def _import_reference():
    if 'gym' not in sys.modules:
        sys.modules['gym'] = types.ModuleType('gym')
    sys.path.insert(0, REF)
    import baselines.a2c      # noqa: F401  (package __init__ is empty)
    utils = _stub_a2c_utils()
    sys.modules['baselines.a2c.utils'] = utils
    from baselines.a2c.runner import Runner
    return Runner, utils


class _Shape(object):
    def __init__(self, dims):
        self.dims = dims

    def as_list(self):
        return list(self.dims)


class _DType(object):
    def __init__(self, np_dtype):
        self.as_numpy_dtype = np_dtype
        self.name = np.dtype(np_dtype).name


class _Tensor(object):
    def __init__(self, dims, np_dtype):
        self.shape, self.dtype = _Shape(dims), _DType(np_dtype)


class A2CReplayModel(MG.ReplayModel):
    """MG.ReplayModel + the train_model attributes a2c/runner.py:17-18 reads"""

    def __init__(self, ro):
        super().__init__(ro)
        self.train_model = types.SimpleNamespace(action=_Tensor([None], np.int64),
                                                 X=_Tensor([None] + list(ro['obs'].shape[2:]), ro['obs'].dtype.type))


def _with_zeros(a, rng, frac):
    """replace a fraction of the entries by +0.0 / -0.0"""
    a = a.copy()
    m = rng.rand(*a.shape) < frac
    a[m] = np.where(rng.rand(int(m.sum())) < 0.5, np.float32(0.0), np.float32(-0.0))
    return a


CASES = [
    # name, T, N, seed, done pattern, gamma
    ('t1_n3_mixed', 1, 3, 10, 'mixed', 0.99),
    ('t5_n64_mixed', 5, 64, 11, 'mixed', 0.99),
    ('t16_n70_mixed', 16, 70, 12, 'mixed', 0.99),
    ('t5_n70_alldone', 5, 70, 13, 'all', 0.99),
    ('t16_n64_nodone', 16, 64, 14, 'none', 0.99),
    ('t1_n64_alldone', 1, 64, 15, 'all', 0.95),
    ('t5_n3_gamma0', 5, 3, 16, 'mixed', 0.0),
    ('t16_n3_zeros', 16, 3, 17, 'mixed', 0.9),
    ('t5_n64_zeros', 5, 64, 18, 'mixed', 0.99),
]


def gen_returns(Runner, out):
    for name, T, N, seed, pattern, gamma in CASES:
        rng = np.random.RandomState(seed)
        ro = MG.small_rollout(T, N, seed, (2,), 'float32', 'discrete', 0.3)
        zf = 0.4 if name.endswith('zeros') else 0.1
        ro['rewards'] = _with_zeros(ro['rewards'], rng, zf)
        ro['values'] = _with_zeros(ro['values'], rng, zf)
        ro['last_values'] = _with_zeros(ro['last_values'], rng, zf)
        first = np.zeros(N, bool)
        if pattern == 'all':
            ro['dones'][:] = True
            ro['last_dones'][:] = True
            first[:] = True
        elif pattern == 'none':
            ro['dones'][:] = False
            ro['last_dones'][:] = False
        else:
            first = rng.rand(N) < 0.3
            ro['dones'][0] = first
            ro['last_dones'] = np.arange(N) % 2 == 0 if N > 1 else np.array([False])
            ro['last_dones'] = ro['last_dones'] ^ (rng.rand(N) < 0.2)
        env, model = MG.ReplayEnv(ro), A2CReplayModel(ro)
        runner = Runner(env, model, nsteps=T, gamma=gamma)
        runner.dones = first.tolist()            # the done flags entering the rollout
        obs, states, rewards, masks, actions, values, epinfos = runner.run()
        assert states is None and epinfos == [] and rewards.dtype == np.float32 and masks.dtype == np.bool_
        for k in ('rewards', 'values', 'last_values'):
            out['%s/in_%s' % (name, k)] = ro[k]
        out[name + '/in_dones'] = ro['dones'].astype(np.uint8)          # entering each step, [T][N]
        out[name + '/in_last_dones'] = ro['last_dones'].astype(np.uint8)
        out[name + '/gamma'] = np.float64(gamma)
        out[name + '/out_returns'] = rewards                           # env-major [N*T]
        out[name + '/out_masks'] = masks
        out[name + '/out_values'] = values
        print('returns', name, rewards[:4], int(ro['last_dones'].sum()), 'last dones')


LR_PAIRS = [(40, 400), (80, 1000)]


def gen_lr(utils, out):
    for sched in sorted(utils.schedules):
        for nbatch, total in LR_PAIRS:
            s = utils.Scheduler(v=7e-4, nvalues=total, schedule=sched)
            seq = []
            for _ in range(total // nbatch):
                for _ in range(nbatch):
                    cur = s.value()
                seq.append(cur)
            out['lr/%s/%d_%d' % (sched, nbatch, total)] = np.array(seq, np.float64)


def main():
    Runner, utils = _import_reference()
    out = {}
    gen_returns(Runner, out)
    gen_lr(utils, out)
    out['cases'] = np.array([c[0] for c in CASES])
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, len(out), 'arrays')


if __name__ == '__main__':
    main()
