"""CPU: the A2C host pieces against the reference -- the learning-rate Scheduler, the checkpoint mapping and the returns
recurrence (tests/golden/a2c.npz, written by scripts/make_golden_a2c.py from the reference's own code)."""
import os

import numpy as np
import pytest

from tests._a2c_oracle import nstep_returns


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'a2c.npz'))


def test_scheduler_matches_reference_lr_sequences(golden):
    from baselines_amd.a2c.utils import Scheduler, schedules
    keys = [k for k in golden.files if k.startswith('lr/')]
    assert {k.split('/')[1] for k in keys} == set(schedules) == {
        'linear', 'constant', 'double_linear_con', 'middle_drop', 'double_middle_drop'}
    for k in keys:
        _, name, pair = k.split('/')
        nbatch, total = (int(x) for x in pair.split('_'))
        s_calls, s_adv = Scheduler(7e-4, total, name), Scheduler(7e-4, total, name)
        seq_calls, seq_adv, seq_formula = [], [], []
        for u in range(1, total // nbatch + 1):
            for _ in range(nbatch):
                v = s_calls.value()
            seq_calls.append(v)
            seq_adv.append(s_adv.advance(nbatch))
            seq_formula.append(7e-4 * schedules[name]((u * nbatch - 1) / total))
        ref = golden[k]
        assert np.array_equal(np.array(seq_calls), ref), k
        assert np.array_equal(np.array(seq_adv), ref), k
        assert np.array_equal(np.array(seq_formula), ref), k


def test_returns_restatement_matches_reference_runner(golden):
    signed_zeros = 0
    for name in golden['cases']:
        g = lambda k: golden['%s/%s' % (name, k)]
        out = nstep_returns(g('in_rewards'), g('in_dones'), g('in_last_values'), g('in_last_dones'), float(g('gamma')))
        T, N = out.shape
        ref = g('out_returns')                                 # env-major [N*T]
        got = out.swapaxes(0, 1).reshape(-1)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), name
        np.testing.assert_array_equal(g('out_masks'), g('in_dones').astype(bool).swapaxes(0, 1).reshape(-1))
        signed_zeros += int(np.sum(ref.view(np.uint32) == np.uint32(0x80000000)))
    assert signed_zeros > 0, 'the golden should exercise -0.0 returns'


def _tensors():
    # (name, shape, offset, size) of a tiny 2-variable model, names under a2c_model/
    return [('a2c_model/pi/w', (3, 2), 0, 6), ('a2c_model/pi/b', (2,), 6, 2)]


def test_checkpoint_dict_format():
    from baselines_amd.a2c.a2c import checkpoint_to_flat
    w, b = np.arange(6, dtype=np.float32).reshape(3, 2), np.array([7, 8], np.float32)
    d = {'a2c_model/pi/w:0': w, 'a2c_model/pi/b:0': b,
         'a2c_model/pi/w/RMSProp:0': w + 10, 'a2c_model/pi/b/RMSProp:0': b + 10,
         'a2c_model/pi/w/RMSProp_1:0': w + 20, 'a2c_model/pi/b/RMSProp_1:0': b + 20}
    out = checkpoint_to_flat(d, _tensors())
    assert [o for o, _ in out['params']] == [0, 6]
    np.testing.assert_array_equal(out['params'][0][1], w.reshape(-1))
    np.testing.assert_array_equal(out['ms'][1][1], b + 10)
    np.testing.assert_array_equal(out['mom'][0][1], (w + 20).reshape(-1))
    # parameters only: slots untouched
    out = checkpoint_to_flat({'a2c_model/pi/w:0': w, 'a2c_model/pi/b:0': b}, _tensors())
    assert out['ms'] == [] and out['mom'] == []
    with pytest.raises(KeyError):
        checkpoint_to_flat({'ppo2_model/pi/w:0': w, 'ppo2_model/pi/b:0': b}, _tensors())
    with pytest.raises(ValueError):
        checkpoint_to_flat({'a2c_model/pi/w:0': w.T, 'a2c_model/pi/b:0': b}, _tensors())


def test_checkpoint_legacy_list_format():
    from baselines_amd.a2c.a2c import checkpoint_to_flat
    w, b = np.arange(6, dtype=np.float32).reshape(3, 2), np.array([7, 8], np.float32)
    # n model variables, then (ms, momentum) for each variable in turn
    out = checkpoint_to_flat([w, b, w + 1, w + 2, b + 1, b + 2], _tensors())
    np.testing.assert_array_equal(out['ms'][0][1], (w + 1).reshape(-1))
    np.testing.assert_array_equal(out['mom'][0][1], (w + 2).reshape(-1))
    np.testing.assert_array_equal(out['ms'][1][1], b + 1)
    np.testing.assert_array_equal(out['mom'][1][1], b + 2)
    out = checkpoint_to_flat([w, b], _tensors())
    np.testing.assert_array_equal(out['params'][1][1], b)
    for bad in ([w], [w, b, w], [w, b, w, w, b, b, b], [w, b, 1.0, 1.0, w, w, b, b]):
        with pytest.raises(ValueError, match='number of variables loaded mismatches len\\(variables\\)'):
            checkpoint_to_flat(bad, _tensors())
