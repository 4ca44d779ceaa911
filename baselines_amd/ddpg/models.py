"""Actor and critic of DDPG (ddpg/models.py) as flat f32 parameter layouts in TF variable-creation order.

    actor/mlp_fc0/w, actor/mlp_fc0/b, [actor/LayerNorm/beta, actor/LayerNorm/gamma], actor/mlp_fc1/w, ...,
    actor/dense/kernel, actor/dense/bias                  (Actor: mlp -> dense(nb_actions) -> tanh)
    critic/mlp_fc0/w, ..., critic/output/kernel, critic/output/bias    (Critic: mlp(concat([obs, action])) -> dense(1))

The same layout is what the HIP kernels index (include/mrl.h, mrl_ddpg_desc).  Initialisation: the mlp body with the
project's orthogonal init (scale sqrt(2), biases zero, LayerNorm beta 0 / gamma 1), the final layer's kernel from
uniform(-3e-3, 3e-3) and its bias zero.  The reference draws all of these from TF's generator, which cannot be reproduced
outside TF; here they come from the seeded global NumPy stream (actor first, then critic, each in creation order), so
`set_global_seeds(seed)` makes a run repeatable."""
import numpy as np

from ..common.models import NetworkDesc, get_network_builder
from ..ppo2.model import ortho_init


def network_desc(network, **network_kwargs):
    desc = get_network_builder(network)(**network_kwargs)
    if not isinstance(desc, NetworkDesc) or desc.kind != 'mlp':
        raise NotImplementedError('DDPG on the device path supports network="mlp" only, got {!r}'.format(network))
    return desc


class Model(object):
    def __init__(self, name, network='mlp', **network_kwargs):
        self.name = name
        self.network = network
        self.network_kwargs = network_kwargs
        self.desc = network_desc(network, **network_kwargs)
        self.num_layers = self.desc.kw['num_layers']
        self.num_hidden = self.desc.kw['num_hidden']
        self.activation = self.desc.kw['activation']
        self.layer_norm = self.desc.kw['layer_norm']

    def _layout(self, nin, nout, final):
        """[(name, shape, offset, init)] with init in 'ortho', 'zeros', 'ones', 'uniform'"""
        out = []
        off = 0
        k = nin
        for i in range(self.num_layers):
            for suffix, shape, init in (('mlp_fc%d/w' % i, (k, self.num_hidden), 'ortho'), ('mlp_fc%d/b' % i, (self.num_hidden,), 'zeros')):
                out.append(('%s/%s' % (self.name, suffix), shape, off, init))
                off += int(np.prod(shape))
            if self.layer_norm:
                ln = 'LayerNorm' if i == 0 else 'LayerNorm_%d' % i
                for suffix, init in (('beta', 'zeros'), ('gamma', 'ones')):
                    out.append(('%s/%s/%s' % (self.name, ln, suffix), (self.num_hidden,), off, init))
                    off += self.num_hidden
            k = self.num_hidden
        out.append(('%s/%s/kernel' % (self.name, final), (k, nout), off, 'uniform'))
        off += k * nout
        out.append(('%s/%s/bias' % (self.name, final), (nout,), off, 'zeros'))
        return out

    @property
    def vars(self):
        return [t[0] for t in self.tensors]

    @property
    def trainable_vars(self):
        return self.vars

    @property
    def perturbable_vars(self):
        return [v for v in self.trainable_vars if 'LayerNorm' not in v]

    @property
    def num_params(self):
        t = self.tensors[-1]
        return t[2] + int(np.prod(t[1]))

    def init_params(self):
        """flat f32 initial parameters, drawn in creation order from the global NumPy stream"""
        flat = np.zeros(self.num_params, np.float32)
        for name, shape, off, init in self.tensors:
            n = int(np.prod(shape))
            if init == 'ortho':
                flat[off:off + n] = ortho_init(shape, np.sqrt(2)).reshape(-1)
            elif init == 'ones':
                flat[off:off + n] = 1.0
            elif init == 'uniform':
                flat[off:off + n] = np.random.uniform(-3e-3, 3e-3, size=shape).astype(np.float32).reshape(-1)
        return flat

    def unflatten(self, flat):
        """{variable name: array} view of a flat parameter vector (host NumPy)"""
        flat = np.asarray(flat)
        return {name: flat[off:off + int(np.prod(shape))].reshape(shape) for name, shape, off, _ in self.tensors}


class Actor(Model):
    def __init__(self, nb_actions, name='actor', network='mlp', **network_kwargs):
        super().__init__(name=name, network=network, **network_kwargs)
        self.nb_actions = nb_actions
        self.ob_dim = None

    def build(self, ob_dim):
        self.ob_dim = int(ob_dim)
        self.tensors = self._layout(self.ob_dim, self.nb_actions, 'dense')
        return self


class Critic(Model):
    def __init__(self, name='critic', network='mlp', **network_kwargs):
        super().__init__(name=name, network=network, **network_kwargs)
        self.ob_dim = self.nb_actions = None

    def build(self, ob_dim, nb_actions):
        self.ob_dim, self.nb_actions = int(ob_dim), int(nb_actions)
        self.tensors = self._layout(self.ob_dim + self.nb_actions, 1, 'output')
        return self

    @property
    def output_vars(self):
        return [v for v in self.trainable_vars if 'output' in v]
