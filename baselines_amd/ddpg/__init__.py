from .ddpg import learn  # noqa: F401
from .ddpg_learner import DDPG  # noqa: F401
from .memory import Memory, RingBuffer  # noqa: F401
from .models import Actor, Critic  # noqa: F401
from .noise import AdaptiveParamNoiseSpec, NormalActionNoise, OrnsteinUhlenbeckActionNoise  # noqa: F401
