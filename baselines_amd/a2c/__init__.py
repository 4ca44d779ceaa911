from .a2c import Model, learn   # noqa: F401
from .runner import Runner   # noqa: F401
from .utils import Scheduler, schedules   # noqa: F401
