"""Learning-rate schedules of the A2C driver (a2c/utils.py:173-211), restated.

`Scheduler.value()` returns v * schedule(n / nvalues) and then advances n by one.  The reference's Model.train calls it once
per SAMPLE of the batch and keeps the last value (a2c.py:94-95), so update u (1-based) trains with
v * schedule((u * nbatch - 1) / nvalues); `advance(k)` is k calls to `value()` in O(1) (n stays an exactly represented
float-valued integer, so the result is the same number).
"""


def constant(p):
    return 1


def linear(p):
    return 1 - p


def middle_drop(p):
    # 1 - p until it falls below 0.75, then a tenth of that
    if 1 - p < 0.75:
        return 0.75 * 0.1
    return 1 - p


def double_linear_con(p):
    # twice as fast a linear decay, floored at 0.125
    p *= 2
    if 1 - p < 0.125:
        return 0.125
    return 1 - p


def double_middle_drop(p):
    # two drops: below 0.75 -> 0.075, below 0.25 -> 0.125
    if 1 - p < 0.75:
        if 1 - p < 0.25:
            return 0.25 * 0.5
        return 0.75 * 0.1
    return 1 - p


schedules = {
    'linear': linear,
    'constant': constant,
    'double_linear_con': double_linear_con,
    'middle_drop': middle_drop,
    'double_middle_drop': double_middle_drop,
}


class Scheduler(object):
    def __init__(self, v, nvalues, schedule):
        self.n = 0.
        self.v = v
        self.nvalues = nvalues
        self.schedule = schedules[schedule]

    def value(self):
        current_value = self.v * self.schedule(self.n / self.nvalues)
        self.n += 1.
        return current_value

    def advance(self, k):
        """the value of the last of k calls to value() (k >= 1)"""
        self.n += float(k - 1)
        return self.value()

    def value_steps(self, steps):
        return self.v * self.schedule(steps / self.nvalues)


def discount_with_dones(rewards, dones, gamma):
    """Host restatement of the returns recurrence (a2c/utils.py:147-153), Python floats: r = reward + gamma*r*(1 - done)
    from the back.  The device path is mrl_nstep_returns."""
    discounted = []
    r = 0
    for reward, done in zip(rewards[::-1], dones[::-1]):
        r = reward + gamma * r * (1. - done)
        discounted.append(r)
    return discounted[::-1]
