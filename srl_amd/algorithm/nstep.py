"""Actor-side n-step return, registered as trajectory post-processor ``"n-step-return"``.

Mirror of ``TrajNstepReturn`` (reference ``legacy/algorithm/modules/n_step_return.py:53-112``).  Like ``gae`` it runs in the actor
worker on one finished episode -- a list of per-step ``SampleBatch`` -- so it is plain numpy on the host; the reference's
``scipy.signal.lfilter`` with the taps ``[gamma^0 .. gamma^(n-1)]`` over the reversed rewards is the short loop below.  The batched
device-side return of the trainer is part of ``srl_dqn_td_fwd_bwd``.
"""
import numpy as np

from srl_amd.api import trainer as trainer_api
from srl_amd.namedarray import array_like


def scalar_transform(x, eps=1e-3):
    """modules/utils.py:324-328: float64 arithmetic, float32 result."""
    x = np.asarray(x, dtype=np.float64)
    return (np.sign(x) * (np.sqrt(np.abs(x) + 1) - 1) + eps * x).astype(np.float32)


def inverse_scalar_transform(x, eps=1e-3):
    """modules/utils.py:331-335."""
    x = np.asarray(x, dtype=np.float64)
    a = np.sqrt(1 + 4 * eps * (np.abs(x) + 1 + eps)) - 1
    return (np.sign(x) * (np.square(a / (2 * eps)) - 1)).astype(np.float32)


class TrajNstepReturn(trainer_api.TrajPostprocessor):

    def __init__(self, n: int, gamma: float, apply_scalar_transform: bool, scalar_transform_eps: float = 1e-3):
        self.n = n
        self.gamma = gamma
        self.apply_scalar_transform = apply_scalar_transform
        self.scalar_transform_eps = scalar_transform_eps

    def process(self, memory):
        last = memory[-1]
        assert np.all(last.done) or np.all(last.truncated)
        gamma, n, ep_len = self.gamma, self.n, len(memory)
        if last.analyzed_result is None:
            last.analyzed_result = array_like(memory[-2].analyzed_result, value=0)
        tail_value = last.analyzed_result.target_value
        if np.all(last.done):  # nothing to bootstrap from behind the episode's end
            pad = [np.zeros_like(memory[0].analyzed_result.target_value) for _ in range(n - 1)]
        else:  # truncated: the last value, so discounted that gamma^n of it is gamma^(steps to the end) (:79-83)
            pad = [tail_value / gamma**(i + 1) for i in range(n - 1)]
        bootstrap = np.array([x.analyzed_result.target_value for x in memory[n:]] + pad, dtype=np.float64)
        reward = np.array([x.reward for x in memory[:-1]], dtype=np.float64)
        assert reward.shape == bootstrap.shape, (n, ep_len, reward.shape, bootstrap.shape)
        if self.apply_scalar_transform:
            bootstrap = inverse_scalar_transform(bootstrap, self.scalar_transform_eps).astype(np.float64)
        ret = np.zeros_like(reward)
        for i in range(min(n, ep_len - 1)):  # ret[t] = sum_i gamma^i reward[t + i] over the steps the episode still has
            ret[:ep_len - 1 - i] += gamma**i * reward[i:]
        ret += gamma**n * bootstrap
        for i, m in enumerate(memory[:-1]):
            m.analyzed_result.ret = scalar_transform(ret[i], self.scalar_transform_eps) if self.apply_scalar_transform else ret[i]
        return memory


trainer_api.register_traj_postprocessor("n-step-return", TrajNstepReturn)
