"""A few `q-learning` steps of the default `atari-dqn` policy (hidden_dim 512, 18 actions) on one synthetic sample of 64
environments x 44 steps (chunk_len 40, bootstrap_steps 4), for a kernel trace:

    rocprofv3 --kernel-trace --stats -d <out> -- python scripts/dqn_step_profile.py

Prints the wall time of the last step (host clock around a synchronised step: a single measurement)."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import srl_amd
from srl_amd.algorithm.dqn_policy import DQNPolicyState
from srl_amd.api import config, trainer as trainer_api
from srl_amd.api.env_utils import DiscreteAction
from srl_amd.api.trainer import SampleBatch
from srl_amd.namedarray import NamedArray
from srl_amd.runtime import synthetic

srl_amd.register_all()
B, TB, N_BOOT, ACT = 64, 44, 4, 18
a = synthetic.make_sample_arrays(seed=0, T=TB - N_BOOT, B=B, obs_spec=synthetic.ATARI_OBS, action_dims=ACT, bootstrap_steps=N_BOOT)
sample = SampleBatch(obs=NamedArray(obs=a["obs.obs"]), policy_state=DQNPolicyState(hx=None, epsilon=np.full((TB, B, 1), 0.1, np.float32)),
                     on_reset=a["on_reset"], done=a["done"], truncated=a["truncated"], action=DiscreteAction(a["action.x"]),
                     reward=a["reward"], info_mask=a["info_mask"])
trainer = trainer_api.make(config.Trainer("q-learning", args=dict(bootstrap_steps=N_BOOT, use_soft_update=True)),
                           config.Policy("atari-dqn", args=dict(act_dim=ACT, dueling=True)))
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
for i in range(steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = trainer.step(sample)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
print(f"q-learning step, {B} x {TB}: {dt * 1e3:.2f} ms (host clock, last of {steps}); value_loss {res.stats['value_loss']:.5f}")
