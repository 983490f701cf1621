"""Shared by the agent-specific SMAC tests: the shapes of tests/golden/gen_smac_attn.py and readers of its packed arrays."""
from collections import OrderedDict

import numpy as np

from srl_amd.namedarray import NamedArray
from srl_amd.runtime import synthetic

H, A, CL, ACT = 32, 3, 5, 9
OBS = dict(obs_allies=(2, 5), obs_enemies=(3, 6), obs_move=(1, 4), obs_self=(7,), obs_mask=(6,))
STATE = dict(state_allies=(2, 8), state_enemies=(3, 7), state_move=(1, 4), state_self=(9,), state_mask=(6,))
POLICY = dict(hidden_dim=H, chunk_len=CL, seed=31, shared=True, agent_specific_obs=True, agent_specific_state=True,
              obs_shape=OBS, state_shape=STATE, act_dim=ACT, n_agents=A)
MIXED_POLICY = dict(POLICY, agent_specific_state=False, state_shape=(11,))
TRAINER = dict(popart=True, ppo_epochs=2, optimizer_config=dict(lr=5e-4, eps=1e-5), max_grad_norm=10.0,
               value_loss="huber", value_loss_config=dict(delta=10.0), clip_value=True, dual_clip=False)
SAMPLE = dict(T=10, B=2, agents=A, obs_spec={"local_obs": ((1,), "f32")}, action_dim=ACT, p_done=0.08,
              policy_state={"actor_hx": (1, 2 * H), "critic_hx": (1, 2 * H)})
BLOCKS = ("a", "b", "c", "d")


def unpack(g, key, f64=False):
    """name -> array of a dict stored by gen_smac_attn.pack; ``f64``: the float64 run's values instead."""
    out, off = OrderedDict(), 0
    flat = g[key + "_flat"]
    for i, (name, shp) in enumerate(zip(g[key + "_names"], g[key + "_shapes"])):
        n = int(shp[0]) * max(int(shp[1]), 1)
        v = flat[off:off + n].reshape((int(shp[0]), int(shp[1])) if shp[1] else (int(shp[0]),))
        if f64:
            v = v.astype(np.float64) + g[key + "_flat64d"][off:off + n].astype(np.float64).reshape(v.shape) * 2.0**-int(g[key + "_flat64e"][i])
        out[str(name)] = v
        off += n
    return out


def state_dict(g, key):
    """The float32 tensors of ``unpack`` and the float64 PopArt statistics stored beside them."""
    sd = dict(unpack(g, key))
    for k in g.files:
        if k.startswith(key + "_f64:"):
            sd[k[len(key) + 5:]] = g[k]
    return sd


def get64(g, key, base=None):
    """The float64 run's value of a quantity stored by gen_smac_attn.put64 (``base``: the name of its float32 array)."""
    return g[base or key].astype(np.float64) + g[key + "64d"].astype(np.float64) * 2.0**-int(g[key + "64e"])


def nested(flat):
    """{"local_obs.obs_self": x, ...} -> {"local_obs": NamedArray, "state": NamedArray}"""
    tree = {}
    for k, v in flat.items():
        top, leaf = k.split(".", 1)
        tree.setdefault(top, {})[leaf] = v
    return {k: NamedArray(**v) for k, v in tree.items()}


def make_sample(g, step, state=None):
    """The trainer sample of gen_smac_attn.make_arrays: flat leaves from synthetic, nested observation leaves from the file."""
    arrays = synthetic.make_multiagent_arrays(seed=400 + step, **SAMPLE)
    arrays.pop("obs.local_obs")
    sample = synthetic.to_sample_batch(arrays)
    pre = f"sample{step}.obs."
    tree = nested({k[len(pre):]: g[k] for k in g.files if k.startswith(pre)})
    if state is not None:
        tree["state"] = state
    sample.obs = NamedArray(available_action=arrays["obs.available_action"], is_alive=arrays["obs.is_alive"], **tree)
    return sample, arrays
