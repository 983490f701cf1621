"""Cases of the PopArt head-rescale fixtures (tests/golden/steps_popart_rescale.npz, gen_golden.py gen_popart_rescale), shared by
the generator, the oracle test and the GPU tests.

``burn_in`` / ``updates``: the head's burn-in and update count before the first step (``PopArtValueHead.__burn_in_updates`` /
``__update_cnt`` in the reference, ``burn_in_updates`` / ``popart_updates`` on the oracle's net, ``_popart_burn_in`` /
``_popart_updates`` on the policy).  ``reward_scale``: factor on the sample's rewards, per step.  PopArt's debiased statistics
are the plain average of the batches seen so far, so between equally distributed batches they hardly move and a rescale is a
factor within a few per cent of one (measured: the head's weight then ends 8e-4 / 1.6e-3 away from a run that never rescales,
parx / smacu); four times larger rewards in the second step move the standard deviation by ~20 % per update there, as a
drifting return scale does in training."""
import numpy as np

from srl_amd.runtime import synthetic

_C1 = dict(obs_dim=4, action_dim=2, hidden_dim=64, num_dense_layers=2, num_rnn_layers=0, popart=True, layernorm=False,
           shared_backbone=False, chunk_len=8)
_C1_SAMPLE = dict(T=32, B=8, obs_spec=synthetic.CARTPOLE_OBS, action_dims=2, p_done=0.05)

CASES = {
    # every update rescales, the first one from the all-zero statistics (std 0.1 -> the targets' own)
    "par0": dict(policy=dict(_C1, seed=7), trainer=dict(popart=True, optimizer_config=dict(lr=3e-4)), sample=_C1_SAMPLE,
                 n_steps=3, burn_in=0, updates=0, reward_scale=(1.0, 1.0, 1.0)),
    # updates 1-4 do not rescale, 5 and 6 do: the onset falls between the epochs of step 1
    "parx": dict(policy=dict(_C1, layernorm=True, shared_backbone=True, seed=8),
                 trainer=dict(popart=True, clip_value=True, dual_clip=False, value_loss='huber', value_loss_config=dict(delta=10.0),
                              value_loss_weight=1.0, ppo_epochs=3, optimizer_config=dict(lr=5e-4), max_grad_norm=40.0),
                 sample=_C1_SAMPLE, n_steps=2, burn_in=4, updates=0, reward_scale=(1.0, 4.0)),
}

# smac_rnn(unbiased_popart=True), the only public route to a finite burn-in (1000): updates 999 and 1000 do not rescale, 1001 and
# 1002 do.  Policy, trainer and sample are otherwise those of the plain SMAC fixture (tests/test_gpu_smac.py)
_H, _A = 32, 3
SMACU = dict(policy=dict(map_name="3m", hidden_dim=_H, chunk_len=5, seed=31, shared=True, unbiased_popart=True),
             trainer=dict(popart=True, ppo_epochs=2, optimizer_config=dict(lr=5e-4, eps=1e-5), max_grad_norm=10.0,
                          value_loss="huber", value_loss_config=dict(delta=10.0), clip_value=True, dual_clip=False),
             sample=dict(T=20, B=4, agents=_A, obs_spec={"local_obs": ((30,), "f32"), "state": ((48,), "f32")}, action_dim=9,
                         p_done=0.08, policy_state={"actor_hx": (1, 2 * _H), "critic_hx": (1, 2 * _H)}),
             n_steps=2, burn_in=1000, updates=998, reward_scale=(1.0, 4.0))


def scale_rewards(arrays, factor):
    """The sample with its rewards multiplied by ``factor`` (exact in float32 for the powers of two used here)."""
    if factor != 1.0:
        arrays["reward"] = arrays["reward"] * np.float32(factor)
    return arrays
