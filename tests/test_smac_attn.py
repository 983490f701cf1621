"""CPU checks of the agent-specific (attention) SMAC encoders: parameter table and initial values against the reference
(tests/golden/gen_smac_attn.py), and what the constructor refuses."""
import numpy as np
import pytest
import torch

import srl_amd
from smac_attn_cases import H, MIXED_POLICY, OBS, POLICY, STATE, state_dict, unpack
from srl_amd.algorithm import netspec as ns
from srl_amd.api import config, policy as policy_api

srl_amd.register_all()


def test_attention_param_table_and_init(golden):
    g = golden("steps_smac_attn.npz")
    spec, vals = ns.build_smac_netspec(dict(OBS), dict(STATE), 9, H, seed=31)
    ref = unpack(g, "init")
    assert [k for k in vals if "_RunningMeanStd__" not in k] == list(ref)  # the reference's state_dict order
    assert len(vals) == 79 and sum(v.numel() for v in vals.values()) == 23217
    for k, v in ref.items():
        assert tuple(vals[k].shape) == v.shape and np.allclose(vals[k].numpy(), v, rtol=1e-4, atol=1e-4), k
    enc = spec.obs_encoders[0]
    kinds = [type(L).__name__ for L in enc.layers]
    assert kinds == ["EntityAttnSpec", "LayerNormSpec", "LinearSpec", "LayerNormSpec"] and enc.out_dim == H
    A = enc.layers[0]
    assert [k for k, _, _ in A.keys] == ["obs_allies", "obs_enemies", "obs_move"] and A.entities == 6 and A.dim == H // 2
    assert spec.state_encoders[0].layers[0].keys == [("state_allies", 2, 8), ("state_enemies", 3, 7), ("state_move", 1, 4)]


def test_mixed_sides_param_table_and_init(golden):
    g = golden("steps_smac_attn.npz")
    spec, vals = ns.build_smac_netspec(dict(OBS), 11, 9, H, seed=31)
    ref = unpack(g, "mixed_init")
    assert [k for k in vals if "_RunningMeanStd__" not in k] == list(ref)
    for k, v in ref.items():
        assert np.allclose(vals[k].numpy(), v, rtol=1e-4, atol=1e-4), k
    assert type(spec.state_encoders[0].layers[0]).__name__ == "LayerNormSpec"


def test_flat_call_is_unchanged(golden):
    g = golden("steps_smac.npz")
    spec, vals = ns.build_smac_netspec(30, 48, 9, 32, seed=31)
    assert [type(L).__name__ for L in spec.obs_encoders[0].layers] == ["LayerNormSpec", "LinearSpec", "LayerNormSpec", "LinearSpec",
                                                                        "LayerNormSpec"]
    assert spec.obs_encoders[0].shape == 30 and spec.state_encoders[0].shape == 48
    for k, v in vals.items():
        assert np.array_equal(v.numpy(), g[f"smac_init_param:{k}"]), k   # bit for bit what the flat builder gave before


def test_policy_constructs_and_checkpoints_under_reference_names(golden):
    g = golden("steps_smac_attn.npz")
    pol = policy_api.make(config.Policy("smac_rnn", args=POLICY))
    sd = pol.get_checkpoint()["state_dict"]
    want = state_dict(g, "init")
    assert set(sd) == set(want) and "actor_base.encoder.attn.k_linear.bias" in sd and "critic_base.state_move_norm.weight" in sd
    for k, v in sd.items():
        assert np.allclose(v.numpy(), want[k], rtol=1e-4, atol=1e-4), k
    assert pol.default_policy_state.actor_hx.shape == (3, 1, 2 * H)
    mixed = policy_api.make(config.Policy("smac_rnn", args=MIXED_POLICY))
    assert "critic_base.1.0.weight" in mixed.get_checkpoint()["state_dict"]


def test_what_the_constructor_refuses():
    make = lambda **kw: policy_api.make(config.Policy("smac_rnn", args=dict(POLICY, **kw)))
    with pytest.raises(NotImplementedError, match="ordered dict"):  # a map name gives flat widths only
        policy_api.make(config.Policy("smac_rnn", args=dict(map_name="3m", agent_specific_obs=True)))
    with pytest.raises(NotImplementedError, match="ordered dict"):
        policy_api.make(config.Policy("smac_rnn", args=dict(map_name="3m", agent_specific_state=True)))
    with pytest.raises(NotImplementedError):  # E = 65
        make(obs_shape=dict(obs_allies=(32, 5), obs_enemies=(33, 6), obs_self=(7,), obs_mask=(65,)))
    with pytest.raises(NotImplementedError):  # features per entity
        make(obs_shape=dict(OBS, obs_enemies=(3, 65)))
    with pytest.raises(NotImplementedError):  # D = 24
        make(hidden_dim=48)
    with pytest.raises(NotImplementedError):  # an entity leaf the reference has no LayerNorm for
        make(obs_shape=dict(OBS, obs_neutral=(1, 4), obs_mask=(7,)))
    with pytest.raises(ValueError):  # the mask does not cover the entities
        make(obs_shape=dict(OBS, obs_mask=(7,)))
    with pytest.raises(ValueError):  # a dict without the flag
        make(agent_specific_obs=False)
    for D, S, keys in ((16, 7, [(2, 5), (3, 6), (1, 4)]), (32, 128, [(31, 64), (32, 64), (1, 64)]), (64, 128, [(63, 64), (1, 64)]),
                       (64, 40, [(31, 4), (32, 4), (1, 4)])):
        assert srl_amd.hip.entity_attn_supported(D, S, keys), (D, S, keys)


def test_block_announces_every_parameter_it_owns():
    """What the block's backward releases to the data-parallel bucket reducer (one prefix per weight / bias pair) is exactly the
    set of parameters in front of the dense tail: a bucket holding one of them must not close before that launch."""
    spec, _ = ns.build_smac_netspec(dict(OBS), dict(STATE), 9, H)
    for root, enc in (("actor_base", spec.obs_encoders[0]), ("critic_base", spec.state_encoders[0])):
        own = {n.rsplit(".", 1)[0] for n in spec.params if n.startswith(root + ".") and ".encoder.dense." not in n}
        assert set(enc.layers[0].prefixes) == own and len(own) == 12
