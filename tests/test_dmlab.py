"""CPU checks of the ``dmlab`` policy: parameter table and initial values against the reference (tests/golden/gen_dmlab.py), the
checkpoint round trip under its names, the policy-state shapes, what the constructor refuses, and that the builders every other
policy uses give what they gave before."""
import numpy as np
import pytest
import torch

import srl_amd
from dmlab_cases import ACT, GRU_POLICY, HID, NORNN_POLICY, OBS, POLICY, make_sample, popart_after, rollout_request, state_after, state_dict, unpack
from srl_amd import hip
from srl_amd.algorithm import netspec as ns
from srl_amd.api import config, policy as policy_api, trainer as trainer_api

srl_amd.register_all()

NAMES = (["word_embedding.weight"] + [f"instructions_lstm.{k}_l0" for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")] +
         [f"pixel_encoder.{i}.{k}" for i in (0, 2, 5) for k in ("weight", "bias")] +
         [f"rnn._AutoResetRNN__net.{k}_l0" for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")] +
         ["actor_head.weight", "actor_head.bias", "critic_head._PopArtValueHead__weight", "critic_head._PopArtValueHead__bias"])


def make(**kw):
    return policy_api.make(config.Policy("dmlab", args=dict(POLICY, **kw)))


def test_param_table_and_init_equal_the_reference(golden):
    g = golden("steps_dmlab.npz")
    spec, vals = ns.build_dmlab_netspec(OBS, ACT, HID, seed=31)
    ref = unpack(g, "init")
    assert list(ref) == NAMES and [k for k in vals if "_RunningMeanStd__" not in k] == NAMES   # the reference's state_dict order
    assert sum(v.size for v in ref.values()) == 99034
    for k, v in ref.items():
        assert tuple(vals[k].shape) == v.shape and np.allclose(vals[k].numpy(), v, rtol=1e-4, atol=1e-4), k
    assert not vals["word_embedding.weight"][0].any() and vals["word_embedding.weight"][1:].std() > 0.9   # N(0, 1), row 0 zeroed
    px, instr = spec.obs_encoders
    assert [type(L).__name__ for L in px.layers] == ["ObsScaleSpec", "ConvSpec", "ConvSpec", "LinearSpec"] and px.out_dim == HID
    assert px.layers[1].out_hw == (8, 10) and px.layers[2].out_hw == (3, 4) and px.layers[3].in_features == 384 and px.layers[3].act == 0
    assert [type(L).__name__ for L in instr.layers] == ["InstrLstmSpec"] and instr.out_dim == 64
    core = spec.actor_backbone
    assert len(core) == 1 and core[0].kind == "lstm" and core[0].input_dim == HID + 64 and core[0].hidden == HID // 2   # no rnn_norm
    assert spec.actor_head.in_features == spec.critic_head.in_features == HID // 2 and spec.shared_backbone
    assert set(instr.layers[0].prefixes) == {n.rsplit(".", 1)[0] for n in NAMES[:5]}   # what the block's backward releases
    # the variants: a GRU core, no core at all
    gspec, gvals = ns.build_dmlab_netspec(OBS, ACT, 32, rnn_type="gru", seed=31)
    assert gspec.actor_backbone[0].kind == "gru" and tuple(gvals["rnn._AutoResetRNN__net.weight_ih_l0"].shape) == (48, 96)
    nspec, nvals = ns.build_dmlab_netspec(OBS, ACT, HID, num_rnn_layers=0, seed=31)
    assert not nspec.actor_backbone and tuple(nvals["actor_head.weight"].shape) == (ACT, HID + 64) and nspec.rnn_state_width == 0
    plain, pvals = ns.build_dmlab_netspec(OBS, ACT, HID, popart=False, seed=31)
    assert "critic_head.weight" in pvals and not plain.popart


def test_checkpoint_round_trips_under_the_reference_names(golden):
    g = golden("steps_dmlab.npz")
    pol = make()
    sd = pol.get_checkpoint()["state_dict"]
    want = state_dict(g, "init")
    assert list(sd) == list(want)   # PopArt's float64 statistics behind the head's weight and bias, as in the module
    for k, v in sd.items():
        assert np.allclose(v.numpy(), want[k], rtol=1e-4, atol=1e-4), k
    trained, _ = state_after(g, 1)
    load = {k: torch.from_numpy(v.astype(np.float32)) for k, v in trained.items()}
    load.update({k: torch.from_numpy(v) for k, v in popart_after(g, 1).items()})
    other = make(seed=5)
    other.load_checkpoint({"steps": 2, "state_dict": load})
    back = other.get_checkpoint()
    assert back["steps"] == 2 and list(back["state_dict"]) == list(want)
    for k, v in load.items():
        assert back["state_dict"][k].dtype == v.dtype and np.array_equal(back["state_dict"][k].numpy(), v.numpy()), k
    assert back["state_dict"]["critic_head._PopArtValueHead__rms._RunningMeanStd__mean"].dtype == torch.float64
    with pytest.raises(KeyError):
        other.load_checkpoint({"steps": 0, "state_dict": {k: v for k, v in load.items() if k != "word_embedding.weight"}})


def test_default_policy_state_shapes():
    assert make().default_policy_state.hx.shape == (1, HID) and make().default_policy_state.hx.dtype == np.float32
    assert make(num_rnn_layers=2).default_policy_state.hx.shape == (2, HID)
    assert policy_api.make(config.Policy("dmlab", args=GRU_POLICY)).default_policy_state.hx.shape == (1, 16)
    assert policy_api.make(config.Policy("dmlab", args=NORNN_POLICY)).default_policy_state is None
    big = policy_api.make(config.Policy("dmlab", args=dict(obs_shapes={"obs": (3, 72, 96), "INSTR": (16,)}, action_dim=15)))
    assert big.default_policy_state.hx.shape == (1, 512) and big._chunk_len == 10 and big._popart_beta == 0.99999   # the defaults
    assert make(popart_beta=0.999)._popart_beta == 0.999   # reaches PopArt's update


def test_what_the_constructor_refuses():
    with pytest.raises(NotImplementedError, match="num_dense_layers"):
        make(num_dense_layers=1)
    with pytest.raises(NotImplementedError, match="gtrxl"):
        make(rnn_type="gtrxl")
    with pytest.raises(ValueError, match="Unknown rnn_type"):
        make(rnn_type="rnn")
    with pytest.raises(NotImplementedError, match="Activation"):
        make(activation="elu")
    with pytest.raises(NotImplementedError, match="language encoder"):
        make(obs_shapes=dict(OBS, INSTR=(65,)))
    with pytest.raises(NotImplementedError, match="language encoder"):
        make(embedding_size=33)
    with pytest.raises(NotImplementedError, match="language encoder"):
        make(instrunctions_lstm_units=48)
    for V, Ed, H, L in ((65536, 32, 64, 64), (1000, 20, 64, 16), (1, 1, 32, 1), (30, 8, 32, 9)):
        assert hip.instr_lstm_supported(V, Ed, H, L), (V, Ed, H, L)
    for V, Ed, H, L in ((65537, 20, 64, 6), (1000, 0, 64, 6), (1000, 20, 128, 6), (1000, 20, 64, 0)):
        assert not hip.instr_lstm_supported(V, Ed, H, L), (V, Ed, H, L)


def test_recurrent_actor_critic_builder_is_unchanged(golden):
    """``GruSpec.in_dim`` defaults to the hidden width: ``build_netspec`` of the recurrent ``actor-critic`` configurations of
    tests/test_gpu_trainer.py gives the reference's initial values bit for bit, as before."""
    g = golden("steps_rnn.npz")
    for tag, pargs in (("gru", dict(obs_dim=4, action_dim=2, hidden_dim=32, num_dense_layers=1, num_rnn_layers=1, popart=False,
                                     layernorm=True, shared_backbone=True, seed=21)),
                       ("gru2", dict(obs_dim=4, action_dim=[3, 2], hidden_dim=16, num_dense_layers=2, num_rnn_layers=2, popart=True,
                                      layernorm=False, shared_backbone=False, seed=22))):
        spec, vals = ns.build_netspec(**pargs)
        keys = [k for k in g.files if k.startswith(f"{tag}_init_param:")]
        assert len(keys) == len(vals)
        for k in keys:
            assert np.array_equal(vals[k[len(tag) + 12:]].numpy(), g[k]), k
        rnn = [L for L in spec.actor_backbone if isinstance(L, ns.GruSpec)]
        assert len(rnn) == 1 and rnn[0].in_dim == 0 and rnn[0].input_dim == rnn[0].hidden == pargs["hidden_dim"]


def test_step_and_rollout_need_a_gpu(golden, monkeypatch):
    """No CPU fall-back: without a device (here: with none visible to ``hip.require_gpu``) both raise."""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    g = golden("steps_dmlab.npz")
    trainer = trainer_api.make(config.Trainer("mappo", args=dict(popart=True)), config.Policy("dmlab", args=POLICY))
    with pytest.raises(hip.HipError):
        trainer.step(make_sample(g, 0)[0])
    with pytest.raises(hip.HipError):
        trainer.policy.rollout(rollout_request(g)[0])
