"""``FlatOptimizer`` (srl_amd/algorithm/optim.py) on the host: torch's ``state_dict`` layout in both directions for every
optimiser kind, against ``torch.optim`` itself (what the reference checkpoints, mappo.py:58-66), the refusal of a state of
another kind, and the config parser's refusals.  No kernel runs: trainers are built on ``device="cpu"``."""
import copy

import pytest
import torch

import srl_amd
from srl_amd.api import config, trainer as trainer_api

srl_amd.register_all()

PARGS = dict(obs_dim=4, action_dim=2, hidden_dim=8, num_dense_layers=1, num_rnn_layers=0, popart=True, seed=1, device="cpu")
TORCH = dict(adam=torch.optim.Adam, adamw=torch.optim.AdamW, rmsprop=torch.optim.RMSprop, sgd=torch.optim.SGD)
# (optimiser, optimizer_config, optimizer.steps after loading torch's state of 3 steps): SGD keeps no step count -- a momentum
# buffer means "not the first step", and without momentum it has no state at all
CASES = [("adam", dict(lr=1e-3), 3), ("adamw", dict(lr=1e-3), 3), ("rmsprop", dict(lr=1e-3, momentum=0.9, centered=True), 3),
         ("rmsprop", dict(lr=1e-3), 3), ("sgd", dict(lr=1e-2, momentum=0.9, nesterov=True), 1), ("sgd", dict(lr=1e-2), 0)]


def make(kind="mappo", policy="actor-critic", **targs):
    return trainer_api.make(config.Trainer(kind, args=dict(popart=True, **targs)), config.Policy(policy, args=PARGS))


def torch_params(trainer):
    """Parameters of the reference's shapes in its order, then the three gradient-less PopArt statistics."""
    sd = trainer.policy.get_checkpoint()["state_dict"]
    names = trainer.policy.net.ref_names()
    return names, ([torch.nn.Parameter(sd[n].clone().float()) for n in names] +
                   [torch.nn.Parameter(torch.zeros(1), requires_grad=False) for _ in range(3)])


def torch_optimizer(trainer, name, cfg, steps=3):
    names, params = torch_params(trainer)
    opt = TORCH[name](params, **cfg)
    gen = torch.Generator().manual_seed(3)
    for _ in range(steps):
        for p in params[:len(names)]:
            p.grad = torch.randn(p.shape, generator=gen)
        opt.step()
    return opt, params


@pytest.mark.parametrize("name,cfg,steps", CASES, ids=[f"{n}-{'-'.join(c)}" for n, c, _ in CASES])
def test_state_dict_roundtrip_against_torch(name, cfg, steps):
    trainer = make(optimizer=name, optimizer_config=cfg)
    topt, tparams = torch_optimizer(trainer, name, cfg)
    ckpt = trainer.get_checkpoint()
    assert ckpt["optimizer_state_dict"]["state"] == {}   # empty before the first step
    trainer.load_checkpoint(dict(ckpt, optimizer_state_dict=copy.deepcopy(topt.state_dict())))
    assert trainer.optimizer.steps == steps
    ours = trainer.get_checkpoint()["optimizer_state_dict"]
    _, fresh_params = torch_params(trainer)
    fresh = TORCH[name](fresh_params, **cfg)
    fresh.load_state_dict(copy.deepcopy(ours))   # torch accepts ours
    theirs = topt.state_dict()
    assert ours["param_groups"][0]["params"] == theirs["param_groups"][0]["params"]
    assert set(ours["state"]) == set(theirs["state"])
    for i, want in theirs["state"].items():
        assert set(ours["state"][i]) == set(want), i
        for k, t in want.items():
            if k != "step":
                assert torch.equal(ours["state"][i][k], t), (i, k)


def snapshot(opt):
    return opt.m.clone(), opt.v.clone(), opt.steps, opt.lr, opt.betas


def assert_untouched(opt, before):
    m, v, steps, lr, betas = before
    assert torch.equal(opt.m, m) and torch.equal(opt.v, v) and float(m.abs().sum()) > 0 and float(v.abs().sum()) > 0
    assert opt.steps == steps == 3 and opt.lr == lr and opt.betas == betas


def test_refused_state_leaves_the_optimizer_untouched():
    trainer = make(optimizer="adam", optimizer_config=dict(lr=2.5e-4, betas=(0.8, 0.95)))
    ckpt = trainer.get_checkpoint()
    topt, _ = torch_optimizer(trainer, "adam", dict(lr=5e-4, betas=(0.7, 0.9)))
    trainer.load_checkpoint(dict(ckpt, optimizer_state_dict=topt.state_dict()))
    before = snapshot(trainer.optimizer)
    assert before[3:] == (5e-4, (0.7, 0.9))
    foreign, _ = torch_optimizer(trainer, "rmsprop", dict(lr=1e-3, momentum=0.9, centered=True), steps=5)
    with pytest.raises(ValueError, match="optimizer_state_dict is not a `adam` state"):
        trainer.load_checkpoint(dict(ckpt, optimizer_state_dict=foreign.state_dict()))
    assert_untouched(trainer.optimizer, before)


def test_refused_aux_state_leaves_the_aux_optimizer_untouched():
    trainer = make("mappg", "actor-critic-auxiliary", ppg_optimizer_config=dict(lr=2.5e-4))
    ckpt = trainer.get_checkpoint()
    topt, _ = torch_optimizer(trainer, "adam", dict(lr=5e-4, betas=(0.7, 0.9)))
    trainer.load_checkpoint(dict(ckpt, aux_optimizer_state_dict=topt.state_dict()))
    before = snapshot(trainer.aux_optimizer)
    assert before[3:] == (5e-4, (0.7, 0.9))
    foreign, _ = torch_optimizer(trainer, "rmsprop", dict(lr=1e-3, momentum=0.9, centered=True), steps=5)
    with pytest.raises(ValueError, match="aux_optimizer_state_dict is not a `adam` state"):
        trainer.load_checkpoint(dict(ckpt, aux_optimizer_state_dict=foreign.state_dict()))
    assert_untouched(trainer.aux_optimizer, before)


def test_unknown_config_entries_are_refused_by_name():
    with pytest.raises(NotImplementedError, match=r"unsupported optimizer_config entries: \['amsgrad'\]"):
        make(optimizer_config=dict(lr=1e-3, amsgrad=True))
    with pytest.raises(NotImplementedError, match=r"unsupported optimizer_config entries: \['momentum'\]"):
        make(optimizer_config=dict(momentum=0.9))   # (another kind's entry)
    with pytest.raises(NotImplementedError, match=r"unsupported ppg_optimizer_config entries: \['amsgrad'\]"):
        make("mappg", "actor-critic-auxiliary", ppg_optimizer_config=dict(amsgrad=True))
    # torch's no-op flags, switched off, are tolerated by both
    make(optimizer_config=dict(amsgrad=False, foreach=None))
    make("mappg", "actor-critic-auxiliary", ppg_optimizer_config=dict(amsgrad=False, fused=None))


def test_nesterov_needs_momentum():
    with pytest.raises(ValueError, match="Nesterov momentum requires a momentum and zero dampening"):
        make(optimizer="sgd", optimizer_config=dict(lr=1e-2, nesterov=True, momentum=0))
