"""``FlatOptimizer``: torch.optim.{Adam, AdamW, RMSprop, SGD} on a ``HipNet``'s flat parameter buffer (``csrc/optim.hip``).

One owner for what a trainer keeps of its optimiser: the parsed config (reference ``modules/utils.py:268-286``:
``torch.optim.X(**optimizer_config)``), the state buffers on the flat layout, torch's ``state_dict`` layout in both directions
(``mappo.py:58-66`` checkpoints ``optimizer.state_dict()``), and the launch of one clipped step.  ``MultiAgentPPO.optimizer``
and ``MultiAgentPPG.aux_optimizer`` are instances.
"""
import numpy as np
import torch

from srl_amd import hip

# what a config may set and a param_group carries, with torch's defaults
_ADAM = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
_DEFAULTS = {'adam': _ADAM, 'adamw': dict(_ADAM, weight_decay=1e-2),
             'rmsprop': dict(lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0.0, momentum=0.0, centered=False),
             'sgd': dict(lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False)}
# what torch's param_group carries besides: switches that are off here
_GROUP_FLAGS = {'adam': dict(amsgrad=False, capturable=False, fused=None), 'adamw': dict(amsgrad=False, capturable=False, fused=None),
                'rmsprop': dict(capturable=False), 'sgd': dict(fused=None)}
# the group keys only that optimiser has: how a state_dict names its kind
_KIND_KEYS = {'adam': ("betas",), 'adamw': ("betas",), 'rmsprop': ("alpha", "centered"), 'sgd': ("dampening", "nesterov")}
# torch's per-parameter state key -> the buffer that holds it
_SLOTS = {'adam': (("exp_avg", "m"), ("exp_avg_sq", "v")), 'adamw': (("exp_avg", "m"), ("exp_avg_sq", "v")),
          'rmsprop': (("momentum_buffer", "m"), ("square_avg", "v"), ("grad_avg", "gavg")), 'sgd': (("momentum_buffer", "m"),)}


class FlatOptimizer:

    def __init__(self, net, name, config, config_name="optimizer_config"):
        if name not in _DEFAULTS:
            raise AssertionError(f"Optimizer name {name} does not match any implemented optimizers "
                                 "(['adam', 'rmsprop', 'sgd', 'adamw']).")
        cfg = dict(config)
        self.net, self.name = net, name
        for k, default in _DEFAULTS[name].items():  # self.lr, self.weight_decay, ...
            v = cfg.pop(k, default)
            setattr(self, k, type(default)(v) if isinstance(default, (tuple, bool)) else v)
        if name == 'sgd' and self.nesterov and (self.momentum <= 0 or self.dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")  # torch/optim/sgd.py
        for flag in ("amsgrad", "maximize", "capturable", "differentiable", "fused", "foreach"):
            if cfg.get(flag) in (None, False):
                cfg.pop(flag, None)
        if cfg:
            raise NotImplementedError(f"unsupported {config_name} entries: {sorted(cfg)}")
        self.m = torch.zeros_like(net.flat)
        self.v = torch.zeros_like(net.flat) if name != 'sgd' else None
        self.gavg = torch.zeros_like(net.flat) if name == 'rmsprop' and self.centered else None
        self.steps = 0

    def _momentum_buffer(self):
        """``m`` where it is a momentum buffer in use (RMSprop, SGD), else None."""
        return self.m if (self.momentum > 0 if self.name == 'rmsprop' else self.momentum != 0) else None

    # ------------------------------------------------------------------ torch's state_dict layout
    def state_dict(self):
        net = self.net
        names = net.ref_names()
        state = {}
        if self.steps > 0:
            held = [(slot, net.flat_to_reference(getattr(self, attr).detach().cpu())) for slot, attr in _SLOTS[self.name]
                    if getattr(self, attr) is not None and (slot != "momentum_buffer" or self._momentum_buffer() is not None)]
            for i, n in enumerate(names if held else ()):  # (SGD without momentum is stateless)
                state[i] = {} if self.name == 'sgd' else dict(step=torch.tensor(float(self.steps)))
                state[i].update((slot, named[n]) for slot, named in held)
        # the PopArt statistics are gradient-less nn.Parameters of the reference: listed, stateless
        params = list(range(len(names) + (3 if net.spec.popart else 0)))
        group = dict({k: getattr(self, k) for k in _DEFAULTS[self.name]}, **_GROUP_FLAGS[self.name], maximize=False, foreach=None,
                     differentiable=False, params=params)
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, osd, key="optimizer_state_dict"):
        """Everything is read from ``osd`` before anything is written: a state that is refused, or that turns out to be
        incomplete half-way, leaves buffers, hyper-parameters and the step count as they were."""
        st, grp = osd["state"], osd["param_groups"][0]
        # the group names its optimiser by the keys only that optimiser has (torch's load_state_dict would overwrite
        # the group and fail on foreign state; mappo.py:58-66): a checkpoint of another kind is refused, not zero-filled
        mine = _KIND_KEYS[self.name]
        foreign = [k for keys in _KIND_KEYS.values() if keys != mine for k in keys if k in grp]
        if foreign or any(k not in grp for k in mine):
            raise ValueError(f"{key} is not a `{self.name}` state (group keys {sorted(grp)})")
        hyper = dict(lr=grp["lr"], weight_decay=grp.get("weight_decay", self.weight_decay))
        if self.name in ('adam', 'adamw'):
            hyper.update(betas=tuple(grp["betas"]), eps=grp["eps"])
        elif self.name == 'rmsprop':
            hyper.update(alpha=grp["alpha"], eps=grp.get("eps", self.eps), momentum=grp.get("momentum", self.momentum),
                         centered=bool(grp["centered"]))
        else:
            hyper.update(momentum=grp.get("momentum", self.momentum), dampening=grp["dampening"], nesterov=bool(grp["nesterov"]))
        names = self.net.ref_names()
        first = st[0] if st else {}
        host = {}  # buffer -> its flat content, None: zeros
        for slot, attr in _SLOTS[self.name]:
            if attr == "gavg" and not hyper["centered"]:
                continue
            host[attr] = None
            if first.get(slot) is not None:
                host[attr] = self.net.reference_to_flat({n: st[i][slot] for i, n in enumerate(names)})
        # SGD keeps no step count: a restored momentum buffer means "not the first step"
        steps = 0 if not st else int(float(first["step"])) if "step" in first else 1

        vars(self).update(hyper)
        self.steps = steps
        if "gavg" not in host:
            self.gavg = None
        for attr, flat in host.items():
            buf = getattr(self, attr)
            if buf is None:  # `centered` re-bound from the group
                buf = self.gavg = torch.zeros_like(self.net.flat)
            buf.zero_() if flat is None else buf.copy_(flat)

    # ------------------------------------------------------------------ the step
    def bias_corrections(self, epochs):
        """Adam bias corrections of the next `epochs` optimiser steps, float32 [epochs, 2] (what srl_adam_step derives
        from its `step` argument, precomputed so that a captured launch carries no per-step scalar)."""
        (b1, b2), ts = self.betas, range(self.steps + 1, self.steps + epochs + 1)
        return np.asarray([[self.lr / (1.0 - b1**t), (1.0 - b2**t)**0.5] for t in ts], dtype=np.float32)

    def step(self, net, *, ahead, grad_scale, max_norm, sumsq, grad_norm_out, step_scalars=None):
        """One update of ``net.flat`` from ``net.grad``, the global-norm clip folded in.  ``steps`` is the caller's to advance,
        once per trainer step: a captured trainer step runs this while capturing and not at all on replay.  ``ahead``: the
        updates already launched since ``steps`` was last advanced."""
        clip = dict(grad_scale=grad_scale, max_norm=max_norm, sumsq=sumsq, grad_norm_out=grad_norm_out)
        if self.name in ('adam', 'adamw'):
            hip.adam_step(net.flat, net.grad, self.m, self.v, self.lr, self.betas[0], self.betas[1], self.eps, self.weight_decay,
                          self.name == 'adamw', self.steps + ahead + 1, step_scalars=step_scalars, **clip)
        elif self.name == 'rmsprop':
            hip.rmsprop_step(net.flat, net.grad, self.v, self._momentum_buffer(), self.gavg, self.lr, self.alpha, self.eps,
                             self.weight_decay, self.momentum, self.centered, **clip)
        else:
            hip.sgd_step(net.flat, net.grad, self._momentum_buffer(), self.lr, self.momentum, self.dampening, self.weight_decay,
                         self.nesterov, self.steps + ahead == 0, **clip)
