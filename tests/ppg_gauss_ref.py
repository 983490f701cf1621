"""CPU restatement of Phasic Policy Gradient's auxiliary phase on Normal action heads (continuous actions), on PyTorch.

Restates ``legacy/algorithm/ppo/phasic_policy_gradient.py`` ``_compute_aux_loss`` (:262-280) with ``_policy_distance`` (:143-150)
for the ``[Normal(mean, std)]`` that ``get_action_distribution`` returns (actor_critic_policy.py:303-309), KL as
``torch.distributions.kl._kl_normal_normal`` in terms of log sigma, and with the reference's two defects on this path repaired as
tests/golden/gen_ppg_gauss.py does: the cached distribution is ``Normal(loc.detach(), scale.detach())`` (modules/utils.py:213
cannot execute), and every action dimension of a row is weighted by that row's ``1 - done``, summed over rows and dimensions and
divided by the number of undone rows (``_policy_distance`` as shipped multiplies ``[T, B, A]`` by ``[T, B]``).

One code for float32 (what the reference computes in) and float64 (the yardstick for rounding): ``dtype``.
"""
from typing import Dict, Optional

import numpy as np
import torch

from oracle.net import OracleActorCritic


def gauss_aux_loss(mean_old, log_std_old, mean, log_std, aux_value, pred_value, target, done, beta_clone=1.0, value_head_weight=1.0,
                   dtype=torch.float32):
    """``mean*`` [..., A]; ``log_std*`` broadcastable to them ([A] or [..., A]); values and target [..., vd]; ``done`` [..., 1].
    Returns (loss, dict of the three terms); gradients flow to whatever of the inputs requires them (inputs already of ``dtype``
    are used as they are)."""
    c = lambda x: x.to(dtype)
    m0, l0, m1, l1, aux, pred, tgt, done = (c(x) for x in (mean_old, log_std_old, mean, log_std, aux_value, pred_value, target, done))
    undone = 1.0 - done
    dls = l0 - l1
    r = torch.exp(2.0 * dls)
    t = ((m0 - m1) * torch.exp(-l1))**2
    kl = 0.5 * (r + t - 1.0) - dls
    pd = (kl * undone).sum() / undone.sum()
    av = 0.5 * (((aux - tgt)**2) * undone).sum() / undone.sum()
    vh = 0.5 * (((pred - tgt)**2) * undone).sum() / undone.sum()
    return av + beta_clone * pd + value_head_weight * vh, dict(auxiliary_value_loss=av, value_head_loss=vh, policy_distance=pd)


class GaussPPGAux:
    """The auxiliary phase over one cache entry (:205-243) for a continuous ``OracleActorCritic``: ``enter`` keeps the means and
    log sigma of that moment (and normalises the stored targets under PopArt), ``epoch`` is one pass of the inner loop."""

    def __init__(self, net: OracleActorCritic, beta_clone=1.0, aux_value_head_weight=1.0, max_grad_norm=None, popart=False,
                 ppg_optimizer_config: Optional[dict] = None):
        assert net.continuous
        self.net, self.beta, self.vhw, self.max_grad_norm, self.popart = net, beta_clone, aux_value_head_weight, max_grad_norm, popart
        self.optimizer = torch.optim.Adam([p for p in net.parameters() if p.requires_grad], **(ppg_optimizer_config or {}))

    def analyze(self, entry: Dict[str, np.ndarray]):
        """(mean [T, B, A], log sigma [T, B, A], auxiliary value, critic value), recurrent nets chunked from the stored states as
        ``OracleActorCritic.analyze_aux`` does.  log sigma of the vector parametrisations is the parameter itself; the second
        head's is read back from the ``std`` the net keeps (its ``forward`` does not hand out the actor's features)."""
        net = self.net
        f = lambda a: torch.from_numpy(np.asarray(a)).to(net.dtype)
        obs = {k[4:]: f(v) for k, v in entry.items() if k.startswith("obs.")}
        if net.num_rnn_layers == 0:
            mean, value, _ = net.forward(obs)
            aux, std = net._aux_value, net._std
        else:
            on_reset = f(entry["on_reset"])
            T = on_reset.shape[0]
            nc = T // net.chunk_len
            chunk = lambda x: torch.cat(torch.split(x, T // nc, dim=0), dim=1)
            unchunk = lambda x: torch.cat(torch.split(x, x.shape[1] // nc, dim=1), dim=0)
            names = ["policy_state.hx"] if net.shared else ["policy_state.actor_hx", "policy_state.critic_hx"]
            state = tuple(chunk(f(entry[n]))[0].transpose(0, 1) for n in names)
            mean, value, _ = net.forward({k: chunk(v) for k, v in obs.items()}, state, chunk(on_reset))
            mean, value, aux, std = unchunk(mean), unchunk(value), unchunk(net._aux_value), unchunk(net._std)
        log_std = std.log() if net.std_type == "shared_learnable" else net._p("log_std") * torch.ones_like(mean)
        return mean, log_std, aux, value

    def enter(self, entry):
        with torch.no_grad():
            mean, log_std, _, _ = self.analyze(entry)
        self.mean_old, self.log_std_old = mean.detach().clone(), log_std.detach().clone()
        self.target = torch.from_numpy(np.asarray(entry["value"])).to(self.net.dtype)
        if self.popart:  # :222-225
            self.target = self.net.normalize_value(self.target).to(self.net.dtype)
        self.done = torch.from_numpy(np.asarray(entry["info_mask"])).to(self.net.dtype)

    def epoch(self, entry):
        mean, log_std, aux, pred = self.analyze(entry)
        loss, terms = gauss_aux_loss(self.mean_old, self.log_std_old, mean, log_std, aux, pred, self.target, self.done, self.beta, self.vhw,
                                     dtype=self.net.dtype)
        self.optimizer.zero_grad()
        loss.backward()
        params = [p for p in self.net.parameters() if p.requires_grad]
        gn = torch.nn.utils.clip_grad_norm_(params, self.max_grad_norm) if self.max_grad_norm is not None else None
        self.optimizer.step()
        out = {k: float(v.detach()) for k, v in terms.items()}
        out["loss"] = float(loss.detach())
        out["grad_norm"] = float(gn) if gn is not None else -1.0
        return out
