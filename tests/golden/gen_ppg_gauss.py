"""Generate tests/golden/ppg_gauss.npz: Phasic Policy Gradient's auxiliary phase on Normal action heads (continuous actions),
computed by the REAL reference (read-only beside this repository) on the CPU.

Run (from the repo root):
    CUDA_VISIBLE_DEVICES="" PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout>:. python3 tests/golden/gen_ppg_gauss.py

Harness-side shims: those of gen_golden.py, imported from it (numpy alias, MagicMock for absent import-time dependencies, the CPU
pass-through for the CUDA prefetcher, ``module`` on a bare PopArt net).  The flow is gen_golden.py ``gen_ppg`` statement for
statement -- the `actor-critic-auxiliary` policy's two analysis targets (actor_critic_policy.py:392-435), then the auxiliary phase
(phasic_policy_gradient.py:205-243, 262-280) driven from here -- on ``continuous_action=True`` policies, whose
``get_action_distribution`` returns ``[Normal(mean, std)]`` (:303-309).  The reference's files stay untouched; two of its lines on
this path cannot execute as shipped and are REPAIRED FROM HERE:

1. ``modules.distribution_detach_to_cpu`` writes ``distribution.scale.cpu.detach()`` for a Normal (modules/utils.py:213):
   AttributeError.  The cached distribution is built by hand as what the line evidently means,
   ``Normal(loc=d.loc.cpu().detach(), scale=d.scale.cpu().detach())``.
2. ``MultiAgentPPG._policy_distance`` multiplies the ``[T, B, A]`` Normal KL by ``undone`` of shape ``[T, B]``
   (phasic_policy_gradient.py:149-150): a shape error for every A that does not happen to broadcast.  The trainer's method is
   monkeypatched to call the reference's OWN method with ``done.unsqueeze(-1)``: ``undone`` is then ``[T, B, 1]``, every action
   dimension of a row is weighted by that row's ``1 - done``, the sum runs over rows and dimensions and is divided by the number of
   undone rows -- the same reduction as ``log_prob(...).sum(-1)`` (actor_critic_policy.py:322).

While generating, the float32 CPU restatement (tests/ppg_gauss_ref.py) is run beside the reference and asserted to agree.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as gg  # the shims run on import

import numpy as np
import torch
from gen_golden import NamedArray, api, modules, recursive_apply

sys.path.insert(0, os.path.dirname(HERE))
from oracle.net import OracleActorCritic
from ppg_gauss_cases import PPG_GAUSS_CASES, TERM_NAMES
from ppg_gauss_ref import GaussPPGAux
from srl_amd.runtime import synthetic


def detach_to_cpu(d):
    """Repair 1: what modules/utils.py:212-213 evidently means."""
    assert isinstance(d, torch.distributions.Normal)
    return torch.distributions.Normal(loc=d.loc.cpu().detach(), scale=d.scale.cpu().detach())


def repair_policy_distance(trainer):
    """Repair 2: the reference's own ``_policy_distance``, called with ``done.unsqueeze(-1)``."""
    shipped = trainer._policy_distance
    trainer._policy_distance = lambda dist1, dist2, done: shipped(dist1, dist2, done=done.unsqueeze(-1))


def gen_ppg_gauss():
    import legacy.algorithm.ppo.phasic_policy_gradient as ppg
    out = {}
    for tag, (pargs, targs, skw) in PPG_GAUSS_CASES.items():
        trainer = api.trainer.make(api.config.Trainer("mappg", args=targs), api.config.Policy("actor-critic-auxiliary", args=pargs))
        if pargs.get("popart"):
            object.__setattr__(trainer.policy.net, "module", trainer.policy.net)
        repair_policy_distance(trainer)
        net = trainer.policy.net
        sd0 = gg.sd_to_np(net.state_dict())
        gg.check_init(dict(pargs, auxiliary_head=True, shared_backbone=False), net.state_dict())
        for k, v in sd0.items():
            out[f"{tag}_init_param:{k}"] = v
        T = skw["T"]
        arrays = synthetic.make_sample_arrays(seed=300, **skw)
        sample = gg.ref_sample({k: v.copy() for k, v in arrays.items()})
        ts = recursive_apply(sample, lambda x: torch.from_numpy(x).float())
        # ---- analyze(target="ppg_ppo_phase") on the sample's first T rows
        with torch.no_grad():
            r1 = trainer.policy.analyze(ts[:T], target="ppg_ppo_phase")
        out[f"{tag}_p1_new_lp"], out[f"{tag}_p1_value"] = r1.new_action_log_probs.numpy(), r1.state_values.numpy()
        out[f"{tag}_p1_aux"], out[f"{tag}_p1_entropy"] = r1.aux_values.numpy(), r1.entropy.numpy()
        # ---- the cache entry and the auxiliary phase
        vd = pargs.get("value_dim", 1)
        e = gg.ppg_entry_arrays(arrays, T, seed=7, value_dim=vd)
        if pargs.get("popart"):  # statistics away from their initial zeros
            with torch.no_grad():
                net.critic_head._PopArtValueHead__rms._RunningMeanStd__mean.copy_(torch.tensor([0.3, -0.2][:vd], dtype=torch.float64))
                net.critic_head._PopArtValueHead__rms._RunningMeanStd__mean_sq.copy_(torch.tensor([1.7, 2.5][:vd], dtype=torch.float64))
                net.critic_head._PopArtValueHead__rms._RunningMeanStd__debiasing_term.fill_(0.9)
            sd0 = gg.sd_to_np(net.state_dict())
            for k, v in sd0.items():
                out[f"{tag}_init_param:{k}"] = v
        obs = NamedArray(**{k[4:]: v for k, v in e.items() if k.startswith("obs.")})
        ps = {k[len("policy_state."):]: v for k, v in e.items() if k.startswith("policy_state.")}
        entry_sample = NamedArray(obs=obs, policy_state=NamedArray(**ps) if ps else None, info_mask=e["info_mask"],
                                  on_reset=e["on_reset"], value=e["value"])
        entry = ppg._PPGLocalCache.CacheEntry(sample=entry_sample)
        to_t = lambda smp: recursive_apply(smp, lambda x: torch.from_numpy(x).to(dtype=torch.float32))
        # :209-225
        r2 = trainer.policy.analyze(to_t(entry.sample), target="ppg_aux_phase")
        [d2] = r2.action_dists
        entry.action_dists = [detach_to_cpu(d) for d in r2.action_dists]
        if trainer.popart:
            entry.sample.value = trainer.policy.normalize_value(torch.from_numpy(entry.sample.value)).cpu().detach().numpy()
        out[f"{tag}_p2_loc"], out[f"{tag}_p2_scale"] = d2.loc.detach().numpy(), d2.scale.detach().numpy()
        out[f"{tag}_p2_aux"], out[f"{tag}_p2_pred"] = r2.auxiliary_value.detach().numpy(), r2.predicted_value.detach().numpy()
        out[f"{tag}_entry_value"], out[f"{tag}_entry_info_mask"] = e["value"], e["info_mask"]
        # the restatement on the same entry
        onet = OracleActorCritic(**pargs)
        onet.load_state_dict(sd0)
        oaux = GaussPPGAux(onet, beta_clone=targs.get("beta_clone", 1), aux_value_head_weight=targs.get("aux_value_head_weight", 1),
                           max_grad_norm=targs.get("max_grad_norm"), popart=targs.get("popart", False),
                           ppg_optimizer_config=targs.get("ppg_optimizer_config", {}))
        oaux.enter(e)
        assert torch.allclose(oaux.mean_old, d2.loc.detach(), rtol=1e-5, atol=1e-6), tag
        assert torch.allclose(oaux.log_std_old.exp(), d2.scale.detach(), rtol=1e-5, atol=1e-6), tag
        # the parameters are moved before the epochs, on both sides, for the reason gen_ppg gives: on the parameters the
        # distributions were kept under, KL = 0 and its gradient is rounding noise that Adam's first steps blow up
        prng = torch.Generator().manual_seed(1234)
        with torch.no_grad():
            for k, p_ in net.state_dict().items():
                if p_.dtype == torch.float32:
                    p_.add_(0.03 * torch.randn(p_.shape, generator=prng))
        sd1 = gg.sd_to_np(net.state_dict())
        for k, v in sd1.items():
            out[f"{tag}_pert_param:{k}"] = v
        for k, p_ in onet.params.items():
            p_.data.copy_(torch.from_numpy(sd1[k]).to(p_.dtype))
        # :232-243
        version0 = trainer.policy.version
        names = TERM_NAMES[:3]
        for ep in range(targs["ppg_epochs"]):
            res = trainer.policy.analyze(to_t(entry.sample), target="ppg_aux_phase")
            aux_l, metrics = trainer._compute_aux_loss(entry, res)
            trainer.ppg_aux_optimizer.zero_grad()
            aux_l.backward()
            gn = None
            if trainer.max_grad_norm is not None:
                gn = torch.nn.utils.clip_grad_norm_(trainer.policy.parameters(), trainer.max_grad_norm)
            trainer.ppg_aux_optimizer.step()
            trainer.policy.inc_version()
            o = oaux.epoch(e)
            vals = [float(getattr(metrics, n).detach()) for n in names] + [float(aux_l.detach()), float(gn) if gn is not None else -1.0]
            for n, v in zip(names, vals):
                assert abs(o[n] - v) <= 1e-5 * max(1.0, abs(v)), (tag, ep, n, o[n], v)
            if gn is not None:
                assert abs(o["grad_norm"] - float(gn)) <= 2e-5 * max(1.0, float(gn)), (tag, ep, o["grad_norm"], float(gn))
            out[f"{tag}_epoch{ep}_terms"] = np.array(vals, dtype=np.float64)
        assert trainer.policy.version == version0 + targs["ppg_epochs"]
        sd = gg.sd_to_np(net.state_dict())
        osd = onet.state_dict()
        for k, v in sd.items():
            assert np.allclose(osd[k].numpy(), v, rtol=1e-4, atol=1e-6), (tag, k)
            out[f"{tag}_final_param:{k}"] = v
        if pargs["std_type"] == "fixed":
            assert np.array_equal(sd["log_std"], sd1["log_std"]), "fixed: log sigma takes no gradient"
        print(f"ppg_gauss case {tag}: terms {out[f'{tag}_epoch0_terms']}")
    out["term_names"] = np.array(TERM_NAMES)
    gg.save("ppg_gauss.npz", **out)


if __name__ == "__main__":
    gen_ppg_gauss()
