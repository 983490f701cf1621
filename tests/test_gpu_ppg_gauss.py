"""Phasic Policy Gradient on Normal action heads (continuous actions) on the device: the fused auxiliary-loss kernel
``srl_ppg_aux_loss_gaussian_fwd_bwd`` against the float64 restatement (tests/ppg_gauss_ref.py), its exact cases, the
`actor-critic-auxiliary` policy's analysis targets and the `mappg` trainer's auxiliary phase against what the reference produced
(tests/golden/ppg_gauss.npz, gen_ppg_gauss.py), chunked against one-piece epochs, and the `mappg.step` flow."""
import numpy as np
import pytest
import torch

import srl_amd
from ppg_cases import entry_arrays, params_of
from ppg_gauss_cases import PPG_GAUSS_CASES
from ppg_gauss_ref import gauss_aux_loss
from srl_amd import hip
from srl_amd.api import config, policy as policy_api, trainer as trainer_api
from srl_amd.namedarray import NamedArray
from srl_amd.runtime import synthetic

srl_amd.register_all()
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BETA, VHW = 1.7, 0.6


def _close(a, b, tol, scale=1.0):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool((np.abs(a - b) <= tol * np.maximum(np.abs(b), scale)).all())


def kernel_inputs(n, A, vd, layout, seed=None):
    """Host float32 inputs of one kernel case.  ``layout``: "vv" (vector / vector log sigma), "rr" (rows / rows), "vr" (old vector,
    new rows).  log sigma uniform in [-1.5, 0.5]; new mean = old + 0.3 N(0, 1); new log sigma = old + 0.2 N(0, 1); about a quarter
    of the rows done (row 0 never: the count stays positive)."""
    rng = np.random.default_rng(n * 131 + A * 7 + vd if seed is None else seed)
    f = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
    old_rows, new_rows = layout[0] == "r", layout[1] == "r"
    m0 = f(rng.standard_normal((n, A)))
    l0 = f(rng.uniform(-1.5, 0.5, (n, A) if old_rows else (A,)))
    m1 = m0 + 0.3 * f(rng.standard_normal((n, A)))
    l1 = (l0 if old_rows == new_rows else l0.expand(n, A)) + 0.2 * f(rng.standard_normal((n, A) if new_rows else (A,)))
    aux, pred, tgt = (f(rng.standard_normal((n, vd))) for _ in range(3))
    done = torch.from_numpy((rng.random((n, 1)) < 0.25).astype(np.uint8))
    done[0] = 0
    return m0, l0, m1.contiguous(), l1.contiguous(), aux, pred, tgt, done


def reference_grads(inp, dtype):
    """Terms and gradients (mean, log sigma -- rows or the vector's --, aux, pred) of the restatement in ``dtype``."""
    m0, l0, m1, l1, aux, pred, tgt, done = inp
    leaf = lambda x: x.to(dtype).requires_grad_(True)
    m1, l1, aux, pred = leaf(m1), leaf(l1), leaf(aux), leaf(pred)
    loss, terms = gauss_aux_loss(m0, l0, m1, l1, aux, pred, tgt, done, BETA, VHW, dtype=dtype)
    loss.backward()
    return [float(terms[k].detach()) for k in ("auxiliary_value_loss", "value_head_loss", "policy_distance")], (m1.grad, l1.grad, aux.grad, pred.grad)


def run_kernel(inp, with_dls=True, pitch=None):
    """The kernel on the device: (terms float64[3] on the host, d_mean, d_log_std rows or None, d_aux, d_pred).  ``pitch``: row
    stride of the new means and of d_mean (> A: rows inside a wider buffer)."""
    m0, l0, m1, l1, aux, pred, tgt, done = inp
    n, A = m1.shape
    vd = aux.shape[1]
    d = lambda x: x.to(DEV)
    if pitch:
        wide = torch.full((n, pitch), float("nan"), device=DEV)
        wide[:, :A] = d(m1)
        m1_d = wide[:, :A]
        d_mean = torch.full((n, pitch), 7.0, device=DEV)[:, :A]
    else:
        m1_d, d_mean = d(m1), torch.empty((n, A), device=DEV)
    done_d = d(done.reshape(n))
    count = torch.zeros(3, dtype=torch.float64, device=DEV)
    if n:
        hip.masked_stats(torch.zeros(n, device=DEV), done_d, count, mask_invert=True)
    d_ls = torch.empty((n, A), device=DEV) if with_dls else None
    d_aux, d_pred = torch.empty((n, vd), device=DEV), torch.empty((n, vd), device=DEV)
    terms = torch.full((3,), 123.0, dtype=torch.float64, device=DEV)
    hip.ppg_aux_loss_gaussian_fwd_bwd(d(m0), d(l0), m1_d, d(l1), d(aux), d(pred), d(tgt), done_d, count[0:1], BETA, VHW, d_mean, d_ls, d_aux,
                                      d_pred, terms)
    if pitch:
        assert bool((d_mean.as_strided((n, pitch - A), (pitch, 1), A) == 7.0).all())   # nothing written between the rows
    return terms.cpu().numpy(), d_mean.cpu(), None if d_ls is None else d_ls.cpu(), d_aux.cpu(), d_pred.cpu()


KERNEL_CASES = [
    # n, A, value_dim, log sigma layout, d_log_std given, mean / d_mean row stride
    (1, 1, 1, "vv", True, None),
    (77, 3, 1, "rr", True, None),
    (77, 17, 3, "vr", False, None),
    (1000, 3, 3, "vv", True, 8),
    (1000, 17, 1, "rr", False, 20),
    (4099, 1, 3, "vr", True, None),
    (4099, 17, 1, "vv", True, 19),
    (4099, 3, 1, "rr", False, 5),
    (512 * 256 + 3, 3, 1, "rr", True, None),      # one row group past the kernel's 512 workgroups: the grid-stride loop's second trip
    (2048 * 256 + 257, 2, 1, "vr", True, None),   # ... and further trips, the last one ragged
    (2048 * 256 + 257, 1, 1, "vv", True, 3),
]


@pytest.mark.parametrize("n,A,vd,layout,with_dls,pitch", KERNEL_CASES)
def test_gaussian_aux_loss_kernel_vs_float64_restatement(n, A, vd, layout, with_dls, pitch):
    """srl_ppg_aux_loss_gaussian_fwd_bwd on its own against autograd of the float64 restatement: the three terms at 1e-5 of
    max(|ref|, 1e-3), every gradient at 1e-5 of its largest magnitude (the bar of test_aux_loss_kernel_vs_oracle).

    CPU pre-check on exactly these inputs (the float32 restatement against the float64 one, the same measure): worst term error
    7.0e-7 (n = 1), worst gradient error 1.1e-6 (the [A] vector's log sigma gradient at 524 545 rows, summed in float32), over all
    cases -- inside the bar, so the inputs are not narrowed.  The pre-check runs here too, first."""
    inp = kernel_inputs(n, A, vd, layout)
    ref_terms, ref_grads = reference_grads(inp, torch.float64)
    f32_terms, f32_grads = reference_grads(inp, torch.float32)

    def check(terms, grads, who):
        for k, (got, ref) in enumerate(zip(terms, ref_terms)):
            err = abs(got - ref) / max(abs(ref), 1e-3)
            print(f"{who} n={n} A={A} term{k} err {err:.3g}")
            assert err <= 1e-5, (who, k, got, ref)
        for name, got, ref in zip(("mean", "log_std", "aux", "pred"), grads, ref_grads):
            if got is None:
                continue
            if name == "log_std" and ref.dim() == 1 and got.dim() == 2:   # the vector's gradient is the rows' column sum
                got = got.double().sum(0)
            scale = max(float(ref.abs().max()), 1e-30)
            err = float((got.double() - ref).abs().max()) / scale
            print(f"{who} n={n} A={A} d_{name} err {err:.3g}")
            assert err <= 1e-5, (who, name, err, scale)

    check(f32_terms, f32_grads, "float32 restatement")
    terms, d_mean, d_ls, d_aux, d_pred = run_kernel(inp, with_dls, pitch)
    check(terms, (d_mean, d_ls, d_aux, d_pred), "kernel")


def test_gaussian_aux_loss_kernel_exact_cases():
    # old == new, bitwise: no distance, no gradient into the head
    for layout in ("vv", "rr"):
        m0, l0, _, _, aux, pred, tgt, done = kernel_inputs(1000, 3, 2, layout)
        terms, d_mean, d_ls, d_aux, d_pred = run_kernel((m0, l0, m0.clone(), l0.clone(), aux, pred, tgt, done))
        assert terms[2] == 0.0 and bool((d_mean == 0).all()) and bool((d_ls == 0).all())
        assert terms[0] > 0 and terms[1] > 0 and float(d_aux.abs().max()) > 0
    # every row done: the count is zero, so are all terms and gradients
    inp = list(kernel_inputs(300, 3, 2, "vr"))
    inp[7] = torch.ones((300, 1), dtype=torch.uint8)
    terms, *grads = run_kernel(tuple(inp))
    assert (terms == 0).all() and all(bool((g == 0).all()) for g in grads)
    # no rows: success, terms zeroed
    empty = (torch.zeros((0, 3)), torch.zeros(3), torch.zeros((0, 3)), torch.zeros(3), torch.zeros((0, 1)), torch.zeros((0, 1)),
             torch.zeros((0, 1)), torch.zeros((0, 1), dtype=torch.uint8))
    terms, *_ = run_kernel(empty)
    assert (terms == 0).all()


def _make(tag, **trainer_extra):
    pargs, targs, skw = PPG_GAUSS_CASES[tag]
    trainer = trainer_api.make(config.Trainer("mappg", args=dict(targs, **trainer_extra)), config.Policy("actor-critic-auxiliary", args=pargs))
    return trainer, pargs, targs, skw


def _load(trainer, params):
    trainer.policy.load_checkpoint(dict(steps=trainer.policy.version, state_dict={k: torch.from_numpy(np.asarray(v)) for k, v in params.items()}))


def _entry(g, tag, skw):
    from srl_amd.algorithm.mappg import _CacheEntry
    arrays = synthetic.make_sample_arrays(seed=300, **skw)
    e = entry_arrays(arrays, skw["T"], g, tag)
    obs = {k[4:]: v for k, v in e.items() if k.startswith("obs.")}
    ps = {k[len("policy_state."):]: v for k, v in e.items() if k.startswith("policy_state.")}
    entry_sample = NamedArray(obs=NamedArray(**obs), policy_state=NamedArray(**ps) if ps else None, on_reset=e["on_reset"],
                              info_mask=e["info_mask"])
    return arrays, entry_sample, _CacheEntry(obs, ps or None, e["info_mask"], e["on_reset"], e["value"])


@pytest.mark.parametrize("tag", list(PPG_GAUSS_CASES))
def test_ppg_gauss_analysis_targets_and_auxiliary_phase_match_reference_golden(tag, golden):
    g = golden("ppg_gauss.npz")
    trainer, pargs, targs, skw = _make(tag)
    pol = trainer.policy
    init = params_of(g, tag, "init")
    assert list(pol.get_checkpoint()["state_dict"]) == list(init)   # the reference's state_dict keys, in its order
    _load(trainer, init)
    T = skw["T"]
    arrays, entry_sample, entry = _entry(g, tag, skw)
    sample = synthetic.to_sample_batch(arrays)
    # ---- analyze(target="ppg_ppo_phase"): actor_critic_policy.py:392-415
    r1 = pol.analyze(sample[:T], target="ppg_ppo_phase")
    assert _close(r1.new_action_log_probs.cpu().numpy(), g[f"{tag}_p1_new_lp"], 1e-5)
    assert _close(r1.state_values.cpu().numpy(), g[f"{tag}_p1_value"], 1e-5)
    assert _close(r1.entropy.cpu().numpy(), g[f"{tag}_p1_entropy"], 1e-5)
    assert _close(r1.aux_values.cpu().numpy(), g[f"{tag}_p1_aux"], 1e-5)
    # ---- analyze(target="ppg_aux_phase") on the cache entry: :417-435, [Normal(mean, std)]
    r2 = pol.analyze(entry_sample, target="ppg_aux_phase")
    [d] = r2.action_dists
    assert d.loc.shape == g[f"{tag}_p2_loc"].shape and d.scale.shape == g[f"{tag}_p2_scale"].shape
    assert _close(d.loc.cpu().numpy(), g[f"{tag}_p2_loc"], 1e-5)
    assert _close(d.scale.cpu().numpy(), g[f"{tag}_p2_scale"], 1e-5)
    assert _close(r2.auxiliary_value.cpu().numpy(), g[f"{tag}_p2_aux"], 1e-5)
    assert _close(r2.predicted_value.cpu().numpy(), g[f"{tag}_p2_pred"], 1e-5)
    # ---- the auxiliary phase: distributions kept under the initial parameters, epochs from the perturbed ones
    trainer.enter_aux_phase(entry)
    pert = params_of(g, tag, "pert")
    _load(trainer, pert)
    names = list(g["term_names"])
    v0 = pol.version
    for ep in range(targs["ppg_epochs"]):
        m = trainer.aux_epoch(entry)
        ref = dict(zip(names, g[f"{tag}_epoch{ep}_terms"]))
        for k in ("auxiliary_value_loss", "value_head_loss", "policy_distance"):
            assert abs(getattr(m, k) - ref[k]) <= 1e-5 * max(abs(ref[k]), 1e-2), (ep, k, getattr(m, k), ref[k])
        if ref["grad_norm"] >= 0:
            assert abs(trainer.last_aux_grad_norm - ref["grad_norm"]) <= 2e-5 * max(ref["grad_norm"], 1e-2), (ep, trainer.last_aux_grad_norm)
    assert pol.version == v0 + targs["ppg_epochs"]
    sd = pol.get_checkpoint()["state_dict"]
    for k, v in params_of(g, tag, "final").items():
        assert np.abs(sd[k].numpy() - v).max() <= 2e-5, (k, np.abs(sd[k].numpy() - v).max())
    if tag == "gfix":   # `fixed`: requires_grad=False (actor_critic_policy.py:90)
        assert np.array_equal(sd["log_std"].numpy(), pert["log_std"])


@pytest.mark.parametrize("tag", ["gfix", "gsep"])
def test_ppg_gauss_chunked_epochs_match_one_piece(tag, golden):
    """``chunk_rows`` such that the entry's rows fall into three pieces, the last one ragged: the same terms as one piece (1e-6
    relative) and the same parameters (2e-5).  `gsep` (`separate_learnable`, the parametrisation of steps_continuous.npz's `csep`)
    accumulates the pieces' column sums into log sigma's gradient."""
    g = golden("ppg_gauss.npz")
    runs = []
    for pieces in (1, 3):
        trainer, pargs, targs, skw = _make(tag)
        n = skw["T"] * skw["B"]
        if pieces == 3:
            trainer.chunk_rows = n // 3 + 5   # e.g. 96 rows: 37 + 37 + 22
            assert [b - a for a, b in trainer._chunks(n, None)][-1] < trainer.chunk_rows and len(trainer._chunks(n, None)) == 3
        else:
            assert len(trainer._chunks(n, None)) == 1
        _load(trainer, params_of(g, tag, "init"))
        _, _, entry = _entry(g, tag, skw)
        trainer.enter_aux_phase(entry)
        _load(trainer, params_of(g, tag, "pert"))
        ms = [trainer.aux_epoch(entry) for _ in range(targs["ppg_epochs"])]
        runs.append((ms, trainer.policy.get_checkpoint()["state_dict"]))
    (m1, sd1), (m3, sd3) = runs
    for a, b in zip(m1, m3):
        for k in ("auxiliary_value_loss", "value_head_loss", "policy_distance"):
            assert abs(getattr(a, k) - getattr(b, k)) <= 1e-6 * abs(getattr(a, k)), (k, getattr(a, k), getattr(b, k))
    for k in sd1:
        assert float((sd1[k].double() - sd3[k].double()).abs().max()) <= 2e-5, k
    if tag == "gsep":
        assert not torch.equal(sd1["log_std"], torch.from_numpy(params_of(g, tag, "pert")["log_std"]))   # the vector was trained


@pytest.mark.parametrize("tag", ["gsep", "gshr"])
def test_policy_backward_ppg_aux_takes_d_log_std(tag, golden):
    """The policy's own route -- ``analyze(target="ppg_aux_phase")``, the kernel, ``backward_ppg_aux(..., d_log_std=rows)`` -- leaves
    the gradient the trainer's epoch computes on the same entry and parameters: the norm over every parameter, log sigma's vector
    (`gsep`: the rows' column sum) or second head (`gshr`) included, to 1e-6 relative."""
    g = golden("ppg_gauss.npz")
    trainer, pargs, targs, skw = _make(tag)
    _load(trainer, params_of(g, tag, "init"))
    _, entry_sample, entry = _entry(g, tag, skw)
    trainer.enter_aux_phase(entry)
    pol, net = trainer.policy, trainer.policy.net
    _load(trainer, params_of(g, tag, "pert"))
    n, vd = entry.mean_old.shape[0], net.spec.value_dim
    r = pol.analyze(entry_sample, target="ppg_aux_phase")
    [d] = r.action_dists
    mean = d.loc.reshape(n, -1).contiguous()
    done = torch.from_numpy(entry.info_mask.reshape(n)).to(DEV)
    count = torch.zeros(3, dtype=torch.float64, device=DEV)
    hip.masked_stats(torch.zeros(n, device=DEV), done, count, mask_invert=True)
    d_mean, d_ls = torch.empty_like(mean), torch.empty_like(mean)
    d_aux, d_pred = torch.empty((n, vd), device=DEV), torch.empty((n, vd), device=DEV)
    terms = torch.empty(3, dtype=torch.float64, device=DEV)
    hip.ppg_aux_loss_gaussian_fwd_bwd(entry.mean_old, entry.log_std_old, mean, pol._log_std(), r.auxiliary_value.reshape(n, vd).contiguous(),
                                      r.predicted_value.reshape(n, vd).contiguous(), entry.target, done, count[0:1], trainer.beta_clone,
                                      trainer.aux_value_head_weight, d_mean, d_ls, d_aux, d_pred, terms)
    net.zero_grad()
    pol.backward_ppg_aux(d_mean, d_aux, d_pred, d_log_std=d_ls)
    norm = float(net.grad.double().pow(2).sum().sqrt())
    assert float(net.grad[net.spec.params["log_std" if tag == "gsep" else "log_std.weight"].offset]) != 0.0
    trainer.aux_epoch(entry)   # the same parameters, the same entry
    assert abs(norm - trainer.last_aux_grad_norm) <= 1e-6 * trainer.last_aux_grad_norm, (norm, trainer.last_aux_grad_norm)


def test_mappg_step_flow_continuous_actions():
    """`mappg.step` on a `gym_mujoco`-style policy with the auxiliary head: the first step fills the cache, the second runs the
    auxiliary phase on the stacked entry (two samples side by side), and the checkpoint round-trips."""
    pargs = dict(obs_dim=7, action_dim=3, hidden_dim=32, num_dense_layers=1, num_rnn_layers=0, popart=False, layernorm=True,
                 chunk_len=8, seed=6, continuous_action=True, std_type="separate_learnable")
    targs = dict(popart=False, ppo_epochs=1, ppo_iterations=2, ppg_epochs=2, local_cache_stack_size=2, max_grad_norm=5.0,
                 optimizer_config=dict(lr=1e-3), ppg_optimizer_config=dict(lr=5e-4))
    skw = dict(T=16, B=6, obs_spec={"obs": ((7,), "f32")}, action_dims=3, p_done=0.1, continuous_action=True)
    ppg = trainer_api.make(config.Trainer("mappg", args=targs), config.Policy("actor-critic-auxiliary", args=pargs))
    v0 = ppg.policy.version
    r1 = ppg.step(synthetic.to_sample_batch(synthetic.make_sample_arrays(seed=1, **skw)))
    assert len(ppg._cache) == 1 and not any(k.startswith("ppg_") for k in r1.stats) and ppg.policy.version == v0 + 1
    r2 = ppg.step(synthetic.to_sample_batch(synthetic.make_sample_arrays(seed=2, **skw)))
    assert len(ppg._cache) == 0 and ppg.aux_optimizer.steps == 2   # one stacked entry x 2 epochs
    assert ppg.policy.version == v0 + 2 + 2
    for k in ("ppg_auxiliary_value_loss", "ppg_value_head_loss"):
        assert np.isfinite(r2.stats[k]) and r2.stats[k] >= 0, k
    assert np.isfinite(r2.stats["ppg_policy_distance"]) and r2.stats["ppg_policy_distance"] >= -1e-6
    ck = ppg.get_checkpoint()
    fresh = trainer_api.make(config.Trainer("mappg", args=targs), config.Policy("actor-critic-auxiliary", args=pargs))
    fresh.load_checkpoint(ck)
    assert fresh.aux_optimizer.steps == 2 and torch.equal(fresh.aux_optimizer.m, ppg.aux_optimizer.m)
    assert torch.equal(fresh.aux_optimizer.v, ppg.aux_optimizer.v)
    a, b = ppg.policy.get_checkpoint()["state_dict"], fresh.policy.get_checkpoint()["state_dict"]
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
