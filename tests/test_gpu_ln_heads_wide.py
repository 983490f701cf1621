"""srl_ln_heads_wide_fwd / srl_ln_heads_wide_bwd (csrc/ln_heads_wide.hip): the closing LayerNorm + heads as one launch per direction
for 9 to 32 head outputs, on the float32 matrix cores -- against float64 autograd, the host query, and one step through the trainer."""
import numpy as np
import pytest
import torch

import srl_amd
from oracle.net import OracleActorCritic
from oracle.trainer import OracleMappo
from srl_amd import hip
from srl_amd.api import config, trainer as trainer_api
from srl_amd.runtime import synthetic

srl_amd.register_all()
pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def rel_close(a, b, rtol, scale):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool((np.abs(a - b) <= rtol * np.maximum(np.abs(b), max(scale, 1e-30))).all())


@pytest.mark.parametrize("n,D,heads,in_act,slabs", [
    (33, 256, (9,), 0, 1),            # one head, the minimum width, a one-row second tile
    (1000, 512, (18, 1), 1, 2),       # Atari's full action set + value, a ragged last tile; the forward finishes two slabs
    (70, 1024, (31, 1), 2, 1),        # all 32 columns in use, the 16-row tiling of D = 1024
    (64, 512, (5, 4), 1, 1),          # a head boundary inside the first 16 columns
    (8229, 256, (12, 1), 1, 1),       # 258 tiles of 32 rows on a grid of min(tiles, CUs) = 256: workgroups 0 and 1 walk two tiles,
])                                    # workgroup 1's second one is the ragged last (5 rows)
def test_ln_heads_wide_vs_float64(n, D, heads, in_act, slabs):
    """Head outputs, mean / rstd, dx (times the derivative of the activation that produced x), max |dx| and every parameter
    gradient (added onto 0.5) against float64 autograd, at test_ln_heads_fused's tolerances.  Outputs and dx start as NaN and
    the heads' rows are wider than the heads, so a store into a padded column or past n shows."""
    rng = np.random.default_rng(n + D)
    t = torch
    act = lambda v: t.relu(v) if in_act == 1 else (t.tanh(v) if in_act == 2 else v)
    assert hip.ln_heads_wide_supported(D, heads) and not hip.ln_heads_supported(D, heads)
    if slabs == 2:   # x = act(slab 0 + slab 1 + bias), finished by the forward launch and written to x_out
        parts = t.from_numpy(rng.standard_normal((2, n, D))).float()
        xbias = t.from_numpy(0.1 * rng.standard_normal(D)).float()
        x32 = act((parts[0] + parts[1]) + xbias)
    else:
        x32 = act(t.from_numpy(rng.standard_normal((n, D)))).float()
    x64 = x32.double()   # the values the kernel sees
    g64 = t.from_numpy(1 + 0.1 * rng.standard_normal(D)).float().double().requires_grad_(True)
    b64 = t.from_numpy(0.1 * rng.standard_normal(D)).float().double().requires_grad_(True)
    W64 = [t.from_numpy(rng.standard_normal((a, D)) / np.sqrt(D)).float().double().requires_grad_(True) for a in heads]
    hb64 = [t.from_numpy(0.1 * rng.standard_normal(a)).float().double().requires_grad_(True) for a in heads]
    xin = x64.clone().requires_grad_(True)
    feat = t.nn.functional.layer_norm(xin, (D,), g64, b64, 1e-5)
    ys = [feat @ W.t() + hb for W, hb in zip(W64, hb64)]
    dys = [t.from_numpy(rng.standard_normal((n, a))).float() for a in heads]
    t.autograd.backward(ys, [d.double() for d in dys])
    P = lambda ts: [v.data_ptr() for v in ts]
    f32 = lambda v: v.detach().float().to(DEV).contiguous()
    x, g, b, W, hb = f32(x64), f32(g64), f32(b64), [f32(w) for w in W64], [f32(v) for v in hb64]
    ldy = [a + 3 for a in heads]
    y = [t.full((n, ld), float("nan"), device=DEV) for ld in ldy]
    mean, rstd = t.empty(n, device=DEV), t.empty(n, device=DEV)
    if slabs == 2:
        xs, xb, x = parts.to(DEV).contiguous(), xbias.to(DEV), t.full((n, D), float("nan"), device=DEV)
        hip.ln_heads_wide_fwd(xs.data_ptr(), D, n, D, g.data_ptr(), b.data_ptr(), P(W), P(hb), list(heads), P(y), ldy, mean.data_ptr(),
                              rstd.data_ptr(), x_slabs=2, x_slab_stride=n * D, x_bias=xb.data_ptr(), x_act=in_act, x_out=x.data_ptr(), ldxo=D)
        assert t.equal(x.cpu(), x32)   # the finished rows, as the backward pass will read them
    else:
        hip.ln_heads_wide_fwd(x.data_ptr(), D, n, D, g.data_ptr(), b.data_ptr(), P(W), P(hb), list(heads), P(y), ldy, mean.data_ptr(),
                              rstd.data_ptr())
    for got, ref, a in zip(y, ys, heads):
        assert rel_close(got[:, :a].cpu().numpy(), ref.detach().numpy(), 1e-5, scale=float(ref.detach().abs().max()))
        assert bool(t.isnan(got[:, a:]).all())
    assert rel_close(mean.cpu().numpy(), x64.mean(1).numpy(), 1e-5, scale=1.0)
    assert rel_close(rstd.cpu().numpy(), (1 / t.sqrt(x64.var(1, unbiased=False) + 1e-5)).numpy(), 1e-5, scale=float(rstd.max()))
    dg, db_ = t.full((D,), 0.5, device=DEV), t.full((D,), 0.5, device=DEV)
    dW, dhb = [t.full((a, D), 0.5, device=DEV) for a in heads], [t.full((a,), 0.5, device=DEV) for a in heads]
    dx = t.full((n, D), float("nan"), device=DEV)
    amax = t.zeros(1, device=DEV)
    ddy = [t.full((n, ld), float("nan"), device=DEV) for ld in ldy]   # (the padding of dy's rows is not read either)
    for d, src, a in zip(ddy, dys, heads):
        d[:, :a] = src.to(DEV)
    hip.ln_heads_wide_bwd(x.data_ptr(), D, n, D, g.data_ptr(), b.data_ptr(), mean.data_ptr(), rstd.data_ptr(), P(W), list(heads), P(ddy),
                          ldy, in_act, dx.data_ptr(), D, dg.data_ptr(), db_.data_ptr(), P(dW), P(dhb), dx_absmax=amax.data_ptr())
    der = (x64 > 0).double() if in_act == 1 else ((1 - x64 * x64) if in_act == 2 else t.ones_like(x64))
    ref_dx = xin.grad * der
    assert rel_close(dx.cpu().numpy(), ref_dx.numpy(), 2e-5, scale=float(ref_dx.abs().max()))
    assert abs(float(amax) - float(dx.abs().max())) <= 1e-6 * float(dx.abs().max())
    for got, ref, name in [(dg, g64, "dgamma"), (db_, b64, "dbeta")] + [(u, v, f"dW{i}") for i, (u, v) in enumerate(zip(dW, W64))] + \
            [(u, v, f"db{i}") for i, (u, v) in enumerate(zip(dhb, hb64))]:
        assert rel_close(got.cpu().numpy() - 0.5, ref.grad.numpy(), 2e-5, scale=float(ref.grad.abs().max()) + 1e-6), name


def test_ln_heads_wide_host_query():
    """The wide family takes 9 to 32 outputs at D in 256 | 512 | 1024 and nothing the narrow one takes (no launch)."""
    for D, heads in [(512, (18, 1)), (256, (9,)), (1024, (31, 1))]:
        assert hip.ln_heads_wide_supported(D, heads), (D, heads)
    for D, heads in [(512, (6, 1)), (512, (32, 1)), (384, (18, 1)), (512, ())]:
        assert not hip.ln_heads_wide_supported(D, heads), (D, heads)


ATARI_TRAINER = dict(discount_rate=0.99, gae_lambda=0.97, eps_clip=0.2, clip_value=True, dual_clip=False,
                     value_loss='huber', value_loss_weight=1.0, value_loss_config=dict(delta=10.0),
                     entropy_bonus_weight=0.01, optimizer='adam', optimizer_config=dict(lr=5e-4), popart=False,
                     max_grad_norm=40.0, bootstrap_steps=1)


def test_full_action_set_step_through_the_trainer(monkeypatch):
    """One mappo step of an image actor-critic with 18 actions (18 + 1 head outputs behind LayerNorm(256)), two row chunks: with
    `HipNet.LNHEADS_WIDE` the tail runs on the wide pair, without it layer by layer and the pair is never called.  Loss terms and
    the gradient norm against the float32 oracle at 2e-5; every tensor's gradient against the float64 oracle no further than 3 x
    the layer-by-layer kernels' error (+ 2e-6 of the tensor's largest element)."""
    from srl_amd.algorithm.hipnet import HipNet
    pargs = dict(obs_dim={"obs": (4, 24, 24)}, action_dim=18, hidden_dim=256, num_dense_layers=0, num_rnn_layers=0, popart=False,
                 layernorm=True, shared_backbone=True, chunk_len=8, seed=32,
                 cnn_layers=dict(obs=[(4, 5, 1, 0, 'zeros'), (8, 3, 1, 0, 'zeros'), (4, 3, 1, 0, 'zeros')]))
    targs = dict(ATARI_TRAINER, chunk_rows=64)
    make = lambda: trainer_api.make(config.Trainer("mappo", args=targs), config.Policy("actor-critic", args=pargs))
    arrays = synthetic.make_sample_arrays(seed=3, T=16, B=8, obs_spec={"obs": ((4, 24, 24), "u8")}, action_dims=18, p_done=0.02)
    calls = dict(fwd=0, bwd=0)

    def counted(name, fn):
        def wrapper(*a, **kw):
            calls[name] += 1
            return fn(*a, **kw)
        return wrapper
    monkeypatch.setattr(hip, "ln_heads_wide_fwd", counted("fwd", hip.ln_heads_wide_fwd))
    monkeypatch.setattr(hip, "ln_heads_wide_bwd", counted("bwd", hip.ln_heads_wide_bwd))
    oargs = {k: v for k, v in targs.items() if k != "chunk_rows"}
    grads = {}
    for wide in (True, False):
        monkeypatch.setattr(HipNet, "LNHEADS_WIDE", wide)
        calls.update(fwd=0, bwd=0)
        trainer = make()
        res = trainer.step(synthetic.to_sample_batch(arrays))
        net = trainer.policy.net
        grads[wide] = {k: v.clone() for k, v in net.flat_to_reference(net.grad.detach().cpu()).items()}
        assert (calls["fwd"] >= 2 and calls["bwd"] >= 2) if wide else (calls["fwd"] == 0 and calls["bwd"] == 0), calls
        if wide:
            onet = OracleActorCritic(**pargs)
            onet.load_state_dict({k: v.numpy() for k, v in make().policy.get_checkpoint()["state_dict"].items()})
            ostats, _ = OracleMappo(onet, **oargs).step(arrays)
            for k in ("policy_loss", "value_loss", "entropy", "grad_norm"):
                assert abs(res.stats[k] - ostats[k]) <= 2e-5 * max(abs(ostats[k]), 1e-2), (k, res.stats[k], ostats[k])
    onet64 = OracleActorCritic(**pargs, dtype=torch.float64)
    onet64.load_state_dict({k: v.numpy() for k, v in make().policy.get_checkpoint()["state_dict"].items()})
    OracleMappo(onet64, **oargs).step(arrays)
    for k, p in onet64.params.items():
        g64 = p.grad.double()
        e_wide = float((grads[True][k].double() - g64).abs().max())
        e_layerwise = float((grads[False][k].double() - g64).abs().max())
        assert e_wide <= 3.0 * e_layerwise + 2e-6 * float(g64.abs().max()), (k, e_wide, e_layerwise)
