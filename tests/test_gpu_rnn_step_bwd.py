"""The one-launch backward step at the wide widths (csrc/rnn_step.hip, `srl_{gru,lstm}_step_bwd`, the path "step" of `rnnpath`).

Test 1 runs `rnnpath`'s own time loop -- the forward on "fused", the backward on "step" -- and holds d pre / d gi and d gh, element
by element, to the float64 restatement tests/rnn_ref.py::chunk by the rule of this kernel family (tests/test_gpu_rnn.py
BOUNDS["step"]): error <= 4 max|float32 chunk - float64| + 1e-7 max|float64| per tensor; the kernel does the same float32 work
with the sum over k in another order.  The carries are not compared: under "step" they hold `direct` / d c_in by contract.  It
prints today's backward (path "fused") beside it: on an MI355X the largest new / old error ratio over all cases and buffers was
1.02 (0.7 to 1.0 elsewhere), the largest error / bound 0.27.  Test 2 reaches the kernels through a policy; test 3 needs no device."""
import pytest
import torch

from rnn_ref import chunk
from srl_amd import cabi, hip
from srl_amd.algorithm import rnnpath

DEV, A_F32, B_ABS = "cuda:0", 4.0, 1e-7   # tests/test_gpu_rnn.py BOUNDS["step"]
SENTINEL, PAD = -7.25, 40  # rows behind the last step's N, where a tile's rows beyond N would land
# (kind, H, N, C, variant): one row, cell-only launch; a ragged second tile, both carry sets; K / 16 = 27 / 36 blocks over four
# wavefronts, a whole tile; no flags / no dy / a wider dy; the DMLab width; the 32-row tile (8 tiles x 32 unit blocks), one row last
CASES = ([(k, 128, 1, 1, "") for k in ("gru", "lstm")] + [(k, 128, 17, 3, "") for k in ("gru", "lstm")]
         + [(k, 144, 16, 2, "") for k in ("gru", "lstm")] + [("gru", 128, 17, 3, v) for v in ("noreset", "nody", "ld")]
         + [("lstm", 256, 33, 2, ""), ("gru", 512, 257, 2, "")])


def make_inputs(kind, H, N, C, variant):
    """Seeded float32 CPU tensors; resets at step 0 (over a non-zero stored state) and inside the chunk."""
    G = 4 if kind == "lstm" else 3
    g = torch.Generator().manual_seed(1000 * N + 10 * C + H + G + len(variant))
    rn = lambda *s: torch.randn(*s, generator=g)
    reset = (torch.rand(C, N, generator=g) < 0.3).to(torch.uint8)
    reset[0, 0] = reset[C - 1, N - 1] = 1
    return dict(pre=rn(C, N, G * H), w=rn(G * H, H) / H ** 0.5, b=0.1 * rn(G * H), h0=0.5 * rn(N, H), c0=0.5 * rn(N, H),
                reset=None if variant == "noreset" else reset, dy=None if variant == "nody" else rn(C, N, H + 8 * (variant == "ld")))


def run_path(kind, inp, path):
    """Forward on "fused", backward on ``path``, in NaN buffers with PAD sentinel rows behind the last step: (d_pre, d_gh), pads."""
    (C, N, GH), H, k = inp["pre"].shape, inp["w"].shape[1], rnnpath.CELLS[kind]
    buf = lambda cols, src=None, rows=C * N: torch.cat((torch.full((rows, cols), float("nan")) if src is None
                                                        else src.reshape(rows, cols), torch.full((PAD, cols), SENTINEL))).to(DEV)
    t = dict(gi=buf(GH, inp["pre"]), gh=buf(3 * H), hin=buf(H), cin=buf(H), cnew=buf(H), y=buf(H))
    w, b, rs = inp["w"].to(DEV), inp["b"].to(DEV), None if inp["reset"] is None else inp["reset"].to(DEV)
    r = (lambda c: rs.data_ptr() + c * N) if rs is not None else (lambda c: None)
    for name, src in (("hin", "h0"), ("cin", "c0")):
        hip.gru_mask_state(inp[src].to(DEV).data_ptr(), r(0), N, H, t[name].data_ptr())
    s = rnnpath.bufs_of(kind, **t)
    k.fwd(s, w.data_ptr(), b.data_ptr(), r, N, H, C, path="fused")
    # the per-step cells read d y in rows of H and want one (zeros); "step" takes a wider buffer, or none
    ld = inp["dy"].shape[2] if inp["dy"] is not None and path == "step" else H
    dy = buf(ld, inp["dy"][..., :ld].contiguous() if inp["dy"] is not None else torch.zeros(C, N, H))
    carries, per = [buf(H, rows=N) for _ in k.carries], len(k.carries) // 2
    k.bwd(s, None if inp["dy"] is None and path == "step" else dy.data_ptr(), ld, w.data_ptr(), r, N, H, C,
          lambda c: [x.data_ptr() for x in carries[per * (c & 1):][:per]], path=path)
    torch.cuda.synchronize()
    got = dict(d_pre=t["gi"][:C * N].cpu(), **({"d_gh": t["gh"][:C * N].cpu()} if kind == "gru" else {}))
    pads = {name: x[-PAD:].cpu() for name, x in list(t.items()) + [("dy", dy)] + [(f"carry{i}", x) for i, x in enumerate(carries)]}
    return got, pads


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_step_bwd_vs_float64(case):
    kind, H, N, C, _ = case
    inp = make_inputs(*case)
    dy = torch.zeros(C, N, H) if inp["dy"] is None else inp["dy"][..., :H]
    ref = lambda dt: chunk(kind, *(inp[x].to(dt) for x in ("pre", "w", "b", "h0", "c0")), inp["reset"], dy.to(dt))
    r64, r32 = ref(torch.float64), ref(torch.float32)
    new, pads = run_path(kind, inp, "step")
    old, _ = run_path(kind, inp, "fused")
    rows = []
    for name, v in new.items():
        assert torch.isfinite(v).all(), (name, "an element not written, or not finite")
        want = r64[name].reshape(C * N, -1)
        err, e_old = (float((x.double() - want).abs().max()) for x in (v, old[name]))
        rows.append((name, err, A_F32 * float((r32[name] - r64[name]).abs().max()) + B_ABS * float(want.abs().max()), e_old))
    print(f"\nstep bwd {case}: (buffer, error of \"step\", bound, error of today's backward)", *rows, sep="\n  ")
    for name, x in pads.items():
        assert bool((x == SENTINEL).all()), (name, "rows beyond N were written")
    for name, err, lim, _ in rows:
        assert err <= lim, (name, err, lim)


NET_REL = 1e-5   # tests/test_gpu_rnn_wseq.py derives it: smoke()'s rule for loss terms


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["gru", "lstm"])
def test_step_bwd_reached_from_a_policy(kind, monkeypatch):
    """One `mappo` step of a recurrent `actor-critic` (the settings of test_wseq_reached_from_a_policy) with "step" named and on the
    default path, from the same seed: the same loss terms and flat gradient; only the named run ran the step_bwd scopes."""
    import srl_amd
    from srl_amd.api import config, trainer as trainer_api
    from srl_amd.runtime import synthetic
    srl_amd.register_all()
    pargs = dict(obs_dim=4, action_dim=2, hidden_dim=128, num_dense_layers=1, num_rnn_layers=1, rnn_type=kind, popart=False,
                 layernorm=True, shared_backbone=True, chunk_len=5, seed=11)
    targs = dict(popart=False, optimizer_config=dict(lr=1e-3), max_grad_norm=10.0)
    arrays = synthetic.make_sample_arrays(seed=3, T=10, B=3, obs_spec=synthetic.CARTPOLE_OBS, action_dims=2, p_done=0.15,
                                          policy_state={"hx": (1, 256 if kind == "lstm" else 128)})
    runs = {}
    for named in ("step", None):
        monkeypatch.setattr(rnnpath, "NAMED", named)
        monkeypatch.setattr(hip, "_prof", hip.KernelProfile())
        trainer = trainer_api.make(config.Trainer("mappo", args=targs), config.Policy("actor-critic", args=pargs))
        stats = trainer.step(synthetic.to_sample_batch(arrays)).stats
        scopes = {rec[0] for rec in hip._prof.records}
        assert {x for x in scopes if x.endswith("_step_bwd")} == ({f"{kind}_step_bwd"} if named else set()), scopes
        assert not (named and any(x.endswith("_cell_bwd") for x in scopes)), scopes
        runs[named] = (stats, trainer.policy.net.grad.detach().double().cpu())
    (s_new, g_new), (s_old, g_old) = runs["step"], runs[None]
    for name in ("policy_loss", "value_loss", "entropy"):
        assert abs(s_new[name] - s_old[name]) <= NET_REL * max(abs(s_old[name]), 1e-2), (name, s_new[name], s_old[name])
    diff, top = float((g_new - g_old).abs().max()), float(g_old.abs().max())
    assert top > 0 and diff <= NET_REL * top, (diff, top)


def test_step_path_is_named_only():
    assert "step" in rnnpath.PATHS
    for name in ("srl_gru_step_bwd", "srl_lstm_step_bwd"):
        assert name in cabi.prototypes and hasattr(hip.lib(), name)
    for kind in ("gru", "lstm"):
        assert rnnpath.time_loop_path(kind, 128) == "fused" and rnnpath.time_loop_path(kind, 64) == "seq"
        assert rnnpath.time_loop_path(kind, 128, "step") == "step"
        with pytest.raises(AssertionError):
            rnnpath.time_loop_path(kind, 64, "step")
