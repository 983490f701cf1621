"""The register-stationary chunk kernels at H = 128 (csrc/rnn_wseq.hip, `srl_{gru,lstm}_wseq_{fwd,bwd}`, the path "wseq").

Test 1 holds every buffer they write to a float64 loop over the steps (below, from the cell equations of autoreset_rnn.py:42-66;
the reset flags mask the state ENTERING step c >= 1).  The tolerance is not a number: the per-step path H = 128 runs today
(`srl_{gru,lstm}_step_fwd`, then `srl_gemm` + `srl_*_cell_bwd`) computes the same thing with the same float32 matrix
instructions and the same libm gates; it runs on the same inputs, and the new path's largest error against float64 may be at
most twice its error, per buffer (the 2: another summation order over K = 128 / 384 / 512).
Test 2 reaches the kernels through a policy; test 3 asks the library what it takes and needs no device."""
import pytest
import torch

from srl_amd import hip
from srl_amd.algorithm import rnnpath

DEV, H = "cuda:0", 128
KINDS = ("gru", "lstm")
# (N, C, variant): one row; a ragged first tile; a ragged second tile; three tiles and more steps than the two LDS buffers
CASES = [(1, 1, "reset"), (31, 2, "reset"), (33, 3, "reset"), (65, 5, "reset"), (33, 3, "noreset"), (33, 3, "nody"), (33, 3, "ld")]
SENTINEL, PAD = -7.25, 40   # rows behind step C - 1's N, where a tile's rows beyond N would land


def make_inputs(kind, N, C, variant):
    G = 4 if kind == "lstm" else 3
    g = torch.Generator().manual_seed(1000 * N + 10 * C + len(variant) + G)
    rn = lambda *s: torch.randn(*s, generator=g)
    reset = None if variant == "noreset" else (torch.rand(C, N, generator=g) < 0.25).to(torch.uint8)
    if reset is not None:
        reset[0] = 0
    dy = None if variant == "nody" else rn(C, N, H + (8 if variant == "ld" else 0))
    return dict(pre=rn(C, N, G * H), w=rn(G * H, H) / H ** 0.5, b=0.1 * rn(G * H), h0=0.5 * rn(N, H), c0=0.5 * rn(N, H), reset=reset,
                dy=dy)


def float64_loop(kind, inp):
    """Every buffer of the forward and, through autograd on the same loop, d pre / d gi / d gh, in float64."""
    pre, w, b, h, c = (inp[k].double() for k in ("pre", "w", "b", "h0", "c0"))
    C, N = pre.shape[:2]
    keep = torch.ones(C, N, 1, dtype=torch.float64) if inp["reset"] is None else 1.0 - inp["reset"].double()[..., None]
    pre, tap = pre.clone().requires_grad_(True), torch.zeros_like(pre, requires_grad=True)   # tap: a zero whose gradient is d gh
    out = {k: [] for k in ("gates", "gh", "y", "cnew", "hin", "cin")}
    for t in range(C):
        if t:
            h, c = h * keep[t], c * keep[t]
            out["hin"].append(h), out["cin"].append(c)
        gh = h @ w.T + b + tap[t]
        if kind == "lstm":
            i, f, g, o = (pre[t] + gh).split(H, 1)
            i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
            c = f * c + i * g
            h = o * torch.tanh(c)
            out["gates"].append(torch.cat((i, f, g, o), 1)), out["cnew"].append(c)
        else:
            (ir, iz, i_n), (hr, hz, hn) = pre[t].split(H, 1), gh.split(H, 1)
            r, z = torch.sigmoid(ir + hr), torch.sigmoid(iz + hz)
            n = torch.tanh(i_n + r * hn)
            h = (1.0 - z) * n + z * h
            out["gates"].append(torch.cat((r, z, n), 1))
        out["gh"].append(gh), out["y"].append(h)
    if inp["dy"] is not None:
        (torch.stack(out["y"]) * inp["dy"][..., :H].double()).sum().backward()
    grad = lambda x: torch.zeros_like(x) if x.grad is None else x.grad
    res = {k: torch.stack(v).detach() if v else torch.zeros(0) for k, v in out.items()}
    res["d_pre"], res["d_gh"] = grad(pre), grad(tap)
    drop = ("gh", "d_gh") if kind == "lstm" else ("cnew", "cin")
    return {k: v.reshape(-1) for k, v in res.items() if k not in drop}


def run_path(kind, inp, path):
    """The time loop `rnnpath.forward / backward` runs, on the path named (None: today's choice at H = 128), in buffers with
    PAD sentinel rows behind the last step; what the kernels left in them, and the sentinel rows."""
    C, N, GH = inp["pre"].shape
    k = rnnpath.CELLS[kind]
    buf = lambda cols, src=None: torch.cat((torch.full((C * N, cols), float("nan")) if src is None else src.reshape(C * N, cols),
                                            torch.full((PAD, cols), SENTINEL))).to(DEV)
    t = dict(gi=buf(GH, inp["pre"]), gh=buf(3 * H), hin=buf(H), cin=buf(H), cnew=buf(H), y=buf(H))
    t["hin"][:N], t["cin"][:N] = inp["h0"].to(DEV), inp["c0"].to(DEV)
    w, b = inp["w"].to(DEV), inp["b"].to(DEV)
    rs = None if inp["reset"] is None else inp["reset"].to(DEV)
    r = (lambda c: rs.data_ptr() + c * N) if rs is not None else (lambda c: None)
    s = rnnpath.bufs_of(kind, **t)
    k.fwd(s, w.data_ptr(), b.data_ptr(), r, N, H, C, path=path)
    got = {name: t[f][:C * N].clone() for name, f in (("gates", "gi"), ("y", "y"))}
    got.update({name: t[name][N:C * N].clone() for name in ("hin",) + (("cin",) if kind == "lstm" else ())})
    got.update({"cnew": t["cnew"][:C * N].clone()} if kind == "lstm" else {"gh": t["gh"][:C * N].clone()})
    # d y: the per-step cells read it in rows of H and want one (zeros); the chunk kernels take a wider buffer, or none
    ld = inp["dy"].shape[2] if inp["dy"] is not None and path == "wseq" else H
    dy = buf(ld, inp["dy"][..., :ld].contiguous() if inp["dy"] is not None else torch.zeros(C, N, H))
    carries, per = [torch.zeros(N, H, device=DEV) for _ in k.carries], len(k.carries) // 2
    k.bwd(s, None if inp["dy"] is None and path == "wseq" else dy.data_ptr(), ld, w.data_ptr(), r, N, H, C,
          lambda c: [x.data_ptr() for x in carries[per * (c & 1):][:per]], path=path)
    got.update({"d_pre": t["gi"][:C * N]}, **({"d_gh": t["gh"][:C * N]} if kind == "gru" else {}))
    torch.cuda.synchronize()
    pads = {name: x[C * N:].cpu() for name, x in list(t.items()) + [("dy", dy)]}
    return {name: v.cpu().double().reshape(-1) for name, v in got.items()}, pads


@pytest.mark.gpu
@pytest.mark.parametrize("N,C,variant", CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("kind", KINDS)
def test_wseq_kernels_vs_float64_loop(kind, N, C, variant):
    inp = make_inputs(kind, N, C, variant)
    ref = float64_loop(kind, inp)
    new, pads = run_path(kind, inp, "wseq")
    old, _ = run_path(kind, inp, None)
    assert set(new) == set(old) == set(ref) and all(new[n].shape == ref[n].shape for n in new)
    rows = []
    for name in sorted(n for n in new if ref[n].numel()):   # (hin[1..] / cin[1..] of a one-step chunk are empty)
        assert torch.isfinite(new[name]).all(), (name, "an element not written, or not finite")
        e_new, e_old = float((new[name] - ref[name]).abs().max()), float((old[name] - ref[name]).abs().max())
        rows.append((name, e_new, e_old, float(ref[name].abs().max())))
    print(f"\nwseq {kind} N={N} C={C} {variant}: buffer, error of wseq, error of the per-step path, max |float64|")
    for row in rows:
        print("  %-6s %.3e %.3e %.3e" % row)
    for name, x in pads.items():
        assert bool((x == SENTINEL).all()), (name, "rows beyond N were written")
    for name, e_new, e_old, _ in rows:
        assert e_new <= 2.0 * e_old, (name, e_new, e_old)


# Test 1 measured, over all its cases on an MI355X, errors of at most 3.0e-7 (wseq) and 2.8e-7 (per-step) of a buffer's largest
# element.  Two runs that differ only in the path differ by at most the sum, 6e-7, in these buffers; the loss terms and the
# parameter gradients are sums over them and over what the same kernels compute from them.  1e-5 of the largest element (the rule
# smoke() holds loss terms to) is that with a factor of 16 for what the layers behind and in front of the recurrent one add.
NET_REL = 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_wseq_reached_from_a_policy(kind, monkeypatch):
    """One `mappo` step of a recurrent `actor-critic` (hidden_dim 128, one layer, chunk_len 5, T = 10, B = 3) with "wseq" named
    and on the default path, from the same seed: the same loss terms and flat gradient, and the named run ran the wseq scopes."""
    import srl_amd
    from srl_amd.api import config, trainer as trainer_api
    from srl_amd.runtime import synthetic
    srl_amd.register_all()
    pargs = dict(obs_dim=4, action_dim=2, hidden_dim=H, num_dense_layers=1, num_rnn_layers=1, rnn_type=kind, popart=False,
                 layernorm=True, shared_backbone=True, chunk_len=5, seed=11)
    targs = dict(popart=False, optimizer_config=dict(lr=1e-3), max_grad_norm=10.0)
    arrays = synthetic.make_sample_arrays(seed=3, T=10, B=3, obs_spec=synthetic.CARTPOLE_OBS, action_dims=2, p_done=0.15,
                                          policy_state={"hx": (1, 2 * H if kind == "lstm" else H)})
    runs = {}
    for named in ("wseq", None):
        monkeypatch.setattr(rnnpath, "NAMED", named)
        monkeypatch.setattr(hip, "_prof", hip.KernelProfile())
        trainer = trainer_api.make(config.Trainer("mappo", args=targs), config.Policy("actor-critic", args=pargs))
        stats = trainer.step(synthetic.to_sample_batch(arrays)).stats
        scopes = {rec[0] for rec in hip._prof.records}
        assert ({f"{kind}_wseq_fwd", f"{kind}_wseq_bwd"} <= scopes) == (named == "wseq"), scopes
        runs[named] = (stats, trainer.policy.net.grad.detach().double().cpu())
    (s_new, g_new), (s_old, g_old) = runs["wseq"], runs[None]
    for name in ("policy_loss", "value_loss", "entropy"):
        assert abs(s_new[name] - s_old[name]) <= NET_REL * max(abs(s_old[name]), 1e-2), (name, s_new[name], s_old[name])
    diff, top = float((g_new - g_old).abs().max()), float(g_old.abs().max())
    print(f"\nwseq {kind} policy step: max |d grad| {diff:.3e}, max |grad| {top:.3e}")
    assert top > 0 and diff <= NET_REL * top, (diff, top)


def test_wseq_supported_widths():
    lib = hip.lib()
    for kind, code in (("gru", 0), ("lstm", 1)):
        assert hip.rnn_wseq_supported(kind, 128)
        assert not any(hip.rnn_wseq_supported(kind, h) for h in (64, 144, 256))
        assert [lib.srl_rnn_seq_supported(code, h) for h in (64, 128, 144, 256)] == [1, 0, 0, 0]
        assert [lib.srl_rnn_step_supported(code, h) for h in (64, 128, 144, 256)] == [0, 1, 1, 1]
    assert not lib.srl_rnn_wseq_supported(2, 128)
