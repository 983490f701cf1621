"""The fused recurrent step (csrc/rnn_step.hip: W_hh h + b_hh and the cell in one launch, H a multiple of 16 from 128 up) against the
float64 restatement of the auto-reset LSTM / GRU (tests/rnn_ref.py::chunk), driven by ``rnnpath``'s own time loop: the fused forward step
by step, then the EXISTING per-step backward (srl_{gru,lstm}_cell_bwd + srl_gemm) on what the forward saved.

Every buffer the kernels write is compared element by element: the activated gates, GRU's gh, hin[1:], cin[1:], y, cnew; d pre /
d gi, d gh and the carries d hin / d cin.  The rule and its constants are tests/test_gpu_rnn.py's for its ``step`` path
(error <= 4 max|f32 - f64| + 1e-7 max|f64| per tensor): the fused step does the same float32 work, the sum over k in another
order.  ``test_the_bar_can_fail`` shows on the same inputs that the restatement's faults exceed that bar."""
import zlib

import pytest
import torch

from rnn_ref import chunk, check_vs_float64
from srl_amd import hip
from srl_amd.algorithm.rnnpath import CELLS, bufs_of

DEV = "cuda:0"
A_F32, B_ABS = 4.0, 1e-7   # tests/test_gpu_rnn.py BOUNDS["step"]
# (kind, H, N, C, extra columns of the dy buffer): 17 and 33 rows: a ragged second tile of 16; one row; 16: one whole tile; H = 144:
# nine k-blocks over four wavefronts (3, 2, 2, 2)
CASES = [("gru", 128, 17, 3, 0), ("lstm", 128, 17, 3, 0), ("gru", 144, 1, 2, 0), ("gru", 512, 33, 2, 5), ("lstm", 512, 16, 2, 0)]
IDS = ["-".join(map(str, c)) for c in CASES]
FAULTS = ("reset_late", "bhn_outside", "if_swap")


def make_inputs(kind, H, N, C, extra):
    """float32 CPU tensors seeded by the case; resets at step 0 (over a non-zero stored state) and inside the chunk."""
    G = 4 if kind == "lstm" else 3
    g = torch.Generator().manual_seed(zlib.crc32(repr((kind, H, N, C, extra)).encode()))
    rn = lambda *s: torch.randn(*s, generator=g)
    w_hh, b_hh = rn(G * H, H) / H ** 0.5, 0.1 * rn(G * H)
    pre_x, h0, c0 = rn(C, N, G * H), 0.5 * rn(N, H), 0.5 * rn(N, H)
    reset = (torch.rand(C, N, generator=g) < 0.3).to(torch.uint8)
    reset[0, 0] = reset[C - 1, N - 1] = 1
    assert reset[0].any() and reset[1:].any()
    return pre_x, w_hh, b_hh, h0, c0, reset, rn(C, N, H + extra)


def references(kind, inputs, fault=None, only64=False):
    pre_x, w_hh, b_hh, h0, c0, reset, dy = inputs
    H = w_hh.shape[1]
    r64 = chunk(kind, pre_x.double(), w_hh.double(), b_hh.double(), h0.double(), c0.double(), reset, dy[..., :H].double(), fault=fault)
    return r64 if only64 else (r64, chunk(kind, pre_x, w_hh, b_hh, h0, c0, reset, dy[..., :H]))


def run_kernels(kind, inputs, fused=True):
    """Output buffers start as NaN: an element a kernel fails to write shows."""
    pre_x, w_hh, b_hh, h0, c0, reset, dy = inputs
    C, N, _ = pre_x.shape
    H, ld = w_hh.shape[1], dy.shape[2]
    d = lambda t: t.to(DEV).contiguous()
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    pre, w, b, rs, h0d, c0d, dyd = d(pre_x), d(w_hh), d(b_hh), d(reset), d(h0), d(c0), d(dy)
    gh, hin, cin, y, cnew = nan(C, N, 3 * H), nan(C, N, H), nan(C, N, H), nan(C, N, H), nan(C, N, H)
    rp = lambda c: rs.data_ptr() + c * N
    P = lambda t, c=0: t[c].data_ptr()
    hip.gru_mask_state(h0d.data_ptr(), rp(0), N, H, hin.data_ptr())
    if kind == "lstm":
        hip.gru_mask_state(c0d.data_ptr(), rp(0), N, H, cin.data_ptr())
    assert hip.rnn_step_supported(kind, H) and not hip.rnn_seq_supported(kind, H)
    k, named = CELLS[kind], "fused" if fused else "cell"
    s = bufs_of(kind, gi=pre, gh=gh, hin=hin, cin=cin, cnew=cnew, y=y)
    k.fwd(s, w.data_ptr(), b.data_ptr(), rp, N, H, C, path=named)
    out = dict(gates=pre.clone(), hin=hin.clone(), y=y.clone())
    out.update(dict(cin=cin.clone(), cnew=cnew.clone()) if kind == "lstm" else dict(gh=gh.clone()))
    if ld != H:   # the per-step cells read d y in rows of H: a view into a wider buffer is made dense first
        dense = nan(C, N, H)
        hip.copy2d(dyd.data_ptr(), ld, dense.data_ptr(), H, C * N, H)
        dyd = dense
    d_hin, d_cin = nan(C, N, H), nan(C, N, H)   # one carry per step, so that every step's is compared
    k.bwd(s, dyd.data_ptr(), H, w.data_ptr(), rp, N, H, C, lambda c: (P(d_hin, c), P(d_cin, c))[:len(k.state)], path=named)
    out["d_pre"], out["d_hin"] = pre, d_hin
    out.update(dict(d_cin=d_cin) if kind == "lstm" else dict(d_gh=gh))
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def bound(r64, r32, name):
    return A_F32 * float((r32[name] - r64[name]).abs().max()) + B_ABS * float(r64[name].abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fused_step_vs_float64(case):
    kind = case[0]
    inputs = make_inputs(*case)
    got = run_kernels(kind, inputs)
    r64, r32 = references(kind, inputs)
    report = []
    for name, v in got.items():
        assert torch.isfinite(v).all(), (name, "an element not written, or not finite")
        err, lim = float((v.double() - r64[name]).abs().max()), bound(r64, r32, name)
        report.append((name, err, lim))
    print(f"\nfused step {case}: worst err/bound {max(e / max(l, 1e-300) for _, e, l in report):.3f}")
    for name, err, lim in report:
        print(f"  {name:6s} err {err:.3e} bound {lim:.3e}")
    for name, err, lim in report:
        assert err <= lim, (name, err, lim)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_bar_can_fail(case):
    """CPU only, on the inputs of the kernel test: the reset applied one step late, GRU's b_hn outside r * (.) and LSTM's i and f
    swapped each move some compared tensor past its bound."""
    kind = case[0]
    inputs = make_inputs(*case)
    r64, r32 = references(kind, inputs)
    names = [k for k in r64 if not (kind == "lstm" and k in ("gh", "d_gh")) and not (kind == "gru" and k in ("cin", "cnew", "d_cin"))]
    applies = dict(reset_late=True, bhn_outside=kind == "gru", if_swap=kind == "lstm")
    for fault in FAULTS:
        if applies[fault]:
            bad = references(kind, inputs, fault=fault, only64=True)
            moved = max(float((bad[k] - r64[k]).abs().max()) / max(bound(r64, r32, k), 1e-300) for k in names)
            assert moved > 1, (fault, moved)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["gru", "lstm"])
@pytest.mark.parametrize("step", ["0", "1"])
def test_net_step_at_512_both_ways_vs_float64_oracle(kind, step, monkeypatch):
    """One trainer step of a recurrent actor-critic at H = 512 with the fused step and with the GEMM and the cell as
    two launches (``hip.RNN_STEP_FUSED`` cleared): both within the rule of tests/test_gpu_rnn.py's net-level test of the same float64 oracle."""
    from oracle.net import OracleActorCritic
    from oracle.trainer import OracleMappo
    from srl_amd.api import config, trainer as trainer_api
    from srl_amd.runtime import synthetic
    import srl_amd
    srl_amd.register_all()
    monkeypatch.setattr(hip, "RNN_STEP_FUSED", step == "1")
    H, layers, T, B = 512, 1, 20, 5
    assert hip.rnn_step_supported(kind, H) == (step == "1") and not hip.rnn_seq_supported(kind, H)
    pargs = dict(obs_dim=4, action_dim=2, hidden_dim=H, num_dense_layers=1, num_rnn_layers=layers, rnn_type=kind, popart=False,
                 layernorm=True, shared_backbone=True, chunk_len=10, seed=90)
    # (no clipping: at this width the gradient's norm exceeds the 10.0 of tests/test_gpu_rnn.py, and a clipped step leaves the oracle's
    # gradients scaled and the executor's raw)
    targs = dict(popart=False, optimizer_config=dict(lr=1e-3), max_grad_norm=1e6)
    arrays = synthetic.make_sample_arrays(seed=H, T=T, B=B, obs_spec=synthetic.CARTPOLE_OBS, action_dims=2, p_done=0.08,
                                          policy_state={"hx": (layers, 2 * H if kind == "lstm" else H)})
    trainer = trainer_api.make(config.Trainer("mappo", args=targs), config.Policy("actor-critic", args=pargs))
    net = trainer.policy.net
    sd = {k: v.numpy() for k, v in trainer.policy.get_checkpoint()["state_dict"].items()}
    res = trainer.step(synthetic.to_sample_batch(arrays))
    grads = net.flat_to_reference(net.grad.detach().cpu())
    oracles = {}
    for dt in (torch.float32, torch.float64):
        onet = OracleActorCritic(**pargs, dtype=dt)
        onet.load_state_dict(sd)
        ostats, _ = OracleMappo(onet, **targs).step(arrays)
        oracles[dt] = (onet, ostats)
    check_vs_float64(res.stats, grads, oracles, ("policy_loss", "value_loss", "entropy"))
