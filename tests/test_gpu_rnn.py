"""The recurrent kernels, entry point by entry point, against a float64 restatement of the auto-reset LSTM / GRU (tests/rnn_ref.py).

Two paths carry a chunk of C steps over N rows, and both are driven here by the time loop `rnnpath.forward / backward` runs
(`rnnpath.CELLS[kind].fwd / .bwd`, the path named), on the same buffers (`pre` / `gi` = W_ih x + b_ih, `hin[0]` / `cin[0]` masked by srl_gru_mask_state, `reset[c]` for c in [0, C)):
  seq   srl_{lstm,gru}_seq_{fwd,bwd} (csrc/rnn_seq.hip): the whole time loop in one launch, H in {32, 64}, gates on the hardware's
        exp2 / rcp (SRL_RNN_FASTMATH);
  step  srl_gemm (W_hh h) + srl_{lstm,gru}_cell_{fwd,bwd} (csrc/gru.hip) per step: every other width, and H in {32, 64} with
        SRL_RNN_SEQ=0.
Every buffer the kernels write is compared element by element with float64: the activated gates, GRU's gh, hin[1:], cin[1:], y,
cnew; d pre / d gi, d gh; on the step path the carries d hin / d cin between steps.

Tolerance: each tensor's error against float64 is held to  a * max|f32 - f64| + b * max|f64|,  where f32 is the same restatement
evaluated in float32 on the CPU (what an honest float32 evaluation of this arithmetic costs) and (a, b) are fixed per path.  Set
from the largest ratios measured on an MI355X over this file's matrix (error / max|f32 - f64| and error / max|f64|, per tensor):
  step  the cells run libm expf / tanhf: the largest error was 1.9x the float32 restatement's -> a = 4, b = 1e-7 (a floor for
        tensors the float32 restatement gets exactly; largest error / bound 0.37);
  seq   the gates' exp2 / rcp: up to 3.3x the float32 restatement's error, and near 0 (`tiny`, tanh's absolute-error regime)
        8.5e-8 absolute on values of 0.03, 18.6x the float32 restatement's error and 2.8e-6 of the largest element
        -> a = 6, b = 5e-6 (largest error / bound 0.47).  Saturated gates are no worse on either path: where 1 - s(x) rounds to
        0 both float32 evaluations lose the gradient alike.
`test_tolerances_can_fail` shows on the same inputs that each of five plausible faults of the restatement moves some tensor by
more than 10x its bound."""
import zlib

import numpy as np
import pytest
import torch

from rnn_ref import FAULTS, check_vs_float64, chunk
from srl_amd import hip
from srl_amd.algorithm.rnnpath import CELLS, bufs_of

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BOUNDS = {"step": (4.0, 1e-7), "seq": (6.0, 5e-6)}

# (kind, H, N, C, resets, scale, extra columns of the dy buffer)
#   N: 1, 31, 33, 129 around the 32-row tiles; 30 720 = SMAC's rows; 32 768 + 33: past the time loop's grid of 256 workgroups x
#   4 wavefronts x 32 rows, so a second grid pass with a ragged 1-row tile.  resets: none (a null pointer), bern (20 %), all,
#   tail (only in the last tile's rows), step0 (only at step 0, over a non-zero stored state).  scale: normal; sat (pre-activations
#   |x| in [20, 60], saturated gates); tiny (|x| ~ 1e-2: tanh near 0, where the fast-math gates' error is absolute).
TIME_LOOP = [  # H in {32, 64}: seq, and step with SRL_RNN_SEQ=0
    ("lstm", 32, 1, 1, "none", "normal", 0),
    ("gru", 32, 31, 10, "bern", "normal", 0),
    ("lstm", 64, 33, 64, "bern", "normal", 0),
    ("gru", 64, 129, 2, "all", "normal", 0),
    ("lstm", 64, 129, 10, "step0", "normal", 0),
    ("gru", 32, 33, 64, "step0", "normal", 0),
    ("lstm", 64, 30720, 2, "bern", "normal", 0),
    ("gru", 64, 30720, 1, "none", "normal", 0),
    ("gru", 32, 32801, 2, "tail", "normal", 0),
    ("lstm", 32, 32801, 2, "tail", "normal", 0),
    ("lstm", 32, 129, 10, "bern", "sat", 0),
    ("gru", 64, 33, 10, "bern", "sat", 0),
    ("lstm", 64, 31, 10, "bern", "tiny", 0),
    ("gru", 32, 129, 10, "bern", "tiny", 0),
]
LD_DY = [  # dy a view into a wider buffer (ld_dy > H): the time loop's entry points take ld_dy, the cells read rows of H
    ("lstm", 32, 33, 10, "bern", "normal", 7),
    ("gru", 64, 129, 10, "bern", "normal", 32),
]
PER_STEP = [  # the other widths: 16, 48 and 128 (the football and overcooked presets)
    ("gru", 16, 1, 1, "none", "normal", 0),
    ("lstm", 16, 33, 10, "bern", "normal", 0),
    ("gru", 48, 129, 10, "bern", "normal", 0),
    ("lstm", 48, 31, 64, "step0", "normal", 0),
    ("lstm", 128, 129, 10, "bern", "normal", 0),
    ("gru", 128, 129, 10, "all", "normal", 0),
    ("lstm", 128, 32801, 2, "tail", "normal", 0),
    ("gru", 128, 30720, 2, "bern", "normal", 0),
    ("lstm", 128, 33, 10, "bern", "sat", 0),
    ("gru", 128, 33, 10, "bern", "tiny", 0),
]
RUNS = ([pytest.param("seq", c, id="seq-" + "-".join(map(str, c))) for c in TIME_LOOP + LD_DY]
        + [pytest.param("step", c, id="step-" + "-".join(map(str, c))) for c in TIME_LOOP + PER_STEP])


def make_inputs(kind, H, N, C, resets, scale, extra):
    """float32 CPU tensors, seeded by the case: pre_x, w_hh, b_hh, h0, c0, reset (uint8 [C, N] or None), dy [C, N, H + extra]."""
    G = 4 if kind == "lstm" else 3
    g = torch.Generator().manual_seed(zlib.crc32(repr((kind, H, N, C, resets, scale, extra)).encode()))
    rn = lambda *s: torch.randn(*s, generator=g)
    w_hh, b_hh = rn(G * H, H) / H ** 0.5, 0.1 * rn(G * H)
    pre_x = rn(C, N, G * H)
    h0, c0 = 0.5 * rn(N, H), 0.5 * rn(N, H)
    if scale == "sat":
        pre_x = torch.sign(pre_x) * (20 + 40 * torch.rand(C, N, G * H, generator=g))
    elif scale == "tiny":
        pre_x, w_hh, b_hh, h0, c0 = 0.02 * pre_x, 0.02 * w_hh, 0.1 * b_hh, 0.04 * h0, 0.04 * c0
    reset = None
    if resets == "bern":
        reset = (torch.rand(C, N, generator=g) < 0.2).to(torch.uint8)
    elif resets == "all":
        reset = torch.ones(C, N, dtype=torch.uint8)
    elif resets == "tail":
        reset = torch.zeros(C, N, dtype=torch.uint8)
        reset[1::2, 32 * ((N - 1) // 32):] = 1
        reset[0, N - 1] = 1
    elif resets == "step0":
        reset = torch.zeros(C, N, dtype=torch.uint8)
        reset[0] = (torch.rand(N, generator=g) < 0.5).to(torch.uint8)
    dy = rn(C, N, H + extra)
    return pre_x, w_hh, b_hh, h0, c0, reset, dy


def references(kind, inputs):
    pre_x, w_hh, b_hh, h0, c0, reset, dy = inputs
    H = w_hh.shape[1]
    r64 = chunk(kind, pre_x.double(), w_hh.double(), b_hh.double(), h0.double(), c0.double(), reset, dy[..., :H].double())
    r32 = chunk(kind, pre_x, w_hh, b_hh, h0, c0, reset, dy[..., :H])
    return r64, r32


def run_kernels(kind, path, inputs):
    """The buffers `HipNet` hands the kernels, its forward and backward time loop of one chunk, and what the kernels leave in them.
    Output buffers start as NaN: an element a kernel fails to write shows."""
    pre_x, w_hh, b_hh, h0, c0, reset, dy = inputs
    C, N, GH = pre_x.shape
    H = w_hh.shape[1]
    ld = dy.shape[2]
    d = lambda t: t.to(DEV).contiguous()
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    pre, w, b = d(pre_x), d(w_hh), d(b_hh)
    gh, hin, cin, y, cnew = nan(C, N, 3 * H), nan(C, N, H), nan(C, N, H), nan(C, N, H), nan(C, N, H)
    rs = None if reset is None else d(reset)
    rp = (lambda c: rs.data_ptr() + c * N) if rs is not None else (lambda c: None)
    h0d, c0d, dyd = d(h0), d(c0), d(dy)
    P = lambda t, c=0: t[c].data_ptr()
    hip.gru_mask_state(h0d.data_ptr(), rp(0), N, H, hin.data_ptr())
    if kind == "lstm":
        hip.gru_mask_state(c0d.data_ptr(), rp(0), N, H, cin.data_ptr())
    seq = hip.rnn_seq_supported(kind, H)
    assert seq == (path == "seq")
    k, named = CELLS[kind], "seq" if seq else "cell"   # "cell": csrc/gru.hip's cells at H = 128 too (the fused step: test_gpu_rnn_step.py)
    s = bufs_of(kind, gi=pre, gh=gh, hin=hin, cin=cin, cnew=cnew, y=y)
    k.fwd(s, w.data_ptr(), b.data_ptr(), rp, N, H, C, path=named)
    out = dict(gates=pre.clone(), hin=hin.clone(), y=y.clone())
    out.update(dict(cin=cin.clone(), cnew=cnew.clone()) if kind == "lstm" else dict(gh=gh.clone()))
    d_hin, d_cin = nan(C, N, H), nan(C, N, H)   # one carry per step, so that every step's is compared
    k.bwd(s, dyd.data_ptr(), ld, w.data_ptr(), rp, N, H, C, lambda c: (P(d_hin, c), P(d_cin, c))[:len(k.state)], path=named)
    out["d_pre"] = pre
    if kind == "gru":
        out["d_gh"] = gh
    if not seq:
        out["d_hin"] = d_hin
        if kind == "lstm":
            out["d_cin"] = d_cin
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def bound(path, r64, r32, name):
    a, b = BOUNDS[path]
    return a * float((r32[name] - r64[name]).abs().max()) + b * float(r64[name].abs().max())


@pytest.mark.parametrize("path,case", RUNS)
def test_rnn_kernels_vs_float64(path, case, monkeypatch):
    kind = case[0]
    if path == "step":
        monkeypatch.setenv("SRL_RNN_SEQ", "0")
    inputs = make_inputs(*case)
    got = run_kernels(kind, path, inputs)
    r64, r32 = references(kind, inputs)
    worst, report = 0.0, []
    for name, v in got.items():
        assert torch.isfinite(v).all(), (name, "an element not written, or not finite")
        err = float((v.double() - r64[name]).abs().max())
        lim = bound(path, r64, r32, name)
        e32 = float((r32[name] - r64[name]).abs().max())
        scale = float(r64[name].abs().max())
        report.append((name, err, lim, err / max(e32, 1e-300), err / max(scale, 1e-300)))
        worst = max(worst, err / max(lim, 1e-300))
    print(f"\nRNN {path} {case} worst err/bound {worst:.3f}")
    for name, err, lim, re32, rsc in report:
        print(f"  {name:6s} err {err:.3e} bound {lim:.3e}  err/f32err {re32:.3f}  err/max {rsc:.3e}")
    for name, err, lim, _, _ in report:
        assert err <= lim, (name, err, lim)


@pytest.mark.parametrize("case", TIME_LOOP + LD_DY + PER_STEP, ids=lambda c: "-".join(map(str, c)))
def test_tolerances_can_fail(case):
    """CPU only, on the inputs of the kernel test: each plausible fault of the float64 restatement (rnn_ref.FAULTS: the reset one
    step late, the carry not cut at a reset in the backward, GRU's b_hn outside r * (.), LSTM's i and f swapped, the last row of
    the last tile dropped) moves some compared tensor by more than 10x the looser of the bounds its paths are held to."""
    kind, H, N, C = case[:4]
    inputs = make_inputs(*case)
    reset = inputs[5]
    r64, r32 = references(kind, inputs)
    paths = ["step"] + (["seq"] if H in (32, 64) else [])
    names = [k for k in r64 if not (kind == "lstm" and k in ("gh", "d_gh")) and not (kind == "gru" and k in ("cin", "cnew", "d_cin"))]
    lims = {k: max(bound(p, r64, r32, k) for p in paths) for k in names}
    applies = dict(reset_late=reset is not None and bool(reset.any()),
                   carry_not_cut=reset is not None and C > 1 and bool(reset[1:].any()),
                   bhn_outside=kind == "gru", if_swap=kind == "lstm", row_dropped=True)
    pre_x, w_hh, b_hh, h0, c0, reset, dy = inputs
    for fault in FAULTS:
        if not applies[fault]:
            continue
        bad = chunk(kind, pre_x.double(), w_hh.double(), b_hh.double(), h0.double(), c0.double(), reset, dy[..., :H].double(),
                    fault=fault)
        moved = max(float((bad[k] - r64[k]).abs().max()) / max(lims[k], 1e-300) for k in names)
        assert moved > 10, (fault, moved)


def test_chunk_rows_and_mask_state_helpers():
    """srl_chunk_rows (time-major rows [T][B] <-> chunk-major [C][K B], K = T / C chunks) forward and inverse against the numpy
    index permutation, odd row widths and T = C included; srl_gru_mask_state (h * (1 - on_reset) per row) with and without a
    reset vector."""
    rng = np.random.default_rng(0)
    for T, B, C, D in [(20, 3, 10, 5), (10, 7, 10, 1), (12, 1, 4, 33), (64, 5, 8, 128), (30, 1024, 10, 3)]:
        K = T // C
        x = rng.standard_normal((T * B, D)).astype(np.float32)
        perm = x.reshape(K, C, B, D).transpose(1, 0, 2, 3).reshape(T * B, D)   # row (c, k B + b) <- row ((k C + c) B + b)
        src, dst, back = torch.from_numpy(x).to(DEV), torch.full((T * B, D), np.nan, device=DEV), torch.full((T * B, D), np.nan, device=DEV)
        hip.chunk_rows(src.data_ptr(), dst.data_ptr(), T, B, C, D)
        hip.chunk_rows(dst.data_ptr(), back.data_ptr(), T, B, C, D, inverse=True)
        assert np.array_equal(dst.cpu().numpy(), perm), (T, B, C, D)
        assert np.array_equal(back.cpu().numpy(), x), (T, B, C, D)
    for N, H in [(1, 1), (37, 5), (300, 64), (4099, 128)]:
        h = torch.from_numpy(rng.standard_normal((N, H)).astype(np.float32)).to(DEV)
        r = torch.from_numpy((rng.random(N) < 0.4).astype(np.uint8)).to(DEV)
        out = torch.full((N, H), np.nan, device=DEV)
        hip.gru_mask_state(h.data_ptr(), r.data_ptr(), N, H, out.data_ptr())
        assert torch.equal(out, torch.where(r[:, None].bool(), torch.zeros_like(h), h))
        hip.gru_mask_state(h.data_ptr(), None, N, H, out.data_ptr())
        assert torch.equal(out, h)


# ------------------------------------------------------------------------------------------------ whole recurrent nets
NET_CASES = [  # (kind, H, layers, T, B, SRL_RNN_SEQ): chunk_len 10, ragged B
    ("gru", 32, 1, 20, 16411, "1"),   # N = T B / C = 32 822 rows: the time loop's second grid pass
    ("gru", 64, 2, 20, 37, "1"),
    ("lstm", 48, 1, 30, 29, "1"),     # per-step (no time-loop kernel for 48)
    ("gru", 128, 1, 20, 19, "1"),     # per-step: the football / overcooked width
    ("lstm", 128, 1, 20, 19, "1"),
    ("lstm", 64, 1, 20, 23, "1"),
    ("lstm", 64, 1, 20, 23, "0"),
    ("lstm", 32, 2, 20, 5, "1"),      # two LSTM layers (layer 1 reads layer 0's y): the time loop
    ("lstm", 16, 2, 20, 5, "1"),      # ... and per-step
]


@pytest.mark.parametrize("kind,H,layers,T,B,seq", NET_CASES, ids=lambda v: str(v))
def test_recurrent_net_step_vs_float64_oracle(kind, H, layers, T, B, seq, monkeypatch):
    """One trainer step of a recurrent actor-critic (dense layer -> LayerNorm -> auto-reset GRU / LSTM -> rnn_norm -> heads) against
    the float64 `OracleActorCritic`: every tensor's gradient -- the recurrent weights and rnn_norm included -- and the loss terms
    within 3x the float32 oracle's error plus 2e-6 of the largest element."""
    from oracle.net import OracleActorCritic
    from oracle.trainer import OracleMappo
    from srl_amd.api import config, trainer as trainer_api
    from srl_amd.runtime import synthetic
    import srl_amd
    srl_amd.register_all()
    monkeypatch.setenv("SRL_RNN_SEQ", seq)
    assert hip.rnn_seq_supported(kind, H) == (seq == "1" and H in (32, 64))
    pargs = dict(obs_dim=4, action_dim=2, hidden_dim=H, num_dense_layers=1, num_rnn_layers=layers, rnn_type=kind, popart=False,
                 layernorm=True, shared_backbone=True, chunk_len=10, seed=40 + H + layers)
    targs = dict(popart=False, optimizer_config=dict(lr=1e-3), max_grad_norm=10.0)
    SW = 2 * H if kind == "lstm" else H
    arrays = synthetic.make_sample_arrays(seed=H, T=T, B=B, obs_spec=synthetic.CARTPOLE_OBS, action_dims=2, p_done=0.08,
                                          policy_state={"hx": (layers, SW)})
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

