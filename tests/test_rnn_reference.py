"""The float64 restatement of a recurrent chunk (tests/rnn_ref.py) that tests/test_gpu_rnn.py holds the HIP kernels to, held in
turn to torch.nn.LSTM / torch.nn.GRU: without resets equal to the modules, with resets equal to the modules run segment by
segment from a zero state, and its hand-wired gradients equal to finite differences (torch.autograd.gradcheck)."""
import pytest
import torch

from rnn_ref import chunk

D = torch.float64


def _setup(kind, N, H, C, seed):
    g = torch.Generator().manual_seed(seed)
    mod = (torch.nn.LSTM if kind == "lstm" else torch.nn.GRU)(H, H).to(D)
    with torch.no_grad():
        for p in mod.parameters():
            p.copy_(torch.randn(p.shape, generator=g, dtype=D) / H ** 0.5)
    x = torch.randn(C, N, H, generator=g, dtype=D)
    h0, c0 = torch.randn(N, H, generator=g, dtype=D), torch.randn(N, H, generator=g, dtype=D)
    dy = torch.randn(C, N, H, generator=g, dtype=D)
    pre_x = x @ mod.weight_ih_l0.detach().T + mod.bias_ih_l0.detach()
    return mod, x, h0, c0, dy, pre_x


def _module_run(kind, mod, x, h0, c0, reset):
    """y of the module over the chunk, column by column, restarted from a zero state at every reset."""
    C, N, H = x.shape
    ys = torch.zeros(C, N, H, dtype=D)
    for b in range(N):
        cuts = [0] + [c for c in range(1, C) if reset is not None and reset[c, b]] + [C]
        h, cc = h0[b:b + 1][None], c0[b:b + 1][None]
        if reset is not None and reset[0, b]:
            h, cc = torch.zeros_like(h), torch.zeros_like(cc)
        for s, e in zip(cuts[:-1], cuts[1:]):
            if s > 0:
                h, cc = torch.zeros_like(h), torch.zeros_like(cc)
            if kind == "lstm":
                y, (h, cc) = mod(x[s:e, b:b + 1], (h, cc))
            else:
                y, h = mod(x[s:e, b:b + 1], h)
            ys[s:e, b] = y[:, 0]
    return ys


@pytest.mark.parametrize("kind", ["lstm", "gru"])
def test_equals_torch_modules_without_resets(kind):
    N, H, C = 5, 8, 6
    mod, x, h0, c0, dy, pre_x = _setup(kind, N, H, C, 1)
    ref = chunk(kind, pre_x, mod.weight_hh_l0.detach(), mod.bias_hh_l0.detach(), h0, c0, None, dy)
    hx = (h0[None], c0[None]) if kind == "lstm" else h0[None]
    xg = x.clone().requires_grad_(True)
    y, _ = mod(xg, hx)
    (y * dy).sum().backward()
    assert float((ref["y"] - y.detach()).abs().max()) <= 1e-12
    # d x = d pre_x . W_ih (pre_x = W_ih x + b_ih)
    assert float((ref["d_pre"] @ mod.weight_ih_l0.detach() - xg.grad).abs().max()) <= 1e-12
    if kind == "lstm":
        assert float((ref["cnew"][-1] - _[1][0].detach()).abs().max()) <= 1e-12


@pytest.mark.parametrize("kind", ["lstm", "gru"])
def test_equals_torch_modules_segment_by_segment_with_resets(kind):
    N, H, C = 7, 8, 9
    mod, x, h0, c0, dy, pre_x = _setup(kind, N, H, C, 2)
    reset = (torch.rand(C, N, generator=torch.Generator().manual_seed(3)) < 0.3).to(torch.uint8)
    reset[0, 0], reset[:, 1] = 1, 0   # a reset at step 0 over a non-zero stored state; a column without any
    reset[:, 2] = 1                   # a column reset at every step
    with torch.no_grad():
        ys = _module_run(kind, mod, x, h0, c0, reset)
    ref = chunk(kind, pre_x, mod.weight_hh_l0.detach(), mod.bias_hh_l0.detach(), h0, c0, reset, dy)
    assert float((ref["y"] - ys).abs().max()) <= 1e-12
    assert float(ref["hin"][reset.bool()].abs().max()) == 0.0
    # the gradient through the segments: d x of the module run with autograd equals d pre_x . W_ih
    xg = x.clone().requires_grad_(True)
    (_module_run(kind, mod, xg, h0, c0, reset) * dy).sum().backward()
    assert float((ref["d_pre"] @ mod.weight_ih_l0.detach() - xg.grad).abs().max()) <= 1e-12


@pytest.mark.parametrize("kind", ["lstm", "gru"])
def test_gradients_agree_with_gradcheck(kind):
    """The gradients the restatement reports -- d pre_x, the d hin / d cin carries, GRU's d gh -- folded into the gradients of
    its inputs (d b_hh = sum of d pre / d gh, d W_hh = sum of d pre^T hin / d gh^T hin, d h0 = d hin[0] where reset[0] is
    clear) against finite differences of its forward y, resets inside the chunk included."""
    N, H, C = 3, 4, 4
    G = 4 if kind == "lstm" else 3
    g = torch.Generator().manual_seed(4)
    args = [torch.randn(C, N, G * H, generator=g, dtype=D), torch.randn(G * H, H, generator=g, dtype=D) / 2,
            torch.randn(G * H, generator=g, dtype=D), torch.randn(N, H, generator=g, dtype=D), torch.randn(N, H, generator=g, dtype=D)]
    reset = torch.tensor([[0, 1, 0], [1, 0, 0], [0, 0, 0], [0, 1, 1]], dtype=torch.uint8)
    keep0 = 1 - reset[0, :, None].to(D)

    class Chunk(torch.autograd.Function):
        @staticmethod
        def forward(ctx, pre_x, w_hh, b_hh, h0, c0):
            ctx.save_for_backward(pre_x, w_hh, b_hh, h0, c0)
            with torch.enable_grad():
                return chunk(kind, pre_x, w_hh, b_hh, h0, c0, reset, torch.zeros(C, N, H, dtype=D))["y"]

        @staticmethod
        def backward(ctx, dy):
            with torch.enable_grad():
                r = chunk(kind, *ctx.saved_tensors, reset, dy)
            dq = r["d_pre"] if kind == "lstm" else r["d_gh"]
            dw = torch.einsum("cnj,cnk->jk", dq, r["hin"])
            dc0 = r["d_cin"][0] * keep0 if kind == "lstm" else torch.zeros(N, H, dtype=D)
            return r["d_pre"], dw, dq.sum((0, 1)), r["d_hin"][0] * keep0, dc0

    assert torch.autograd.gradcheck(Chunk.apply, [a.requires_grad_(True) for a in args])
