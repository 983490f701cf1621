"""The recurrent stack of the executor (`HipNet`): the auto-reset LSTM / GRU layers of a `GruSpec` (modules/autoreset_rnn.py:42-66)
forward and backward, and the row order of a recurrent pass.

The n = T*B rows of a pass are time-major; the layers want them chunk-major (step c of all T/C chunks side by side, N = (T/C)*B
rows per step).  `forward` / `backward` are the layer loop, once for both cells; `CELLS` holds what differs, the time loop of a
chunk included: `CELLS[kind].fwd / .bwd` on raw device addresses, on the path `time_loop_path` chooses or the caller names.
"""
from collections import namedtuple
from typing import NamedTuple, Optional

import torch

from srl_amd import hip


class RnnCtx(NamedTuple):
    """How the n = T*B time-major rows of a forward pass are laid out for the recurrent layers: chunks of C time
    steps (T % C == 0), N = (T/C)*B environment columns per step; h0[tag] float32 [layers, N, H] initial states
    ("a:" actor / shared backbone, "c:" critic backbone); reset uint8 [C, N] chunk-major on_reset flags, or None
    (rollout: the state is used as given, actor_critic_policy.py:476-481)."""
    T: int
    B: int
    C: int
    h0: dict
    reset: Optional[torch.Tensor]


# layers: per layer (its input rows, the cell's `Bufs` as the time loop left them); cm: the whole pass ran on chunk-major rows
RnnSaved = NamedTuple("RnnSaved", [("layers", list), ("ctx", RnnCtx), ("cm", bool)])


# The two cells.  `Bufs` / `fields`: the [n, width * H] buffers of a layer, named `{tag}{prefix}.{field}{l}`; both have `gi`
# (W_ih x + b_ih; d gi after the backward's time loop), `hin` (the state each step starts from) and `y`.  `state`: per H columns
# of the stored state, (where the masked state goes, where the time loop leaves it).  `d_hh`: what holds d(W_hh h + b_hh) after
# the backward's time loop.  `carries`: the [N, H] buffers the per-step backward hands from step to step, two of each.
#
# `fwd` / `bwd` are THE time loop of a chunk (C steps of N rows, step c at byte offset 4 c N width H of every buffer): the layer
# loop below, the kernel tests and scripts/rnn_step_bench.py all run these.  `s`: the cell's `Bufs` of raw device addresses;
# `r(c)`: the address of step c's reset flags, or None; `path`: one of PATHS, by default `time_loop_path`'s.  The backward of
# "fused" is "cell"'s (the fused step saves what the cell saves); it writes d h_in (d c_in) of step c to the addresses
# `carry(c)` gives, which stay untouched until step c - 1 has read them.
PATHS = ("seq", "fused", "cell")


def time_loop_path(kind: str, H: int, named: Optional[str] = None) -> str:
    """Where the path is chosen: the whole chunk in one launch (csrc/rnn_seq.hip) where the library has the width; else W_hh h and
    the cell of a step in one launch (csrc/rnn_step.hip); else srl_gemm plus a cell of csrc/gru.hip per step.  ``named``: the
    caller's choice instead (the tests' and the bench's reference sides)."""
    assert named is None or named in PATHS, named
    return named or ("seq" if hip.rnn_seq_supported(kind, H) else "fused" if hip.rnn_step_supported(kind, H) else "cell")


class _Lstm:
    """`gi` becomes the pre-activations W_ih x + b_ih + W_hh h + b_hh, then the activated gates i|f|g|o, then their gradient."""
    kind, gates, carries, d_hh = "lstm", 4, ("dh0", "dc0", "dh1", "dc1"), "gi"
    Bufs, fields = namedtuple("LstmBufs", "gi hin cin cnew y"), (("gi", 4), ("hin", 1), ("cin", 1), ("cnew", 1), ("y", 1))
    state = (("hin", "y"), ("cin", "cnew"))   # cat(h, c) per row (autoreset_rnn.py:31-39); both halves are reset together

    def fwd(self, s, w_hh, b_hh, r, N, H, C, path=None):
        path = time_loop_path(self.kind, H, path)
        pre, hin, cin, cnew, y = s
        if path == "seq":
            return hip.lstm_seq_fwd(pre, w_hh, b_hh, hin, cin, r(0), N, H, C, y, cnew)
        for c in range(C):
            o4, o1, o1n, nxt = 4 * c * N * 4 * H, 4 * c * N * H, 4 * (c + 1) * N * H, c + 1 < C
            out = (r(c + 1) if nxt else None, N, H, y + o1, cnew + o1, hin + o1n if nxt else None, cin + o1n if nxt else None)
            if path == "fused":   # the product and the cell in one launch
                hip.lstm_step_fwd(pre + o4, w_hh, b_hh, hin + o1, cin + o1, *out)
                continue
            hip.gemm(N, 4 * H, H, hin + o1, H, 0, w_hh, H, 0, pre + o4, 4 * H, bias=b_hh, accumulate=True)
            hip.lstm_cell_fwd(pre + o4, cin + o1, *out)

    def bwd(self, s, dy, ld_dy, w_hh, r, N, H, C, carry, path=None):
        path = time_loop_path(self.kind, H, path)
        assert path == "seq" or ld_dy == H, "the per-step cells read d y in rows of H"
        pre, _, cin, cnew, _ = s
        if path == "seq":
            return hip.lstm_seq_bwd(dy, ld_dy, pre, w_hh, cin, cnew, r(0), N, H, C)
        ch = cc = None
        for c in range(C - 1, -1, -1):
            o4, o1, (dh, dc) = 4 * c * N * 4 * H, 4 * c * N * H, carry(c)
            hip.lstm_cell_bwd(dy + 4 * c * N * ld_dy, ch, cc, r(c + 1) if c + 1 < C else None, pre + o4, cin + o1, cnew + o1, N, H, dc)
            hip.gemm(N, H, 4 * H, pre + o4, 4 * H, 0, w_hh, H, 1, dh, H)  # d h_in(c) = d pre . W_hh
            ch, cc = dh, dc


class _Gru:
    """`gh` = W_hh h + b_hh stays apart from `gi` (b_hn sits inside r * (.)); both become their gradients."""
    kind, gates, carries, d_hh = "gru", 3, ("dh0", "dh1"), "gh"
    Bufs, fields = namedtuple("GruBufs", "gi gh hin y"), (("gi", 3), ("gh", 3), ("hin", 1), ("y", 1))
    state = (("hin", "y"),)

    def fwd(self, s, w_hh, b_hh, r, N, H, C, path=None):
        path = time_loop_path(self.kind, H, path)
        gi, gh, hin, y = s
        if path == "seq":
            return hip.gru_seq_fwd(gi, gh, w_hh, b_hh, hin, r(0), N, H, C, y)
        for c in range(C):
            o3, o1, nxt = 4 * c * N * 3 * H, 4 * c * N * H, c + 1 < C
            out = (r(c + 1) if nxt else None, N, H, y + o1, hin + 4 * (c + 1) * N * H if nxt else None)
            if path == "fused":   # the product and the cell in one launch
                hip.gru_step_fwd(gi + o3, gh + o3, w_hh, b_hh, hin + o1, *out)
                continue
            hip.gemm(N, 3 * H, H, hin + o1, H, 0, w_hh, H, 0, gh + o3, 3 * H, bias=b_hh)
            hip.gru_cell_fwd(gi + o3, gh + o3, hin + o1, *out)

    def bwd(self, s, dy, ld_dy, w_hh, r, N, H, C, carry, path=None):
        path = time_loop_path(self.kind, H, path)
        assert path == "seq" or ld_dy == H, "the per-step cells read d y in rows of H"
        gi, gh, hin, _ = s
        if path == "seq":
            return hip.gru_seq_bwd(dy, ld_dy, gi, gh, w_hh, hin, r(0), N, H, C)
        prev = None
        for c in range(C - 1, -1, -1):
            o3, o1, (cur,) = 4 * c * N * 3 * H, 4 * c * N * H, carry(c)
            hip.gru_cell_bwd(dy + 4 * c * N * ld_dy, prev, r(c + 1) if c + 1 < C else None, gi + o3, gh + o3, hin + o1, N, H, cur)
            # d h_in(c) = dh*z + d gh . W_hh: the carry of step c-1 (masked there by on_reset[c])
            hip.gemm(N, H, 3 * H, gh + o3, 3 * H, 0, w_hh, H, 1, cur, H, accumulate=True)
            prev = cur


CELLS = {"lstm": _Lstm(), "gru": _Gru()}


def bufs_of(kind: str, **tensors):
    """The cell's `Bufs` of the addresses of the torch tensors named by field (other names are ignored): for the callers of the
    time loop outside `HipNet`."""
    return CELLS[kind].Bufs(*[tensors[f].data_ptr() for f in CELLS[kind].Bufs._fields])


def _encoders(spec):
    return list(spec.obs_encoders) + ([] if spec.shared_backbone else list(spec.state_encoders))


def chunk_major(spec, rnn: Optional[RnnCtx], obs) -> bool:
    """Whether a whole pass runs on chunk-major rows: recurrent nets over vector observations, more than one chunk.  Only the
    recurrent layers care about row order.  Instead of re-ordering the 64-wide features in front of and behind every recurrent
    layer, in both directions (8 launches, 0.45 ms of the SMAC-sized step), the OBSERVATIONS are re-ordered once (`obs_chunk_major`),
    and only the heads' outputs (`heads_time_major`) and their gradients on the way back (`rows`) change order: a fifth of the bytes."""
    return bool(spec.num_rnn_layers and rnn is not None and rnn.T // rnn.C > 1 and spec.std_type != "shared_learnable"
                and spec.aux_head is None
                and all(isinstance(x, torch.Tensor) and x.dim() == 2 and x.dtype == torch.float32 and x.is_contiguous()
                        for x in [obs.get(e.key) for e in _encoders(spec)]))


def obs_chunk_major(net, rnn: RnnCtx, obs: dict) -> dict:
    """`obs` with the leaf of every encoder in chunk-major order (copies in the workspace)."""
    obs = dict(obs)
    for key in {e.key for e in _encoders(net.spec)}:
        x = obs[key]
        obs[key] = net.ws.get(f"cm.obs.{key}", x.numel())[:x.numel()].view(x.shape)
        hip.chunk_rows(x.data_ptr(), obs[key].data_ptr(), rnn.T, rnn.B, rnn.C, x.shape[1])
    return obs


def heads_time_major(rnn: RnnCtx, *heads):
    """``heads``: (chunk-major output, where its time-major rows go, columns) per head."""
    for src, dst, cols in heads:
        hip.chunk_rows(src.data_ptr(), dst.data_ptr(), rnn.T, rnn.B, rnn.C, cols, inverse=True)


def rows(net, rnn: RnnCtx, name: str, x, inverse=False):
    """The dense rows of the Buf ``x`` chunk-major (``inverse``: time-major again) in the workspace buffer ``name``."""
    assert x.ld == x.cols
    out = net._buf(name, x.rows, x.cols)
    hip.chunk_rows(x.ptr, out.ptr, rnn.T, rnn.B, rnn.C, x.cols, inverse=inverse)
    return out


def forward(net, G, x, tag: str, ctx: RnnCtx, cm: bool):
    """x: [T*B, I0], time-major (chunk-major when ``cm``).  Returns (y [T*B, H] in the same order, RnnSaved, last states
    [layers, N, state width])."""
    k, C, H, I0, SW, name = CELLS[G.kind], ctx.C, G.hidden, G.input_dim, G.state_width, f"{tag}{G.prefix}"
    n, N, rs = ctx.T * ctx.B, ctx.T // C * ctx.B, ctx.reset
    r = (lambda c: rs.data_ptr() + c * N) if rs is not None else (lambda c: None)   # step -> its reset flags
    assert x.rows == n and x.cols == I0 and x.ld == I0 and ctx.T % C == 0   # (layer 0 reads I0 columns, the others H)
    reorder = ctx.T > C and not cm   # (else: one chunk, or the whole pass runs on chunk-major rows already)
    inp = rows(net, ctx, f"{name}.xc", x) if reorder else x
    h0 = ctx.h0[tag]
    assert tuple(h0.shape) == (G.layers, N, SW) and h0.dtype == torch.float32 and h0.is_contiguous()
    last = net.ws.get(f"{name}.last", G.layers * N * SW)[:G.layers * N * SW].view(G.layers, N, SW)
    saved, end = [], 4 * (C - 1) * N * H
    for l in range(G.layers):
        w_ih, w_hh = net._p(f"{G.prefix}.weight_ih_l{l}"), net._p(f"{G.prefix}.weight_hh_l{l}")
        b_ih, b_hh = net._p(f"{G.prefix}.bias_ih_l{l}"), net._p(f"{G.prefix}.bias_hh_l{l}")
        s = k.Bufs(*[net._buf(f"{name}.{f}{l}", n, w * H) for f, w in k.fields])
        hip.gemm(n, k.gates * H, inp.cols, inp.ptr, inp.ld, 0, w_ih, inp.cols, 0, s.gi.ptr, k.gates * H, bias=b_ih)  # every step at once
        for j, (first, _) in enumerate(k.state):
            src = h0[l].data_ptr() + 4 * j * H
            if SW != H:   # a split state: its H columns made dense first (y is free until the time loop)
                hip.copy2d(src, SW, s.y.ptr, H, N, H)
                src = s.y.ptr
            hip.gru_mask_state(src, r(0), N, H, getattr(s, first).ptr)
        k.fwd(k.Bufs(*[b.ptr for b in s]), w_hh, b_hh, r, N, H, C)   # the time loop: in one launch, or step by step
        for j, (_, final) in enumerate(k.state):
            hip.copy2d(getattr(s, final).ptr + end, H, last[l].data_ptr() + 4 * j * H, SW, N, H)
        saved.append((inp, s))
        inp = s.y
    return (rows(net, ctx, f"{name}.ytm", inp, inverse=True) if reorder else inp), RnnSaved(saved, ctx, cm), last


def backward(net, G, saved: RnnSaved, dy, in_act: int, need_dx: bool, tag: str):
    """dy: d loss / d y in the forward's row order.  Accumulates the parameter gradients; returns d loss / d x before the
    producer's activation ``in_act`` (None unless ``need_dx``)."""
    k, ctx, H, name = CELLS[G.kind], saved.ctx, G.hidden, f"{tag}{G.prefix}"
    n, N, rs, reorder = ctx.T * ctx.B, ctx.T // ctx.C * ctx.B, ctx.reset, ctx.T > ctx.C and not saved.cm
    r = (lambda c: rs.data_ptr() + c * N) if rs is not None else (lambda c: None)
    dout = rows(net, ctx, f"{name}.dyc", dy) if reorder else dy
    for l in range(G.layers - 1, -1, -1):
        inp, s = saved.layers[l]
        w_ih, w_hh = net._p(f"{G.prefix}.weight_ih_l{l}"), net._p(f"{G.prefix}.weight_hh_l{l}")
        carry, per = [net._buf(f"{name}.{b}", N, H).ptr for b in k.carries], len(k.carries) // 2   # two alternating sets
        k.bwd(k.Bufs(*[b.ptr for b in s]), dout.ptr, dout.ld, w_hh, r, N, H, ctx.C, lambda c: carry[per * (c & 1):][:per])
        # parameter gradients over all steps at once (the bias gradients, column sums, come out of the same kernels)
        net._wgrad(k.gates * H, H, n, getattr(s, k.d_hh), s.hin.ptr, H, net._g(f"{G.prefix}.weight_hh_l{l}"),
                   net._g(f"{G.prefix}.bias_hh_l{l}"))
        net._wgrad(k.gates * H, inp.cols, n, s.gi, inp.ptr, inp.ld, net._g(f"{G.prefix}.weight_ih_l{l}"),
                   net._g(f"{G.prefix}.bias_ih_l{l}"))
        if l == 0 and not need_dx:
            return None
        dout = net._buf(f"{name}.dx{l}", n, inp.cols)
        act = in_act if l == 0 else 0  # layer 0 reads the (activated) output of the dense stack
        hip.gemm(n, inp.cols, k.gates * H, s.gi.ptr, k.gates * H, 0, w_ih, inp.cols, 1, dout.ptr, inp.cols,
                 dact_src=inp.ptr if act else None, ld_dact=inp.ld, dact=act)
    return rows(net, ctx, f"{name}.dxt", dout, inverse=True) if reorder else dout
