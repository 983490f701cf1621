"""A plain restatement of the DMLab instruction encoder as the HIP kernel sees it (csrc/instr_lstm.hip, include/srl_hip.h:
srl_instr_lstm_*), in torch on the CPU with autograd for the backward, and the seeded cases the kernel is held to beyond a
workgroup's first tile (tests/test_gpu_instr_lstm.py).

Run in float64 it is the reference; run in float32 it measures how far an honest float32 evaluation of the same arithmetic lands
from float64, which sets the tolerance (tests/rnn_ref.py).  tests/test_instr_lstm_reference.py holds it against the golden blocks
of the real reference (tests/golden/instr_lstm_blocks.npz).

Per row of tokens [L]: a token is its value truncated towards zero, and padding (0) when that lies outside [1, V) or is not a
number (test_gpu_dmlab.py::test_block_treats_out_of_range_tokens_as_padding); len = max(1, number of non-zero tokens); the FIRST
len tokens, zeros inside that prefix included, are looked up in the table (row 0 is read from the parameter and never receives
gradient); torch's LSTM arithmetic (gates i | f | g | o, both biases) runs over them from a zero state; the feature is h at step
len - 1.  Parameters go by the reference's names (dmlab_cases.BLOCK_PARAMS).
`FAULTS` are deliberate errors of this restatement, used only to show that the tolerances can fail."""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

FAULTS = ("later_tiles_dropped", "len_off_by_one", "row0_gets_gradient")
EMB, W_IH, W_HH, B_IH, B_HH = ("word_embedding.weight", "instructions_lstm.weight_ih_l0", "instructions_lstm.weight_hh_l0",
                               "instructions_lstm.bias_ih_l0", "instructions_lstm.bias_hh_l0")


def read_tokens(tok, V):
    """[n, L] int64: float32 / int32 token values as the kernel reads them."""
    tok = np.asarray(tok)
    if tok.dtype.kind == "f":
        ok = (tok >= 1.0) & (tok < float(V))   # (false for NaN)
        return np.where(ok, np.trunc(np.where(ok, tok, 0.0)), 0.0).astype(np.int64)
    return np.where((tok > 0) & (tok < V), tok, 0).astype(np.int64)


def encoder(params, tok, cot, dtype, fault=None, fault_row=None):
    """params: name -> array; tok [n, L]; cot [n, H] = d loss / d out.  Computes in ``dtype``; returns numpy arrays:
    out [n, H] and {name: gradient}."""
    p = OrderedDict((k, torch.as_tensor(np.asarray(v)).to(dtype).clone().requires_grad_(True)) for k, v in params.items())
    V, H = p[EMB].shape[0], p[W_HH].shape[1]
    tok = torch.from_numpy(read_tokens(tok, V))
    n, L = tok.shape
    lens = (tok != 0).sum(-1).clamp(min=1)
    if fault == "len_off_by_one":   # a time loop that runs `t <= len`
        lens = (lens + 1).clamp(max=L)
    h = c = torch.zeros(n, H, dtype=dtype)
    for t in range(int(lens.max())):
        x = F.embedding(tok[:, t], p[EMB], padding_idx=None if fault == "row0_gets_gradient" else 0)
        i, f, g, o = (x @ p[W_IH].T + p[B_IH] + h @ p[W_HH].T + p[B_HH]).chunk(4, -1)
        c2 = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h2 = torch.sigmoid(o) * torch.tanh(c2)
        on = (t < lens).unsqueeze(-1)
        h, c = torch.where(on, h2, h), torch.where(on, c2, c)
    seen = torch.ones(n, 1, dtype=dtype)
    if fault == "later_tiles_dropped":   # rows from `fault_row` on add nothing to the gradients
        seen[fault_row:] = 0
    (h * torch.as_tensor(np.asarray(cot)).to(dtype) * seen).sum().backward()
    return h.detach().numpy(), OrderedDict((k, v.grad.numpy()) for k, v in p.items())


# name: (V, Ed, H, L)
CASES = OrderedDict([
    ("many_tiles_h64", (1000, 20, 64, 12)),   # forward and backward over 2-3 tiles per workgroup; register dW sums over tiles
    ("many_tiles_h32", (30, 8, 32, 9)),       # instr_lstm_kernel<1, ...>
    ("one_slab_h64", (1000, 20, 64, 16)),     # backward through one workgroup's workspace
    ("one_slab_h32", (30, 7, 32, 9)),         # the same, Ed odd (padded to EdP)
    ("longest", (50, 20, 64, 64)),            # L = 64
])


def draw_case(name, rows, seed):
    """Seeded data of case ``name``: the table N(0, 1) (row 0 included: a checkpoint may hold anything there), weights N(0, 1 / in),
    biases 0.1 N, a standard normal cotangent; token rows of every kind -- empty, full-length, a random prefix, zeros inside the
    prefix, one more token behind a gap -- and a few out-of-range tokens in rows whose cotangent is zero.  Tokens are float32.
    Returns dict(V, Ed, H, L, params, tok, cot)."""
    V, Ed, H, L = CASES[name]
    rng = np.random.default_rng(seed)
    params = OrderedDict([(EMB, rng.standard_normal((V, Ed))), (W_IH, rng.standard_normal((4 * H, Ed)) / np.sqrt(Ed)),
                          (W_HH, rng.standard_normal((4 * H, H)) / np.sqrt(H)), (B_IH, 0.1 * rng.standard_normal(4 * H)),
                          (B_HH, 0.1 * rng.standard_normal(4 * H))])
    params = OrderedDict((k, v.astype(np.float32)) for k, v in params.items())
    kind = rng.integers(0, 6, size=rows)
    kind[:6] = np.arange(6)                    # every kind at any row count; row 0 is empty
    kind[rows - 1] = 1                         # the last row (of the ragged tile) is full-length
    ln = np.where(kind == 0, 0, np.where(kind == 1, L, rng.integers(1, L + 1, size=rows)))
    tok = np.where(np.arange(L)[None] < ln[:, None], rng.integers(1, V, size=(rows, L)), 0).astype(np.float32)
    gap = np.flatnonzero((kind == 2) & (ln >= 3))          # a zero inside the prefix: counted out, but embedded
    tok[gap, rng.integers(0, ln[gap] - 1)] = 0
    far = np.flatnonzero((kind == 3) & (ln + 1 < L))       # one more token behind a gap: counted, but outside the prefix
    tok[far, ln[far] + 1] = rng.integers(1, V, size=len(far))
    cot = rng.standard_normal((rows, H)).astype(np.float32)
    bad = np.flatnonzero(kind == 4)[::7]                   # out-of-range tokens, in rows without gradient
    tok[bad, 0] = np.resize(np.array([V, -3.0, 1e9, np.nan, V + 7, 0.5], np.float32), len(bad))
    cot[bad] = 0
    return dict(V=V, Ed=Ed, H=H, L=L, params=params, tok=tok, cot=cot)
