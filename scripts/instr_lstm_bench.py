"""Forward and backward time of the fused language encoder (csrc/instr_lstm.hip) at one chunk-sized slice of the flagship batch
(4096 x 128 / 8 = 65 536 rows, L = 16, the reference's sizes: 1000 words of 20 columns, 64 units), once with realistic tokens (nine
rows in ten empty, the rest 1..16 tokens) and once with every row full; in the same process torch-ROCm's own composition
(nn.Embedding -> pack_padded_sequence -> nn.LSTM -> the output at each row's last step, as dmlab_policy.py:144-158 runs it) on the
same tensors as the yardstick.  Device events around windows of at least `--min-ms` of work, after a warm-up of every shape; the two
implementations alternate.  Prints one line per token mix and a JSON line at the end.

    python scripts/instr_lstm_bench.py [--rows 65536] [--min-ms 300]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from srl_amd import hip

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=4096 * 128 // 8)
ap.add_argument("--min-ms", type=float, default=300.0)
args = ap.parse_args()
hip.require_gpu()
n, V, Ed, H, L = args.rows, 1000, 20, 64, 16
dev = "cuda"
torch.manual_seed(0)
emb = torch.nn.Embedding(V, Ed, padding_idx=0).to(dev)
lstm = torch.nn.LSTM(Ed, H, batch_first=True).to(dev)
names = dict(emb=emb.weight, w_ih=lstm.weight_ih_l0, w_hh=lstm.weight_hh_l0, b_ih=lstm.bias_ih_l0, b_hh=lstm.bias_hh_l0)
P = {k: v.detach().clone().contiguous() for k, v in names.items()}
G = {k: torch.zeros_like(v) for k, v in P.items()}
desc = hip.instr_lstm_desc(V, Ed, H, L, {k: t.data_ptr() for k, t in P.items()}, {k: t.data_ptr() for k, t in G.items()})
nbytes = hip.instr_lstm_bwd_workspace(desc, n)
ws = torch.empty(nbytes // 4, device=dev)
out = torch.empty(n, H, device=dev)
dout = torch.randn(n, H, device=dev)


def tokens(empty):
    g = torch.Generator().manual_seed(1)
    lens = torch.randint(1, L + 1, (n,), generator=g)
    lens[torch.rand(n, generator=g) < empty] = 0
    tok = torch.randint(1, V, (n, L), generator=g) * (torch.arange(L)[None] < lens[:, None])
    return tok.float().to(dev)


def ours_fwd(tok):
    hip.instr_lstm_fwd(desc, tok.data_ptr(), L, False, n, out.data_ptr(), H)


def ours_bwd(tok):
    hip.instr_lstm_bwd(desc, tok.data_ptr(), L, False, n, dout.data_ptr(), H, ws.data_ptr(), nbytes)


def torch_fwd(tok):
    t = tok.long()
    lens = (t != 0).sum(-1).clamp(min=1)
    x = emb(t[:, :int(lens.max())])
    packed = torch.nn.utils.rnn.pack_padded_sequence(x, lens.cpu(), batch_first=True, enforce_sorted=False)
    y, _ = lstm(packed)
    y, sl = torch.nn.utils.rnn.pad_packed_sequence(y, batch_first=True)
    return y[torch.arange(n, device=dev), sl.to(dev) - 1]


@torch.no_grad()
def torch_fwd_only(tok):
    torch_fwd(tok)


def torch_fwd_bwd(tok):
    for p in names.values():
        p.grad = None
    (torch_fwd(tok) * dout).sum().backward()


def timed(fn, tok):
    """ms per call: windows of at least --min-ms between device events, the count found from a first window."""
    for _ in range(3):
        fn(tok)
    torch.cuda.synchronize()
    reps = 4
    while True:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn(tok)
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        if ms >= args.min_ms or reps >= 1 << 16:
            return ms / reps
        reps = int(reps * max(2.0, 1.2 * args.min_ms / max(ms, 1e-3)))


result = dict(rows=n, V=V, Ed=Ed, H=H, L=L)
for mix, empty in (("realistic", 0.9), ("full", 0.0)):
    tok = tokens(empty)
    with torch.no_grad():
        ours_fwd(tok)
        err = float((out - torch_fwd(tok)).abs().max())
    r = {}
    for rnd in range(2):   # alternate; keep the better of two rounds of each
        for name, fn in (("fwd", ours_fwd), ("bwd", ours_bwd), ("torch_fwd", torch_fwd_only), ("torch_fwd_bwd", torch_fwd_bwd)):
            r[name] = min(timed(fn, tok), r.get(name, 1e30))
    steps = int(((tok != 0).sum(-1).clamp(min=1)).sum())
    floor = 4 * n * (L + H) + 4 * (V * Ed + 4 * H * (Ed + H + 2))   # tokens in, features out, the parameters once
    result[mix] = dict(r, row_steps=steps, max_abs_diff_to_torch=err, floor_bytes=floor)
    print(f"{mix}: rows {n} row-steps {steps}: forward {r['fwd']:.3f} ms, backward {r['bwd']:.3f} ms; torch forward {r['torch_fwd']:.3f} ms, "
          f"torch forward + backward {r['torch_fwd_bwd']:.3f} ms; largest |difference| of the outputs {err:.2e}; "
          f"byte floor {floor / 1e6:.1f} MB = {floor / 8e12 * 1e3:.4f} ms at 8 TB/s (backward: d_out for the features)")
print(json.dumps(result))
