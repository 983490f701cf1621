"""srl_ln_heads_fwd / srl_ln_heads_bwd -- or, from 9 head outputs, srl_ln_heads_wide_fwd / srl_ln_heads_wide_bwd -- alone at the
Atari chunk's size (16 384 x 512; heads 6 + 1 by default, --heads 18,1 for the full action set): launch times by HIP events and
the fraction of the pair's byte floor (forward: x read once; backward: x read, dx written) at 8 TB/s.
    python scripts/ln_heads_probe.py [rows] [--heads 18,1] [--dim 512]"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from srl_amd import hip
ap = argparse.ArgumentParser()
ap.add_argument("rows", nargs="?", type=int, default=16384)
ap.add_argument("--heads", default="6,1")
ap.add_argument("--dim", type=int, default=512)
args = ap.parse_args()
n, D, heads = args.rows, args.dim, tuple(int(v) for v in args.heads.split(","))
wide = not hip.ln_heads_supported(D, heads)
assert not wide or hip.ln_heads_wide_supported(D, heads), (D, heads)
fwd, bwd = (hip.ln_heads_wide_fwd, hip.ln_heads_wide_bwd) if wide else (hip.ln_heads_fwd, hip.ln_heads_bwd)
d = "cuda:0"
g = torch.Generator(device=d).manual_seed(0)
f = lambda *s: torch.randn(*s, device=d, generator=g)
x = torch.relu(f(n, D)); gam, bet = 1 + 0.1 * f(D), 0.1 * f(D)
W, b = [f(a, D) / D ** 0.5 for a in heads], [0.1 * f(a) for a in heads]
y = [torch.empty(n, a, device=d) for a in heads]
mean, rstd = torch.empty(n, device=d), torch.empty(n, device=d)
dy = [f(n, a) for a in heads]
dx = torch.empty(n, D, device=d)
dg, db = torch.zeros(D, device=d), torch.zeros(D, device=d)
dW, dhb = [torch.zeros_like(w) for w in W], [torch.zeros_like(v) for v in b]
P = lambda ts: [t.data_ptr() for t in ts]
fw = lambda: fwd(x.data_ptr(), D, n, D, gam.data_ptr(), bet.data_ptr(), P(W), P(b), list(heads), P(y), list(heads), mean.data_ptr(), rstd.data_ptr())
bw = lambda: bwd(x.data_ptr(), D, n, D, gam.data_ptr(), bet.data_ptr(), mean.data_ptr(), rstd.data_ptr(), P(W), list(heads), P(dy), list(heads), 1,
                 dx.data_ptr(), D, dg.data_ptr(), db.data_ptr(), P(dW), P(dhb))
def timeit(fn, k=50):
    for _ in range(5): fn()
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); a.record()
    for _ in range(k): fn()
    e.record(); torch.cuda.synchronize()
    return a.elapsed_time(e) / k * 1e3
tf, tb = timeit(fw), timeit(bw)
floor_f, floor_b = n * D * 4 / 8e12 * 1e6, 2 * n * D * 4 / 8e12 * 1e6
print(f"{'wide' if wide else 'narrow'} n {n} D {D} heads {heads}: fwd {tf:7.1f} us ({floor_f / tf:.2f} of the byte floor {floor_f:.1f} us)  "
      f"bwd {tb:7.1f} us ({floor_b / tb:.2f} of {floor_b:.1f} us)")
