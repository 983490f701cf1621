"""srl_mlp_fwd / srl_mlp_bwd on one of the chains with kernels instantiated for their shape (csrc/mlp_sig.h) alone:
scripts/mlp_c1_probe.py [rows = 524288] [chain = c1]; per-launch times by HIP events, and the output / gradient sums as a fingerprint.
  c1         the C1 tower: LN4, 4->64 relu, LN64, 64->64 relu, 64->64 relu, 64->2
  smac-obs   the SMAC observation encoder: LN30, 30->64 relu, LN64, 64->64 relu, LN64
  smac-tail  the SMAC actor tail: LN64, 64->9, its backward pass with the input gradient (srl_mlp_bwd_dx)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from srl_amd import hip
DEV = "cuda:0"
CHAINS = {
    "c1": [(0, 4, 4, 0), (1, 4, 64, 1), (0, 64, 64, 0), (1, 64, 64, 1), (1, 64, 64, 1), (1, 64, 2, 0)],
    "smac-obs": [(0, 30, 30, 0), (1, 30, 64, 1), (0, 64, 64, 0), (1, 64, 64, 1), (0, 64, 64, 0)],
    "smac-tail": [(0, 64, 64, 0), (1, 64, 9, 0)],
}
rows = int(sys.argv[1]) if len(sys.argv) > 1 else 524288
name = sys.argv[2] if len(sys.argv) > 2 else "c1"
chain = CHAINS[name]
din, dout = chain[0][1], (chain[-1][2] if chain[-1][0] == 1 else chain[-1][1])
g = torch.Generator(device=DEV).manual_seed(0)
f = lambda *s: torch.randn(*s, device=DEV, generator=g)
keep, desc = [], []
for kind, i, o, act in chain:
    if kind == 0:
        w, b = 1 + 0.1 * f(i), 0.1 * f(i)
    else:
        w, b = f(o, i) / i ** 0.5, 0.1 * f(o)
    gw, gb = torch.zeros_like(w), torch.zeros_like(b)
    keep += [w, b, gw, gb]
    desc.append((kind, i, o, act, w.data_ptr(), b.data_ptr(), gw.data_ptr(), gb.data_ptr()))
arr = hip.mlp_layers(desc)
tld = hip.mlp_tape_floats_at(arr, rows)
x, dy = f(rows, din), f(rows, dout)
tape = torch.empty(rows, max(tld, 1), device=DEV) if tld else None
tp = tape.data_ptr() if tape is not None else 0
y = torch.empty(rows, dout, device=DEV)
fw = lambda: hip.mlp_fwd(arr, x.data_ptr(), din, rows, tp, tld, y.data_ptr(), dout)
if name == "smac-tail":
    dx = torch.empty(rows, din, device=DEV)
    bw = lambda: hip.mlp_bwd_dx(arr, x.data_ptr(), din, rows, dy.data_ptr(), dout, dx.data_ptr(), din)
else:
    bw = lambda: hip.mlp_bwd(arr, x.data_ptr(), din, rows, tp, tld, dy.data_ptr(), dout)
def timeit(fn, n=20):
    for _ in range(3):
        fn()
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return a.elapsed_time(e) / n * 1e3
fw()
for t in keep[2::4] + keep[3::4]:
    t.zero_()
bw()
torch.cuda.synchronize()
print(f"rows {rows} tape floats {tld}: y sum {float(y.double().sum()):.6f}  grads " + " ".join(f"{float(t.double().sum()):.5f}" for t in keep[2::4]))
print(f"fwd {timeit(fw):8.1f} us   bwd {timeit(bw):8.1f} us", flush=True)
