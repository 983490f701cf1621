"""Forward and backward time of the fused attention block at the SMAC batch (307 200 rows, H = 64, the 3m split)."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from srl_amd import hip

n, D, S = 307200, 32, 1
keys = [(2, 5), (3, 5), (1, 4)]
E = sum(c for c, _ in keys)
dev = "cuda"
torch.manual_seed(0)
sizes = {hip.EATTN_LN_SELF_W: S, hip.EATTN_LN_SELF_B: S, hip.EATTN_SELF_W: D * S, hip.EATTN_SELF_B: D, hip.EATTN_PRE_W: D,
         hip.EATTN_PRE_B: D}
for s in (hip.EATTN_Q_W, hip.EATTN_K_W, hip.EATTN_V_W):
    sizes[s], sizes[s + 1] = D * D, D
for k, (c, f) in enumerate(keys):
    sizes[hip.EATTN_LN_KEY_W + k] = sizes[hip.EATTN_LN_KEY_B + k] = f
    sizes[hip.EATTN_KEY_W + k], sizes[hip.EATTN_KEY_B + k] = D * (S + f), D
P = {s: (torch.randn(m, device=dev) * 0.2 + (1.0 if s in (0, 2, 3, 4, 16) else 0.0)) for s, m in sizes.items()}
G = {s: torch.zeros(m, device=dev) for s, m in sizes.items()}
desc = hip.entity_attn_desc(D, S, keys, {s: t.data_ptr() for s, t in P.items()}, {s: t.data_ptr() for s, t in G.items()})
xs = torch.randn(n, S, device=dev)
xk = [torch.randn(n, c, f, device=dev) for c, f in keys]
mask = (torch.rand(n, E, device=dev) < 0.8).to(torch.uint8)
out = torch.empty(n, 2 * D, device=dev)
dout = torch.randn(n, 2 * D, device=dev)
leaves = ((xs.data_ptr(), S), [(t.data_ptr(), c * f) for t, (c, f) in zip(xk, keys)], (mask.data_ptr(), E))
for _ in range(5):
    hip.entity_attn_fwd(desc, *leaves, n, out.data_ptr(), 2 * D)
    hip.entity_attn_bwd(desc, *leaves, n, dout.data_ptr(), 2 * D)
torch.cuda.synchronize()
ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
ev[0].record()
for _ in range(10):
    hip.entity_attn_fwd(desc, *leaves, n, out.data_ptr(), 2 * D)
ev[1].record()
for _ in range(10):
    hip.entity_attn_bwd(desc, *leaves, n, dout.data_ptr(), 2 * D)
ev[2].record()
torch.cuda.synchronize()
nbytes = 4 * n * (S + sum(c * f for c, f in keys) + 2 * D) + n * E
print(f"rows {n} D {D} E {E}: forward {ev[0].elapsed_time(ev[1]) / 10:.3f} ms, backward {ev[1].elapsed_time(ev[2]) / 10:.3f} ms; "
      f"leaves + output {nbytes / 1e6:.1f} MB (backward: leaves + d_out the same)")
print("finite", bool(torch.isfinite(out).all()), bool(all(torch.isfinite(t).all() for t in G.values())))
