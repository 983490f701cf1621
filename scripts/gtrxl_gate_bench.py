"""GTrXL's GRU-style gating unit (csrc/gtrxl_gate.hip) against the same arithmetic composed from torch operators, on one GPU.

Three shapes (D, rows): (256, 32 * 4096), (128, 32 * 4096) and the rollout step (256, 4096).  Per shape: forward and backward of the
kernel (``hip.gtrxl_gate_fwd`` saving the gates / ``hip.gtrxl_gate_bwd``, the fold launch included, the weight gradients not) and
of the torch composition (six F.linear and the row arithmetic; its backward through autograd with respect to x and y), device
events around 10 calls, 9 repetitions, the two ways alternating; microseconds per call, median / min / max.  Also the torch /
kernel ratio, the kernel's byte floor -- forward x, y read and g, gates written, backward dg, x, y, gates read and dx, dy, A, rx
written, once, at 8 TB/s -- and its float32-matrix flop floor (12 rows D^2 flops per direction at 157.3 TFLOP/s), each over the
median, and the largest difference of the two outputs.  Prints one JSON line per shape; ``--out FILE`` writes them all.

    python scripts/gtrxl_gate_bench.py [--out gtrxl_gate_bench.json]
"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from srl_amd import hip

DEV, HBM_BYTES_PER_S, F32_MATRIX_FLOPS = "cuda:0", 8e12, 157.3e12
SHAPES = [(256, 32 * 4096), (128, 32 * 4096), (256, 4096)]


def torch_gate(x, y, W, U, bg):
    """GRUGatingUnit.forward, operator for operator: W = (Wr, Wz, Wg), U = (Ur, Uz, Ug)."""
    r = torch.sigmoid(F.linear(y, W[0]) + F.linear(x, U[0]))
    z = torch.sigmoid(F.linear(y, W[1]) + F.linear(x, U[1]) - bg)
    h = torch.tanh(F.linear(y, W[2]) + F.linear(r * x, U[2]))
    return (1 - z) * x + z * h


def timed(fns, reps=9, inner=10):
    times = {name: [] for name in fns}
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / inner * 1e3)
    return {name: dict(median_us=statistics.median(v), min_us=min(v), max_us=max(v)) for name, v in times.items()}


def case(D, rows):
    g = torch.Generator().manual_seed(1)
    rn = lambda *sh: torch.randn(*sh, generator=g).to(DEV)
    x, y, dg, w_y, w_x, bg = rn(rows, D), rn(rows, D), rn(rows, D), D ** -0.5 * rn(3 * D, D), D ** -0.5 * rn(3 * D, D), 2 + 0.1 * rn(D)
    out, gates, saved = torch.empty(rows, D, device=DEV), torch.empty(rows, 3 * D, device=DEV), torch.empty(rows, 3 * D, device=DEV)
    dx, dy, rx, d_bg = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x), torch.empty(D, device=DEV)
    ws = torch.empty(hip.gtrxl_gate_bwd_workspace(D, rows) // 4, device=DEV)

    def k_fwd():
        hip.gtrxl_gate_fwd(x.data_ptr(), D, y.data_ptr(), D, w_y.data_ptr(), w_x.data_ptr(), bg.data_ptr(), rows, D, out.data_ptr(), D,
                           gates.data_ptr(), 3 * D)

    def k_bwd():   # (overwrites `gates` with A: from the second call on it runs on A as if it were gates -- the same work)
        hip.gtrxl_gate_bwd(dg.data_ptr(), D, x.data_ptr(), D, y.data_ptr(), D, w_y.data_ptr(), w_x.data_ptr(), saved.data_ptr(), 3 * D,
                           rows, D, dx.data_ptr(), D, dy.data_ptr(), D, rx.data_ptr(), D, d_bg.data_ptr(), ws.data_ptr(), ws.numel() * 4)

    xl, yl = x.clone().requires_grad_(), y.clone().requires_grad_()
    W, U = [w_y[i * D:(i + 1) * D] for i in range(3)], [w_x[i * D:(i + 1) * D] for i in range(3)]
    t_fwd = lambda: torch_gate(xl, yl, W, U, bg)
    ref = t_fwd()

    def t_bwd():
        torch.autograd.grad(ref, [xl, yl], dg, retain_graph=True)

    k_fwd()
    saved.copy_(gates)
    k_bwd()
    torch.cuda.synchronize()
    tdx, tdy = torch.autograd.grad(ref, [xl, yl], dg, retain_graph=True)
    rec = dict(max_abs_out_diff=float((out - ref.detach()).abs().max()), max_abs_dx_diff=float((dx - tdx).abs().max()),
               max_abs_dy_diff=float((dy - tdy).abs().max()))
    rec.update(timed({"kernel_fwd": k_fwd, "torch_fwd": lambda: t_fwd().detach(), "kernel_bwd": k_bwd, "torch_bwd": t_bwd}))
    for d, cols in (("fwd", 6), ("bwd", 12)):   # [rows, D] float32 blocks moved once: x, y, g, 3 gates / dg, x, y, 3 gates, dx, dy, 3 A, rx
        med = rec[f"kernel_{d}"]["median_us"]
        rec[f"{d}_byte_floor_us"] = cols * rows * D * 4 / HBM_BYTES_PER_S * 1e6
        rec[f"{d}_flop_floor_us"] = 12.0 * rows * D * D / F32_MATRIX_FLOPS * 1e6
        rec[f"{d}_fraction_of_byte_floor"] = rec[f"{d}_byte_floor_us"] / med
        rec[f"{d}_fraction_of_flop_floor"] = rec[f"{d}_flop_floor_us"] / med
        rec[f"{d}_torch_over_kernel"] = rec[f"torch_{d}"]["median_us"] / med
    print(json.dumps({"shape": [D, rows], **rec}), flush=True)
    return rec


if __name__ == "__main__":
    assert torch.cuda.is_available()
    res = {"-".join(map(str, sh)): case(*sh) for sh in SHAPES}
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(res, f, indent=1)
